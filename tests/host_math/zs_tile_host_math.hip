// The matrix-core tile map of the topic, matvar, svgd and mix kernels (csrc/zs_tile_math.h: __host__ __device__) compiled for the
// HOST and run under AddressSanitizer + UndefinedBehaviorSanitizer (tests/test_tile_host_math.py):
//     hipcc -x hip --cuda-host-only -Xarch_host -fsanitize=address,undefined ...
// For float and double: (a) (lane, v) -> (acc_row(q, v), m) covers a 16 x 16 tile, an exactly-sized heap array, exactly once;
// (b) the output rows 2 t and 2 t + 1 are neighbours -- one lane, registers v and v | 1 (float); lanes q and q ^ 1, one register
// (double) --, which is what the mix kernels' gradients rest on; (c) the panel arithmetic and the 16-wide round-up, with the
// libraries' own sizes that are built on them; (d) the LDS bank figures that the comments of zs_tile_math.h, zs_matvar_math.h and
// zs_svgd_math.h quote, COMPUTED over 64 banks of 4 bytes (an element of T is sizeof(T) / 4 consecutive words) for every step of
// every tile shape the kernels run.  Prints "tile host math ok: N checks".
#include <set>
#include <vector>

#include "../../zhusuan-pytorch_amd/csrc/zs_tile_math.h"
#include "../../zhusuan-pytorch_amd/csrc/zs_topic_math.h"
#include "../../zhusuan-pytorch_amd/csrc/zs_matvar_math.h"
#include "../../zhusuan-pytorch_amd/csrc/zs_svgd_math.h"
#include "../../zhusuan-pytorch_amd/csrc/zs_mix_math.h"
#include "zs_host_check.h"

// ---------------------------------------------------------------- (a), (b): the map
template <typename T>
static void check_map() {
  for (int thread = 0; thread < 1024; ++thread) {
    const int m = zs::mfma_m(thread), q = zs::mfma_q(thread), wave = zs::mfma_wave(thread);
    expect(m >= 0 && m < 16 && q >= 0 && q < 4 && 64 * wave + 16 * q + m == thread, "thread = 64 wave + 16 q + m", 64 * wave + 16 * q + m, thread);
  }
  int* tile = new int[256]();           // exactly 16 x 16: a row or a column past the tile is a heap overrun
  int* lane_of = new int[256];
  int* reg_of = new int[256];
  for (int lane = 0; lane < 64; ++lane) {
    for (int v = 0; v < 4; ++v) {
      const int at = zs::MfmaTile<T>::acc_row(zs::mfma_q(lane), v) * 16 + zs::mfma_m(lane);
      ++tile[at];
      lane_of[at] = lane;
      reg_of[at] = v;
    }
  }
  for (int i = 0; i < 256; ++i) expect(tile[i] == 1, "every element of the tile held once", tile[i], 1);
  const bool f32 = sizeof(T) == 4;
  for (int t = 0; t < 8; ++t) {
    for (int m = 0; m < 16; ++m) {
      const int even = (2 * t) * 16 + m, odd = (2 * t + 1) * 16 + m;
      const int le = lane_of[even], lo = lane_of[odd], ve = reg_of[even], vo = reg_of[odd];
      if (f32) {
        expect(lo == le && (ve & 1) == 0 && vo == (ve | 1), "float: rows 2 t and 2 t + 1 in one lane, registers v and v | 1", vo, ve | 1);
      } else {
        expect(vo == ve && (zs::mfma_q(le) & 1) == 0 && lo == (le ^ 16) && zs::mfma_q(lo) == (zs::mfma_q(le) ^ 1),
               "double: rows 2 t and 2 t + 1 in the lanes q and q ^ 1 (lane ^ 16), one register", lo, le ^ 16);
      }
      // the holder of the even row as the mix kernels find it
      expect((zs::MfmaTile<T>::acc_row(zs::mfma_q(le), ve) & 1) == 0 && (zs::MfmaTile<T>::acc_row(zs::mfma_q(lo), vo) & 1) == 1, "acc_row's parity picks the even row's holder", le, lo);
    }
  }
  delete[] tile;
  delete[] lane_of;
  delete[] reg_of;
}

// ---------------------------------------------------------------- (c): the panel arithmetic and the round-up
template <typename T>
static void check_panels() {
  const int eb = (int)sizeof(T), p = zs::panel_cols(eb);
  expect(p == zs::MfmaPanel<T>::PANEL && p == (eb == 4 ? 64 : 32) && p % 16 == 0, "panel columns", p, zs::MfmaPanel<T>::PANEL);
  expect(zs::MfmaPanel<T>::LD == p + 17, "LD = PANEL + 17", zs::MfmaPanel<T>::LD, p + 17);
  for (int64_t k = 1; k <= 5; ++k) {
    for (int64_t n = k * p - 3; n <= k * p + 3; ++n) {
      if (n < 1) continue;
      const int64_t P = zs::panels(eb, n);
      expect(P * p >= n && n > (P - 1) * p, "panels cover n and no more", (double)P, (double)n);
      expect(zs::mix_cpad(eb, n) == P * p, "mix: the padded components", (double)zs::mix_cpad(eb, n), (double)(P * p));
    }
  }
  for (int64_t n : {(int64_t)1 << 31, ((int64_t)1 << 31) + 1, ((int64_t)1 << 40) - 1}) {
    const int64_t P = zs::panels(eb, n);
    expect(P * p >= n && n > (P - 1) * p, "panels cover a large n", (double)P, (double)n);
  }
  expect(zs::panels(eb, 0) == 0 && zs::panels(eb, -1) == 0 && zs::panels(eb, INT64_MIN) == 0, "no panels for n < 1", 0, 0);
}

static void check_round_ups() {
  for (int bad : {0, 1, 2, 3, 5, 16, -4}) expect(zs::panel_cols(bad) == 0 && zs::panels(bad, 64) == 0, "no panels for an unknown element size", bad, 0);
  for (int d = 1; d <= 300; ++d) {
    const int b = zs::blocks16(d);
    expect(16 * b >= d && d > 16 * (b - 1), "blocks16 covers d and no more", b, d);
    expect(zs::blocks16((int64_t)d) == b && zs::svgd_blocks(d) == b, "blocks16 of either integer type", b, d);
    expect(zs::topic_k16(d) == 16 * b && zs::mix_k16(d) == 16 * zs::blocks16(2 * d), "the staged panels' rows", (double)zs::topic_k16(d), 16 * b);
    expect(4 * zs::topic_steps(d) >= d && 4 * zs::topic_steps(d) <= zs::topic_k16(d) && 4 * zs::mix_steps(d) >= 2 * d && 4 * zs::mix_steps(d) <= zs::mix_k16(d),
           "the matrix steps cover k inside the staged rows", zs::topic_steps(d), d);
    expect(zs::matvar_ld(d) == 16 * b + ZS_MATVAR_PAD, "matvar: LD = p16 + 12", zs::matvar_ld(d), 16 * b + 12);
  }
  expect(zs::blocks16(((int64_t)1 << 31) + 1) == ((int64_t)1 << 27) + 1, "blocks16 past 2^31", 0, 0);
  expect(4 * ZS_TOPIC_MAX_STEPS == ZS_TOPIC_MAX_TOPICS && 4 * ZS_MIX_MAX_STEPS == 2 * ZS_MIX_MAX_DIM, "the step caps hold the largest k", 0, 0);
}

// ---------------------------------------------------------------- (d): banks
struct Banks {
  int distinct, worst;          // banks reached by the 64 lanes' words; the most words in one bank
};
// the 64 lanes of one matrix step, lane 16 q + m reading element addr(q, m) of an array of T
template <typename T, typename F>
static Banks bank_load(F addr) {
  const int words = (int)sizeof(T) / 4;
  int count[64] = {0};
  for (int q = 0; q < 4; ++q)
    for (int m = 0; m < 16; ++m)
      for (int w = 0; w < words; ++w) ++count[(addr(q, m) * words + w) % 64];
  Banks b = {0, 0};
  for (int c : count) {
    b.distinct += c > 0;
    b.worst = c > b.worst ? c : b.worst;
  }
  return b;
}
// the banks in which the four k-rows of a step start (m = 0)
template <typename T, typename F>
static std::vector<int> row_starts(F addr) {
  std::vector<int> s;
  for (int q = 0; q < 4; ++q) s.push_back((int)(addr(q, 0) * (sizeof(T) / 4) % 64));
  return s;
}
static bool all_different(const std::vector<int>& s) { return std::set<int>(s.begin(), s.end()).size() == s.size(); }

template <typename T>
static void check_banks() {
  const bool f32 = sizeof(T) == 4;
  const int ideal = (int)sizeof(T) / 4;          // 64 lanes' words over 64 banks
  // the staged panel of the topic and mix kernels: (4 s + q) LD + m, from any tile of the panel
  constexpr int LD = zs::MfmaPanel<T>::LD, P = zs::MfmaPanel<T>::PANEL;
  for (int s = 0; s < ZS_TOPIC_MAX_STEPS; ++s) {
    for (int ct = 0; ct < P / 16; ++ct) {
      auto addr = [&](int q, int m) { return (long)(4 * s + q) * LD + ct * 16 + m; };
      const Banks b = bank_load<T>(addr);
      const std::vector<int> st = row_starts<T>(addr);
      expect(all_different(st), "panel: the four k-rows start in four different banks", st[1], st[0]);
      if (f32) {
        for (int q = 1; q < 4; ++q) expect((st[q] - st[q - 1] + 64) % 64 == 17, "panel, float: the k-rows start 17 banks apart", st[q], st[q - 1]);
        expect(b.distinct == 61 && b.worst == 2, "panel, float: 61 banks, three of them twice", b.distinct, 61);
      } else {
        expect((st[1] - st[0] + 64) % 64 == 34 && (st[2] - st[0] + 64) % 64 == 4 && (st[3] - st[0] + 64) % 64 == 38, "panel, double: the k-rows start at words 0, 34, 4, 38", st[1], st[0]);
        expect(b.distinct == 64 && b.worst == 3, "panel, double: every bank, none more than three times", b.worst, 3);
      }
    }
  }
  // matvar: LD = p16 + 12 = 4 (4 j + 3); along a row m LD + 4 s + q, down a column (4 s + q) LD + 16 jb + m
  for (int p16 = 16; p16 <= 128; p16 += 16) {
    const int ld = zs::matvar_ld(p16);
    expect(ld == p16 + 12 && ld % 4 == 0 && (ld / 4) % 2 == 1, "matvar: LD is four times an odd number", ld, p16 + 12);
    for (int s = 0; s < p16 / 4; ++s) {
      const Banks row = bank_load<T>([&](int q, int m) { return (long)m * ld + 4 * s + q; });
      expect(row.distinct == 64 && row.worst == ideal, "matvar: a row read reaches every bank equally", row.worst, ideal);
      auto col = [&](int q, int m) { return (long)(4 * s + q) * ld + m; };
      const std::vector<int> st = row_starts<float>(col);
      const int apart = (st[1] - st[0] + 64) % 64;
      expect(all_different(row_starts<T>(col)) && apart == ld % 64 && (apart == 12 || apart == 28 || apart == 44 || apart == 60),
             "matvar: the k-rows of a column read start in four different banks, LD mod 64 apart", apart, ld % 64);
    }
  }
  // svgd: gram m LD + 4 s + q with LD = 36; update (4 s + q) LD + 16 cb + m with LD = 48
  expect(ZS_SVGD_LD_GRAM == 36 && ZS_SVGD_LD_UPDATE == 48 && ZS_SVGD_LD_GRAM % 4 == 0 && (ZS_SVGD_LD_GRAM / 4) % 2 == 1, "svgd: the leading dimensions", ZS_SVGD_LD_GRAM, ZS_SVGD_LD_UPDATE);
  for (int s = 0; s < ZS_SVGD_SLAB / 4; ++s) {
    const Banks g = bank_load<T>([&](int q, int m) { return (long)m * ZS_SVGD_LD_GRAM + 4 * s + q; });
    expect(g.distinct == 64 && g.worst == ideal, "svgd gram: a step reaches every bank equally", g.worst, ideal);
  }
  for (int s = 0; s < zs::SvgdCap<T>::MAX_K / 4; ++s) {
    for (int cb = 0; cb < ZS_SVGD_SLAB / 16; ++cb) {
      auto addr = [&](int q, int m) { return (long)(4 * s + q) * ZS_SVGD_LD_UPDATE + 16 * cb + m; };
      const Banks u = bank_load<T>(addr);
      expect(u.distinct == 64 && u.worst == ideal, "svgd update: a step reaches every bank equally", u.worst, ideal);
      const std::vector<int> st = row_starts<float>(addr);
      expect((st[1] - st[0] + 64) % 64 == 48 && (st[2] - st[0] + 64) % 64 == 32 && (st[3] - st[0] + 64) % 64 == 16, "svgd update: the k-rows start 48 float32 banks apart", st[1], st[0]);
    }
  }
}

int main() {
  check_map<float>();
  check_map<double>();
  check_panels<float>();
  check_panels<double>();
  check_round_ups();
  check_banks<float>();
  check_banks<double>();
  return finish("tile host math ok");
}
