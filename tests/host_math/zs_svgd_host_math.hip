// The index maps and the selection of Stein variational gradient descent (csrc/zs_svgd_math.h: __host__ __device__) compiled for
// the HOST and run under AddressSanitizer + UndefinedBehaviorSanitizer (tests/test_svgd_host_math.py):
//     hipcc -x hip --cuda-host-only -Xarch_host -fsanitize=address,undefined ...
// Exhaustively for K = 1 .. 256: (1) the tile-pair <-> wave map of the gram kernel -- every pair of the lower triangle of blocks is
// accumulator slot p / 8 of wave p % 8, exactly once, inside the tier the host picks, and the lanes' (row, column) of a pair cover
// an exactly-sized K x K heap array once per triangle; (2) the padded-row mask; (3) the bit-pattern selection, restated as the
// finish kernel runs it (one count per bit), against a sorted array: ties, even and odd counts, zeros, K^2 distances of integer
// lattices; and the bandwidth and the distance clamp.  Prints "svgd host math ok: N checks".
#include <algorithm>
#include <vector>

#include "../../zhusuan-pytorch_amd/csrc/zs_svgd_math.h"
#include "zs_host_check.h"

template <typename T>
static void check_pairs(int K) {
  const int nb = zs::svgd_blocks(K), npairs = zs::svgd_pairs(nb), ppw = zs::svgd_pairs_per_wave(nb);
  const int tier = ppw <= 1 ? 1 : (ppw <= 5 ? 5 : 17);
  expect(16 * nb >= K && 16 * nb < K + 16, "blocks cover K", nb, K);
  expect(ppw <= tier && (tier < 17 || K > 128), "the tier holds the pairs of a wave", ppw, tier);
  std::vector<int> seen(nb * nb, 0);
  std::vector<int> written((size_t)K * K, 0);
  for (int wave = 0; wave < ZS_SVGD_GRAM_WAVES; ++wave) {
    for (int slot = 0; slot < tier; ++slot) {
      const int p = zs::svgd_pair_index(wave, slot);
      if (p >= npairs) continue;
      expect(p % ZS_SVGD_GRAM_WAVES == wave && p / ZS_SVGD_GRAM_WAVES == slot, "pair p is slot p / 8 of wave p % 8", p, wave);
      int bi, bj;
      zs::svgd_pair_of(p, bi, bj);
      expect(bj >= 0 && bj <= bi && bi < nb && bi * (bi + 1) / 2 + bj == p, "a pair of the lower triangle", bi, bj);
      ++seen.at(bi * nb + bj);
      for (int lane = 0; lane < 64; ++lane) {
        for (int v = 0; v < 4; ++v) {
          const int r = 16 * bi + zs::MfmaTile<T>::acc_row(lane >> 4, v), c = 16 * bj + (lane & 15);
          if (r < K && c < K) {
            ++written.at((size_t)r * K + c);
            if (bi != bj) ++written.at((size_t)c * K + r);
          }
        }
      }
    }
  }
  for (int bi = 0; bi < nb; ++bi)
    for (int bj = 0; bj < nb; ++bj) expect(seen[bi * nb + bj] == (bj <= bi ? 1 : 0), "every pair once", seen[bi * nb + bj], bj <= bi);
  long bad = 0;
  for (int w : written) bad += w != 1;
  expect(bad == 0, "every element of a partial written once", (double)bad, 0);
  for (int row = 0; row < 16 * nb; ++row) expect(zs::svgd_row_live(row, K) == (row < K), "padded rows are dead", row, K);
}

// the finish kernel's loop: both ranks at once, one count per bit
static double select_median(const std::vector<double>& x) {
  const int64_t n = (int64_t)x.size(), r0 = zs::svgd_rank_lo(n), r1 = zs::svgd_rank_hi(n);
  uint64_t a0 = 0, a1 = 0;
  for (int bit = 62; bit >= 0; --bit) {
    const uint64_t c0 = zs::svgd_candidate(a0, bit), c1 = zs::svgd_candidate(a1, bit);
    int64_t n0 = 0, n1 = 0;
    for (double v : x) {
      n0 += zs::svgd_bits(v) < c0;
      n1 += zs::svgd_bits(v) < c1;
    }
    a0 = zs::svgd_select_step(a0, bit, n0, r0);
    a1 = zs::svgd_select_step(a1, bit, n1, r1);
  }
  std::vector<double> s(x);
  std::sort(s.begin(), s.end());
  expect(zs::svgd_from_bits(a0) == s[r0] && zs::svgd_from_bits(a1) == s[r1], "the selected ranks", zs::svgd_from_bits(a0), s[r0]);
  expect(r0 + r1 == n - 1, "the two middle ranks", (double)r0, (double)r1);
  return zs::svgd_median_of(zs::svgd_from_bits(a0), zs::svgd_from_bits(a1));
}

static void check_selection() {
  for (int n = 1; n <= 300; ++n) {
    std::vector<double> x(n);
    for (int style = 0; style < 4; ++style) {
      for (double& v : x) {
        const double u = uniform01();
        v = style == 0 ? u * 1e3 : (style == 1 ? floor(u * 4.0) : (style == 2 ? (u < 0.7 ? 0.0 : ldexp(u, -1060)) : ldexp(1.0 + u, (int)(u * 600) - 300)));
      }
      const double med = select_median(x);
      std::vector<double> s(x);
      std::sort(s.begin(), s.end());
      const double want = n % 2 ? s[n / 2] : 0.5 * (s[n / 2 - 1] + s[n / 2]);
      expect(med == want, "the median as numpy.median defines it", med, want);
    }
  }
  for (int K : {1, 2, 7, 16, 33, 100, 256}) {          // the K^2 distances of an integer lattice in the plane: zero diagonal, many ties
    std::vector<double> d;
    for (int i = 0; i < K; ++i)
      for (int j = 0; j < K; ++j) {
        const double dx = i % 5 - j % 5, dy = i / 5 % 3 - j / 5 % 3;
        d.push_back(zs::svgd_dist(dx * dx + dy * dy, 0.0, 0.0, i == j));
      }
    const double med = select_median(d);
    const double h = zs::svgd_bandwidth(med, K);
    expect(med > 0 ? fabs(h - med / log(K + 1.0)) <= 1e-15 * h : h == 1.0, "the bandwidth", h, med);
  }
  expect(zs::svgd_dist(1.0, 1.0, 1.0 + 1e-9, false) == 0.0 && zs::svgd_dist(3.0, 5.0, 1.0, true) == 0.0 && zs::svgd_dist(3.0, 5.0, 1.0, false) == 6.0 &&
             zs::svgd_dist(NAN, 1.0, 1.0, false) == 0.0, "d is clamped, its diagonal zero", 0, 0);
}

int main() {
  for (int K = 1; K <= 256; ++K) {
    check_pairs<float>(K);
    if (K <= ZS_SVGD_MAX_PARTICLES_F64) check_pairs<double>(K);
  }
  expect(zs::svgd_max_particles_of(4) == 256 && zs::svgd_max_particles_of(8) == 128 && zs::svgd_max_particles_of(2) == 0, "caps", 0, 0);
  expect(zs::svgd_gram_slots(1) == 1 && zs::svgd_gram_slots(ZS_SVGD_SLAB + 1) == 2 && zs::svgd_gram_slots((int64_t)1 << 40) == ZS_SVGD_GRID_CAP, "slots", 0, 0);
  check_selection();
  return finish("svgd host math ok");
}
