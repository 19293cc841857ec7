// The flow kernels' per-element arithmetic and index maps (csrc/zs_flow_math.h: __host__ __device__) compiled for the HOST and
// run under AddressSanitizer + UndefinedBehaviorSanitizer (tests/test_flow_host_math.py):
//     hipcc -x hip --cuda-host-only -Xarch_host -fsanitize=address,undefined ...
// (1) every formula over a grid of operands -- zero, binary and non-binary masks, shift = 0, log_scale = +-80, tiny and large
// values -- against long-double restatements of the expressions of include/zs_flow.h, bound |err| <= 2^-20 S (float) /
// 2^-48 S (double), S the sum of the absolute values of the terms added (the bound of tests/test_flow_kernel.py); (2) the
// INTERLEAVE pair maps and the strided [B, 2D] maps of MADE's affine walked exactly as the kernels walk them, over exactly-sized
// heap arrays, against plain nested loops.  Prints "flow host math ok: N checks".
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <vector>

#include "../../zhusuan-pytorch_amd/csrc/zs_flow_math.h"
#include "zs_host_check.h"

template <typename T> static ld rel_bound() { return sizeof(T) == 4 ? ldexpl(1.0L, -20) : ldexpl(1.0L, -48); }
// results below the normal range of T carry an absolute, not a relative, rounding error: not held to the relative bound
template <typename T> static bool representable(ld want) { return want == 0 || fabsl(want) > (sizeof(T) == 4 ? 1e-30L : 1e-290L); }
template <typename T>
static void near(T got, ld want, ld S, const char* what) {
  if (!representable<T>(want)) return;
  expect(isfinite((double)got) && fabsl((ld)got - want) <= rel_bound<T>() * S, what, (double)got, (double)want);
}

template <typename T>
static void check_coupling() {
  const double masks[] = {0.0, 1.0, 0.25, -1.5, 0.5, 2.0};
  const double vals[] = {0.0, 1e-6, -1e-3, 0.37, -1.0, 2.5, -40.0, 1e3};
  for (double md : masks) for (double xd : vals) for (double sd : vals) for (double sg : {1.0, -1.0}) {
    const T m = (T)md, x = (T)xd, s = (T)sd, sign = (T)sg;
    const ld M = m, X = x, S = s, OM = 1.0L - M;
    near<T>(zs::flow_split_mask(m, x), M * X, fabsl(M * X), "split");
    near<T>(zs::flow_merge_mask(m, x, s, sign), M * X + (OM * X + sg * S * OM), fabsl(M * X) + fabsl(OM * X) + fabsl(S * OM), "merge");
    T gx, gs;
    zs::flow_merge_mask_bwd(m, x, sign, gx, gs);                                  // (x stands for gy)
    near<T>(gx, M * X + OM * X, fabsl(M * X) + fabsl(OM * X), "merge_bwd gx");
    near<T>(gs, sg * X * OM, fabsl(X * OM), "merge_bwd gshift");
    near<T>(zs::flow_shift_add(x, s, sign), X + sg * S, fabsl(X) + fabsl(S), "shift_add");
    if (md == 1.0 || md == 0.0) {                                                 // a binary mask passes x / adds the shift exactly
      expect(zs::flow_merge_mask(m, x, s, sign) == (md == 1.0 ? x : (T)(x + sign * s)), "merge binary exact",
             (double)zs::flow_merge_mask(m, x, s, sign), (double)(md == 1.0 ? x : (T)(x + sign * s)));
      expect(gx == x, "merge_bwd binary exact", (double)gx, (double)x);
    }
    if (sd == 0.0 && (md == 0.0 || md == 1.0))
      expect(zs::flow_merge_mask(m, x, s, sign) == x, "shift 0 is the identity", (double)zs::flow_merge_mask(m, x, s, sign), (double)x);
  }
}

template <typename T>
static void check_scale_and_made() {
  const double lss[] = {0.0, 1e-4, -0.5, 1.0, 3.0, -7.0, 80.0, -80.0};
  const double vals[] = {0.0, 1e-6, -1e-3, 0.37, -1.0, 2.5, -40.0};
  for (double ls : lss) for (double xd : vals) for (double sg : {1.0, -1.0}) {
    const T l = (T)ls, x = (T)xd, sign = (T)sg;
    const ld L = l, X = x;
    const T f = zs::flow_scale_factor(l, sign);
    near<T>(f, expl(sg * L), expl(sg * L), "scale factor");
    near<T>((T)(x * f), X * expl(sg * L), fabsl(X * expl(sg * L)), "scale y");
    for (double md : vals) {
      const T m = (T)md;
      const ld M = m, E = expl(-L);
      const ld U = (X - M) * E, Su = (fabsl(X) + fabsl(M)) * E;
      near<T>(zs::flow_made_u(x, m, l), U, Su, "made u");
      near<T>(zs::flow_made_inv(x, m, l), X * expl(L) + M, fabsl(X * expl(L)) + fabsl(M), "made inverse");
      for (double gd : {0.0, 1.0, -0.3}) for (double gl : {0.0, 0.7}) {
        const T gu = (T)gd, gld = (T)gl;
        T gx, gm, ga;
        zs::flow_made_bwd(gu, gld, x, m, l, gx, gm, ga);
        const ld GU = gu, GL = gld;
        near<T>(gx, GU * E, fabsl(GU * E), "made gx");
        near<T>(gm, -GU * E, fabsl(GU * E), "made gm");
        if (representable<T>(U)) near<T>(ga, -(GU * U) - GL, fabsl(GU) * Su + fabsl(GL), "made gloga");
      }
    }
  }
}

template <typename T>
static void check_tail() {
  const double zs_[] = {0.0, 1e-6, -1e-3, 0.37, -1.0, 2.5, -40.0, 30.0};
  const double locs[] = {0.0, 0.37, -2.0};
  const double scales[] = {1.0, 1e-2, 0.5, 3.0, 50.0};
  for (double zd : zs_) for (double ld_ : locs) for (double sd : scales) {
    const T z = (T)zd, loc = (T)ld_, sc = (T)sd;
    const ld Z = z, L = loc, S = sc;
    const ld c = -0.91893853320467274178L, prec = 1.0L / (S * S), q = 0.5L * prec * (Z - L) * (Z - L);
    near<T>(zs::flow_normal_lp(z, loc, sc), (c - logl(S)) - q, fabsl(c) + fabsl(logl(S)) + q, "normal lp");
    near<T>(zs::flow_normal_dz(z, loc, sc), -(prec * (Z - L)), fabsl(prec * (Z - L)), "normal dz");
    const ld t = (Z - L) / S, at = fabsl(t), sp = 2.0L * log1pl(expl(-at));
    near<T>(zs::flow_logistic_lp(z, loc, sc), -(at + sp) - logl(S), at + sp + fabsl(logl(S)), "logistic lp");
    near<T>(zs::flow_logistic_dz(z, loc, sc), -(tanhl(t / 2) / S), fabsl(tanhl(t / 2) / S), "logistic dz");
    expect(zs::flow_base_lp<T>(ZS_FLOW_NORMAL, z, loc, sc) == zs::flow_normal_lp(z, loc, sc) &&
               zs::flow_base_lp<T>(ZS_FLOW_LOGISTIC, z, loc, sc) == zs::flow_logistic_lp(z, loc, sc) &&
               zs::flow_base_dz<T>(ZS_FLOW_NORMAL, z, loc, sc) == zs::flow_normal_dz(z, loc, sc) &&
               zs::flow_base_dz<T>(ZS_FLOW_LOGISTIC, z, loc, sc) == zs::flow_logistic_dz(z, loc, sc),
           "base dispatch", 0, 0);
  }
}

// (2) the kernels' walks over exactly-sized heap arrays
static void check_index_maps() {
  const int64_t Bs[] = {1, 3, 65}, Ds[] = {2, 4, 6, 130};
  for (int64_t B : Bs) for (int64_t D : Ds) for (int sel = 0; sel < 2; ++sel) {
    const int64_t H = D / 2, n = B * H;
    std::vector<float> x(B * D), half(B * H), gx(B * D, -1.f), y(B * D, -1.f), shift(B * H), gs(B * H);
    for (int64_t i = 0; i < B * D; ++i) x[i] = (float)(i + 1);
    for (int64_t i = 0; i < B * H; ++i) shift[i] = 0.5f * (float)(i + 1);
    for (int64_t p = 0; p < n; ++p) {                       // k_split_pairs, k_split_pairs_bwd, k_merge_pairs, k_merge_pairs_bwd
      half[p] = x[zs::flow_pair_column(p, sel)];
      gx[zs::flow_pair_column(p, sel)] = half[p];
      gx[zs::flow_pair_column(p, 1 - sel)] = 0.f;
      const int64_t off = zs::flow_pair_column(p, sel), on = zs::flow_pair_column(p, 1 - sel);
      y[off] = x[off];
      y[on] = zs::flow_shift_add(x[on], shift[p], 1.f);
      gs[p] = x[on];
    }
    for (int64_t b = 0; b < B; ++b) for (int64_t j = 0; j < H; ++j) {
      const int64_t on = 1 - sel;
      expect(half[b * H + j] == x[b * D + 2 * j + sel], "split map", half[b * H + j], x[b * D + 2 * j + sel]);
      expect(gx[b * D + 2 * j + sel] == x[b * D + 2 * j + sel] && gx[b * D + 2 * j + on] == 0.f, "split_bwd map", 0, 0);
      expect(y[b * D + 2 * j + sel] == x[b * D + 2 * j + sel] && y[b * D + 2 * j + on] == x[b * D + 2 * j + on] + shift[b * H + j],
             "merge map", y[b * D + 2 * j + on], x[b * D + 2 * j + on] + shift[b * H + j]);
      expect(gs[b * H + j] == x[b * D + 2 * j + on], "merge_bwd map", gs[b * H + j], x[b * D + 2 * j + on]);
    }
  }
  const int64_t Dm[] = {1, 3, 4, 65};
  for (int64_t B : Bs) for (int64_t D : Dm) {
    std::vector<double> net(B * 2 * D), xs(B * D), u(B * D), gnet(B * 2 * D, -1.0);
    for (int64_t i = 0; i < B * 2 * D; ++i) net[i] = 1e-3 * (double)(i % 97) - 0.04;
    for (int64_t i = 0; i < B * D; ++i) xs[i] = 0.01 * (double)(i % 53);
    const int W[] = {1, 4};
    for (int w : W) {
      if (w == 4 && (D & 3)) continue;                      // the 4-element groups exist only when D % 4 == 0
      for (int64_t i = 0; i < B * D; i += w) {              // k_made_fwd / k_made_bwd: a group never straddles a row
        const int64_t b = i / D, d = i - b * D;
        for (int j = 0; j < w; ++j) {
          const int64_t im = zs::flow_made_m_at(b, d, D) + j, ia = zs::flow_made_loga_at(b, d, D) + j;
          u[i + j] = zs::flow_made_u(xs[i + j], net[im], net[ia]);
          gnet[im] = 1.0;
          gnet[ia] = 2.0;
        }
      }
      for (int64_t b = 0; b < B; ++b) for (int64_t d = 0; d < D; ++d) {
        expect(u[zs::flow_at(b, d, D)] == zs::flow_made_u(xs[b * D + d], net[b * 2 * D + d], net[b * 2 * D + D + d]), "made map", 0, 0);
        expect(gnet[b * 2 * D + d] == 1.0 && gnet[b * 2 * D + D + d] == 2.0, "made gradient map", 0, 0);
      }
    }
    for (int64_t col = 0; col < D; ++col)                   // k_made_inv_col
      for (int64_t b = 0; b < B; ++b) {
        const double v = zs::flow_made_inv(u[zs::flow_at(b, col, D)], net[zs::flow_made_m_at(b, col, D)], net[zs::flow_made_loga_at(b, col, D)]);
        expect(fabs(v - xs[b * D + col]) <= 1e-12 * (1.0 + fabs(xs[b * D + col])), "made inverse column", v, xs[b * D + col]);
      }
  }
}

int main() {
  check_coupling<float>();
  check_coupling<double>();
  check_scale_and_made<float>();
  check_scale_and_made<double>();
  check_tail<float>();
  check_tail<double>();
  check_index_maps();
  return finish("flow host math ok");
}
