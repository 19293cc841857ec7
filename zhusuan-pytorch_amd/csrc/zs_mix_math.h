// The arithmetic of the mixture-of-Gaussians density (include/zs_mix.h) that is not scheduling: the interleaved operand, the
// sizes and the layout of the workspaces, the split of the grad_params grid, and the per-element expressions of the prologue,
// the epilogues and the finish; the tile of the two matrix instructions, its row map and the staged panel are zs_tile_math.h's
// (MfmaTile, MfmaPanel, panel_tile).  __host__ __device__ like the other *_math.h headers; zs_mix.hip only stages, multiplies
// and reduces.
#pragma once
#include "zs_common.h"
#include "zs_flat_math.h"
#include "zs_group_math.h"
#include "zs_tile_math.h"

#define ZS_MIX_MAX_DIM 64
#define ZS_MIX_MAX_COMPONENTS 65536
#define ZS_MIX_MAX_STEPS (2 * ZS_MIX_MAX_DIM / 4)          // matrix instructions per 16 x 16 score tile: the k axis in fours
#define ZS_MIX_MAX_NTILES (2 * ZS_MIX_MAX_DIM / 16)        // 16-row tiles of the second products' output
#define ZS_MIX_ROWS_PER_BLOCK 64                           // logprob, grad_x: four waves of 16 rows
#define ZS_MIX_GRID_TARGET 512                             // grad_params: workgroups wanted at small C (two per CU)
#define ZS_MIX_LOG_2PI 1.8378770664093454835606594728112

namespace zs {

// The k axis of the packed operand interleaves the two halves of [y | y^2] -- k = 2 d and 2 d + 1 --, so that the two output
// rows a gradient element needs are the neighbours of zs_tile_math.h's row map: in one lane (f32) or in the lanes q and q ^ 1
// (f64).
ZS_HD int mix_k16(int64_t D) { return (int)(blocks16(2 * D) * 16); }          // rows of the staged panel
ZS_HD int mix_steps(int64_t D) { return (int)((2 * D + 3) / 4); }
ZS_HD int64_t mix_cpad(int elem_bytes, int64_t C) { return panels(elem_bytes, C) * panel_cols(elem_bytes); }
ZS_HD int64_t mix_row_shares(int elem_bytes, int64_t R, int64_t C) {
  const int64_t panels = zs::panels(elem_bytes, C);
  if (panels == 0 || R < 1) return 0;
  const int64_t s = (ZS_MIX_GRID_TARGET + panels - 1) / panels, tiles = blocks16(R);
  return s > tiles ? tiles : s;
}

// the prep workspace: cen[D], lse[1], lsm[Cpad], b[Cpad], W[K16, Cpad]
template <typename T>
struct MixPrep {
  T *cen, *lse, *lsm, *b, *w;
  int64_t cpad;
};
template <typename T>
ZS_HD MixPrep<T> mix_prep(T* p, int64_t C, int64_t D) {
  MixPrep<T> w;
  w.cpad = mix_cpad((int)sizeof(T), C);
  w.cen = p;
  w.lse = w.cen + D;
  w.lsm = w.lse + 1;
  w.b = w.lsm + w.cpad;
  w.w = w.b + w.cpad;
  return w;
}
ZS_HD int64_t mix_prep_elems(int elem_bytes, int64_t C, int64_t D) { return D + 1 + (2 + mix_k16(D)) * mix_cpad(elem_bytes, C); }
// the partials of grad_params: [shares][K16 + 1][Cpad], then the shares' sums of g
ZS_HD int64_t mix_part_elems(int elem_bytes, int64_t C, int64_t D, int64_t shares) {
  return shares * ((mix_k16(D) + 1) * mix_cpad(elem_bytes, C) + 1);
}

// float: the 1-ulp instruction where an expression runs per element of the [R, C] scores (the exponential of the epilogues),
// libm-grade everywhere else (the prologue and the finish run once per element of the parameters, the logarithm once per row)
ZS_HD float mix_exp(float x) { return expf(x); }
ZS_HD double mix_exp(double x) { return exp(x); }
ZS_HD float mix_log(float x) { return logf(x); }
ZS_HD double mix_log(double x) { return log(x); }
ZS_HD float mix_exp_acc(float x) { return exp_fast(x); }
ZS_HD double mix_exp_acc(double x) { return exp(x); }

// element k of the row operand [y_0, y_0^2, y_1, y_1^2, ...] given y of dimension k / 2
template <typename T>
ZS_HD T mix_row_elem(T y, int k) { return (k & 1) ? y * y : y; }

// Fold four scores (tm their maximum) into a running maximum mx and the sum sm of exp(score - mx).  A score of -inf (a padded
// component) adds exactly 0; while everything seen is -inf nothing changes.
template <typename T>
ZS_HD void mix_fold(T& mx, T& sm, const T (&s)[4], T tm) {
  const T nm = max_of(mx, tm);
  if (nm > -(T)INFINITY) {
    sm = sm * mix_exp_acc(mx - nm);
#pragma unroll
    for (int v = 0; v < 4; ++v) sm += mix_exp_acc(s[v] - nm);
    mx = nm;
  }
}
// the share of a lane in the sum of its row once the row's maximum M is known
template <typename T>
ZS_HD T mix_rescale(T mx, T sm, T M) { return mx > -(T)INFINITY ? sm * mix_exp_acc(mx - M) : (T)0; }

// G = g exp(s - lp); exactly 0 for a row past the end (its lp is not a number of this problem)
template <typename T>
ZS_HD T mix_weight(bool live, T g, T s, T lp) { return live ? g * mix_exp_acc(s - lp) : (T)0; }

// the closed forms of the finish: w = exp(-2 logstd), nu = mean - centre
template <typename T>
ZS_HD T mix_dmean(T w, T nu, T gy, T n) { return w * (gy - nu * n); }
template <typename T>
ZS_HD T mix_dlogstd(T w, T nu, T gy, T gy2, T n) { return w * (gy2 - (T)2 * nu * gy + nu * nu * n) - n; }
template <typename T>
ZS_HD T mix_dlogits(T n, T lsm, T sumg) { return n - mix_exp(lsm) * sumg; }

}  // namespace zs
