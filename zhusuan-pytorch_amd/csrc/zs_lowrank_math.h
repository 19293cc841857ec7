// The arithmetic of MultivariateNormalLowRank (include/zs_lowrank.h) that is not scheduling: the panel and its paddings, the
// sizes and the layout of the workspaces, the split of the prepare and of the backward grids, and the per-element expressions
// of the epilogues and the finishes; the tile of the two matrix instructions and its row map are zs_tile_math.h's (MfmaTile,
// Mfma).  __host__ __device__ like the other *_math.h headers; zs_lowrank.hip only stages, multiplies and reduces.
#pragma once
#include "zs_common.h"
#include "zs_flat_math.h"
#include "zs_group_math.h"
#include "zs_tile_math.h"

#define ZS_LOWRANK_MAX_DIM 65536
#define ZS_LOWRANK_MAX_RANK 64
#define ZS_LOWRANK_GRID_TARGET 512          // workgroups wanted when the rows alone do not fill the device (two per CU)
#define ZS_LOWRANK_LOG_2PI 1.8378770664093454835606594728112

namespace zs {

// The staged panel of the factor: PANEL rows of the D axis by up to 64 rank columns, row-major with a row of LD = 81 elements.
// The kernels read it BOTH ways -- a k-row across 16 columns (u = y Wd, the capacitance) and a column across 16 d-rows (a = ...
// - v W^T, the draw) -- and 81 = 64 + 17 serves both: float, direct: the four k-rows of a matrix step start 17 banks apart (61 of
// the 64 banks, three serve two lanes: MfmaPanel's figure); float, transposed: the 16 d-rows start at 17 m mod 64 = {0, 17, 34,
// 51, 4, 21, ...}, each followed by its q = 0..3, 64 distinct words but for the last row's wrap onto banks 0..2; double, direct:
// words 0, 34, 4, 38 (mod 64) as MfmaPanel's double panel.  The particle operands (y, u, v, the rank noise) are [16][LDY = 68]:
// read as A operands at m LDY + 4 s + q, 68 = 64 + 4 puts lane (q, m) of float in bank 4 m + q: all 64 banks once.
constexpr int LR_PANEL = 64, LR_LD = 81, LR_LDY = 68;
constexpr int LR_WS = LR_PANEL * LR_LD, LR_YS = 16 * LR_LDY, LR_MISC = 160;
// dynamic LDS of the density and draw kernels, in elements: the panel (reused for the four waves' partial u: 4 * 16 * 68 <= 64 * 81),
// 1 / d of the panel, y of the particle tile, u (then v, or the rank noise), and the small sums
constexpr int LR_LDS_ELEMS = LR_WS + LR_PANEL + 2 * LR_YS + LR_MISC;
constexpr int LR_CLD = 65;          // row of the capacitance matrix in LDS (the finishes)

ZS_HD int lr_rp(int64_t r) { return (int)(blocks16(r) * 16); }          // the rank rounded up to whole tiles
ZS_HD int64_t lr_panels(int64_t D) { return (D + LR_PANEL - 1) / LR_PANEL; }
ZS_HD int64_t lr_clamp(int64_t v, int64_t hi) { return v < 1 ? 1 : (v > hi ? hi : v); }
// D-splits of the prepare: enough workgroups for R rows to fill the device, at most the panels
ZS_HD int64_t lr_splits(int64_t R, int64_t D) {
  if (R < 1 || D < 1) return 0;
  return lr_clamp((ZS_LOWRANK_GRID_TARGET + R - 1) / R, lr_panels(D));
}
// particle shares of the density's backward: likewise, at most the 16-particle tiles
ZS_HD int64_t lr_shares(int64_t K, int64_t R) {
  if (R < 1 || K < 1) return 0;
  return lr_clamp((ZS_LOWRANK_GRID_TARGET + R - 1) / R, blocks16(K));
}

// the prep workspace, per row: Mt[rp, rp] = (L^-1)^T of C = L L^T (zero below the diagonal and past r), Cinv[rp, rp], log|C|, sum log d
ZS_HD int64_t lr_prep_row(int64_t r) { return 2 * (int64_t)lr_rp(r) * lr_rp(r) + 2; }
// the partials of the prepare, per row and split: C[rp, rp], sum log d
ZS_HD int64_t lr_cap_part(int64_t r) { return (int64_t)lr_rp(r) * lr_rp(r) + 1; }
// the partials of the density's backward, per row and share: gW[D, r], gmean[D], sum g a^2 [D]
ZS_HD int64_t lr_bwd_part(int64_t D, int64_t r) { return D * (r + 2); }

ZS_HD float lr_log(float x) { return logf(x); }
ZS_HD double lr_log(double x) { return log(x); }
ZS_HD float lr_sqrt(float x) { return sqrtf(x); }
ZS_HD double lr_sqrt(double x) { return sqrt(x); }

// lp from q = sum y^2 / d, quad = u C^-1 u^T, the two log-determinants and c0 = -D/2 log 2 pi
template <typename T>
ZS_HD T lr_lp(T q, T quad, T sumlogd, T logdet, T c0) { return ((T)-0.5 * (q - quad) - (T)0.5 * (sumlogd + logdet)) + c0; }
// an element of a = Sigma^-1 y from y, (v W^T) and 1 / d
template <typename T>
ZS_HD T lr_a(T y, T vw, T rd) { return (y - vw) * rd; }
// the closed forms of the backward's finish: e = (Wd C^-1)_dj, h = rowsum((Wd C^-1) o Wd)_d
template <typename T>
ZS_HD T lr_gfactor(T part, T sumg, T e) { return part - sumg * e; }
template <typename T>
ZS_HD T lr_gdiag(T ga2, T sumg, T rd, T h) { return (T)0.5 * (ga2 - sumg * (rd - h)); }
// the draw and the diagonal's gradient of its backward
template <typename T>
ZS_HD T lr_draw(T mean, T d, T eps_d, T ew) { return mean + (lr_sqrt(d) * eps_d + ew); }
template <typename T>
ZS_HD T lr_draw_gdiag(T ge, T d) { return ge / ((T)2 * lr_sqrt(d)); }

}  // namespace zs
