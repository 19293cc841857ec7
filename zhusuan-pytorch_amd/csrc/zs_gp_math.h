// The arithmetic of GPConditional (include/zs_gp.h) that is not scheduling: the caps, the paddings of the operands in LDS, the
// LDS budgets, the layout of the prepare's workspace and of the backward's partials, the row shares, and the per-element
// expressions; the tile of the two matrix instructions and its row map are zs_tile_math.h's.  __host__ __device__ like the other
// *_math.h headers; zs_gp.hip only stages, multiplies and reduces.
#pragma once
#include "zs_common.h"
#include "zs_flat_math.h"
#include "zs_group_math.h"
#include "zs_tile_math.h"

#define ZS_GP_MAX_INDUCING_F32 128
#define ZS_GP_MAX_INDUCING_F64 64
#define ZS_GP_MAX_INPUT_DIM 64
#define ZS_GP_MAX_PARTICLES 65536          // Mp Kp stays an int
#define ZS_GP_MAX_SHARES 128          // backward: at most this many partials, whatever N is (a partial is up to 132 KB)
#define ZS_GP_LDS_BYTES (160 * 1024)

namespace zs {

constexpr int GP_THREADS = 256, GP_ROWS = 64;          // four waves, 16 rows of x each

ZS_HD int gp_max_inducing(int elem_bytes) { return elem_bytes == 4 ? ZS_GP_MAX_INDUCING_F32 : (elem_bytes == 8 ? ZS_GP_MAX_INDUCING_F64 : 0); }
ZS_HD int gp_p16(int64_t n) { return (int)(16 * blocks16(n)); }
ZS_HD int64_t gp_row_blocks(int64_t N) { return (N + GP_ROWS - 1) / GP_ROWS; }
// Operands read down a column -- B[k = 4 s + q][16 t + m]: L^-T, Z^T / l -- have rows of (columns) + 17 elements, MfmaPanel's
// padding: the four k-rows of a matrix step start 17 banks apart.  Operands read along a row -- A[m][4 s + q]: the strips of
// K_xz, A and P, the rows of x / l -- have rows of (columns) + 4: lane (q, m) of float falls in bank 4 m + q, all 64 once
// (zs_lowrank_math.h's LDY).
ZS_HD int gp_ldb(int cols) { return cols + 17; }
ZS_HD int gp_lda(int cols) { return cols + 4; }

// LDS of the forward, in elements: L^-T [Mp][ldb], Z^T / l [d16][ldb], the strips [64][lda], centre [64], |z|^2 [Mp]
//   float32, M = 128, d = 64: (128 + 64) * 145 + 64 * 132 + 64 + 128 = 36 480 elements, 145 920 bytes <= 163 840
//   float64, M =  64, d = 64: (64 + 64) * 81 + 64 * 68 + 64 + 64 = 14 848 elements, 118 784 bytes
ZS_HD int64_t gp_fwd_lds_elems(int Mp, int d16) { return (int64_t)(Mp + d16) * gp_ldb(Mp) + GP_ROWS * gp_lda(Mp) + 64 + Mp; }
// LDS of the backward: Z^T / l, the strips of K_xz (then P) and of A, x / l [64][lda(d16)], centre, |z|^2, rowsum(P), gvar [64].
// L^-1 does not fit next to two strips: the backward reads it from the workspace (64 KB, resident in the L2).
//   float32, M = 128, d = 64: 64 * 145 + 2 * 64 * 132 + 64 * 68 + 64 + 128 + 128 = 30 848 elements, 123 392 bytes
//   float64, M =  64, d = 64: 64 * 81 + 2 * 64 * 68 + 64 * 68 + 64 + 64 + 128 = 18 496 elements, 147 968 bytes
ZS_HD int64_t gp_bwd_lds_elems(int Mp, int d16) {
  return (int64_t)d16 * gp_ldb(Mp) + 2 * GP_ROWS * gp_lda(Mp) + GP_ROWS * gp_lda(d16) + 64 + Mp + 2 * GP_ROWS;
}
// LDS of the prepare: L and (L^-1)^T, [Mp][Mp + 1] each (a thread per column: rows Mp + 1 apart are in different banks)
ZS_HD int64_t gp_prep_lds_elems(int Mp) { return 2 * (int64_t)Mp * (Mp + 1); }

// the prepare's workspace: (L^-1)^T [Mp, Mp] (zero below the diagonal and past M), c = L^-T L^-1 fz^T [Mp, Kp], w = L^-1 fz^T [Mp, Kp]
ZS_HD int64_t gp_prep_elems(int64_t M, int64_t K) { return (int64_t)gp_p16(M) * (gp_p16(M) + 2 * (int64_t)gp_p16(K)); }
// a share's partial: K_xz^T gmean^T [Mp, Kp] | P^T x~ [Mp, d16] | A^T diag(gvar) A [Mp, Mp] | colsum P [Mp] | sum x~ gx~ [d16] | sum P, sum gvar
struct GpPart {
  int64_t B, PtX, Q, colP, lsum, sums, stride;
};
ZS_HD GpPart gp_part(int64_t M, int64_t d, int64_t K) {
  const int64_t Mp = gp_p16(M), d16 = gp_p16(d), Kp = gp_p16(K);
  GpPart p;
  p.B = 0;
  p.PtX = p.B + Mp * Kp;
  p.Q = p.PtX + Mp * d16;
  p.colP = p.Q + Mp * Mp;
  p.lsum = p.colP + Mp;
  p.sums = p.lsum + d16;
  p.stride = p.sums + 2;
  return p;
}
// the backward's workspace: the shares' partials, then the finish's own: one summed partial, h = L^-1 G_c and e = L^-T h [Mp, Kp] each
ZS_HD int64_t gp_bwd_elems(int64_t M, int64_t d, int64_t K, int64_t shares) {
  return (shares + 1) * gp_part(M, d, K).stride + 2 * (int64_t)gp_p16(M) * gp_p16(K);
}
// row shares of the backward: one per 64-row block, at most ZS_GP_MAX_SHARES
ZS_HD int64_t gp_shares(int64_t N) {
  if (N < 1) return 0;
  const int64_t b = gp_row_blocks(N);
  return b < ZS_GP_MAX_SHARES ? b : ZS_GP_MAX_SHARES;
}

ZS_HD float gp_exp(float x) { return expf(x); }
ZS_HD double gp_exp(double x) { return exp(x); }

// k(x, z) from the centred product x~ . z~ and the two squared norms
template <typename T>
ZS_HD T gp_kernel(T dot, T xn, T zn, T amp2) { return amp2 * gp_exp(dot - (T)0.5 * (xn + zn)); }
template <typename T>
ZS_HD T gp_var(T amp2, T sq) { return amp2 - sq; }
// the gradients of the scaled operands: gx~ = P z~ - rowsum(P) x~,  gz~ = P^T x~ - colsum(P) z~
template <typename T>
ZS_HD T gp_gscaled(T prod, T sum, T own) { return prod - sum * own; }
// gl_j = -(sum_n x~ gx~ + sum_m z~ gz~) / l_j (the square's gradient for the lengthscale, by Euler's identity)
template <typename T>
ZS_HD T gp_glength(T sx, T sz, T l) { return -(sx + sz) / l; }
// ga = 2 sum(P) / a + 2 a sum(gvar)
template <typename T>
ZS_HD T gp_gamp(T sumP, T sumgv, T a) { return (T)2 * sumP / a + (T)2 * a * sumgv; }

}  // namespace zs
