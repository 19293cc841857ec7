/*
 * zs_gp.h -- C ABI of GPConditional (libzs_gp.so, gfx950): the predictive moments of a sparse Gaussian process at inputs x given
 * values fz at inducing inputs Z, for the ARD squared-exponential kernel, and their backward.  The cross-covariance K_xz [N, M]
 * is never stored: a wave forms its 16 rows of it in the accumulators of v_mfma_f32_16x16x4_f32 / v_mfma_f64_16x16x4_f64,
 * exponentiates them there and keeps them as a strip in LDS, the row operand of every product that follows.
 *
 * A fifteenth library next to libzs_hip.so and the other satellites, with the conventions of zs_lowrank.h: every pointer is a
 * DEVICE pointer owned by the caller, nothing is allocated, freed or synchronised inside a call, `stream` is a hipStream_t passed
 * as void* (NULL = the null stream), the return value is 0 on success, a positive hipError_t if a launch failed, ZS_EINVAL /
 * ZS_ENOTSUP (the codes of zs_hip.h) for rejected arguments, which write nothing.  T is the element type of the suffix (_f32:
 * float, _f64: double).  Every access is one element wide and there are no atomics: the results do not depend on the alignment
 * of the operands, and the same call gives the same bits.
 *
 * Shapes.  N inputs, M inducing inputs, d input dimensions, K particles; every operand is contiguous:
 *   x T[N, d];  inducing T[M, d];  lengthscale T[d] (> 0, not checked);  amplitude T[1] (> 0, not checked);
 *   kzz_tril T[M, M], the lower Cholesky factor L of k(Z, Z) + jitter I: only i >= j is read;
 *   fz T[K, M] or T[M] (Pf = K M or M elements; without the particle axis it is shared by the particles);
 *   mean T[K, N];  var T[N].
 *
 * The arithmetic, with k(p, q) = a^2 exp(-1/2 sum_j ((p_j - q_j) / l_j)^2) and x~ = x / l, z~ = Z / l, both centred per dimension
 * on the mean of z~ so that the expanded square -1/2 (|x~|^2 + |z~|^2) + x~ . z~ does not cancel:
 *   A = K_xz L^-T  [N, M];   c = L^-T L^-1 fz^T  [M, K];   mean = (K_xz c)^T;   var = a^2 - rowsum(A o A)
 *   G_A = -2 gvar A;   G_K = gmean^T c^T + G_A L^-1;   P = G_K o K_xz
 *   gx = (P z~ - rowsum(P) x~) / l;   gZ = (P^T x~ - colsum(P) z~) / l;   gl = -(sum x~ o gx~ + sum z~ o gz~) / l
 *   ga = 2 sum(P) / a + 2 a sum(gvar);   G_c = K_xz^T gmean^T;   h = L^-1 G_c;   gfz = (L^-T h)^T
 *   gL = tril(2 L^-T (A^T diag(gvar) A) - c h^T - gfz^T (L^-1 fz^T)^T)
 *
 * Calling order.  zs_gp_prepare writes the `prep` workspace of (kzz_tril, fz) -- (L^-1)^T, c and L^-1 fz^T, padded to whole
 * tiles -- which zs_gp_moments and zs_gp_moments_bwd read.  zs_gp_moments_bwd needs a `part` workspace and a number of row
 * shares; zs_gp_row_shares gives the count that fills the device, zs_gp_workspace_elems the sizes in elements of T.
 *
 * ZS_EINVAL: a NULL operand, required output or workspace, N < 0 (the backward: N < 1), M < 1, d < 1, K < 1, a Pf that is
 * neither K M nor M, shares outside [1, ceil(N / 64)].  ZS_ENOTSUP: M > zs_gp_max_inducing(sizeof(T)) (128 / 64),
 * d > zs_gp_max_input_dim() (64), K > 65536, more than 2^31 - 1 workgroups.  zs_gp_moments with N == 0 returns 0 and launches
 * nothing.  In the backward gmean, gvar and every output may be NULL.
 *
 * Kernel shape.  A workgroup is four waves; a wave owns 16 rows of x.
 *   prepare      one workgroup.  L in LDS; (L^-1)^T by forward substitution, a thread per column; w = L^-1 fz^T and c = L^-T w.
 *   moments      grid = 64-row blocks.  (L^-1)^T and the centred Z^T / l in LDS; the wave's x / l in registers; the score tiles
 *                x~ . z~ on the matrix cores, exponentiated in the accumulator, into the wave's [16, M] strip; A = K_xz L^-T
 *                over the blocks of the triangle only, squared and summed per lane; mean = K_xz c with K walked in tiles of 16,
 *                c read from prep.  Both moments are written with 16 lanes along n.
 *   moments_bwd  grid = shares; a share walks its 64-row blocks.  Per block the strip and A are recomputed; G_K is formed tile
 *                by tile and multiplied into the strip in place (P).  gx is final.  The sums over n -- K_xz^T gmean^T, P^T x~,
 *                A^T diag(gvar) A (tiles on and below the diagonal) -- contract over the block's 64 rows, their output tiles
 *                dealt to the waves, and are added into the share's partial by the same thread in block order.  (L^-1)^T is
 *                read from prep here: it does not fit in LDS next to two strips.
 *   finish       one workgroup: the shares in order, the closed forms of gZ, gl, ga, then the prepare's backward.
 */
#ifndef ZS_GP_H
#define ZS_GP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ZS_GP_ABI_VERSION 1

/* which workspace zs_gp_workspace_elems sizes */
#define ZS_GP_WS_PREP 0 /* prep: Mp (Mp + 2 Kp), Mp / Kp = M / K rounded up to 16 */
#define ZS_GP_WS_BWD 1  /* part of zs_gp_moments_bwd, n row shares */

/* ABI version of the loaded library (== ZS_GP_ABI_VERSION). */
int zs_gp_abi_version(void);
/* the most inducing inputs the kernels take for an element of `elem_bytes` bytes (4: 128, 8: 64; else 0), and the widest input (64) */
int zs_gp_max_inducing(int elem_bytes);
int zs_gp_max_input_dim(void);
/* the row shares zs_gp_moments_bwd should be called with (host arithmetic; 0 for N < 1) */
int64_t zs_gp_row_shares(int64_t N);
/* elements of T in workspace `which` (n: the shares, read for ZS_GP_WS_BWD only); -1 for rejected arguments */
int64_t zs_gp_workspace_elems(int which, int64_t M, int64_t d, int64_t K, int64_t n);

/* prep from (kzz_tril, fz): one launch of one workgroup */
int zs_gp_prepare_f32(const void* kzz_tril, const void* fz, int64_t Pf, void* prep, int64_t M, int64_t K, void* stream);
int zs_gp_prepare_f64(const void* kzz_tril, const void* fz, int64_t Pf, void* prep, int64_t M, int64_t K, void* stream);

/* mean T[K, N] and var T[N]: one launch */
int zs_gp_moments_f32(const void* x, const void* inducing, const void* lengthscale, const void* amplitude, const void* prep, void* mean,
                      void* var, int64_t N, int64_t M, int64_t d, int64_t K, void* stream);
int zs_gp_moments_f64(const void* x, const void* inducing, const void* lengthscale, const void* amplitude, const void* prep, void* mean,
                      void* var, int64_t N, int64_t M, int64_t d, int64_t K, void* stream);

/* gx T[N, d], ginducing T[M, d], glengthscale T[d], gamplitude T[1], gtril T[M, M] (zero above the diagonal), gfz (the shape of
 * fz) from gmean T[K, N] and gvar T[N]: two launches */
int zs_gp_moments_bwd_f32(const void* x, const void* inducing, const void* lengthscale, const void* amplitude, int64_t Pf,
                          const void* prep, const void* gmean, const void* gvar, void* part, void* gx, void* ginducing,
                          void* glengthscale, void* gamplitude, void* gtril, void* gfz, int64_t N, int64_t M, int64_t d, int64_t K,
                          int64_t shares, void* stream);
int zs_gp_moments_bwd_f64(const void* x, const void* inducing, const void* lengthscale, const void* amplitude, int64_t Pf,
                          const void* prep, const void* gmean, const void* gvar, void* part, void* gx, void* ginducing,
                          void* glengthscale, void* gamplitude, void* gtril, void* gfz, int64_t N, int64_t M, int64_t d, int64_t K,
                          int64_t shares, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ZS_GP_H */
