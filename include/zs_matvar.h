/*
 * zs_matvar.h -- C ABI of MatrixVariateNormalCholesky (libzs_matvar.so, gfx950): a normal over n x p matrices with mean `mean`,
 * row covariance U U^T and column covariance V V^T, U and V lower triangular.  The draw Z = mean + U E V^T with its log-density,
 * the log-density of a given value, and their backwards, on the matrix cores (v_mfma_f32_16x16x4_f32 / v_mfma_f64_16x16x4_f64).
 *
 * An eleventh library next to libzs_hip.so and the other satellites, with the conventions of zs_topic.h: every pointer is a
 * DEVICE pointer owned by the caller, nothing is allocated, freed or synchronised inside a call, `stream` is a hipStream_t passed
 * as void* (NULL = the null stream), the return value is 0 on success, a positive hipError_t if a launch failed, ZS_EINVAL /
 * ZS_ENOTSUP (the codes of zs_hip.h) for rejected arguments, which write nothing.  T is the element type of the suffix (_f32:
 * float, _f64: double).  Every access is one element wide and there are no floating-point atomics: the results do not depend on
 * the alignment of the operands, and the same call gives the same bits.
 *
 * Shapes.  R rows (the product of the batch shape), K particles, an n x p event; every operand is contiguous and row-major:
 *   mean T[R, n, p];  u_tril T[R, n, n];  v_tril T[R, p, p];  per-particle tensors T[K, R, n, p];  lp T[K, R].
 * ONLY THE LOWER TRIANGLES OF u_tril AND v_tril ARE EVER READ; THE UPPER TRIANGLES OF gu AND gv ARE WRITTEN AS ZEROS.  A zero or
 * negative diagonal gives -inf / NaN through log, with no check and no trap.
 *
 *   c(U, V) = -(n p / 2) log 2 pi - p sum_i log U_ii - n sum_j log V_jj
 *   M1 draw    Z = mean + U E V^T ;  lp = c - 1/2 |E|_F^2                                    (no solve)
 *   M2 value   A = U^-1 (X - mean) V^-T ;  lp = c - 1/2 |A|_F^2
 *   M1 bwd     gmean = sum_k gZ ;  gU = tril(sum_k gZ V E^T) - p (sum_k glp) diag(1 / U_ii) ;
 *              gV = tril(sum_k gZ^T U E) - n (sum_k glp) diag(1 / V_jj)
 *   M2 bwd     B = U^-T A ;  C = A V^-1 ;  S = B V^-1 ;  gX = -glp S ;  gmean = sum_k glp S ;
 *              gU = tril(sum_k glp B A^T) - p (sum_k glp) diag(1 / U_ii) ;  gV = tril(sum_k glp C^T A) - n (sum_k glp) diag(1 / V_jj)
 * A detached draw differentiates its density through M2's backward at the fixed Z; it has no mode of its own.
 *
 * ZS_EINVAL: a NULL mean / u_tril / v_tril, n < 1, p < 1, K < 0, R < 0, a period that is neither the full size nor the size
 * without the particle axis, a call with nothing to read the value or the cotangent from, nothing to write, or a k-sum asked for
 * without the `part` workspace.  ZS_ENOTSUP: n or p above zs_matvar_max_dim (each on its own), K R >= 2^31,
 * R (n p + n n + p p) above 2^31 workgroups of 256 threads.  K R == 0 returns 0
 * and launches nothing.
 *
 * Kernel shape.  A workgroup of four waves holds an event in LDS as a tile of 16 x 16 blocks (ragged edges zero filled) and does
 * every product and every substitution step on the matrix cores; the factors' blocks are read from memory as operands, blocks
 * above the diagonal never.  The forward entry points run a workgroup per (k, r), one launch.  M2 is blocked substitution: the
 * inverses of the 16 x 16 diagonal blocks are formed at the head of the workgroup (scalar substitution, a column per thread), then
 * Y_i = inv(U_ii) (D_i - sum_{j<i} U_ij Y_j) block row by block row, and the solve from the right is the same routine on the
 * other axis of the tile.  The backward entry points cut a row's particles into zs_matvar_shares(K, R) contiguous shares; a
 * workgroup walks one share in ascending k and adds each particle's tiles to its partial in `part` (one owner per element); a
 * second launch adds the shares in share order, adds the diagonal terms and writes the zeros above the diagonals.  LDS: a
 * 128 x 128 float32 event takes 159 760 of the 163 840 bytes of a gfx950 workgroup (zs_matvar_math.h has the arithmetic).
 *
 * Noise contract, that of zs_mvn.h.  With `eps` NULL, flat element i of [K, R, n, p] takes element i of what
 * zs_philox_normal_f32(out, K R n p, seed, call, rng_state) of zs_hip.h writes -- bit-identical, widened for _f64; with rng_state
 * (DEVICE pointer to two uint64 {seed, base}) non-NULL the kernel itself reads seed = rng_state[0] and uses call + rng_state[1].
 * A non-NULL `eps` (T[K, R, n, p]) replaces the draw and changes nothing else.
 */
#ifndef ZS_MATVAR_H
#define ZS_MATVAR_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ZS_MATVAR_ABI_VERSION 1

/* which workspace zs_matvar_workspace_elems sizes: the `part` of the two backwards, both
 * zs_matvar_shares(K, R) R (n p + n n + p p) elements */
#define ZS_MATVAR_WS_SAMPLE_BWD 0
#define ZS_MATVAR_WS_LOGPROB_BWD 1

/* ABI version of the loaded library (== ZS_MATVAR_ABI_VERSION). */
int zs_matvar_abi_version(void);
/* the largest n and the largest p the kernels take for elements of elem_bytes: 128 for 4, 64 for 8, 0 for another size */
int zs_matvar_max_dim(int elem_bytes);
/* the shares the backwards cut a row's K particles into (host arithmetic; 0 for K < 1 or R < 1): at most 16, and enough for 256
 * workgroups when the rows are few */
int64_t zs_matvar_shares(int64_t K, int64_t R);
/* elements of T in workspace `which` (host arithmetic); -1 for rejected arguments */
int64_t zs_matvar_workspace_elems(int which, int elem_bytes, int64_t K, int64_t R, int64_t n, int64_t p);

/* M1  the draw with its log-density, one launch.  z T[K, R, n, p] and lp T[K, R] may be NULL, not both. */
int zs_matvar_sample_logprob_f32(const void* mean, const void* u_tril, const void* v_tril, const void* eps, void* z, void* lp,
                                 int64_t K, int64_t R, int64_t n, int64_t p, uint64_t seed, uint64_t call,
                                 const uint64_t* rng_state, void* stream);
int zs_matvar_sample_logprob_f64(const void* mean, const void* u_tril, const void* v_tril, const void* eps, void* z, void* lp,
                                 int64_t K, int64_t R, int64_t n, int64_t p, uint64_t seed, uint64_t call,
                                 const uint64_t* rng_state, void* stream);

/* Backward of M1 (reparameterised) from gz T[K, R, n, p] and glp T[K, R] (either may be NULL, not both), eps injected or
 * regenerated from the same (seed, call, rng_state).  gmean T[R, n, p], gu T[R, n, n], gv T[R, p, p] may be NULL, not all.
 * Two launches (the finish alone when gz is NULL, and then `part` may be NULL). */
int zs_matvar_sample_logprob_bwd_f32(const void* u_tril, const void* v_tril, const void* eps, const void* gz, const void* glp,
                                     void* part, void* gmean, void* gu, void* gv, int64_t K, int64_t R, int64_t n, int64_t p,
                                     uint64_t seed, uint64_t call, const uint64_t* rng_state, void* stream);
int zs_matvar_sample_logprob_bwd_f64(const void* u_tril, const void* v_tril, const void* eps, const void* gz, const void* glp,
                                     void* part, void* gmean, void* gu, void* gv, int64_t K, int64_t R, int64_t n, int64_t p,
                                     uint64_t seed, uint64_t call, const uint64_t* rng_state, void* stream);

/* M2  the log-density of a given x (T[K, R, n, p] or T[R, n, p]: Px = K R n p or R n p elements; a value without the particle axis
 * is shared by the particles), one launch. */
int zs_matvar_logprob_f32(const void* mean, const void* u_tril, const void* v_tril, const void* x, int64_t Px, void* lp, int64_t K,
                          int64_t R, int64_t n, int64_t p, void* stream);
int zs_matvar_logprob_f64(const void* mean, const void* u_tril, const void* v_tril, const void* x, int64_t Px, void* lp, int64_t K,
                          int64_t R, int64_t n, int64_t p, void* stream);

/* Backward of M2 with glp T[K, R].  gx is T[K, R, n, p] whatever Px is.  Any output may be NULL, not all; `part` may be NULL when
 * only gx is asked for (one launch; two otherwise). */
int zs_matvar_logprob_bwd_f32(const void* mean, const void* u_tril, const void* v_tril, const void* x, int64_t Px, const void* glp,
                              void* part, void* gx, void* gmean, void* gu, void* gv, int64_t K, int64_t R, int64_t n, int64_t p,
                              void* stream);
int zs_matvar_logprob_bwd_f64(const void* mean, const void* u_tril, const void* v_tril, const void* x, int64_t Px, const void* glp,
                              void* part, void* gx, void* gmean, void* gu, void* gv, int64_t K, int64_t R, int64_t n, int64_t p,
                              void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ZS_MATVAR_H */
