/*
 * zs_cat.h -- C ABI of the categorical families (libzs_cat.so, gfx950): Categorical / OnehotCategorical (Gumbel-max draw with
 * its log-mass, log-mass of a given value) and ExpConcrete / Concrete (relaxed draw in log space with its log-density, density
 * of a given value), each one launch forward and one launch backward.
 *
 * A fifth library next to libzs_hip.so, libzs_mcmc.so, libzs_flow.so and libzs_hmc.so, with the conventions of zs_hmc.h: every
 * pointer is a DEVICE pointer owned by the caller, nothing is allocated, freed or synchronised inside a call, `stream` is a
 * hipStream_t passed as void* (NULL = the null stream), the return value is 0 on success, a positive hipError_t if the launch
 * failed, ZS_EINVAL / ZS_ENOTSUP (the codes of zs_hip.h) for rejected arguments, which write nothing.  A call only enqueues one
 * kernel.  T is the element type of the suffix (_f32: float, _f64: double).
 *
 * Shapes.  R rows (the product of the batch shape), N categories (the last axis of `logits`), K particles:
 *   logits T[R, N] (not normalised);  lse_r = logsumexp_j logits[r, j];  per-particle operands are [K, R(, N)], particle-major.
 * ZS_EINVAL: NULL logits, N < 1, K < 0, R < 0, a temperature that is not > 0, a period that is neither the full size nor the
 * size without the particle axis, a call with nothing to read the value from or nothing to write.  ZS_ENOTSUP: N >= 2^31.
 * K R == 0 returns 0 and launches nothing.
 *
 * Kernel shape.  A row is cut into chunks of four consecutive categories; a group of G = min(64, next_pow2(ceil(N / 4)))
 * consecutive lanes owns a row, lane g the chunks g, g + G, ...  A wave therefore holds 64 / G rows, a row's reductions (a
 * running (max, sum-exp) pair, sums, the (value, index) pairs of the argmax) are butterflies inside that lane group and never
 * leave the wave; there is no LDS, no scratch and no atomic.  When N is a multiple of 4 and every pointer 16-byte aligned a
 * chunk is one 16-byte access per operand (two for _f64); every other layout reads and writes the same chunks element by
 * element, with the same results bit for bit.  Sums over the particles (the gradients w.r.t. logits) are made by the lane that
 * owns the element, particle after particle in ascending k: the same bits on every call.
 *
 * Limit of the backward entry points.  They give a lane group one ROW and walk its K particles in turn, so their parallelism is
 * R * G lanes whatever K is, and the backward of C3 and C4 reads glogits back once per particle.  With few rows and many
 * particles -- R = 1 with K in the thousands, e.g. one vector of logits against a batch of observed indices passed as K -- the
 * launch runs on one wave and its time grows linearly in K.  Such a caller should present the observations as rows (R = the
 * batch, K = 1, logits expanded), which is what the Python layer does for a value with leading axes; a cross-wave K-sum (LDS,
 * fixed-order combine) is not implemented.
 *
 * Noise contract, as in zs_hmc.h.  With `u` NULL, flat element i of [K, R, N] takes element i of what
 * zs_philox_uniform_f32(out, K R N, seed, call, rng_state) of zs_hip.h writes -- bit-identical, widened for _f64; with
 * rng_state (DEVICE pointer to two uint64 {seed, base}) non-NULL the kernel itself reads seed = rng_state[0] and uses
 * call + rng_state[1].  A non-NULL `u` (T[K, R, N], strictly inside (0, 1)) replaces the draw and changes nothing else.
 *
 * The temperature tau is a scalar argument and is NOT differentiable: no entry point returns a gradient w.r.t. it.
 */
#ifndef ZS_CAT_H
#define ZS_CAT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ZS_CAT_ABI_VERSION 1

/* ABI version of the loaded library (== ZS_CAT_ABI_VERSION). */
int zs_cat_abi_version(void);

/* lanes per row for N categories (host arithmetic; 0 for N < 1) */
int zs_cat_group_lanes(int64_t N);

/* out[i] = exp(x[i]) by the device function the kernels below use (exp_space's exp(y), the softmax weights), i in [0, n): what
 * a caller needs to reproduce exp(y) bit for bit.  ZS_EINVAL: n < 0 or a NULL pointer with n > 0. */
int zs_cat_exp_f32(const void* x, void* out, int64_t n, void* stream);
int zs_cat_exp_f64(const void* x, void* out, int64_t n, void* stream);

/* C1  Gumbel-max draw with its log-mass.
 *   v[k,r,j] = logits[r,j] - log(-log u[k,r,j]) ;  idx[k,r] = argmax_j v (ties: the lowest j) ;  lp[k,r] = logits[r,idx] - lse_r
 * idx int64[K, R], onehot T[K, R, N] (the indicator of idx), lp T[K, R]: any may be NULL (all NULL: ZS_EINVAL).  A category
 * with logits = -inf is never drawn unless the whole row is -inf (then category 0 with lp = NaN). */
int zs_cat_sample_logprob_f32(const void* logits, const void* u, int64_t* idx, void* onehot, void* lp, int64_t K, int64_t R,
                              int64_t N, uint64_t seed, uint64_t call, const uint64_t* rng_state, void* stream);
int zs_cat_sample_logprob_f64(const void* logits, const void* u, int64_t* idx, void* onehot, void* lp, int64_t K, int64_t R,
                              int64_t N, uint64_t seed, uint64_t call, const uint64_t* rng_state, void* stream);

/* C2  log-mass of a given value: exactly one of idx (index form) and x (weights form) is non-NULL.
 *   index form    lp[k,r] = logits[r, idx[k,r]] - lse_r ; an index outside [0, N) reads nothing and gives NaN (kernel guard)
 *   weights form  lp[k,r] = sum_j x[k,r,j] logits[r,j] - (sum_j x[k,r,j]) lse_r ; a term with x == 0 is exactly 0, also at
 *                 logits = -inf
 * Px: the period of the value in elements -- K R or R (index form), K R N or R N (weights form): a value without the particle
 * axis is shared by the particles. */
int zs_cat_logprob_f32(const void* logits, const int64_t* idx, const void* x, int64_t Px, void* lp, int64_t K, int64_t R,
                       int64_t N, void* stream);
int zs_cat_logprob_f64(const void* logits, const int64_t* idx, const void* x, int64_t Px, void* lp, int64_t K, int64_t R,
                       int64_t N, void* stream);

/* Backward of C2 with g = glp T[K, R]:
 *   glogits[r,j] = sum_k g[k,r] (x[k,r,j] - sx[k,r] softmax(logits)[r,j])        T[R, N], the k-sum in ascending k
 *   gx[k,r,j]    = g[k,r] (logits[r,j] - lse_r)                                 T[K, R, N], optional, weights form only
 * In the index form x is the indicator of idx and sx = 1; a particle whose index is outside [0, N) contributes nothing.
 * glogits may be NULL when gx is not. */
int zs_cat_logprob_bwd_f32(const void* logits, const int64_t* idx, const void* x, int64_t Px, const void* glp, void* glogits,
                           void* gx, int64_t K, int64_t R, int64_t N, void* stream);
int zs_cat_logprob_bwd_f64(const void* logits, const int64_t* idx, const void* x, int64_t Px, const void* glp, void* glogits,
                           void* gx, int64_t K, int64_t R, int64_t N, void* stream);

/* C3  relaxed draw in log space with its log-density (ExpConcrete; Maddison et al. 2017, eq. 26).
 *   a[k,r,j] = (logits[r,j] - log(-log u[k,r,j])) / tau ;  y = a - logsumexp_j a ;  t_j = logits[r,j] - tau y_j
 *   lp(y)    = lgamma(N) + (N - 1) log tau + sum_j t_j - N logsumexp_j t_j
 * y T[K, R, N] and lp T[K, R] may be NULL (not both, unless ey is given).  exp_space != 0 additionally writes ey = exp(y)
 * (T[K, R, N], may be NULL) and returns the Concrete density lp(y) - sum_j y_j instead. */
int zs_cat_expconcrete_sample_logprob_f32(const void* logits, const void* u, double tau, int exp_space, void* y, void* ey,
                                          void* lp, int64_t K, int64_t R, int64_t N, uint64_t seed, uint64_t call,
                                          const uint64_t* rng_state, void* stream);
int zs_cat_expconcrete_sample_logprob_f64(const void* logits, const void* u, double tau, int exp_space, void* y, void* ey,
                                          void* lp, int64_t K, int64_t R, int64_t N, uint64_t seed, uint64_t call,
                                          const uint64_t* rng_state, void* stream);

/* Backward of C3.  It reads the SAVED y of the forward call (nothing is drawn again): y T[K, R, N], and the incoming
 * gradients gy (w.r.t. y), gey (w.r.t. exp(y); exp_space only) -- T[K, R, N] -- and glp T[K, R]; any may be NULL, not all.
 *   glogits[r,j] = sum_k ( (G_kj - exp(y_kj) sum_i G_ki) / tau + glp_k q_kj ) ,  the k-sum in ascending k        T[R, N]
 *   G_kj = gy_kj + gey_kj exp(y_kj) + glp_k (-tau q_kj - e) ,  q_kj = 1 - N softmax(t_k)_j ,  e = 1 in exp space, else 0
 * i.e. the pathwise gradient through y plus the direct dependence of lp on logits (sum_i G_ki is formed with sum_i q_ki = 0). */
int zs_cat_expconcrete_sample_logprob_bwd_f32(const void* logits, const void* y, double tau, int exp_space, const void* gy,
                                              const void* gey, const void* glp, void* glogits, int64_t K, int64_t R, int64_t N,
                                              void* stream);
int zs_cat_expconcrete_sample_logprob_bwd_f64(const void* logits, const void* y, double tau, int exp_space, const void* gy,
                                              const void* gey, const void* glp, void* glogits, int64_t K, int64_t R, int64_t N,
                                              void* stream);

/* C4  the same density at a given y (T[K, R, N] or T[R, N]: Py = K R N or R N); exp_space != 0: lp(y) - sum_j y_j. */
int zs_cat_expconcrete_logprob_f32(const void* logits, const void* y, int64_t Py, double tau, int exp_space, void* lp, int64_t K,
                                   int64_t R, int64_t N, void* stream);
int zs_cat_expconcrete_logprob_f64(const void* logits, const void* y, int64_t Py, double tau, int exp_space, void* lp, int64_t K,
                                   int64_t R, int64_t N, void* stream);

/* Backward of C4 with g = glp T[K, R] (either output may be NULL, not both):
 *   gy[k,r,j]    = g[k,r] (-tau q_kj - e)            T[K, R, N]
 *   glogits[r,j] = sum_k g[k,r] q_kj                  T[R, N], the k-sum in ascending k */
int zs_cat_expconcrete_logprob_bwd_f32(const void* logits, const void* y, int64_t Py, double tau, int exp_space, const void* glp,
                                       void* gy, void* glogits, int64_t K, int64_t R, int64_t N, void* stream);
int zs_cat_expconcrete_logprob_bwd_f64(const void* logits, const void* y, int64_t Py, double tau, int exp_space, const void* glp,
                                       void* gy, void* glogits, int64_t K, int64_t R, int64_t N, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ZS_CAT_H */
