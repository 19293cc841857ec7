/*
 * zs_mvn.h -- C ABI of MultivariateNormalCholesky (libzs_mvn.so, gfx950): the draw z = mean + L eps with its log-density, the
 * log-density of a given value, and their backwards, each one launch.
 *
 * A sixth library next to libzs_hip.so, libzs_mcmc.so, libzs_flow.so, libzs_hmc.so and libzs_cat.so, with the conventions of
 * zs_cat.h: every pointer is a DEVICE pointer owned by the caller, nothing is allocated, freed or synchronised inside a call,
 * `stream` is a hipStream_t passed as void* (NULL = the null stream), the return value is 0 on success, a positive hipError_t if
 * the launch failed, ZS_EINVAL / ZS_ENOTSUP (the codes of zs_hip.h) for rejected arguments, which write nothing.  A call only
 * enqueues one kernel.  T is the element type of the suffix (_f32: float, _f64: double).
 *
 * Shapes.  R rows (the product of the batch shape), D dimensions, K particles; every operand is contiguous:
 *   mean T[R, D];  tril T[R, D, D], row-major, tril[r, i, j] = L_ij;  per-particle tensors T[K, R, D];  lp T[K, R].
 * ONLY i >= j OF tril IS EVER READ: the upper triangle may hold anything (upstream's dense matmul would read it).  THE UPPER
 * TRIANGLE OF gtril IS WRITTEN AS ZEROS.  A zero or negative diagonal gives -inf / NaN in lp through log, with no check and no
 * trap.
 * ZS_EINVAL: a NULL mean / tril, D < 1, K < 0, R < 0, a period that is neither the full size nor the size without the particle
 * axis, a call with nothing to read the value or the cotangent from, or nothing to write.  ZS_ENOTSUP: D > zs_mvn_max_dim().
 * K R == 0 returns 0 and launches nothing.
 *
 * Kernel shape.  A group of G = next_pow2(D) consecutive lanes of one wave owns a row, lane i its component i, so a wave (= a
 * workgroup) holds 64 / G rows.  The lower triangle of L of those rows is copied once into LDS and reused by all the particles
 * the workgroup walks; vectors live one element per lane and are exchanged by shuffles inside the group (the matvec and the
 * column-oriented substitutions broadcast one component per step, row sums are butterflies).  1 / L_ii is formed once per row and
 * a solved component is b_j * (1 / L_jj).  No atomics, no scratch.  Every access is one element wide: the results do not depend
 * on the alignment of the operands, and the same call gives the same bits.
 *
 * Limit of the backward entry points.  They give a lane group one ROW and walk its K particles in ascending k (the k-sums of
 * gmean and gtril are made by the lane that owns the element), so their parallelism is R * G lanes whatever K is: with few rows
 * and many particles the launch runs on a few waves and its time grows linearly in K.  A cross-wave K-sum is not implemented.
 * The forward entry points have no k-sum and cut the particles into contiguous shares over workgroups.
 *
 * Noise contract, as in zs_cat.h.  With `eps` NULL, flat element (k R + r) D + i of [K, R, D] takes element (k R + r) D + i of
 * what zs_philox_normal_f32(out, K R D, seed, call, rng_state) of zs_hip.h writes -- bit-identical, widened for _f64; with
 * rng_state (DEVICE pointer to two uint64 {seed, base}) non-NULL the kernel itself reads seed = rng_state[0] and uses
 * call + rng_state[1].  A non-NULL `eps` (T[K, R, D]) replaces the draw and changes nothing else.
 */
#ifndef ZS_MVN_H
#define ZS_MVN_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ZS_MVN_ABI_VERSION 1

/* ABI version of the loaded library (== ZS_MVN_ABI_VERSION). */
int zs_mvn_abi_version(void);
/* the widest row the fused kernels take (64) */
int zs_mvn_max_dim(void);
/* lanes per row for D dimensions (host arithmetic; 0 outside [1, zs_mvn_max_dim()]) */
int zs_mvn_group_lanes(int64_t D);

/* V1  the draw with its log-density.
 *   z[k,r,:] = mean[r,:] + L_r eps[k,r,:] ;  lp[k,r] = -D/2 log 2 pi - sum_i log L_ii - 1/2 sum_i eps_i^2   (no solve)
 * z T[K, R, D] and lp T[K, R] may be NULL, not both. */
int zs_mvn_sample_logprob_f32(const void* mean, const void* tril, const void* eps, void* z, void* lp, int64_t K, int64_t R,
                              int64_t D, uint64_t seed, uint64_t call, const uint64_t* rng_state, void* stream);
int zs_mvn_sample_logprob_f64(const void* mean, const void* tril, const void* eps, void* z, void* lp, int64_t K, int64_t R,
                              int64_t D, uint64_t seed, uint64_t call, const uint64_t* rng_state, void* stream);

/* Backward of V1 from gz T[K, R, D] and glp T[K, R] (either may be NULL, not both), eps injected or regenerated from the same
 * (seed, call, rng_state).  gmean T[R, D] and gtril T[R, D, D] may be NULL, not both; the k-sums run in ascending k.
 *   reparameterized != 0   gmean = sum_k gz ;  gtril_ij = sum_k gz_i eps_j - delta_ij (sum_k glp) / L_ii
 *   reparameterized == 0   (the draw is detached, the density keeps its direct dependence; needs glp, ignores gz)
 *                          w = L^-T eps ;  gmean = sum_k glp w ;  gtril_ij = sum_k glp (w_i eps_j - delta_ij / L_ii) */
int zs_mvn_sample_logprob_bwd_f32(const void* tril, const void* eps, const void* gz, const void* glp, int reparameterized,
                                  void* gmean, void* gtril, int64_t K, int64_t R, int64_t D, uint64_t seed, uint64_t call,
                                  const uint64_t* rng_state, void* stream);
int zs_mvn_sample_logprob_bwd_f64(const void* tril, const void* eps, const void* gz, const void* glp, int reparameterized,
                                  void* gmean, void* gtril, int64_t K, int64_t R, int64_t D, uint64_t seed, uint64_t call,
                                  const uint64_t* rng_state, void* stream);

/* V2  the log-density of a given x (T[K, R, D] or T[R, D]: Px = K R D or R D elements; a value without the particle axis is
 * shared by the particles):  y = L^-1 (x - mean) by forward substitution, lp as above with y for eps. */
int zs_mvn_logprob_f32(const void* mean, const void* tril, const void* x, int64_t Px, void* lp, int64_t K, int64_t R, int64_t D,
                       void* stream);
int zs_mvn_logprob_f64(const void* mean, const void* tril, const void* x, int64_t Px, void* lp, int64_t K, int64_t R, int64_t D,
                       void* stream);

/* Backward of V2 with glp T[K, R]:  w = L^-T y by back substitution,
 *   gx[k,r,:] = -glp w  (T[K, R, D] whatever Px is; optional) ;  gmean = sum_k glp w ;  gtril_ij = sum_k glp (w_i y_j - delta_ij / L_ii)
 * Any output may be NULL, not all. */
int zs_mvn_logprob_bwd_f32(const void* mean, const void* tril, const void* x, int64_t Px, const void* glp, void* gx, void* gmean,
                           void* gtril, int64_t K, int64_t R, int64_t D, void* stream);
int zs_mvn_logprob_bwd_f64(const void* mean, const void* tril, const void* x, int64_t Px, const void* glp, void* gx, void* gmean,
                           void* gtril, int64_t K, int64_t R, int64_t D, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ZS_MVN_H */
