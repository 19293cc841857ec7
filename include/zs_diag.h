/*
 * zs_diag.h -- C ABI of the chain diagnostics (libzs_diag.so, gfx950): the mean, the marginal posterior variance estimate
 * var+, the (split) potential scale reduction R-hat and the effective sample size of every element of a stack of Markov chains
 * in one launch, and the autocorrelation curve of every chain in one more.  After Gelman et al., Bayesian Data Analysis (3rd
 * ed., section 11.4-11.5) and Vehtari, Gelman, Simpson, Carpenter, Buerkner (2021), without the rank normalisation.
 *
 * An eighth library next to libzs_hip.so and the seven other satellites, with the conventions of zs_hmc.h and zs_klpq.h: every
 * pointer is a DEVICE pointer owned by the caller, nothing is allocated, freed or synchronised inside a call, `stream` is a
 * hipStream_t passed as void* (NULL = the null stream), the return value is 0 on success, a positive hipError_t if the launch
 * failed, ZS_EINVAL / ZS_ENOTSUP (the codes of zs_hip.h) for rejected arguments, which write nothing.  A call only enqueues one
 * kernel.  T is the element type of the suffix (_f32: float, _f64: double).
 *
 * Operand.  x holds T draws of C chains of E elements: draw t of chain c of element e is x[t st + c sc + e], st and sc strides
 * in ELEMENTS, the stride along e is 1.  A [T, C, E] stack is st = C E, sc = E; a [C, T, E] stack is st = E, sc = T E; both
 * run without a copy.
 * ZS_EINVAL: a NULL x, a negative size, N < 2 after the split (summary) or L > T - 1 or L < 0 (autocorr), a stride smaller than
 * the extent it steps over (the inner of st, sc below E, the outer below the inner times its count; with C = 1, sc is not
 * looked at), nothing to write.  ZS_ENOTSUP: E >= 2^31.  T C E == 0 returns 0 and launches nothing.
 *
 * The arithmetic is the specification (tests/diag_host.py restates it in float64).
 *   1. Split.  With split != 0 every chain becomes two of length N = T / 2 (integer division): draws [0, N) and [T - N, T); an
 *      odd T drops the middle draw.  M = 2 C chains, all first halves in chain order, then all second halves.  Without split
 *      N = T, M = C.
 *   2. Per chain m:   mean_m = (sum_t x) / N ;   s2_m = sum_t (x - mean_m)^2 / (N - 1)        (centred, a second pass)
 *   3. Across chains: mean = (sum_m mean_m) / M ;  W = (sum_m s2_m) / M ;
 *                     BN = sum_m (mean_m - mean)^2 / (M - 1), 0 for M = 1 ;
 *                     var+ = (N - 1) / N * W + BN ;   rhat = sqrt(var+ / W)
 *   4. Autocovariance: g_{l,m} = (1 / N) sum_{t = 0}^{N - l - 1} (x_t - mean_m) (x_{t+l} - mean_m) ;
 *                      rho_l = 1 - (W - (sum_m g_{l,m}) / M) / var+
 *   5. Lag cap.  Lcap = min(max_lag, N - 1); max_lag < 0 means N - 1.
 *   6. Geyer's initial monotone sequence.  tau = -1.  For k = 0, 1, ... while 2 k + 1 <= Lcap:  P_k = rho_{2k} + rho_{2k+1};
 *      stop if !(P_k > 0);  otherwise P_k = min(P_k, P_{k-1}) and tau += 2 P_k.
 *   7. tau = max(tau, 1 / log10(M N)) ;  ess = M N / tau.
 *   8. lags = 2 k at the stop: the number of lags that entered tau.  capped = 1 if the loop ended at Lcap, 0 if it ended on a
 *      pair that was not positive.
 * Every sum is a double whatever T is, accumulated in ascending t, then ascending m; products enter a sum by a fused
 * multiply-add; the outputs are rounded once to T.
 *   Edge cases.  An element with a NaN or infinite draw among the draws that enter (the middle draw of an odd split T does not)
 * gets NaN in mean, var_plus, rhat and ess, and lags = capped = 0; its neighbours are unaffected.  A constant series (W == 0)
 * gets NaN rhat and ess and lags = capped = 0; its mean and var_plus are what the formulas give.
 *
 * Kernel shape.  One lane per element e, 256 threads per workgroup, ceil(E / 256) workgroups: every load of a draw is one
 * coalesced row across the lanes of a wave.  Pass 1 forms the chain means, pass 2 the centred squares, and the lag loop walks t
 * for one pair of lags at a time over all chains, each lane leaving the loop at its own stopping pair.  All passes after the
 * first read the tile of x a workgroup owns (256 elements x C T draws) again, from L2 and the Infinity Cache while it fits.  A
 * lane keeps the means of its first 16 chains (a private array: 136 bytes of scratch per lane); those of further chains are
 * summed again where they are needed, with the same bits.  No LDS, no atomics, no floating-point reduction across lanes, one
 * element wide accesses: the same call gives the same bits, and so do an aligned and a shifted operand and the two stack orders.
 *
 * Limit.  The parallelism is E lanes whatever T and C are, and the cost per element is C T (3 + lags) double fused
 * multiply-adds and about as many loads: a two-parameter toy model runs on ONE wave, and its time grows with C T times its
 * autocorrelation time.  The launch pays off for what it was written for -- posteriors of 10^4 .. 10^6 elements.  A lane group
 * per element that splits t (partial sums combined in a fixed order) is not implemented; zs_diag_autocorr costs C T (L + 2)
 * per element in the same way.
 */
#ifndef ZS_DIAG_H
#define ZS_DIAG_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ZS_DIAG_ABI_VERSION 1

/* ABI version of the loaded library (== ZS_DIAG_ABI_VERSION). */
int zs_diag_abi_version(void);

/* Steps 1 - 8 for every element.  mean, var_plus, rhat, ess: T[E]; lags, capped: int32[E].  Any output may be NULL, not all.
 * The lag loop runs only when ess, lags or capped is given: with all three NULL the call is the R-hat-only mode (passes 1 and 2). */
int zs_diag_summary_f32(const void* x, int64_t st, int64_t sc, int64_t T, int64_t C, int64_t E, int split, int64_t max_lag,
                        void* mean, void* var_plus, void* rhat, void* ess, int32_t* lags, int32_t* capped, void* stream);
int zs_diag_summary_f64(const void* x, int64_t st, int64_t sc, int64_t T, int64_t C, int64_t E, int split, int64_t max_lag,
                        void* mean, void* var_plus, void* rhat, void* ess, int32_t* lags, int32_t* capped, void* stream);

/* The autocorrelation curve of every unsplit chain: acf[l, c, e] = g_{l,c} / g_{0,c} for l in [0, L] with N = T, acf T[L + 1, C, E]
 * contiguous.  A chain with a non-finite draw, or a constant one, gets NaN along its curve. */
int zs_diag_autocorr_f32(const void* x, int64_t st, int64_t sc, int64_t T, int64_t C, int64_t E, int64_t L, void* acf, void* stream);
int zs_diag_autocorr_f64(const void* x, int64_t st, int64_t sc, int64_t T, int64_t C, int64_t E, int64_t L, void* acf, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ZS_DIAG_H */
