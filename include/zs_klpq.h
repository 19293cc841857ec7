/*
 * zs_klpq.h -- C ABI of the inclusive-KL objective (libzs_klpq.so, gfx950): the self-normalised importance weights of K
 * particles, the KL(p||q) cost of reweighted wake-sleep, the importance-weighted bound and the effective sample size in one
 * launch (Q1), and the gradient w.r.t. every log-probability term in one more.
 *
 * A seventh library next to libzs_hip.so, libzs_mcmc.so, libzs_flow.so, libzs_hmc.so, libzs_cat.so and libzs_mvn.so, with the
 * conventions of zs_mvn.h: every pointer inside a table and every operand is a DEVICE pointer owned by the caller, the tables
 * themselves are HOST arrays read during the call, nothing is allocated, freed or synchronised inside a call, `stream` is a
 * hipStream_t passed as void* (NULL = the null stream), the return value is 0 on success, a positive hipError_t if the launch
 * failed, ZS_EINVAL / ZS_ENOTSUP (the codes of zs_hip.h) for rejected arguments, which write nothing.  A call only enqueues one
 * kernel.  T is the element type of the suffix (_f32: float, _f64: double).
 *
 * Operands.  Tp generator terms and Tq variational terms (1 .. ZS_KLPQ_MAX_TERMS each), every one a log-probability matrix over
 * K particles x B datapoints: element (k, b) of a term is value[k sk + b sb] (strides in ELEMENTS, per term, any sign of layout):
 *   [K, B] contiguous   sk = B, sb = 1          [B, K] contiguous       sk = 1, sb = K
 *   shared by the batch sk = 1, sb = 0          shared by the particles sk = 0, sb = 1
 * ZS_EINVAL: a NULL table, Tp or Tq < 1, K < 0, B < 0, a NULL value pointer (forward), nothing to write, a backward without w or
 * gcost.  ZS_ENOTSUP: Tp or Tq > ZS_KLPQ_MAX_TERMS, a mean_cost with B > zs_klpq_mean_max_batch().  K B == 0 returns 0 and
 * launches nothing.
 *
 * Kernel shape.  A group of G = next_pow2(min(K, 64)) consecutive lanes of one wave owns a datapoint; lane j walks particles
 * j, j + G, j + 2 G ...  Each of the reductions over k (max, sum of exponentials, cost, sum of squared weights) is the lane's own
 * partial in ascending k followed by an xor butterfly inside the group, which leaves the same bits in every lane.  That order
 * depends on K alone -- not on the grid, the block size or the strides -- so the same values in any layout give the same bits,
 * and so does the same call again.  The terms are read three times for K > 64 (max, sum, weights) and once below that, where a
 * lane's single particle stays in registers.  Every access is one element wide: the results do not depend on the alignment of
 * the operands.  With [K, B]-contiguous terms the lanes of a group read B elements apart; at the sizes this objective is
 * trained at (K B of a few ten thousand) the launch, not the traffic, is what it costs.
 *   The batch mean is formed by ONE workgroup: a call with mean_cost runs as a single workgroup of 1024 threads that keeps each
 * datapoint's cost in LDS (B <= zs_klpq_mean_max_batch() = 1024; T[1024] is the only LDS of the library) and lets its first wave
 * add them up -- lane l takes b = l, l + 64, ... in ascending order, then a butterfly -- and divide by B.  No atomics, no
 * workspace, the same bits on every call.  Beyond that B the caller takes `cost` and forms the mean itself.  A call without
 * mean_cost runs 256 / G datapoints per workgroup over as many workgroups as B needs.
 *   The backward computes each (k, b) coefficient once and writes it to every term in that term's own layout; the gradient of a
 * term with a zero stride is the sum over the broadcast axis, formed by one lane per output element in ascending index (b
 * outermost where both strides are zero): its time grows with the length of that axis.
 */
#ifndef ZS_KLPQ_H
#define ZS_KLPQ_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ZS_KLPQ_ABI_VERSION 1
#define ZS_KLPQ_MAX_TERMS 8          /* per side; the caller pre-adds what does not fit */

/* flags */
#define ZS_KLPQ_MODEL_GRAD 1         /* the cost also carries log p: -sum_k w_k (lq_k + lp_k); the backward hands -gcost w to the generator terms */
#define ZS_KLPQ_BOUND_ONLY 2         /* forward: only `bound` is formed and written */
#define ZS_KLPQ_GCOST_MEAN 4         /* backward: gcost is ONE element, the cotangent of mean_cost; the kernel folds in 1 / B */

/* One log-probability term (HOST table; the pointers in it are device pointers to T). */
struct zs_klpq_term {
  const void* value;                 /* forward: element (k, b) at value[k sk + b sb]; not read by the backward */
  void* grad;                        /* backward: the gradient in the same layout, NULL = skipped; not touched by the forward */
  int64_t sk, sb;                    /* strides in elements; 0 = the term is shared along that axis */
};

/* ABI version of the loaded library (== ZS_KLPQ_ABI_VERSION). */
int zs_klpq_abi_version(void);
/* ZS_KLPQ_MAX_TERMS */
int zs_klpq_max_terms(void);
/* the largest B a call with mean_cost takes (1024) */
int64_t zs_klpq_mean_max_batch(void);
/* lanes per datapoint for K particles (host arithmetic; 0 for K < 1) */
int zs_klpq_group_lanes(int64_t K);

/* Q1.  Per datapoint b, with lp_k = sum_t p_t[k, b] and lq_k = sum_t q_t[k, b], each summed left to right in table order:
 *   lw_k = lp_k - lq_k ;  m = max_k lw_k ;  e_k = exp(lw_k - m) ;  s = sum_k e_k ;  w_k = e_k / s
 *   bound_b = (m + log s) - log K
 *   cost_b  = -sum_k w_k lq_k            (ZS_KLPQ_MODEL_GRAD: -sum_k w_k (lq_k + lp_k))
 *   ess_b   = 1 / sum_k w_k^2
 *   mean_cost = (sum_b cost_b) / B
 * A particle whose weight is exactly 0 (lw_k = -inf next to a finite one) contributes exactly 0 to cost_b.  A datapoint whose
 * lw are all -inf gets NaN in w, cost, bound and ess, and makes mean_cost NaN; other datapoints are untouched.
 * w T[B, K] (K fastest), cost, bound, ess T[B], mean_cost T[1]: any may be NULL, not all.  With ZS_KLPQ_BOUND_ONLY only `bound`
 * is written and it must not be NULL. */
int zs_klpq_forward_f32(const struct zs_klpq_term* p, int Tp, const struct zs_klpq_term* q, int Tq, int64_t K, int64_t B,
                        int flags, void* w, void* cost, void* bound, void* ess, void* mean_cost, void* stream);
int zs_klpq_forward_f64(const struct zs_klpq_term* p, int Tp, const struct zs_klpq_term* q, int Tq, int64_t K, int64_t B,
                        int flags, void* w, void* cost, void* bound, void* ess, void* mean_cost, void* stream);

/* Backward of Q1 with the weights held constant.  w T[B, K] as the forward wrote it; gcost T[B] (ZS_KLPQ_GCOST_MEAN: T[1], used
 * as gcost[0] / B for every b); gbound T[B] or NULL (= 0).  With gc = gcost_b and gb = gbound_b:
 *   every variational term   g[k, b] = -gc w_k - gb w_k
 *   every generator term     g[k, b] = -gc w_k + gb w_k   with ZS_KLPQ_MODEL_GRAD, else gb w_k
 * written to term.grad at [k sk + b sb]; a zero stride receives the sum over that axis; a NULL grad is skipped.  At least one
 * grad must be non-NULL. */
int zs_klpq_backward_f32(const struct zs_klpq_term* p, int Tp, const struct zs_klpq_term* q, int Tq, int64_t K, int64_t B,
                         int flags, const void* w, const void* gcost, const void* gbound, void* stream);
int zs_klpq_backward_f64(const struct zs_klpq_term* p, int Tp, const struct zs_klpq_term* q, int Tq, int64_t K, int64_t B,
                         int flags, const void* w, const void* gcost, const void* gbound, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ZS_KLPQ_H */
