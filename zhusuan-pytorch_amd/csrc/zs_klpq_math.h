// The arithmetic of the inclusive-KL kernels (include/zs_klpq.h, zs_klpq.hip): the stride addressing of a term, the
// left-to-right sums of the two sides, each lane's partial of the four k-reductions of a datapoint (its lane group is
// zs_group_math.h's), the first wave's partial of the batch mean, and the whole per-thread body of the backward.  __host__
// __device__, so that tests/host_math/zs_klpq_host_math.hip walks the same code on the host under the sanitizers (a table of host
// pointers works there like a table of device pointers does in a kernel).
#pragma once
#include <math.h>
#include "zs_group_math.h"
#include "../../include/zs_klpq.h"

// a * b + c stays two roundings: the same bits whatever the compiler would like to fuse
#pragma clang fp contract(off)

namespace zs {

#define ZS_KLPQ_THREADS 256           // a launch without the batch mean: 256 / G datapoints per workgroup
#define ZS_KLPQ_MEAN_THREADS 1024     // a launch with the batch mean: ONE workgroup of 16 waves
#define ZS_KLPQ_MEAN_MAX_B 1024       // ... whose LDS holds one cost per datapoint
#define ZS_KLPQ_WAVE 64

ZS_HD float klpq_exp(float x) { return expf(x); }
ZS_HD double klpq_exp(double x) { return exp(x); }
ZS_HD float klpq_log(float x) { return logf(x); }
ZS_HD double klpq_log(double x) { return log(x); }

// ---------------------------------------------------------------- terms
// One side of the objective as the kernels receive it (by value): the first n rows of the caller's table.
struct KlpqSide {
  zs_klpq_term t[ZS_KLPQ_MAX_TERMS];
  int n;
};
// element (k, b) of a term, in elements from its base
ZS_HD int64_t klpq_offset(const zs_klpq_term& t, int64_t k, int64_t b) { return k * t.sk + b * t.sb; }
// the side's log-probability of particle k of datapoint b: the terms added left to right, like log_joint
template <typename T>
ZS_HD T klpq_side_sum(const KlpqSide& s, int64_t k, int64_t b) {
  T acc = ((const T*)s.t[0].value)[klpq_offset(s.t[0], k, b)];
  for (int i = 1; i < s.n; ++i) acc += ((const T*)s.t[i].value)[klpq_offset(s.t[i], k, b)];
  return acc;
}
template <typename T>
struct KlpqParticle { T lp, lq, lw; };
template <typename T>
ZS_HD KlpqParticle<T> klpq_particle(const KlpqSide& p, const KlpqSide& q, int64_t k, int64_t b) {
  KlpqParticle<T> v;
  v.lp = klpq_side_sum<T>(p, k, b);
  v.lq = klpq_side_sum<T>(q, k, b);
  v.lw = v.lp - v.lq;
  return v;
}

// ---------------------------------------------------------------- a lane's partials of the k-reductions
// A group of G = group_lanes(K) consecutive lanes of one wave owns a datapoint (the row of zs_group_math.h); lane pl.lane = j of
// the group walks the particles j, j + G, j + 2 G, ... (one particle per lane up to K = 64; idle when j >= K).  A workgroup of
// blockDim.x threads holds blockDim.x / G datapoints; a group past the last datapoint walks K = 0 particles.
// Each partial walks k = j, j + G, ... < K in ascending order; `first` is particle j, read once by the caller and kept in registers (for
// K <= 64 it is all a lane has).  The group's value is the xor butterfly over the G partials: group_butterfly_host on the host,
// shuffles in the kernel (zs_group_math.h).  Neutral partials (-inf, 0) come from lanes without a particle.
template <typename T>
ZS_HD KlpqParticle<T> klpq_at(const KlpqSide& p, const KlpqSide& q, int64_t k, int64_t b, int j, const KlpqParticle<T>& first) {
  return k == j ? first : klpq_particle<T>(p, q, k, b);
}
template <typename T>
ZS_HD T klpq_lane_max(const KlpqSide& p, const KlpqSide& q, int64_t b, int j, int G, int64_t K, const KlpqParticle<T>& first) {
  T m = (T)-INFINITY;
  for (int64_t k = j; k < K; k += G) m = group_fmax(m, klpq_at<T>(p, q, k, b, j, first).lw);          // group_max's own operator
  return m;
}
template <typename T>
ZS_HD T klpq_lane_sumexp(const KlpqSide& p, const KlpqSide& q, int64_t b, int j, int G, int64_t K, const KlpqParticle<T>& first, T m) {
  T s = (T)0;
  for (int64_t k = j; k < K; k += G) s += klpq_exp(klpq_at<T>(p, q, k, b, j, first).lw - m);
  return s;
}
// bound_b = (m + log s) - log K
template <typename T>
ZS_HD T klpq_bound(T m, T s, T logK) { return (m + klpq_log(s)) - logK; }
// one particle's share of sum_k w_k lq_k (model_grad: of sum_k w_k (lq_k + lp_k)); a weight of exactly 0 contributes exactly 0,
// also where the log-probability it would multiply is -inf
template <typename T>
ZS_HD T klpq_cost_term(T w, T lq, T lp, bool model_grad) {
  if (w == (T)0) return (T)0;
  return w * (model_grad ? lq + lp : lq);
}
template <typename T>
struct KlpqSums { T cost, sq; };
// w_k = exp(lw_k - m) / s, written to wrow[k] (the datapoint's row of w; may be NULL), with the lane's partials of
// sum_k w_k (lq_k [+ lp_k]) and of sum_k w_k^2
template <typename T>
ZS_HD KlpqSums<T> klpq_lane_weights(const KlpqSide& p, const KlpqSide& q, int64_t b, int j, int G, int64_t K,
                                    const KlpqParticle<T>& first, T m, T s, bool model_grad, T* wrow) {
  KlpqSums<T> a = {(T)0, (T)0};
  for (int64_t k = j; k < K; k += G) {
    const KlpqParticle<T> v = klpq_at<T>(p, q, k, b, j, first);
    const T w = klpq_exp(v.lw - m) / s;
    if (wrow) wrow[k] = w;
    a.cost += klpq_cost_term(w, v.lq, v.lp, model_grad);
    a.sq += w * w;
  }
  return a;
}

// ---------------------------------------------------------------- the batch mean
// Lane `lane` of the first wave adds costs[lane], costs[lane + 64], ... in ascending order; the 64 partials meet in a butterfly
// and the total is divided by B.
template <typename T>
ZS_HD T klpq_mean_lane(const T* costs, int64_t B, int lane) {
  T a = (T)0;
  for (int64_t b = lane; b < B; b += ZS_KLPQ_WAVE) a += costs[b];
  return a;
}

// ---------------------------------------------------------------- the backward
// The coefficients of one (k, b): what every variational term and every generator term receive there.
template <typename T>
struct KlpqCoef { T q, p; };
template <typename T>
ZS_HD KlpqCoef<T> klpq_coef(T w, T gc, T gb, bool model_grad) {
  KlpqCoef<T> c;
  c.q = -gc * w - gb * w;
  c.p = model_grad ? -gc * w + gb * w : gb * w;
  return c;
}
template <typename T>
ZS_HD KlpqCoef<T> klpq_coef_at(const T* w, const T* gcost, T gmean, const T* gbound, bool model_grad, int64_t k, int64_t b, int64_t K) {
  return klpq_coef<T>(w[b * K + k], gcost ? gcost[b] : gmean, gbound ? gbound[b] : (T)0, model_grad);
}
template <typename T>
ZS_HD T klpq_pick(const KlpqCoef<T>& c, bool generator) { return generator ? c.p : c.q; }
// The gradient of a term with a zero stride: the sum over the broadcast axis, by the thread that owns the output element, in
// ascending index.  `gcost` NULL means the scalar gmean for every datapoint.
template <typename T>
ZS_HD void klpq_broadcast_grad(const zs_klpq_term& t, bool generator, int64_t K, int64_t B, const T* w, const T* gcost, T gmean,
                               const T* gbound, bool model_grad, int64_t tid, int64_t nth) {
  T* g = (T*)t.grad;
  if (t.sb != 0) {                  // shared by the particles: one output per datapoint
    for (int64_t b = tid; b < B; b += nth) {
      T acc = (T)0;
      for (int64_t k = 0; k < K; ++k) acc += klpq_pick(klpq_coef_at<T>(w, gcost, gmean, gbound, model_grad, k, b, K), generator);
      g[b * t.sb] = acc;
    }
  } else if (t.sk != 0) {           // shared by the batch: one output per particle
    for (int64_t k = tid; k < K; k += nth) {
      T acc = (T)0;
      for (int64_t b = 0; b < B; ++b) acc += klpq_pick(klpq_coef_at<T>(w, gcost, gmean, gbound, model_grad, k, b, K), generator);
      g[k * t.sk] = acc;
    }
  } else if (tid == 0) {            // one number: the k-sum of each datapoint, added up over the datapoints
    T acc = (T)0;
    for (int64_t b = 0; b < B; ++b) {
      T row = (T)0;
      for (int64_t k = 0; k < K; ++k) row += klpq_pick(klpq_coef_at<T>(w, gcost, gmean, gbound, model_grad, k, b, K), generator);
      acc += row;
    }
    g[0] = acc;
  }
}
// Everything thread `tid` of `nth` does in the backward launch.  gcost_is_mean: gcost[0] / B stands for every gcost_b.
template <typename T>
ZS_HD void klpq_backward_thread(const KlpqSide& p, const KlpqSide& q, int64_t K, int64_t B, bool model_grad, bool gcost_is_mean,
                                const T* w, const T* gcost, const T* gbound, int64_t tid, int64_t nth) {
  const T gmean = gcost_is_mean ? gcost[0] / (T)B : (T)0;
  const T* gc = gcost_is_mean ? nullptr : gcost;
  for (int64_t i = tid; i < K * B; i += nth) {          // flat element i of w[B, K]
    const int64_t b = i / K, k = i - b * K;
    const KlpqCoef<T> c = klpq_coef_at<T>(w, gc, gmean, gbound, model_grad, k, b, K);
    for (int t = 0; t < q.n; ++t)
      if (q.t[t].grad && q.t[t].sk != 0 && q.t[t].sb != 0) ((T*)q.t[t].grad)[klpq_offset(q.t[t], k, b)] = c.q;
    for (int t = 0; t < p.n; ++t)
      if (p.t[t].grad && p.t[t].sk != 0 && p.t[t].sb != 0) ((T*)p.t[t].grad)[klpq_offset(p.t[t], k, b)] = c.p;
  }
  for (int t = 0; t < q.n; ++t)
    if (q.t[t].grad && (q.t[t].sk == 0 || q.t[t].sb == 0)) klpq_broadcast_grad<T>(q.t[t], false, K, B, w, gc, gmean, gbound, model_grad, tid, nth);
  for (int t = 0; t < p.n; ++t)
    if (p.t[t].grad && (p.t[t].sk == 0 || p.t[t].sb == 0)) klpq_broadcast_grad<T>(p.t[t], true, K, B, w, gc, gmean, gbound, model_grad, tid, nth);
}

}  // namespace zs
