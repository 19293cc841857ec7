// Q1 and its backward: the inclusive-KL objective over K particles (include/zs_klpq.h; its own library, ../lib/libzs_klpq.so,
// `make klpq`).
//
// A torch composition of the objective costs a dozen launches each way (the additions of the two log-joints, a subtraction, max,
// exp, sum, divide, multiply, sum, mean ...); here it is one launch each way.  A group of G = next_pow2(min(K, 64)) lanes owns a
// datapoint, lane j its particles j, j + G, ... (zs_klpq_math.h); every k-reduction is the lane's partial in ascending k, then an
// xor butterfly inside the group, so its bits depend on K alone.  A launch that also forms the batch mean is ONE workgroup that
// parks each datapoint's cost in LDS and lets its first wave add them in a fixed order: no atomics, no workspace.  No scratch;
// the only LDS is that array of costs.  Every access is one element wide.
#include "zs_common.h"
#include "zs_klpq_math.h"
#include "../../include/zs_hip.h"
#include "../../include/zs_klpq.h"

#pragma clang fp contract(off)

using namespace zs;

namespace {

// ---------------------------------------------------------------- Q1
// gridDim.x workgroups of blockDim.x threads, blockDim.x / G datapoints each per step.  With mean_cost the launch is one workgroup.
template <typename T>
__global__ __launch_bounds__(ZS_KLPQ_MEAN_THREADS) void k_klpq_forward(const KlpqSide p, const KlpqSide q, int64_t K, int64_t B, int G,
                                                                       int flags, T logK, T* __restrict__ w, T* __restrict__ cost,
                                                                       T* __restrict__ bound, T* __restrict__ ess,
                                                                       T* __restrict__ mean_cost) {
  __shared__ T costs[ZS_KLPQ_MEAN_MAX_B];
  const bool model_grad = (flags & ZS_KLPQ_MODEL_GRAD) != 0, bound_only = (flags & ZS_KLPQ_BOUND_ONLY) != 0;
  const GroupPlace pl = group_place((int)threadIdx.x, (int)blockDim.x, G);
  for (int64_t rb = group_row_first((int)blockIdx.x, pl); rb < B; rb += group_row_step((int)gridDim.x, pl)) {
    const int64_t b = rb + pl.grp;
    const bool valid = b < B;
    const int64_t Kv = valid ? K : 0;          // a group past the last datapoint walks no particle
    KlpqParticle<T> first = {(T)0, (T)0, (T)0};
    if (pl.lane < Kv) first = klpq_particle<T>(p, q, pl.lane, b);
    const T m = group_max(klpq_lane_max<T>(p, q, b, pl.lane, G, Kv, first), G);
    const T s = group_sum(klpq_lane_sumexp<T>(p, q, b, pl.lane, G, Kv, first, m), G);
    if (bound && valid && pl.lane == 0) bound[b] = klpq_bound(m, s, logK);
    if (bound_only) continue;
    const KlpqSums<T> part = klpq_lane_weights<T>(p, q, b, pl.lane, G, Kv, first, m, s, model_grad, (w && valid) ? w + b * K : nullptr);
    const T c = -group_sum(part.cost, G);
    const T sq = group_sum(part.sq, G);
    if (valid && pl.lane == 0) {
      if (cost) cost[b] = c;
      if (ess) ess[b] = (T)1 / sq;
      if (mean_cost) costs[b] = c;             // (one workgroup, B <= ZS_KLPQ_MEAN_MAX_B: checked on the host)
    }
  }
  if (mean_cost) {
    __syncthreads();
    if (threadIdx.x < ZS_KLPQ_WAVE) {
      const T total = group_sum(klpq_mean_lane<T>(costs, B, (int)threadIdx.x), ZS_KLPQ_WAVE);
      if (threadIdx.x == 0) mean_cost[0] = total / (T)B;
    }
  }
}

// ---------------------------------------------------------------- the backward
template <typename T>
__global__ __launch_bounds__(ZS_KLPQ_THREADS) void k_klpq_backward(const KlpqSide p, const KlpqSide q, int64_t K, int64_t B, int flags,
                                                                   const T* __restrict__ w, const T* __restrict__ gcost,
                                                                   const T* __restrict__ gbound) {
  klpq_backward_thread<T>(p, q, K, B, (flags & ZS_KLPQ_MODEL_GRAD) != 0, (flags & ZS_KLPQ_GCOST_MEAN) != 0, w, gcost, gbound,
                          (int64_t)blockIdx.x * blockDim.x + threadIdx.x, (int64_t)gridDim.x * blockDim.x);
}

// ---------------------------------------------------------------- host side
// the table rows of one side, checked: 0, ZS_EINVAL or ZS_ENOTSUP
int take_side(const zs_klpq_term* tab, int n, bool need_values, KlpqSide& s) {
  if (!tab || n < 1) return ZS_EINVAL;
  if (n > ZS_KLPQ_MAX_TERMS) return ZS_ENOTSUP;
  memset(&s, 0, sizeof(s));
  s.n = n;
  for (int i = 0; i < n; ++i) {
    if (need_values && !tab[i].value) return ZS_EINVAL;
    s.t[i] = tab[i];
  }
  return 0;
}
bool any_grad(const KlpqSide& s) {
  for (int i = 0; i < s.n; ++i)
    if (s.t[i].grad) return true;
  return false;
}

template <typename T>
int klpq_forward(const zs_klpq_term* pt, int Tp, const zs_klpq_term* qt, int Tq, int64_t K, int64_t B, int flags, void* w, void* cost,
                 void* bound, void* ess, void* mean_cost, void* stream) {
  KlpqSide p, q;
  if (K < 0 || B < 0) return ZS_EINVAL;
  int rc = take_side(pt, Tp, true, p);
  if (rc == ZS_EINVAL) return rc;
  const int rq = take_side(qt, Tq, true, q);
  if (rq == ZS_EINVAL) return rq;
  if (rc || rq) return ZS_ENOTSUP;
  const bool bound_only = (flags & ZS_KLPQ_BOUND_ONLY) != 0;
  if (bound_only ? !bound : (!w && !cost && !bound && !ess && !mean_cost)) return ZS_EINVAL;
  if (bound_only) w = cost = ess = mean_cost = nullptr;
  if (mean_cost && B > ZS_KLPQ_MEAN_MAX_B) return ZS_ENOTSUP;
  if (K == 0 || B == 0) return 0;
  const int G = group_lanes(K);
  const unsigned threads = mean_cost ? ZS_KLPQ_MEAN_THREADS : ZS_KLPQ_THREADS;
  const unsigned grid = mean_cost ? 1u : grid_for(B, (int)threads / G, 256u * 16u);
  hipLaunchKernelGGL((k_klpq_forward<T>), dim3(grid), dim3(threads), 0, (hipStream_t)stream, p, q, K, B, G, flags,
                     (T)log((double)K), (T*)w, (T*)cost, (T*)bound, (T*)ess, (T*)mean_cost);
  ZS_CHECK_LAUNCH();
  return 0;
}

template <typename T>
int klpq_backward(const zs_klpq_term* pt, int Tp, const zs_klpq_term* qt, int Tq, int64_t K, int64_t B, int flags, const void* w,
                  const void* gcost, const void* gbound, void* stream) {
  KlpqSide p, q;
  if (K < 0 || B < 0) return ZS_EINVAL;
  int rc = take_side(pt, Tp, false, p);
  if (rc == ZS_EINVAL) return rc;
  const int rq = take_side(qt, Tq, false, q);
  if (rq == ZS_EINVAL) return rq;
  if (rc || rq) return ZS_ENOTSUP;
  if (!w || !gcost || (!any_grad(p) && !any_grad(q))) return ZS_EINVAL;
  if (K == 0 || B == 0) return 0;
  hipLaunchKernelGGL((k_klpq_backward<T>), dim3(grid_for(K * B, ZS_KLPQ_THREADS, 256u * 16u)), dim3(ZS_KLPQ_THREADS), 0,
                     (hipStream_t)stream, p, q, K, B, flags, (const T*)w, (const T*)gcost, (const T*)gbound);
  ZS_CHECK_LAUNCH();
  return 0;
}

}  // namespace

extern "C" int zs_klpq_abi_version(void) { return ZS_KLPQ_ABI_VERSION; }
extern "C" int zs_klpq_max_terms(void) { return ZS_KLPQ_MAX_TERMS; }
extern "C" int64_t zs_klpq_mean_max_batch(void) { return ZS_KLPQ_MEAN_MAX_B; }
extern "C" int zs_klpq_group_lanes(int64_t K) { return K < 1 ? 0 : group_lanes(K); }

#define ZS_KLPQ_ENTRY(SFX, T)                                                                                                       \
  extern "C" int zs_klpq_forward##SFX(const struct zs_klpq_term* p, int Tp, const struct zs_klpq_term* q, int Tq, int64_t K,        \
                                      int64_t B, int flags, void* w, void* cost, void* bound, void* ess, void* mean_cost,           \
                                      void* stream) {                                                                               \
    return klpq_forward<T>(p, Tp, q, Tq, K, B, flags, w, cost, bound, ess, mean_cost, stream);                                      \
  }                                                                                                                                 \
  extern "C" int zs_klpq_backward##SFX(const struct zs_klpq_term* p, int Tp, const struct zs_klpq_term* q, int Tq, int64_t K,       \
                                       int64_t B, int flags, const void* w, const void* gcost, const void* gbound, void* stream) {  \
    return klpq_backward<T>(p, Tp, q, Tq, K, B, flags, w, gcost, gbound, stream);                                                   \
  }

ZS_KLPQ_ENTRY(_f32, float)
ZS_KLPQ_ENTRY(_f64, double)
