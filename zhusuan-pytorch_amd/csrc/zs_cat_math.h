// The arithmetic of the categorical kernels (include/zs_cat.h, zs_cat.hip): the Gumbel transform, the running (max, sum-exp)
// pair of a row and its merge, what a row adds to the lane-group map of zs_group_math.h (chunks of four, work items) and the
// density formulas.  __host__ __device__, so that tests/host_math/zs_cat_host_math.hip runs the same code on the host under the
// sanitizers.
//
// Logarithms and exponentials are the accurate library ones (logf / expf, log / exp): the winner of a Gumbel-max draw is the
// element with u closest to 1, where -log u is tiny and a base-2 hardware logarithm loses the relative accuracy the draw needs.
#pragma once
#include <math.h>
#include "zs_group_math.h"

// a * b + c rounds once only where flat_fma says so: the aligned and the element path must agree bit for bit
#pragma clang fp contract(off)

namespace zs {

ZS_HD float cat_log(float x) { return logf(x); }
ZS_HD double cat_log(double x) { return log(x); }
ZS_HD float cat_exp(float x) { return expf(x); }
ZS_HD double cat_exp(double x) { return exp(x); }
template <typename T>
ZS_HD T cat_neg_inf() { return -(T)INFINITY; }
template <typename T>
ZS_HD T cat_nan() { return (T)NAN; }

// ---------------------------------------------------------------- lane groups
// A row of N categories is cut into chunks of four consecutive categories (one 16-byte access).  A group of
// G = group_lanes(ceil(N / 4)) consecutive lanes owns a row: lane g = pl.lane of the group owns the chunks g, g + G, g + 2G, ...
// So N <= 4 takes one lane per row (64 rows per wave), N <= 256 one chunk per lane, and a wider row is strided over by a whole
// wave; a row never leaves its wave.
ZS_HD int cat_group_lanes(int64_t N) { return group_lanes((N + 3) >> 2); }
// The walk of lane g over its chunks, as every kernel writes it:
//   for (int64_t j0 = cat_chunk_first(g); j0 < N; j0 += cat_chunk_step(G))   -- j0: the first category of a chunk
ZS_HD int64_t cat_chunk_first(int g) { return (int64_t)g << 2; }
ZS_HD int64_t cat_chunk_step(int G) { return (int64_t)G << 2; }

// Workgroups of ZS_CAT_THREADS threads hold ZS_CAT_THREADS / G lane groups (the place is zs_group_math.h's); the groups of the
// grid stride over the work items (rows or particle-rows), and each group leaves the loop on its own:
//   item0 = cat_item_first(block, pl), stride = cat_item_step(blocks, pl);   for (int64_t it = item0; it < items; it += stride)
#define ZS_CAT_THREADS 256
ZS_HD int64_t cat_item_first(int block, const GroupPlace& p) { return group_row_first(block, p) + p.grp; }
ZS_HD int64_t cat_item_step(int blocks, const GroupPlace& p) { return group_row_step(blocks, p); }

// ---------------------------------------------------------------- the Gumbel transform
// v = l - log(-log u): u lies strictly inside (0, 1), so both logarithms are finite
template <typename T>
ZS_HD T cat_gumbel(T u) { return -cat_log(-cat_log(u)); }
template <typename T>
ZS_HD T cat_perturbed(T l, T u) { return l + cat_gumbel(u); }
// (value, index) order of the argmax: larger value first, ties to the lower index
template <typename T>
ZS_HD bool cat_better(T v, int32_t j, T bv, int32_t bj) { return v > bv || (v == bv && j < bj); }

// ---------------------------------------------------------------- running (max, sum-exp)
template <typename T>
struct CatMS { T m, s; };
template <typename T>
ZS_HD CatMS<T> cat_ms_empty() { CatMS<T> a = {cat_neg_inf<T>(), (T)0}; return a; }
// four more elements (an element that is not there is -inf)
template <typename T>
ZS_HD void cat_ms_push4(CatMS<T>& a, const T x[4]) {
  const T m01 = x[0] > x[1] ? x[0] : x[1], m23 = x[2] > x[3] ? x[2] : x[3];
  const T cm = m01 > m23 ? m01 : m23;
  const T nm = a.m > cm ? a.m : cm;
  if (!(nm > cat_neg_inf<T>())) return;          // nothing finite so far
  T s = a.s * cat_exp(a.m - nm);
  s += cat_exp(x[0] - nm);
  s += cat_exp(x[1] - nm);
  s += cat_exp(x[2] - nm);
  s += cat_exp(x[3] - nm);
  a.m = nm;
  a.s = s;
}
template <typename T>
ZS_HD CatMS<T> cat_ms_merge(const CatMS<T>& a, const CatMS<T>& b) {
  const T nm = a.m > b.m ? a.m : b.m;
  if (!(nm > cat_neg_inf<T>())) return a;
  CatMS<T> o;
  o.m = nm;
  o.s = a.s * cat_exp(a.m - nm) + b.s * cat_exp(b.m - nm);
  return o;
}
template <typename T>
ZS_HD T cat_lse(const CatMS<T>& a) { return a.m + cat_log(a.s); }

// ---------------------------------------------------------------- densities
// log-mass of category j: l_j - lse
template <typename T>
ZS_HD T cat_logmass(T lj, T lse) { return lj - lse; }
// one term of the weights form: exactly 0 where x == 0, also at l = -inf
template <typename T>
ZS_HD T cat_weight_term(T x, T l) { return x == (T)0 ? (T)0 : x * l; }
// weights form: sum_j x_j l_j - (sum_j x_j) lse
template <typename T>
ZS_HD T cat_weight_logmass(T sxl, T sx, T lse) { return flat_fma(-sx, lse, sxl); }

// ExpConcrete (Maddison et al. 2017, eq. 26): a = (l + gumbel) / tau ;  y = a - lse(a) ;  t = l - tau y
template <typename T>
ZS_HD T cat_relaxed_a(T l, T u, T tau) { return cat_perturbed(l, u) / tau; }
template <typename T>
ZS_HD T cat_relaxed_t(T l, T y, T tau) { return flat_fma(-tau, y, l); }
// lp = c0 + sum t - N lse(t) [- sum y in exp space], c0 = lgamma(N) + (N - 1) log tau (formed in double on the host)
template <typename T>
ZS_HD T cat_relaxed_lp(T c0, T sum_t, T n, T lse_t, T sum_y, bool exp_space) {
  const T lp = flat_fma(-n, lse_t, c0 + sum_t);
  return exp_space ? lp - sum_y : lp;
}
// q_j = d lp / d t_j = 1 - N softmax(t)_j
template <typename T>
ZS_HD T cat_relaxed_q(T t, T lse_t, T n) { return flat_fma(-n, cat_exp(t - lse_t), (T)1); }

}  // namespace zs
