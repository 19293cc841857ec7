// Per-element arithmetic and index maps of the normalising-flow kernels (zs_flow.hip, C ABI: include/zs_flow.h),
// __host__ __device__ like zs_mcmc_math.h so that the host-side sanitizer test (tests/host_math/zs_flow_host_math.hip) runs
// the same code.  The formulas restate zhusuan/invertible/coupling.py:65-75,102-147, scaling.py:26-34, made.py:106-122 and
// zhusuan/distributions/flow_distribution.py:48-51 of the reference.
//
// Masks are user-supplied floats, not necessarily 0 / 1, and the reference evaluates its expressions one torch op at a time:
// contraction is switched off in every function here, so that each written operation rounds once, the vector and the element
// form of a kernel agree bit for bit and a restatement with separate torch ops reproduces the kernel.
#pragma once
#include <math.h>
#include <stdint.h>
#include <hip/hip_runtime.h>
#include "../../include/zs_flow.h"

#ifndef ZS_HD
#define ZS_HD __host__ __device__ __forceinline__
#endif

namespace zs {

// exp / log / log1p of the platform's math library (<= 1 ulp on the device): |log_scale| reaches tens in a trained NICE, where
// the base-2 hardware instruction behind a rounded multiply by log2(e) loses seven bits.
ZS_HD float flow_exp(float x) { return expf(x); }
ZS_HD double flow_exp(double x) { return exp(x); }
ZS_HD float flow_log(float x) { return logf(x); }
ZS_HD double flow_log(double x) { return log(x); }
ZS_HD float flow_log1p(float x) { return log1pf(x); }
ZS_HD double flow_log1p(double x) { return log1p(x); }
ZS_HD float flow_tanh(float x) { return tanhf(x); }
ZS_HD double flow_tanh(double x) { return tanh(x); }
ZS_HD float flow_abs(float x) { return fabsf(x); }
ZS_HD double flow_abs(double x) { return fabs(x); }

// ---------------------------------------------------------------- coupling, MASK mode
// coupling.py:66   x1 = mask * x
template <typename T>
ZS_HD T flow_split_mask(T mask, T x) {
#pragma clang fp contract(off)
  return mask * x;
}
// coupling.py:66-69   y = mask*x + ((1 - mask)*x + (sign*shift)*(1 - mask))     (sign = -1: coupling.py:72-75)
template <typename T>
ZS_HD T flow_merge_mask(T mask, T x, T shift, T sign) {
#pragma clang fp contract(off)
  const T om = (T)1 - mask;
  const T x1 = mask * x;
  const T x2 = om * x;
  const T sh = (sign * shift) * om;
  const T y2 = x2 + sh;
  return x1 + y2;
}
// backward of the line above from one read of gy
template <typename T>
ZS_HD void flow_merge_mask_bwd(T mask, T gy, T sign, T& gx, T& gshift) {
#pragma clang fp contract(off)
  const T om = (T)1 - mask;
  const T a = mask * gy;
  const T b = om * gy;
  gx = a + b;
  gshift = sign * (gy * om);
}

// ---------------------------------------------------------------- coupling, INTERLEAVE mode: index maps
// column of x that element j of the [B, D/2] half comes from / goes to (coupling.py:111-115: reshape to [B, D/2, 2])
ZS_HD int64_t flow_pair_column(int64_t j, int pos) { return 2 * j + pos; }
// flat offset of (b, column) in a row-major [B, D]
ZS_HD int64_t flow_at(int64_t b, int64_t d, int64_t D) { return b * D + d; }
// flat offsets of m and loga of element (b, d) inside the inner network's [B, 2D] output (made.py:108: chunk(2, dim=1))
ZS_HD int64_t flow_made_m_at(int64_t b, int64_t d, int64_t D) { return b * (2 * D) + d; }
ZS_HD int64_t flow_made_loga_at(int64_t b, int64_t d, int64_t D) { return b * (2 * D) + D + d; }

template <typename T>
ZS_HD T flow_shift_add(T x, T shift, T sign) {
#pragma clang fp contract(off)
  return x + sign * shift;
}

// ---------------------------------------------------------------- Scaling
// scaling.py:28,33   y = x * exp(sign * log_scale)
template <typename T>
ZS_HD T flow_scale_factor(T log_scale, T sign) {
#pragma clang fp contract(off)
  return flow_exp(sign * log_scale);
}

// scaling.py backward: one term gy * y of a column sum, and the sum's epilogue sign * s + g_logdet -- the products round before
// they are added, like the separate multiply and sum of a torch restatement
template <typename T>
ZS_HD T flow_mul(T a, T b) {
#pragma clang fp contract(off)
  return a * b;
}
template <typename T>
ZS_HD T flow_add(T a, T b) {
#pragma clang fp contract(off)
  return a + b;
}
template <typename T>
ZS_HD T flow_scale_gls(T sign, T s, T g_logdet) {
#pragma clang fp contract(off)
  const T t = sign * s;
  return t + g_logdet;
}

// ---------------------------------------------------------------- MADE's affine
// made.py:109   u = (x - m) * exp(-loga)
template <typename T>
ZS_HD T flow_made_u(T x, T m, T loga) {
#pragma clang fp contract(off)
  return (x - m) * flow_exp(-loga);
}
// backward: e = exp(-loga);  gx = gu e;  gm = -(gu e);  gloga = -(gu u) - gld
template <typename T>
ZS_HD void flow_made_bwd(T gu, T gld, T x, T m, T loga, T& gx, T& gm, T& gloga) {
#pragma clang fp contract(off)
  const T e = flow_exp(-loga);
  const T u = (x - m) * e;
  gx = gu * e;
  gm = -gx;
  gloga = -(gu * u) - gld;
}
// made.py:120   x = u * exp(loga) + m
template <typename T>
ZS_HD T flow_made_inv(T u, T m, T loga) {
#pragma clang fp contract(off)
  return u * flow_exp(loga) + m;
}

// ---------------------------------------------------------------- FlowDistribution tail: base log-densities
// normal.py:121-124   c - log(std) - 0.5 * precision * (z - mean)^2,  precision = 1 / std^2
template <typename T>
ZS_HD T flow_normal_lp(T z, T loc, T scale) {
#pragma clang fp contract(off)
  const T c = (T)-0.91893853320467274178;
  const T diff = z - loc;
  const T prec = (T)1 / (scale * scale);
  return (c - flow_log(scale)) - (T)0.5 * prec * (diff * diff);
}
template <typename T>
ZS_HD T flow_normal_dz(T z, T loc, T scale) {
#pragma clang fp contract(off)
  return -(((T)1 / (scale * scale)) * (z - loc));
}
// logistic.py:81-82   -t - 2 softplus(-t) - log(scale) with t = (z - loc) / scale, in its even, overflow-free form
template <typename T>
ZS_HD T flow_logistic_lp(T z, T loc, T scale) {
#pragma clang fp contract(off)
  const T at = flow_abs((z - loc) / scale);
  return -(at + (T)2 * flow_log1p(flow_exp(-at))) - flow_log(scale);
}
// d/dz = -tanh(t / 2) / scale   (tanh itself: (1 - e) / (1 + e) with e = exp(-|t|) cancels for small t)
template <typename T>
ZS_HD T flow_logistic_dz(T z, T loc, T scale) {
#pragma clang fp contract(off)
  const T t = (z - loc) / scale;
  return -(flow_tanh((T)0.5 * t) / scale);
}
template <typename T>
ZS_HD T flow_base_lp(int base, T z, T loc, T scale) {
  return base == ZS_FLOW_NORMAL ? flow_normal_lp(z, loc, scale) : flow_logistic_lp(z, loc, scale);
}
template <typename T>
ZS_HD T flow_base_dz(int base, T z, T loc, T scale) {
  return base == ZS_FLOW_NORMAL ? flow_normal_dz(z, loc, scale) : flow_logistic_dz(z, loc, scale);
}

// ---------------------------------------------------------------- the fixed summation orders
// A row of D terms summed by one wavefront: lane l adds terms l, l + 64, ... in ascending order, then the 64 lane sums are
// combined by a butterfly (offsets 32, 16, ..., 1).  A column of B terms summed by R row lanes: row lane r adds rows r, r + R,
// ... in ascending order, then row lane 0 adds the R partial sums in ascending order.  The host restatement of either is the
// same loops.
#define ZS_FLOW_COL_TILE 64     // columns per workgroup of the column reduction
#define ZS_FLOW_ROW_LANES 16    // row lanes per column of the column reduction

}  // namespace zs
