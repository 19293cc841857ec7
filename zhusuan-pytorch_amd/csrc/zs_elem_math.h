// Per-element arithmetic of the Normal and Bernoulli families of the main library, in float and in double: ONE definition of
// every expression the kernels of libzs_hip.so evaluate per element (zs_normal.hip, zs_bernoulli.hip, zs_sample_tile.h,
// zs_iwpersist.h, zs_logjoint.hip, zs_f64.hip, zs_locscale.hip).  The kernel files only schedule.  Free functions overloaded or
// templated on the precision; everything is __host__ __device__ like zs_common.h's primitives, so
// tests/host_math/zs_host_math.hip runs the same code on the host under AddressSanitizer + UndefinedBehaviorSanitizer.
// float: the gfx950 fast instructions (v_log_f32 / v_exp_f32 / v_rcp_f32, 1 ulp); double: libm-grade.
#pragma once
#include "zs_common.h"

#define ZS_NEG_HALF_LOG_2PI_D (-0.91893853320467274178)   // -0.5*log(2*pi), normal.py:122
#define ZS_BERN_EPS 1e-8f                                 // bernoulli.py:94
#define ZS_BERN_EPS_D 1e-8

namespace zs {

// ---------------------------------------------------------------- location-scale sample
// round-to-nearest mul / add that the compiler may not contract into an FMA: the sample z = mean + std * eps must round
// twice like the reference's separate mul and add (normal.py:105, logistic.py:66, uniform.py:70) so that z is bit-identical
// for identical eps.
template <typename T>
ZS_HD T mul_add_2round(T m, T s, T e) {
#pragma clang fp contract(off)   // HIP's __fmul_rn/__fadd_rn are plain * and + and would still fuse
  const T prod = s * e;
  return m + prod;
}

// `sigma` operand given as log(sigma) (Normal(logstd=...), normal.py:56: std = exp(logstd)): the kernels form sigma
// themselves instead of the caller launching an exp (and a multiply in backward).  Precise expf / exp: it runs once per
// parameter, not per particle.  d/d logstd = sigma * d/d sigma.
ZS_HD float sigma_of(float v, bool is_logstd) { return is_logstd ? expf(v) : v; }
ZS_HD double sigma_of(double v, bool is_logstd) { return is_logstd ? exp(v) : v; }
ZS_HD float4 sigma_of(float4 v, bool is_logstd) {
  if (is_logstd) { v.x = expf(v.x); v.y = expf(v.y); v.z = expf(v.z); v.w = expf(v.w); }
  return v;
}

// ---------------------------------------------------------------- Normal
// log(sigma) and sigma^-2 (normal.py:121,123: precision = exp(-2 logstd)); float: one v_log_f32 serves both
ZS_HD void normal_parts(float s, float& logstd, float& prec) {
  const float l2 = log2_fast(s);
  logstd = l2 * ZS_LN2;
  prec = exp2_fast(-2.0f * l2);
}
ZS_HD void normal_parts(double s, double& logstd, double& prec) {
  logstd = log(s);
  prec = exp(-2.0 * logstd);
}
// log-density term of one element given d = x - mean, log(sigma) and prec = sigma^-2
// (normal.py:121-124: c - logstd - 0.5 * precision * (x - mean)^2)
ZS_HD float normal_term(float d, float logstd, float prec) { return (ZS_NEG_HALF_LOG_2PI - logstd) - 0.5f * prec * (d * d); }
ZS_HD double normal_term(double d, double logstd, double prec) { return (ZS_NEG_HALF_LOG_2PI_D - logstd) - 0.5 * prec * (d * d); }
// ... of x under (mu, sigma): the two together
template <typename T>
ZS_HD T normal_lp(T x, T mu, T sigma) {
  T logstd, prec;
  normal_parts(sigma, logstd, prec);
  return normal_term(x - mu, logstd, prec);
}
// g times d term / d (x, mu, sigma operand); `sg` is the operand as given (sigma, or log sigma when `ls`):
// d/d logstd = sigma * d/d sigma
template <typename T>
ZS_HD void normal_partials(T x, T mu, T sg, T g, bool ls, T& gx, T& gm, T& gs) {
  sg = sigma_of(sg, ls);
  T logstd, prec;
  normal_parts(sg, logstd, prec);
  const T d = x - mu;
  const T t = g * prec * d;
  gx = -t;
  gm = t;
  const T v = g * (prec * d * d - (T)1);
  gs = ls ? v : v / sg;
}

// ---------------------------------------------------------------- Bernoulli
// term in log2 units (bernoulli.py:94); caller multiplies the row sum by ln 2
ZS_HD float bern_lp2_term(float p, float x) {
  float a = log2_fast(p + ZS_BERN_EPS);
  float b = log2_fast((1.0f - p) + ZS_BERN_EPS);
  return x * a + (1.0f - x) * b;
}
// the same term in natural-log units, element by element
ZS_HD float bern_term(float p, float x) { return bern_lp2_term(p, x) * ZS_LN2; }
ZS_HD double bern_term(double p, double x) { return x * log(p + ZS_BERN_EPS_D) + (1.0 - x) * log((1.0 - p) + ZS_BERN_EPS_D); }
// The same term for one 16-byte piece (four elements) in PACKED fp32 arithmetic (v_pk_add / v_pk_mul / v_pk_fma_f32: two elements
// per instruction), accumulated pairwise into `acc`: per element 2.5 full-rate instructions + the two logarithms instead of 7 + 2.
// The kernels that give a workgroup a fixed share of the rows (IW1) are bound by exactly this arithmetic.  `omx` = 1 - x.
__device__ __forceinline__ void bern_piece_acc(const float4& p, const float4& x, const float4& omx, zs_f2v& acc) {
  const zs_f2v eps = {ZS_BERN_EPS, ZS_BERN_EPS}, one = {1.0f, 1.0f};
  const zs_f2v p0 = {p.x, p.y}, p1 = {p.z, p.w};
  const zs_f2v a0 = p0 + eps, a1 = p1 + eps;
  const zs_f2v b0 = (one - p0) + eps, b1 = (one - p1) + eps;
  const zs_f2v la0 = {log2_fast(a0.x), log2_fast(a0.y)}, la1 = {log2_fast(a1.x), log2_fast(a1.y)};
  const zs_f2v lb0 = {log2_fast(b0.x), log2_fast(b0.y)}, lb1 = {log2_fast(b1.x), log2_fast(b1.y)};
  const zs_f2v x0 = {x.x, x.y}, x1 = {x.z, x.w}, o0 = {omx.x, omx.y}, o1 = {omx.z, omx.w};
  acc += __builtin_elementwise_fma(o0, lb0, x0 * la0);
  acc += __builtin_elementwise_fma(o1, lb1, x1 * la1);
}
// The same piece when every x of the row is exactly 0 or 1 (binarised observations: the examples' data): with s = 2x - 1 and
// c = 1 - x the selected argument is fma(p, s, c) -- p for x = 1, 1 - p (rounded as above) for x = 0 -- and the term is ONE
// logarithm: x * la + (1 - x) * lb has a factor exactly 1 and a factor exactly 0.  Bit-identical to bern_piece_acc for every p
// whose two arguments are positive (any p in [0, 1]); for an invalid p (outside [-1e-8, 1 + 1e-8]) the general form returns NaN
// through 0 * log(negative) where this one does not evaluate the other branch.
__device__ __forceinline__ void bern_piece_acc_bits(const float4& p, const float4& s, zs_f2v& acc) {
  const zs_f2v eps = {ZS_BERN_EPS, ZS_BERN_EPS}, half = {0.5f, 0.5f}, mhalf = {-0.5f, -0.5f};
  const zs_f2v p0 = {p.x, p.y}, p1 = {p.z, p.w}, s0 = {s.x, s.y}, s1 = {s.z, s.w};
  const zs_f2v c0 = __builtin_elementwise_fma(s0, mhalf, half), c1 = __builtin_elementwise_fma(s1, mhalf, half);     // 1 - x, exactly
  const zs_f2v a0 = __builtin_elementwise_fma(p0, s0, c0) + eps, a1 = __builtin_elementwise_fma(p1, s1, c1) + eps;
  const zs_f2v l0 = {log2_fast(a0.x), log2_fast(a0.y)}, l1 = {log2_fast(a1.x), log2_fast(a1.y)};
  acc += l0;
  acc += l1;
}
// ... with s = 2x - 1 AND c = 1 - x handed in (both parked in LDS once per datapoint by the persistent fused kernel): the same bits
// for rows of 0s and 1s, two packed instructions fewer per piece.  (s = 0, c = 1 makes the piece contribute log 1 = 0: padding.)
__device__ __forceinline__ void bern_piece_acc_bits2(const float4& p, const float4& s, const float4& c, zs_f2v& acc) {
  const zs_f2v eps = {ZS_BERN_EPS, ZS_BERN_EPS};
  const zs_f2v p0 = {p.x, p.y}, p1 = {p.z, p.w}, s0 = {s.x, s.y}, s1 = {s.z, s.w}, c0 = {c.x, c.y}, c1 = {c.z, c.w};
  const zs_f2v a0 = __builtin_elementwise_fma(p0, s0, c0) + eps, a1 = __builtin_elementwise_fma(p1, s1, c1) + eps;
  const zs_f2v l0 = {log2_fast(a0.x), log2_fast(a0.y)}, l1 = {log2_fast(a1.x), log2_fast(a1.y)};
  acc += l0;
  acc += l1;
}
// Gradient of that term w.r.t. p for one 16-byte piece, times the row gradient g, in packed fp32 arithmetic:
//   g * (x / (p + eps) - (1 - x) / ((1 - p) + eps))            [LOGITS: p = sigmoid(l), result times p (1 - p)]
// 3.5 packed instructions + two reciprocals per element instead of ~9 + 2: K3's backward stalls on instruction issue for half
// of its wave cycles (SQ_WAIT_INST_ANY 0.50 at 6.6 GB, 0.59 in IW1's merged backward; profiles/r04_pmc_*.json).
template <bool LOGITS>
__device__ __forceinline__ float4 bern_piece_grad(const float4& pl, const float4& x, float g) {
  const zs_f2v eps = {ZS_BERN_EPS, ZS_BERN_EPS}, one = {1.0f, 1.0f}, gg = {g, g};
  zs_f2v p0 = {pl.x, pl.y}, p1 = {pl.z, pl.w};
  if (LOGITS) {
    p0.x = rcp_fast(1.0f + exp_fast(-p0.x)); p0.y = rcp_fast(1.0f + exp_fast(-p0.y));
    p1.x = rcp_fast(1.0f + exp_fast(-p1.x)); p1.y = rcp_fast(1.0f + exp_fast(-p1.y));
  }
  const zs_f2v q0 = one - p0, q1 = one - p1;
  const zs_f2v a0 = p0 + eps, a1 = p1 + eps, b0 = q0 + eps, b1 = q1 + eps;
  const zs_f2v ra0 = {rcp_fast(a0.x), rcp_fast(a0.y)}, ra1 = {rcp_fast(a1.x), rcp_fast(a1.y)};
  const zs_f2v rb0 = {rcp_fast(b0.x), rcp_fast(b0.y)}, rb1 = {rcp_fast(b1.x), rcp_fast(b1.y)};
  const zs_f2v x0 = {x.x, x.y}, x1 = {x.z, x.w};
  zs_f2v t0 = __builtin_elementwise_fma(x0 - one, rb0, x0 * ra0);          // x ra - (1 - x) rb
  zs_f2v t1 = __builtin_elementwise_fma(x1 - one, rb1, x1 * ra1);
  t0 = gg * t0;
  t1 = gg * t1;
  if (LOGITS) {
    t0 = t0 * p0 * q0;
    t1 = t1 * p1 * q1;
  }
  return make_float4(t0.x, t0.y, t1.x, t1.y);
}
// torch.sigmoid: 1 / (1 + exp(-l)), bernoulli.py:50.  (sigmoid_fast: the float form by name, for the fp32-only kernels.)
ZS_HD float sigmoid_fast(float l) { return rcp_fast(1.0f + exp_fast(-l)); }
ZS_HD float sigmoid_any(float l) { return sigmoid_fast(l); }
ZS_HD double sigmoid_any(double l) { return 1.0 / (1.0 + exp(-l)); }
// d/dp of x*log(p+e) + (1-x)*log((1-p)+e)
ZS_HD float bern_dp(float p, float x) {
  return x * rcp_fast(p + ZS_BERN_EPS) - (1.0f - x) * rcp_fast((1.0f - p) + ZS_BERN_EPS);
}
ZS_HD double bern_dp(double p, double x) { return x / (p + ZS_BERN_EPS_D) - (1.0 - x) / ((1.0 - p) + ZS_BERN_EPS_D); }
// d/dx of the same = log(p+e) - log((1-p)+e): the gradient w.r.t. the observation (bernoulli.py:94)
ZS_HD float log_ratio_any(float p) { return (log2_fast(p + ZS_BERN_EPS) - log2_fast((1.0f - p) + ZS_BERN_EPS)) * ZS_LN2; }
ZS_HD double log_ratio_any(double p) { return log(p + ZS_BERN_EPS_D) - log((1.0 - p) + ZS_BERN_EPS_D); }

}  // namespace zs
