// Per-element arithmetic and indexing of the stochastic-gradient MCMC update (zs_mcmc.hip, C ABI: include/zs_mcmc.h),
// __host__ __device__ like zs_common.h's helpers so that the host-side sanitizer test (tests/host_math/zs_mcmc_host_math.hip)
// runs the same code.  One function per kind; the formulas restate zhusuan/mcmc/SGLD.py:42-54,67-82 and SGHMC.py:25-56 of the
// reference.  Every multiply-add is written as an explicit fma, so that the vector and the element form of the kernel, and
// the host build, round alike: nothing is left for the compiler to contract or not.
#pragma once
#include <math.h>
#include "zs_common.h"
#include "zs_flat_math.h"          // flat_fma and the flat index maps (flat_tensor_of, flat_clamped_index, flat_element_live)
#include "../../include/zs_mcmc.h"

namespace zs {

ZS_HD float mcmc_sqrt(float x) { return sqrt_fast(x); }        // v_sqrt_f32, 1 ulp
ZS_HD double mcmc_sqrt(double x) { return __builtin_sqrt(x); }
ZS_HD float mcmc_rcp(float x) { return rcp_fast(x); }          // v_rcp_f32, 1 ulp
ZS_HD double mcmc_rcp(double x) { return 1.0 / x; }

// Scalars derived from the hyper-parameters: formed once per launch in double on the host, rounded to T.
//   SGLD        half_lr, sqrt_lr
//   PSGLD       half_lr, lr, decay, one_minus_decay, epsilon
//   SGHMC_PRE   sqrt_lr
//   SGHMC_POST  lr, damp = 1 - alpha (first order) or exp(-alpha/2) (second order), noise = sqrt(2 (alpha - beta) lr)
template <typename T>
struct McmcCoef {
  T half_lr, sqrt_lr, lr, decay, one_minus_decay, epsilon, damp, noise;
  int second_order, resample_v;
};

template <typename T>
__host__ inline McmcCoef<T> mcmc_coef(int kind, int flags, double lr, double decay, double epsilon, double alpha, double beta) {
  McmcCoef<T> c;
  c.half_lr = (T)(0.5 * lr);
  c.sqrt_lr = (T)sqrt(lr);
  c.lr = (T)lr;
  c.decay = (T)decay;
  c.one_minus_decay = (T)(1.0 - decay);
  c.epsilon = (T)epsilon;
  c.second_order = (flags & ZS_MCMC_SECOND_ORDER) ? 1 : 0;
  c.resample_v = (flags & ZS_MCMC_RESAMPLE_V) ? 1 : 0;
  c.damp = (T)(c.second_order ? exp(-0.5 * alpha) : 1.0 - alpha);
  c.noise = (T)(kind == ZS_MCMC_SGHMC_POST ? sqrt(2.0 * (alpha - beta) * lr) : 0.0);
  return c;
}

// SGLD.py:50-52   q' = q + (lr/2) g + sqrt(lr) z
template <typename T>
ZS_HD void mcmc_sgld(T& q, T g, T z, const McmcCoef<T>& c) {
  q = flat_fma(c.sqrt_lr, z, flat_fma(c.half_lr, g, q));
}

// SGLD.py:77-80   a' = decay a + (1 - decay) g^2;  G = 1 / (epsilon + sqrt(a'));  q' = q + (lr/2) G g + sqrt(lr G) z
template <typename T>
ZS_HD void mcmc_psgld(T& q, T& a, T g, T z, const McmcCoef<T>& c) {
  a = flat_fma(c.decay, a, c.one_minus_decay * (g * g));
  const T G = mcmc_rcp(c.epsilon + mcmc_sqrt(a));
  q = flat_fma(mcmc_sqrt(c.lr * G), z, flat_fma(c.half_lr * G, g, q));
}

// SGHMC.py:26-27,32-33,35-36 (before the gradient)   v' = resample_v ? sqrt(lr) z : v;  q' = second_order ? q + v'/2 : q
template <typename T>
ZS_HD void mcmc_sghmc_pre(T& q, T& v, T z, const McmcCoef<T>& c) {
  if (c.resample_v) v = c.sqrt_lr * z;
  if (c.second_order) q = flat_fma((T)0.5, v, q);
}

// SGHMC.py:47-48   v' = (1 - alpha) v + lr g + noise z;  q' = q + v'
// SGHMC.py:52-54   v' = d (d v + lr g + noise z);  q' = q + v'/2        (d = exp(-alpha/2))
template <typename T>
ZS_HD void mcmc_sghmc_post(T& q, T& v, T g, T z, const McmcCoef<T>& c) {
  const T t = flat_fma(c.noise, z, flat_fma(c.lr, g, c.damp * v));
  if (c.second_order) {
    v = c.damp * t;
    q = flat_fma((T)0.5, v, q);
  } else {
    v = t;
    q = q + v;
  }
}

template <typename T, int KIND>
ZS_HD void mcmc_apply(T& q, T& s, T g, T z, const McmcCoef<T>& c) {
  if (KIND == ZS_MCMC_SGLD) mcmc_sgld(q, g, z, c);
  else if (KIND == ZS_MCMC_PSGLD) mcmc_psgld(q, s, g, z, c);
  else if (KIND == ZS_MCMC_SGHMC_PRE) mcmc_sghmc_pre(q, s, z, c);
  else mcmc_sghmc_post(q, s, g, z, c);
}

// which operands a kind reads
ZS_HD bool mcmc_reads_grad(int kind) { return kind != ZS_MCMC_SGHMC_PRE; }
ZS_HD bool mcmc_has_state(int kind) { return kind != ZS_MCMC_SGLD; }
ZS_HD bool mcmc_draws(int kind, int flags) { return kind != ZS_MCMC_SGHMC_PRE || (flags & ZS_MCMC_RESAMPLE_V); }

}  // namespace zs
