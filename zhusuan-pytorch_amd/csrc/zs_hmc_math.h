// Per-element arithmetic, index maps and the accept / step-size arithmetic of Hamiltonian Monte Carlo (zs_hmc.hip, C ABI:
// include/zs_hmc.h), __host__ __device__ like zs_mcmc_math.h so that the host-side sanitizer test
// (tests/host_math/zs_hmc_host_math.hip) runs the same code.  Every multiply-add of the leapfrog is an explicit fma, so that
// the vector and the element form of the kernel, and the host build, round alike.
#pragma once
#include <math.h>
#include "zs_common.h"
#include "zs_flat_math.h"          // flat_fma, flat_tensor_of and the element form's walk (flat_clamped_index, flat_element_live)
#include "../../include/zs_hmc.h"

namespace zs {

// eps is held in double; the element arithmetic uses it, and eps/2, rounded to T
template <typename T>
struct HmcStep { T eps, half; };
template <typename T>
ZS_HD HmcStep<T> hmc_step_of(double eps) {
  HmcStep<T> s;
  s.eps = (T)eps;
  s.half = (T)(0.5 * eps);
  return s;
}

// BEGIN   p0 = z;  p = p0 + (eps/2) g;  q = q0 + eps p;  returns p0^2 (the kinetic term, in T)
template <typename T>
ZS_HD T hmc_begin(T q0, T g, T z, const HmcStep<T>& s, T& q, T& p) {
  p = flat_fma(s.half, g, z);
  q = flat_fma(s.eps, p, q0);
  return z * z;
}
// STEP    p = p + eps g;  q = q + eps p
template <typename T>
ZS_HD void hmc_step(T& q, T& p, T g, const HmcStep<T>& s) {
  p = flat_fma(s.eps, g, p);
  q = flat_fma(s.eps, p, q);
}
// END     pL = p + (eps/2) g;  returns pL^2
template <typename T>
ZS_HD T hmc_end(T p, T g, const HmcStep<T>& s) {
  const T pl = flat_fma(s.half, g, p);
  return pl * pl;
}

// ---------------------------------------------------------------- decide, in double
ZS_HD bool hmc_finite(double x) { return x - x == 0.0; }       // false for NaN and +-inf
ZS_HD double hmc_delta_h(double logp0, double logp1, double k0, double k1) { return (logp1 - logp0) - (k1 - k0); }
ZS_HD double hmc_accept_prob(double dh) { return hmc_finite(dh) ? exp(dh < 0.0 ? dh : 0.0) : 0.0; }
ZS_HD bool hmc_accept(double dh, double u) { return hmc_finite(dh) && log(u) < dh; }

// the state block of include/zs_hmc.h
enum { HMC_EPS = 0, HMC_EPS_INIT, HMC_M, HMC_HBAR, HMC_LOG_EPS, HMC_LOG_EPSBAR, HMC_ABAR, HMC_NACC };

// the step-size update after a decide whose mean acceptance probability is abar
ZS_HD void hmc_adapt(double* st, double abar, int adapting, double delta, double gamma, double t0, double kappa) {
  if (adapting) {
    const double m = st[HMC_M] + 1.0;
    const double w = 1.0 / (m + t0);
    const double hbar = (1.0 - w) * st[HMC_HBAR] + w * (delta - abar);
    const double log_eps = log(10.0 * st[HMC_EPS_INIT]) - (sqrt(m) / gamma) * hbar;
    const double eta = pow(m, -kappa);
    st[HMC_M] = m;
    st[HMC_HBAR] = hbar;
    st[HMC_LOG_EPS] = log_eps;
    st[HMC_LOG_EPSBAR] = eta * log_eps + (1.0 - eta) * st[HMC_LOG_EPSBAR];
    st[HMC_EPS] = exp(log_eps);
  } else if (st[HMC_M] > 0.0) {
    st[HMC_EPS] = exp(st[HMC_LOG_EPSBAR]);
  }
}

// ---------------------------------------------------------------- index maps
// where flat element i lives: its tensor, its chain, and the flat index at which that chain's row of that tensor begins
struct HmcLoc {
  int s;
  int64_t off, chain, run_start;
};
ZS_HD HmcLoc hmc_locate(const int64_t* start, const int64_t* row, int n_tensors, int64_t i) {
  HmcLoc l;
  l.s = flat_tensor_of(start, n_tensors, i);
  l.off = i - start[l.s];
  int64_t r;
  divmod(l.off, row[l.s], l.chain, r);
  l.run_start = i - r;
  return l;
}

// tiles of ZS_HMC_TILE flat elements that `row` consecutive elements can touch
ZS_HD int64_t hmc_pieces(int64_t row) { return (row + ZS_HMC_TILE - 2) / ZS_HMC_TILE + 1; }
// tiles the row that begins at run_start does touch
ZS_HD int64_t hmc_pieces_of(int64_t run_start, int64_t row) {
  return (run_start + row - 1) / ZS_HMC_TILE - run_start / ZS_HMC_TILE + 1;
}
// key of an element inside tile `tile`: equal for the elements of one (tensor, chain), ascending with the flat index
ZS_HD int hmc_key(int64_t run_start, int64_t tile) {
  const int64_t t0 = tile * ZS_HMC_TILE;
  return run_start < t0 ? -1 : (int)(run_start - t0);
}
// slot of the partial of (chain, tensor with piece offset poff, tile) in a workspace with `slots` slots per chain
ZS_HD int64_t hmc_slot(int64_t chain, int64_t slots, int64_t poff, int64_t run_start, int64_t tile) {
  return chain * slots + poff + (tile - run_start / ZS_HMC_TILE);
}

}  // namespace zs
