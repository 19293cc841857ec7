// The per-element arithmetic of the chain diagnostics (include/zs_diag.h): the three passes over one element's strided series
// (chain means, centred squares, one pair of autocovariance lags) and Geyer's initial monotone sequence.  __host__ __device__:
// zs_diag.hip gives every lane one element, tests/host_math/zs_diag_host_math.hip runs the same functions on the host under
// AddressSanitizer + UndefinedBehaviorSanitizer.  Every sum is a double, accumulated in ascending t, then ascending m, with the
// explicit fma of zs_flat_math.h: the bits depend on the values alone, not on strides, alignment, grid or build.
#pragma once
#include <math.h>
#include <stdint.h>

#include "zs_flat_math.h"

#define ZS_DIAG_THREADS 256
#define ZS_DIAG_KEPT 16          // chain means a lane keeps; a chain beyond them has its mean formed again where it is needed

namespace zs {

// One element's view of the operand: draw t of chain c at x[t st + c sc].  With `split`, chain m < C is the first N draws of
// chain m and chain m >= C the last N draws of chain m - C.
template <typename T>
struct DiagSeries {
  const T* x;          // already offset by the element
  int64_t st, sc;
  int64_t T_, C, N, M;
};

template <typename T>
ZS_HD DiagSeries<T> diag_series(const T* x, int64_t st, int64_t sc, int64_t T_, int64_t C, int split, int64_t e) {
  DiagSeries<T> s;
  s.x = x + e;
  s.st = st;
  s.sc = sc;
  s.T_ = T_;
  s.C = C;
  s.N = split ? T_ / 2 : T_;
  s.M = split ? 2 * C : C;
  return s;
}

// the first draw of chain m
template <typename T>
ZS_HD const T* diag_chain(const DiagSeries<T>& s, int64_t m) {
  return m < s.C ? s.x + m * s.sc : s.x + (m - s.C) * s.sc + (s.T_ - s.N) * s.st;
}

// pass 1 of one chain: the plain sum over N, in ascending t
template <typename T>
ZS_HD double diag_chain_mean(const DiagSeries<T>& s, int64_t m) {
  const T* p = diag_chain(s, m);
  double sum = 0.0;
#pragma unroll 4
  for (int64_t t = 0; t < s.N; ++t) sum += (double)p[t * s.st];
  return sum / (double)s.N;
}

// The chain means of one element: the first ZS_DIAG_KEPT are kept, the others are formed again on demand -- the same loop over
// the same values, hence the same bits.
struct DiagMeans {
  double kept[ZS_DIAG_KEPT];
};
template <typename T>
ZS_HD double diag_mean_of(const DiagSeries<T>& s, const DiagMeans& mu, int64_t m) {
  return m < ZS_DIAG_KEPT ? mu.kept[m] : diag_chain_mean(s, m);
}

// pass 2 of one chain: sum_t (x_t - mean)^2, centred
template <typename T>
ZS_HD double diag_chain_sumsq(const DiagSeries<T>& s, int64_t m, double mean) {
  const T* p = diag_chain(s, m);
  double acc = 0.0;
#pragma unroll 4
  for (int64_t t = 0; t < s.N; ++t) {
    const double d = (double)p[t * s.st] - mean;
    acc = flat_fma(d, d, acc);
  }
  return acc;
}

// One chain's share of a pair of lags l0 = 2k, l1 = 2k + 1 <= N - 1: g0 = sum_{t < N - l0} d_t d_{t + l0} and
// g1 = sum_{t < N - l1} d_t d_{t + l1}, each in ascending t.  d_{t + l0} of one step is d_{t + l1} of the step before it, so
// a step loads two draws.
template <typename T>
ZS_HD void diag_chain_lag_pair(const DiagSeries<T>& s, int64_t m, double mean, int64_t l0, double& g0, double& g1) {
  const T* p = diag_chain(s, m);
  const int64_t l1 = l0 + 1, n1 = s.N - l1;
  double a0 = 0.0, a1 = 0.0;
  double b = (double)p[l0 * s.st] - mean;
#pragma unroll 4
  for (int64_t t = 0; t < n1; ++t) {
    const double a = (double)p[t * s.st] - mean;
    const double c = (double)p[(t + l1) * s.st] - mean;
    a0 = flat_fma(a, b, a0);
    a1 = flat_fma(a, c, a1);
    b = c;
  }
  a0 = flat_fma((double)p[n1 * s.st] - mean, b, a0);          // t = N - l0 - 1: the last product of the even lag
  g0 = a0;
  g1 = a1;
}

// one chain's autocovariance sum at a single lag l <= N - 1 (the autocorrelation curve)
template <typename T>
ZS_HD double diag_chain_lag(const DiagSeries<T>& s, int64_t m, double mean, int64_t l) {
  const T* p = diag_chain(s, m);
  double acc = 0.0;
#pragma unroll 4
  for (int64_t t = 0; t < s.N - l; ++t) acc = flat_fma((double)p[t * s.st] - mean, (double)p[(t + l) * s.st] - mean, acc);
  return acc;
}

// What passes 1 and 2 leave: everything but the lag loop.
struct DiagMoments {
  double mean, W, BN, var_plus;
  bool finite;          // W is finite: no draw that entered is NaN or infinite
};

template <typename T>
ZS_HD DiagMoments diag_moments(const DiagSeries<T>& s, DiagMeans& mu) {
  const double N = (double)s.N, M = (double)s.M;
  double msum = 0.0, wsum = 0.0;
  for (int64_t m = 0; m < s.M; ++m) {
    const double mean = diag_chain_mean(s, m);
    if (m < ZS_DIAG_KEPT) mu.kept[m] = mean;
    msum += mean;
    wsum += diag_chain_sumsq(s, m, mean) / (N - 1.0);
  }
  DiagMoments r;
  r.mean = msum / M;
  r.W = wsum / M;
  double bsum = 0.0;
  for (int64_t m = 0; m < s.M; ++m) {
    const double d = diag_mean_of(s, mu, m) - r.mean;
    bsum = flat_fma(d, d, bsum);
  }
  r.BN = s.M > 1 ? bsum / (M - 1.0) : 0.0;
  r.var_plus = (N - 1.0) / N * r.W + r.BN;
  r.finite = (r.W - r.W) == 0.0;
  return r;
}

// rho_l of one lag from the chains' sums: gsum = sum_m (g_{l,m} / N)
ZS_HD double diag_rho(double gsum, double M, double W, double var_plus) { return 1.0 - (W - gsum / M) / var_plus; }

struct DiagEss {
  double tau, ess;
  int lags, capped;
};

// Geyer's initial monotone sequence over pairs of lags up to Lcap, then the effective sample size.
template <typename T>
ZS_HD DiagEss diag_geyer(const DiagSeries<T>& s, const DiagMeans& mu, const DiagMoments& mo, int64_t max_lag) {
  const double N = (double)s.N, M = (double)s.M;
  const int64_t Lcap = (max_lag < 0 || max_lag > s.N - 1) ? s.N - 1 : max_lag;
  DiagEss r;
  double tau = -1.0, prev = INFINITY;
  int64_t k = 0;
  r.capped = 1;
  for (; 2 * k + 1 <= Lcap; ++k) {
    double s0 = 0.0, s1 = 0.0;
    for (int64_t m = 0; m < s.M; ++m) {
      double g0, g1;
      diag_chain_lag_pair(s, m, diag_mean_of(s, mu, m), 2 * k, g0, g1);
      s0 += g0 / N;
      s1 += g1 / N;
    }
    double P = diag_rho(s0, M, mo.W, mo.var_plus) + diag_rho(s1, M, mo.W, mo.var_plus);
    if (!(P > 0.0)) {
      r.capped = 0;
      break;
    }
    if (prev < P) P = prev;
    prev = P;
    tau += 2.0 * P;
  }
  const double floor_ = 1.0 / log10(M * N);
  if (!(tau > floor_)) tau = floor_;
  r.tau = tau;
  r.ess = M * N / tau;
  r.lags = (int)(2 * k);
  return r;
}

// One element of zs_diag_summary: any output may be NULL; the lag loop runs only when ess, lags or capped is asked for.
template <typename T>
ZS_HD void diag_summary_element(const T* x, int64_t st, int64_t sc, int64_t T_, int64_t C, int split, int64_t max_lag, int64_t e,
                                T* mean, T* var_plus, T* rhat, T* ess, int32_t* lags, int32_t* capped) {
  const DiagSeries<T> s = diag_series(x, st, sc, T_, C, split, e);
  DiagMeans mu;
  const DiagMoments mo = diag_moments(s, mu);
  const bool live = mo.finite && mo.W != 0.0;          // a non-finite draw, or a constant series: no ratio exists
  if (mean) mean[e] = mo.finite ? (T)mo.mean : (T)NAN;
  if (var_plus) var_plus[e] = mo.finite ? (T)mo.var_plus : (T)NAN;
  if (rhat) rhat[e] = live ? (T)sqrt(mo.var_plus / mo.W) : (T)NAN;
  if (!ess && !lags && !capped) return;
  if (!live) {
    if (ess) ess[e] = (T)NAN;
    if (lags) lags[e] = 0;
    if (capped) capped[e] = 0;
    return;
  }
  const DiagEss r = diag_geyer(s, mu, mo, max_lag);
  if (ess) ess[e] = (T)r.ess;
  if (lags) lags[e] = r.lags;
  if (capped) capped[e] = r.capped;
}

// One element of zs_diag_autocorr: acf[l, c, e] = g_{l,c} / g_{0,c}, l = 0 .. L, per unsplit chain.
template <typename T>
ZS_HD void diag_autocorr_element(const T* x, int64_t st, int64_t sc, int64_t T_, int64_t C, int64_t E, int64_t L, int64_t e, T* acf) {
  const DiagSeries<T> s = diag_series(x, st, sc, T_, C, 0, e);
  for (int64_t c = 0; c < C; ++c) {
    const double mean = diag_chain_mean(s, c);
    const double g0 = diag_chain_lag(s, c, mean, 0) / (double)T_;
    for (int64_t l = 0; l <= L; ++l) {
      const double g = l == 0 ? g0 : diag_chain_lag(s, c, mean, l) / (double)T_;
      acf[(l * C + c) * E + e] = (T)(g / g0);
    }
  }
}

// ---------------------------------------------------------------- argument checks (host arithmetic, shared by both entry points)
// the strides step over the extents: the element axis (E, stride 1) innermost, then the two outer axes in either order
ZS_HD bool diag_strides_ok(int64_t st, int64_t sc, int64_t T_, int64_t C, int64_t E) {
  if (C == 1) return T_ == 1 || st >= E;          // (one chain: sc is never stepped)
  if (T_ == 1) return sc >= E;
  if (st >= sc) return sc >= E && sc <= INT64_MAX / C && st >= sc * C;
  return st >= E && st <= INT64_MAX / T_ && sc >= st * T_;
}

}  // namespace zs
