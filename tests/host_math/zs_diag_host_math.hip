// The per-element arithmetic of the chain diagnostics (csrc/zs_diag_math.h: __host__ __device__) compiled for the HOST and run
// under AddressSanitizer + UndefinedBehaviorSanitizer (tests/test_diag_host_math.py):
//     hipcc -x hip --cuda-host-only -Xarch_host -fsanitize=address,undefined ...
// (1) the three passes and the Geyer loop -- the whole per-lane body of zs_diag_summary -- over exactly-sized heap arrays against
//     long double, for every (T, C, split, max_lag) of tests/test_diag_kernel.py, as a [T, C, E] and as a [C, T, E] stack (the
//     same bits), with every output and with each output alone;
// (2) N = 2, a cap at an odd and at an even Lcap, more chains than a lane keeps means of, a series with a NaN, one with an
//     infinity and a constant one next to ordinary neighbours;
// (3) the autocorrelation curve for L = 0, 1, T - 1 against long double, its array exactly sized;
// (4) the stride check of the entry points.
// Prints "diag host math ok: N checks".
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

#include "../../zhusuan-pytorch_amd/csrc/zs_diag_math.h"
#include "zs_host_check.h"

using namespace zs;

template <typename T> static ld unit() { return sizeof(T) == 4 ? ldexpl(1.0L, -24) : ldexpl(1.0L, -53); }
static const ld V = ldexpl(1.0L, -53);

static const int Ts[] = {4, 5, 8, 9, 64, 65, 257};
static const int Cs[] = {1, 2, 3};
static const int MaxLags[] = {-1, 1, 6};

template <typename T> static T* heap(size_t n, T fill) {          // exactly sized: a step outside is the sanitizer's
  T* p = (T*)malloc(sizeof(T) * (n ? n : 1));
  for (size_t i = 0; i < n; ++i) p[i] = fill;
  return p;
}

// AR(1) draws [T, C, E], float32-representable: phi from -0.5 to 0.9 over the elements, the last chain shifted
static std::vector<float> draws(int T_, int C, int E) {
  std::vector<float> x((size_t)T_ * C * E);
  for (int c = 0; c < C; ++c) for (int e = 0; e < E; ++e) {
    const float phi = E > 1 ? -0.5f + 1.4f * (float)e / (float)(E - 1) : 0.2f;
    float prev = 0.0f;
    for (int t = 0; t < T_; ++t) {
      prev = phi * prev + (float)normal01();
      x[((size_t)t * C + c) * E + e] = prev + (c == C - 1 ? 0.25f : 0.0f);
    }
  }
  return x;
}

struct Truth { ld mean, varp, rhat, ess, tau, W, absx, kappa, gamma0, min_abs_p; int lags, capped; bool finite, live; };

// the header's steps 1 - 8 in long double for element e of a [T, C, E] stack
static Truth truth_of(const std::vector<float>& x, int T_, int C, int E, int e, int split, int64_t max_lag) {
  const int N = split ? T_ / 2 : T_, M = split ? 2 * C : C;
  std::vector<std::vector<ld>> d(M, std::vector<ld>(N));
  std::vector<ld> mean_m(M);
  Truth r;
  r.finite = true;
  ld absx = 0, W = 0, msum = 0, kmax = 0, g0 = 0;
  for (int m = 0; m < M; ++m) {
    const int c = m < C ? m : m - C, t0 = m < C ? 0 : T_ - N;
    ld s = 0;
    for (int t = 0; t < N; ++t) {
      const ld v = x[((size_t)(t0 + t) * C + c) * E + e];
      d[m][t] = v;
      s += v;
      absx += fabsl(v);
      if (!isfinite((double)v)) r.finite = false;
    }
    mean_m[m] = s / N;
    ld ss = 0;
    for (int t = 0; t < N; ++t) { d[m][t] -= mean_m[m]; ss += d[m][t] * d[m][t]; }
    W += ss / (N - 1);
    msum += mean_m[m];
    g0 += ss / N;
    if (ss > kmax) kmax = ss;
  }
  r.mean = msum / M;
  r.W = W / M;
  ld BN = 0;
  for (int m = 0; m < M; ++m) BN += (mean_m[m] - r.mean) * (mean_m[m] - r.mean);
  BN = M > 1 ? BN / (M - 1) : 0;
  r.varp = (ld)(N - 1) / N * r.W + BN;
  r.live = r.finite && r.W != 0;
  r.absx = absx / ((ld)M * N);
  r.gamma0 = g0 / M;
  r.kappa = r.live ? kmax / (N * r.W) : 0;
  r.rhat = r.live ? sqrtl(r.varp / r.W) : NAN;
  r.lags = 0;
  r.capped = r.live ? 1 : 0;
  r.min_abs_p = INFINITY;
  r.tau = -1;
  r.ess = NAN;
  if (!r.live) return r;
  const int64_t Lcap = (max_lag < 0 || max_lag > N - 1) ? N - 1 : max_lag;
  ld prev = INFINITY;
  int k = 0;
  for (; 2 * k + 1 <= Lcap; ++k) {
    ld P = 0;
    for (int l = 2 * k; l <= 2 * k + 1; ++l) {
      ld gs = 0;
      for (int m = 0; m < M; ++m) {
        ld g = 0;
        for (int t = 0; t + l < N; ++t) g += d[m][t] * d[m][t + l];
        gs += g / N;
      }
      P += 1 - (r.W - gs / M) / r.varp;
    }
    if (fabsl(P) < r.min_abs_p) r.min_abs_p = fabsl(P);
    if (!(P > 0)) { r.capped = 0; break; }
    if (prev < P) P = prev;
    prev = P;
    r.tau += 2 * P;
  }
  const ld fl = 1 / log10l((ld)M * N);
  if (!(r.tau > fl)) r.tau = fl;
  r.ess = (ld)M * N / r.tau;
  r.lags = 2 * k;
  return r;
}

template <typename T> struct Out { T mean, varp, rhat, ess; int32_t lags, capped; };

// every element of one case through diag_summary_element, outputs exactly sized; `which` < 0: all outputs, else that one alone
template <typename T>
static std::vector<Out<T>> run(const T* x, int64_t st, int64_t sc, int T_, int C, int E, int split, int64_t max_lag, int which) {
  T* f[4];
  int32_t* g[2];
  for (int i = 0; i < 4; ++i) f[i] = (which < 0 || which == i) ? heap<T>(E, (T)777) : nullptr;
  for (int i = 0; i < 2; ++i) g[i] = (which < 0 || which == 4 + i) ? heap<int32_t>(E, 777) : nullptr;
  for (int e = 0; e < E; ++e) diag_summary_element<T>(x, st, sc, T_, C, split, max_lag, e, f[0], f[1], f[2], f[3], g[0], g[1]);
  std::vector<Out<T>> out(E);
  for (int e = 0; e < E; ++e)
    out[e] = Out<T>{f[0] ? f[0][e] : (T)0, f[1] ? f[1][e] : (T)0, f[2] ? f[2][e] : (T)0, f[3] ? f[3][e] : (T)0, g[0] ? g[0][e] : 0, g[1] ? g[1][e] : 0};
  for (int i = 0; i < 4; ++i) free(f[i]);
  for (int i = 0; i < 2; ++i) free(g[i]);
  return out;
}

template <typename T> static bool same(T a, T b) { return memcmp(&a, &b, sizeof(T)) == 0; }

template <typename T>
static void check_case(const std::vector<float>& x32, int T_, int C, int E, int split, int64_t max_lag) {
  const ld u = unit<T>();
  const int N = split ? T_ / 2 : T_, M = split ? 2 * C : C;
  const size_t n = (size_t)T_ * C * E;
  T* tce = heap<T>(n, 0);
  T* cte = heap<T>(n, 0);
  for (int t = 0; t < T_; ++t) for (int c = 0; c < C; ++c) for (int e = 0; e < E; ++e)
    tce[((size_t)t * C + c) * E + e] = cte[((size_t)c * T_ + t) * E + e] = (T)x32[((size_t)t * C + c) * E + e];
  const std::vector<Out<T>> a = run<T>(tce, (int64_t)C * E, E, T_, C, E, split, max_lag, -1);
  const std::vector<Out<T>> b = run<T>(cte, E, (int64_t)T_ * E, T_, C, E, split, max_lag, -1);
  for (int w = 0; w < 6; ++w) {
    const std::vector<Out<T>> one = run<T>(tce, (int64_t)C * E, E, T_, C, E, split, max_lag, w);
    bool ok = true;
    for (int e = 0; e < E; ++e) {
      const Out<T>&o = one[e], &f = a[e];
      ok = ok && (w == 0 ? same(o.mean, f.mean) : w == 1 ? same(o.varp, f.varp) : w == 2 ? same(o.rhat, f.rhat) : w == 3 ? same(o.ess, f.ess)
                         : w == 4 ? o.lags == f.lags : o.capped == f.capped);
    }
    expect(ok, "an output alone equals the same output among the others", w, T_);
  }
  for (int e = 0; e < E; ++e) {
    expect(same(a[e].mean, b[e].mean) && same(a[e].varp, b[e].varp) && same(a[e].rhat, b[e].rhat) && same(a[e].ess, b[e].ess) &&
           a[e].lags == b[e].lags && a[e].capped == b[e].capped, "the two stack orders give the same bits", T_, C);
    const Truth r = truth_of(x32, T_, C, E, e, split, max_lag);
    if (!r.finite) {
      expect(isnan((double)a[e].mean) && isnan((double)a[e].varp) && isnan((double)a[e].rhat) && isnan((double)a[e].ess) && a[e].lags == 0 &&
             a[e].capped == 0, "a non-finite draw gives NaN and no lags", (double)a[e].mean, NAN);
      continue;
    }
    const ld nm = (ld)N * M;
    expect(fabsl((ld)a[e].mean - r.mean) <= u * fabsl(r.mean) + nm * V * r.absx, "mean against long double", (double)a[e].mean, (double)r.mean);
    if (!r.live) {
      expect(isnan((double)a[e].rhat) && isnan((double)a[e].ess) && a[e].lags == 0 && a[e].capped == 0 && a[e].varp == (T)0,
             "a constant series has no ratio", (double)a[e].rhat, NAN);
      continue;
    }
    const ld rel = 4 * u + 4 * nm * V * r.kappa;
    expect(fabsl((ld)a[e].varp - r.varp) <= rel * r.varp, "var+ against long double", (double)a[e].varp, (double)r.varp);
    expect(fabsl((ld)a[e].rhat - r.rhat) <= rel * r.rhat, "rhat against long double", (double)a[e].rhat, (double)r.rhat);
    // the margin of the stop decision, as tests/test_diag_kernel.py asserts it: no element is left out
    expect(r.min_abs_p >= 1e-9L, "every pair sum examined is at least 1e-9 away from zero", (double)r.min_abs_p, 1e-9);
    expect(a[e].lags == r.lags && a[e].capped == r.capped, "lags and capped exactly", a[e].lags, r.lags);
    const ld rel_ess = 4 * u + (r.lags + 2) * 4 * nm * V * r.gamma0 / (r.tau * r.varp);
    expect(fabsl((ld)a[e].ess - r.ess) <= rel_ess * r.ess, "ess against long double", (double)a[e].ess, (double)r.ess);
    expect(a[e].ess > (T)0 && (ld)a[e].ess <= nm * log10l(nm) * (1 + 2 * u), "0 < ess <= M N log10(M N)", (double)a[e].ess, (double)(nm * log10l(nm)));
  }
  free(tce); free(cte);
}

template <typename T>
static void check_autocorr(int T_, int C, int E) {
  const ld u = unit<T>();
  const std::vector<float> x32 = draws(T_, C, E);
  T* x = heap<T>(x32.size(), 0);
  for (size_t i = 0; i < x32.size(); ++i) x[i] = (T)x32[i];
  const int Ls[] = {0, 1, T_ - 1};
  for (int L : Ls) {
    T* acf = heap<T>((size_t)(L + 1) * C * E, (T)777);
    for (int e = 0; e < E; ++e) diag_autocorr_element<T>(x, (int64_t)C * E, E, T_, C, E, L, e, acf);
    for (int c = 0; c < C; ++c) for (int e = 0; e < E; ++e) {
      ld mean = 0;
      for (int t = 0; t < T_; ++t) mean += x32[((size_t)t * C + c) * E + e];
      mean /= T_;
      std::vector<ld> g(L + 1, 0);
      for (int l = 0; l <= L; ++l)
        for (int t = 0; t + l < T_; ++t) g[l] += (x32[((size_t)t * C + c) * E + e] - mean) * (x32[((size_t)(t + l) * C + c) * E + e] - mean);
      for (int l = 0; l <= L; ++l) {
        const ld want = g[l] / g[0], got = acf[((size_t)l * C + c) * E + e];
        expect(fabsl(got - want) <= 4 * u * fabsl(want) + 4 * (T_ + 2) * V, "acf against long double", (double)got, (double)want);
      }
    }
    free(acf);
  }
  free(x);
}

static void check_strides() {
  const int64_t T_ = 8, C = 2, E = 5;
  expect(diag_strides_ok(C * E, E, T_, C, E) && diag_strides_ok(E, T_ * E, T_, C, E), "the two dense stacks", 0, 0);
  expect(diag_strides_ok(C * E + 3, E + 1, T_, C, E) && diag_strides_ok(E + 2, T_ * (E + 2), T_, C, E), "padded stacks", 0, 0);
  expect(!diag_strides_ok(C * E, E - 1, T_, C, E) && !diag_strides_ok(C * E - 1, E, T_, C, E), "[T, C, E]: a short stride", 0, 0);
  expect(!diag_strides_ok(E - 1, T_ * E, T_, C, E) && !diag_strides_ok(E, T_ * E - 1, T_, C, E), "[C, T, E]: a short stride", 0, 0);
  expect(!diag_strides_ok(-C * E, E, T_, C, E) && !diag_strides_ok(C * E, -E, T_, C, E) && !diag_strides_ok(0, 0, T_, C, E), "negative or zero", 0, 0);
  expect(diag_strides_ok(E, 0, T_, 1, E) && diag_strides_ok(E, -7, T_, 1, E) && !diag_strides_ok(E - 1, 0, T_, 1, E), "one chain: sc is not looked at", 0, 0);
  expect(!diag_strides_ok(INT64_MAX, INT64_MAX / 2 + 1, T_, C, E) && !diag_strides_ok(INT64_MAX / 4, INT64_MAX, T_, C, E), "no overflow", 0, 0);
}

template <typename T>
static void check_all() {
  int i = 0;
  for (int T_ : Ts) for (int C : Cs) for (int split = 0; split < 2; ++split) for (int64_t ml : MaxLags) {
    const int E = 3 + (i++ % 3);
    check_case<T>(draws(T_, C, E), T_, C, E, split, ml);
  }
  check_case<T>(draws(2, 2, 3), 2, 2, 3, 0, -1);          // N = 2
  check_case<T>(draws(4, 1, 3), 4, 1, 3, 1, -1);          // N = 2 after the split
  check_case<T>(draws(64, 2, 2), 64, 2, 2, 0, 5);         // an odd Lcap: pairs (0, 1), (2, 3), (4, 5)
  check_case<T>(draws(64, 2, 2), 64, 2, 2, 0, 4);         // an even Lcap: lag 4 has no partner and does not enter
  check_case<T>(draws(64, 2, 2), 64, 2, 2, 0, 0);         // no pair at all: tau is its floor
  check_case<T>(draws(12, 11, 2), 12, 11, 2, 1, -1);      // M = 22 chains: more than ZS_DIAG_KEPT means
  std::vector<float> bad = draws(16, 2, 5);
  bad[(size_t)(7 * 2 + 1) * 5 + 1] = NAN;
  bad[(size_t)(3 * 2 + 0) * 5 + 3] = INFINITY;
  for (int t = 0; t < 16; ++t) for (int c = 0; c < 2; ++c) bad[(size_t)(t * 2 + c) * 5 + 2] = 1.5f;
  for (int split = 0; split < 2; ++split) check_case<T>(bad, 16, 2, 5, split, -1);
  check_autocorr<T>(4, 1, 3);
  check_autocorr<T>(65, 3, 2);
  check_autocorr<T>(257, 2, 3);
}

int main() {
  check_all<float>();
  check_all<double>();
  check_strides();
  return finish("diag host math ok");
}
