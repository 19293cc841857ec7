// The arithmetic of the planar / Householder flow kernels (include/zs_nf.h, zs_nf.hip) and what they add to the lane-group map
// of zs_group_math.h: the LDS places of the layer inputs z_l, the place of a workgroup's partial sums, and the steps of a layer,
// of its backward and of the parameter chain.  __host__ __device__, so that tests/host_math/zs_nf_host_math.hip walks the same
// code on the host under the sanitizers.
#pragma once
#include <math.h>
#include "zs_group_math.h"

// one rounding per written operation: nothing here is contracted into an fma
#pragma clang fp contract(off)

namespace zs {

#define ZS_NF_MAX_DIM 64
#define ZS_NF_MAX_LAYERS 32
#define ZS_NF_THREADS 64            // a workgroup is ONE wave: its barriers are the wave's own
#define ZS_NF_MAX_WORKGROUPS 4096   // the grid cap; past it a workgroup walks row tiles
#define ZS_NF_FINISH_THREADS 512    // P1f: one workgroup, a wave per layer in turn (8 waves: 256 VGPRs each for the loads in flight)

ZS_HD float nf_tanh(float x) { return tanhf(x); }
ZS_HD double nf_tanh(double x) { return tanh(x); }
ZS_HD float nf_log(float x) { return logf(x); }
ZS_HD double nf_log(double x) { return log(x); }
ZS_HD float nf_exp(float x) { return expf(x); }
ZS_HD double nf_exp(double x) { return exp(x); }
ZS_HD float nf_log1p(float x) { return log1pf(x); }
ZS_HD double nf_log1p(double x) { return log1p(x); }
ZS_HD float nf_abs(float x) { return fabsf(x); }
ZS_HD double nf_abs(double x) { return fabs(x); }

// ---------------------------------------------------------------- lane groups and row tiles
// A group of G = group_lanes(D) consecutive lanes of one wave owns a row; lane pl.lane = i < D of the group owns component i
// (idle when i >= D).  The place and the row tiles of a workgroup are zs_group_math.h's, with ZS_NF_THREADS threads.
// workgroups for R >= 1 rows in groups of G lanes = the leading extent of the partials
ZS_HD int nf_workgroups(int64_t R, int G) { return group_workgroups(R, G, ZS_NF_THREADS, ZS_NF_MAX_WORKGROUPS); }

// LDS of a backward workgroup: lane `thread` keeps the input z_l of its row's layer l at nf_z_index (read back by the same lane);
// the group's tanh of layer l sits at nf_t_index (planar only).  Planar: uh[L D], c[L], t[L groups], z[L 64]; Householder: z[L 64].
ZS_HD int nf_z_index(int l, int thread) { return l * ZS_NF_THREADS + thread; }
ZS_HD int nf_t_index(int l, int grp, int groups) { return l * groups + grp; }
ZS_HD int64_t nf_planar_fwd_lds(int64_t D, int64_t L) { return L * D + L; }
ZS_HD int64_t nf_planar_bwd_lds(int64_t D, int64_t L, int G) { return L * D + L + L * (ZS_NF_THREADS / G) + L * ZS_NF_THREADS; }
ZS_HD int64_t nf_householder_bwd_lds(int64_t L) { return L * ZS_NF_THREADS; }

// partials T[n_wg, L, 2 D + 2]: per layer Guh[D], Gw[D], Gb, Gc
ZS_HD int64_t nf_partial_row(int64_t wg, int64_t l, int64_t D, int64_t L) { return (wg * L + l) * (2 * D + 2); }
ZS_HD int64_t nf_partial_guh(int64_t d) { return d; }
ZS_HD int64_t nf_partial_gw(int64_t d, int64_t D) { return D + d; }
ZS_HD int64_t nf_partial_gb(int64_t D) { return 2 * D; }
ZS_HD int64_t nf_partial_gc(int64_t D) { return 2 * D + 1; }

// ---------------------------------------------------------------- planar: parameter quantities
template <typename T>
ZS_HD T nf_softplus(T s) { return (s > (T)0 ? s : (T)0) + nf_log1p(nf_exp(-nf_abs(s))); }
// k = softplus(s) - 1 - s
template <typename T>
ZS_HD T nf_planar_k(T s) { return nf_softplus(s) - (T)1 - s; }
// uh_d = u_d + k w_d / n
template <typename T>
ZS_HD T nf_planar_uhat(T u, T w, T k, T n) { return u + (k * w) / n; }
// dk/ds = sigmoid(s) - 1 = -1 / (1 + exp(s)), the form without cancellation
template <typename T>
ZS_HD T nf_planar_dk(T s) { return (T)-1 / ((T)1 + nf_exp(s)); }

// ---------------------------------------------------------------- planar: a layer
template <typename T>
ZS_HD T nf_planar_t(T dot_wz, T b) { return nf_tanh(dot_wz + b); }
template <typename T>
ZS_HD T nf_planar_z(T z, T uh, T t) { return z + uh * t; }
template <typename T>
ZS_HD T nf_planar_h(T t) { return (T)1 - t * t; }
template <typename T>
ZS_HD T nf_planar_m(T h, T c) { return (T)1 + h * c; }
template <typename T>
ZS_HD T nf_planar_logdet(T ld, T t, T c) { return ld + nf_log(nf_abs(nf_planar_m(nf_planar_h(t), c))); }
// backward: gt = g.uh + gld (c / m) (-2 t) ;  Gc term = gld h / m ;  g <- g + ga w
template <typename T>
ZS_HD T nf_planar_gt(T dot_guh, T gld, T c, T m, T t) { return dot_guh + (gld * (c / m)) * ((T)-2 * t); }
template <typename T>
ZS_HD T nf_planar_gc(T gld, T h, T m) { return (gld * h) / m; }
template <typename T>
ZS_HD T nf_planar_g(T g, T ga, T w) { return g + ga * w; }

// ---------------------------------------------------------------- planar: the parameter chain of P1f (lane d of layer l)
template <typename T>
ZS_HD T nf_finish_guh(T Guh, T Gc, T w) { return Guh + Gc * w; }
template <typename T>
ZS_HD T nf_finish_gw0(T Gw, T Gc, T uh) { return Gw + Gc * uh; }
// gu = Guh + (p / n) s' w
template <typename T>
ZS_HD T nf_finish_gu(T Guh, T p, T n, T dk, T w) { return Guh + ((p / n) * dk) * w; }
// gw = Gw + Guh k / n + (p / n) s' u - 2 k p / n^2 w
template <typename T>
ZS_HD T nf_finish_gw(T Gw, T Guh, T p, T n, T k, T dk, T u, T w) {
  return ((Gw + Guh * (k / n)) + ((p / n) * dk) * u) - ((((T)2 * k) * p) / (n * n)) * w;
}

// ---------------------------------------------------------------- Householder
// z <- z - 2 v (p / n)
template <typename T>
ZS_HD T nf_householder_z(T z, T v, T p, T n) { return z - ((T)2 * v) * (p / n); }
// gv = -2 (p g + q z) / n + 4 p q v / n^2
template <typename T>
ZS_HD T nf_householder_gv(T g, T z, T v, T p, T q, T n) {
  return ((T)-2 * (p * g + q * z)) / n + ((((T)4 * p) * q) * v) / (n * n);
}

// ---------------------------------------------------------------- sequential restatements (one row, one layer)
// What the lanes of a group compute together, written for one thread: ascending-d sums stand for the butterflies.  The host
// program runs these against long double, and they document the order of the kernels' loops.
template <typename T>
ZS_HD T nf_dot_row(const T* a, const T* b, int D) {
  T s = (T)0;
  for (int d = 0; d < D; ++d) s += a[d] * b[d];
  return s;
}
template <typename T>
struct NfParams { T s, n, k, c; };
template <typename T>
ZS_HD NfParams<T> nf_planar_params_row(const T* u, const T* w, T* uh, int D) {
  NfParams<T> p;
  p.s = nf_dot_row(w, u, D);
  p.n = nf_dot_row(w, w, D);
  p.k = nf_planar_k(p.s);
  for (int d = 0; d < D; ++d) uh[d] = nf_planar_uhat(u[d], w[d], p.k, p.n);
  p.c = nf_dot_row(w, uh, D);
  return p;
}
// one layer on z (in place); returns t, adds the layer's term to *ld
template <typename T>
ZS_HD T nf_planar_layer_row(const T* w, T b, const T* uh, T c, T* z, T* ld, int D) {
  const T t = nf_planar_t(nf_dot_row(w, z, D), b);
  for (int d = 0; d < D; ++d) z[d] = nf_planar_z(z[d], uh[d], t);
  *ld = nf_planar_logdet(*ld, t, c);
  return t;
}
// backward of one layer: zl the layer's input, g the cotangent (in place); the four sums get this row's terms
template <typename T>
ZS_HD void nf_planar_layer_bwd_row(const T* w, const T* uh, T c, T t, const T* zl, T gld, T* g, T* Guh, T* Gw, T* Gb, T* Gc, int D) {
  const T h = nf_planar_h(t), m = nf_planar_m(h, c);
  const T ga = nf_planar_gt(nf_dot_row(g, uh, D), gld, c, m, t) * h;
  for (int d = 0; d < D; ++d) {
    Guh[d] += g[d] * t;
    Gw[d] += ga * zl[d];
    g[d] = nf_planar_g(g[d], ga, w[d]);
  }
  *Gb += ga;
  *Gc += nf_planar_gc(gld, h, m);
}
template <typename T>
ZS_HD void nf_planar_finish_row(const T* u, const T* w, T* Guh, T* Gw, T Gc, T* gu, T* gw, int D) {
  T uh[ZS_NF_MAX_DIM];
  const NfParams<T> p = nf_planar_params_row(u, w, uh, D);
  for (int d = 0; d < D; ++d) {
    Guh[d] = nf_finish_guh(Guh[d], Gc, w[d]);
    Gw[d] = nf_finish_gw0(Gw[d], Gc, uh[d]);
  }
  const T pp = nf_dot_row(Guh, w, D), dk = nf_planar_dk(p.s);
  for (int d = 0; d < D; ++d) {
    gu[d] = nf_finish_gu(Guh[d], pp, p.n, dk, w[d]);
    gw[d] = nf_finish_gw(Gw[d], Guh[d], pp, p.n, p.k, dk, u[d], w[d]);
  }
}
template <typename T>
ZS_HD void nf_householder_layer_row(const T* v, T* z, int D) {
  const T n = nf_dot_row(v, v, D), p = nf_dot_row(v, z, D);
  for (int d = 0; d < D; ++d) z[d] = nf_householder_z(z[d], v[d], p, n);
}
template <typename T>
ZS_HD void nf_householder_layer_bwd_row(const T* v, const T* zl, T* g, T* gv, int D) {
  const T n = nf_dot_row(v, v, D), p = nf_dot_row(v, zl, D), q = nf_dot_row(v, g, D);
  for (int d = 0; d < D; ++d) {
    gv[d] = nf_householder_gv(g[d], zl[d], v[d], p, q, n);
    g[d] = nf_householder_z(g[d], v[d], q, n);
  }
}

}  // namespace zs
