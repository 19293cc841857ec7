// The arithmetic of the multivariate-normal kernels (include/zs_mvn.h, zs_mvn.hip) and what they add to the lane-group map of
// zs_group_math.h: the walk of a group over the lower triangle, the place of an element of L in the group's LDS tile, and the
// steps of the matvec, of the two substitutions and of the density.  __host__ __device__, so that
// tests/host_math/zs_mvn_host_math.hip walks the same code on the host under the sanitizers.
#pragma once
#include <math.h>
#include "zs_group_math.h"

// a * b + c rounds once only where flat_fma says so: the same bits whatever the alignment of the operands
#pragma clang fp contract(off)

namespace zs {

#define ZS_MVN_MAX_DIM 64
#define ZS_MVN_THREADS 64          // a workgroup is ONE wave: its barriers are the wave's own, its LDS tile at most 33 KB

ZS_HD float mvn_log(float x) { return logf(x); }
ZS_HD double mvn_log(double x) { return log(x); }

// ---------------------------------------------------------------- lane groups
// A group of G = group_lanes(D) consecutive lanes of one wave owns a row of the batch (mean[r, :], tril[r, :, :]); lane
// pl.lane = i < D of the group owns component i: element i of every vector and row i of every triangular accumulator (idle when
// i >= D).  A wave holds 64 / G rows; the place and the row loop are zs_group_math.h's, with ZS_MVN_THREADS threads.

// The walk of lane `lane` of a group over the D x D elements of a row-major matrix, G consecutive elements per step (the group's
// accesses are contiguous):   for (MvnWalk w = mvn_walk_first(lane, D); w.i < D; mvn_walk_next(w, G, D))
// Element (w.i, w.j) is touched only where w.j <= w.i on the way in; G < 2 D, so a step wraps at most twice.
struct MvnWalk { int i, j; };
ZS_HD MvnWalk mvn_walk_first(int lane, int D) {
  MvnWalk w = {0, lane};
  if (w.j >= D) { w.j -= D; w.i = 1; }
  return w;
}
ZS_HD void mvn_walk_next(MvnWalk& w, int G, int D) {
  w.j += G;
  if (w.j >= D) { w.j -= D; ++w.i; }
  if (w.j >= D) { w.j -= D; ++w.i; }
}

// L of the wave's rows lives in LDS: group `grp` holds element (i, j) at mvn_tile_index.  The odd row stride G + 1 keeps both the
// walk along a column (lane i reads (i, j): forward substitution, matvec) and along a row (lane i reads (j, i): back
// substitution) on distinct banks.  A wave's tile has 64 (G + 1) elements.
ZS_HD int mvn_tile_index(int grp, int i, int j, int G) { return (grp * G + i) * (G + 1) + j; }
ZS_HD int mvn_tile_elements(int G) { return ZS_MVN_THREADS * (G + 1); }

// ---------------------------------------------------------------- per-element steps
// matvec, lane i, column j <= i in ascending j from acc = mean_i:   acc += L_ij eps_j
template <typename T>
ZS_HD T mvn_matvec_step(T acc, T l, T e) { return flat_fma(l, e, acc); }
// 1 / L_ii, formed once per row and reused by every particle
template <typename T>
ZS_HD T mvn_rdiag(T d) { return (T)1 / d; }
// a substitution step: the component solved last, t = b_j / L_jj, leaves the right-hand sides still open:  b_i -= L t
template <typename T>
ZS_HD T mvn_solved(T b, T rdiag) { return b * rdiag; }
template <typename T>
ZS_HD T mvn_subst_step(T b, T l, T t) { return flat_fma(-l, t, b); }
// lp = -D/2 log 2 pi - sum_i log L_ii - 1/2 sum_i y_i^2   (c0 = -D/2 log 2 pi is formed in double on the host)
template <typename T>
ZS_HD T mvn_lp(T c0, T sum_log_diag, T sum_sq) { return flat_fma((T)-0.5, sum_sq, c0 - sum_log_diag); }
// one particle's term of gtril_ij:  g (w_i y_j - delta_ij / L_ii)
template <typename T>
ZS_HD T mvn_gtril_step(T acc, T g, T w, T yj, bool diagonal, T rdiag) {
  T t = w * yj;
  if (diagonal) t -= rdiag;
  return flat_fma(g, t, acc);
}

// ---------------------------------------------------------------- sequential restatements (one row, the kernels' order)
// What the D lanes of a group compute together, written for one thread: the host program runs these against long double, and
// they document the order of the kernels' loops.  L is row-major with row stride ld; only i >= j is read.
template <typename T>
ZS_HD void mvn_matvec_row(const T* L, int ld, const T* mean, const T* e, T* z, int D) {
  for (int i = 0; i < D; ++i) {
    T acc = mean[i];
    for (int j = 0; j <= i; ++j) acc = mvn_matvec_step(acc, L[i * ld + j], e[j]);
    z[i] = acc;
  }
}
// y = L^-1 b, column-oriented; b is overwritten by y
template <typename T>
ZS_HD void mvn_forward_row(const T* L, int ld, T* b, int D) {
  for (int j = 0; j < D; ++j) {
    const T t = mvn_solved(b[j], mvn_rdiag(L[j * ld + j]));
    b[j] = t;
    for (int i = j + 1; i < D; ++i) b[i] = mvn_subst_step(b[i], L[i * ld + j], t);
  }
}
// w = L^-T c, column-oriented over L^T (the rows of L, last to first); c is overwritten by w
template <typename T>
ZS_HD void mvn_backward_row(const T* L, int ld, T* c, int D) {
  for (int j = D - 1; j >= 0; --j) {
    const T t = mvn_solved(c[j], mvn_rdiag(L[j * ld + j]));
    c[j] = t;
    for (int i = 0; i < j; ++i) c[i] = mvn_subst_step(c[i], L[j * ld + i], t);
  }
}

}  // namespace zs
