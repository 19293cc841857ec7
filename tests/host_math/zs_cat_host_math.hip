// The arithmetic and the lane-group maps of the categorical kernels (csrc/zs_cat_math.h with zs_group_math.h: __host__ __device__)
// compiled for the HOST and run under AddressSanitizer + UndefinedBehaviorSanitizer (tests/test_cat_host_math.py):
//     hipcc -x hip --cuda-host-only -Xarch_host -fsanitize=address,undefined ...
// (1) the Gumbel transform at the smallest and the largest u01 and over the range between, finite and against long double;
// (2) the running (max, sum-exp) pair: a host restatement of the kernel's walk -- lane g of a group of G pushes its chunks
//     g, g + G, ... four elements at a time, then the group merges by the xor butterfly and takes its first lane's pair -- against
//     a long-double logsumexp for every N of tests/test_cat_kernel.py, logits at scale 0 / 1 / 5, offset by +-80, with a -inf
//     entry and all -inf; also the merges in the opposite operand order (every lane's pair must agree to the bound);
// (3) the lane-group map for every N of the kernel test and R in {1, 3, 65}: each (row, category) is owned by exactly one
//     (block, thread, chunk, element) of the kernels' own loops (group_place, cat_item_first / step, cat_chunk_first / step), over
//     exactly-sized heap arrays;
// (4) the densities at tau in {1e-3, 1e3} and between against long double.   Prints "cat host math ok: N checks".
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <limits>
#include <vector>

#include "../../zhusuan-pytorch_amd/csrc/zs_cat_math.h"
#include "zs_host_check.h"

template <typename T> static ld eps_elem() { return sizeof(T) == 4 ? ldexpl(1.0L, -20) : ldexpl(1.0L, -48); }
template <typename T> static ld eps_sum(ld n) { return sizeof(T) == 4 ? ldexpl(1.0L, -20) + n * ldexpl(1.0L, -24) : ldexpl(1.0L, -48) + n * ldexpl(1.0L, -53); }

// ---------------------------------------------------------------- (1)
template <typename T>
static void check_gumbel() {
  const double lo = ldexp(1.0, -24), hi = 1.0 - ldexp(1.0, -24);          // the smallest and the largest u01
  std::vector<double> us = {lo, hi, 0.5, 1.0 / 2.718281828459045, 3.0 * lo, 1.0 - 3.0 * lo};
  for (int i = 0; i < 4000; ++i) us.push_back(((double)(uint32_t)(uniform01() * 8388608.0) + 0.5) * ldexp(1.0, -23));
  for (double ud : us) {
    const T u = (T)ud;
    const T g = zs::cat_gumbel(u);
    const ld want = -logl(-logl((ld)u));
    // two roundings: the inner logarithm's relative error enters the outer one absolutely
    expect(isfinite((double)g) && fabsl((ld)g - want) <= eps_elem<T>() * (1 + fabsl(want)), "gumbel", (double)g, (double)want);
    const T v = zs::cat_perturbed((T)-3.25, u);
    expect(isfinite((double)v) && fabsl((ld)v - ((ld)-3.25 + want)) <= eps_elem<T>() * (1 + 3.25L + fabsl(want)), "perturbed", (double)v,
           (double)(-3.25L + want));
    expect(zs::cat_perturbed(zs::cat_neg_inf<T>(), u) == zs::cat_neg_inf<T>(), "perturbed -inf", 0, 0);
  }
  expect(zs::cat_better<T>((T)1, 5, (T)0, 2), "better value", 0, 0);
  expect(zs::cat_better<T>((T)1, 2, (T)1, 5) && !zs::cat_better<T>((T)1, 5, (T)1, 2), "ties to the lower index", 0, 0);
  expect(zs::cat_better<T>(zs::cat_neg_inf<T>(), 0, zs::cat_neg_inf<T>(), INT32_MAX), "an all -inf row draws category 0", 0, 0);
}

// ---------------------------------------------------------------- (2)
// the kernel's walk over one row; `flip`: merge with the operands exchanged.  Returns the pair of group lane `take`.
template <typename T>
static zs::CatMS<T> row_pair(const T* row, int64_t N, bool flip, int take) {
  const int G = zs::cat_group_lanes(N);
  std::vector<zs::CatMS<T>> lane(G);
  for (int g = 0; g < G; ++g) {
    zs::CatMS<T> ms = zs::cat_ms_empty<T>();
    for (int64_t j0 = zs::cat_chunk_first(g); j0 < N; j0 += zs::cat_chunk_step(G)) {
      T x[4];
      for (int c = 0; c < 4; ++c) x[c] = j0 + c < N ? row[j0 + c] : zs::cat_neg_inf<T>();
      zs::cat_ms_push4(ms, x);
    }
    lane[g] = ms;
  }
  if (flip) zs::group_butterfly_host(lane.data(), G, [](const zs::CatMS<T>& a, const zs::CatMS<T>& b) { return zs::cat_ms_merge(b, a); });
  else zs::group_butterfly_host(lane.data(), G, [](const zs::CatMS<T>& a, const zs::CatMS<T>& b) { return zs::cat_ms_merge(a, b); });
  return lane[take % G];
}

template <typename T>
static void check_running_pair() {
  const int64_t Ns[] = {1, 2, 3, 4, 5, 31, 32, 33, 63, 64, 65, 127, 257, 1000, 4099};
  const double scales[] = {0.0, 1.0, 5.0};
  const double offsets[] = {0.0, 80.0, -80.0};
  for (int64_t N : Ns) for (double sc : scales) for (double off : offsets) for (int hole = 0; hole < 3; ++hole) {
    T* row = (T*)malloc(sizeof(T) * N);          // exactly sized: a chunk read past N would be caught
    for (int64_t j = 0; j < N; ++j) row[j] = (T)(off + sc * normal01());
    if (hole == 1 && N > 1) row[N / 2] = zs::cat_neg_inf<T>();
    if (hole == 2) for (int64_t j = 0; j < N; ++j) row[j] = zs::cat_neg_inf<T>();
    ld m = -INFINITY, s = 0, sabs = 0;
    for (int64_t j = 0; j < N; ++j) m = fmaxl(m, (ld)row[j]);
    for (int64_t j = 0; j < N; ++j) s += expl((ld)row[j] - m);
    const ld want = m + logl(s);
    const int G = zs::cat_group_lanes(N);
    for (int flip = 0; flip < 2; ++flip) for (int take = 0; take < G; take += (G > 4 ? G / 4 : 1)) {
      const T got = zs::cat_lse(row_pair<T>(row, N, flip != 0, take));
      if (hole == 2) {
        expect(got == zs::cat_neg_inf<T>(), "lse of an all -inf row", (double)got, -INFINITY);
      } else {
        sabs = fabsl(m) + logl((ld)N) + 1;
        expect(isfinite((double)got) && fabsl((ld)got - want) <= eps_sum<T>((ld)N) * sabs, "lse", (double)got, (double)want);
      }
    }
    free(row);
  }
}

// ---------------------------------------------------------------- (3)
static void check_lane_groups() {
  const int64_t Ns[] = {1, 2, 3, 4, 5, 31, 32, 33, 63, 64, 65, 127, 257, 1000, 4099};
  const int64_t Rs[] = {1, 3, 65};
  const int THREADS = ZS_CAT_THREADS;
  for (int64_t N : Ns) {
    const int G = zs::cat_group_lanes(N);
    expect(G >= 1 && G <= 64 && (G & (G - 1)) == 0 && 64 % G == 0, "group lanes", G, 0);
    expect((int64_t)G * 4 >= N || G == 64, "one chunk per lane up to 256 categories", G, (double)N);
    expect(G == 1 || (int64_t)(G / 2) * 4 < N, "no lane group wider than the row needs", G, (double)N);
    for (int64_t R : Rs) for (int grid = 1; grid <= 3; grid += 2) {
      unsigned char* owned = (unsigned char*)calloc((size_t)(R * N), 1);
      for (int b = 0; b < grid; ++b) for (int tid = 0; tid < THREADS; ++tid) {
        const zs::GroupPlace pl = zs::group_place(tid, THREADS, G);          // what the kernels call
        expect(pl.lane >= 0 && pl.lane < G && pl.first % G == 0 && pl.first + G <= 64 && ((tid & 63) - pl.first) == pl.lane,
               "a group stays inside its wave", pl.first, pl.lane);
        for (int64_t it = zs::cat_item_first(b, pl); it < R; it += zs::cat_item_step(grid, pl))
          for (int64_t j0 = zs::cat_chunk_first(pl.lane); j0 < N; j0 += zs::cat_chunk_step(G))
            for (int c = 0; c < 4; ++c)
              if (j0 + c < N) ++owned[it * N + j0 + c];
      }
      bool once = true;
      for (int64_t i = 0; i < R * N; ++i) once = once && owned[i] == 1;
      expect(once, "every (row, category) owned exactly once", (double)N, (double)R);
      free(owned);
    }
  }
}

// ---------------------------------------------------------------- (4)
template <typename T>
static void check_densities() {
  const double taus[] = {1e-3, 0.1, 1.0, 5.0, 1e3};
  const int64_t Ns[] = {1, 2, 5, 33, 257};
  for (double taud : taus) for (int64_t N : Ns) for (int rep = 0; rep < 8; ++rep) {
    const T tau = (T)taud;
    std::vector<T> l(N), u(N), a(N), y(N), t(N);
    for (int64_t j = 0; j < N; ++j) {
      l[j] = (T)(2.0 * normal01());
      u[j] = (T)(((double)(uint32_t)(uniform01() * 8388608.0) + 0.5) * ldexp(1.0, -23));
    }
    // long double restatement from the same rounded inputs
    std::vector<ld> A(N), Y(N), Tt(N);
    ld ma = -INFINITY, amax = 0;
    for (int64_t j = 0; j < N; ++j) {
      A[j] = ((ld)l[j] - logl(-logl((ld)u[j]))) / (ld)tau;
      ma = fmaxl(ma, A[j]);
      amax = fmaxl(amax, fabsl(A[j]));
    }
    ld sa = 0;
    for (int64_t j = 0; j < N; ++j) sa += expl(A[j] - ma);
    const ld LA = ma + logl(sa);
    zs::CatMS<T> msa = zs::cat_ms_empty<T>();
    for (int64_t j0 = 0; j0 < N; j0 += 4) {
      T x[4];
      for (int c = 0; c < 4; ++c) x[c] = j0 + c < N ? (a[j0 + c] = zs::cat_relaxed_a(l[j0 + c], u[j0 + c], tau)) : zs::cat_neg_inf<T>();
      zs::cat_ms_push4(msa, x);
    }
    const T lse_a = zs::cat_lse(msa);
    zs::CatMS<T> mst = zs::cat_ms_empty<T>();
    T sum_t = 0, sum_y = 0;
    ld ST = 0, SY = 0, SabsT = 0, mt = -INFINITY;
    for (int64_t j = 0; j < N; ++j) {
      y[j] = a[j] - lse_a;
      Y[j] = A[j] - LA;
      expect(fabsl((ld)y[j] - Y[j]) <= eps_elem<T>() * (1 + amax + fabsl(LA)), "y", (double)y[j], (double)Y[j]);
      // the density is checked at the y the kernel holds
      Tt[j] = (ld)l[j] - (ld)tau * (ld)y[j];
      ST += Tt[j]; SY += (ld)y[j]; SabsT += fabsl(Tt[j]); mt = fmaxl(mt, Tt[j]);
    }
    for (int64_t j0 = 0; j0 < N; j0 += 4) {
      T x[4];
      for (int c = 0; c < 4; ++c) {
        x[c] = zs::cat_neg_inf<T>();
        if (j0 + c < N) { x[c] = t[j0 + c] = zs::cat_relaxed_t(l[j0 + c], y[j0 + c], tau); sum_t += x[c]; sum_y += y[j0 + c]; }
      }
      zs::cat_ms_push4(mst, x);
    }
    ld st = 0;
    for (int64_t j = 0; j < N; ++j) st += expl(Tt[j] - mt);
    const ld LT = mt + logl(st);
    const ld c0 = lgammal((ld)N) + (ld)(N - 1) * logl((ld)taud);
    for (int e = 0; e < 2; ++e) {
      const T lp = zs::cat_relaxed_lp((T)c0, sum_t, (T)N, zs::cat_lse(mst), sum_y, e != 0);
      const ld want = c0 + ST - (ld)N * LT - (e ? SY : 0);
      ld SySum = 0;
      for (int64_t j = 0; j < N; ++j) SySum += fabsl((ld)y[j]);
      const ld S = 1 + SabsT + (ld)N * fabsl(LT) + fabsl(c0) + (e ? SySum : 0);
      expect(isfinite((double)lp) && fabsl((ld)lp - want) <= eps_sum<T>((ld)N) * S, "relaxed lp", (double)lp, (double)want);
    }
    ld sq = 0;
    for (int64_t j = 0; j < N; ++j) {
      const T q = zs::cat_relaxed_q(t[j], zs::cat_lse(mst), (T)N);
      const ld want = 1 - (ld)N * expl(Tt[j] - LT);
      expect(fabsl((ld)q - want) <= eps_sum<T>((ld)N) * (1 + (ld)N * expl(Tt[j] - LT) * (1 + fabsl(Tt[j]) + fabsl(LT))), "q", (double)q, (double)want);
      sq += want;
    }
    expect(fabsl(sq) <= 1e-12L * (ld)N * (ld)N, "sum_j q_j = 0", (double)sq, 0);
  }
  // the log-mass forms
  expect(zs::cat_weight_term<T>((T)0, zs::cat_neg_inf<T>()) == (T)0, "x == 0 at -inf contributes exactly 0", 0, 0);
  expect(zs::cat_weight_term<T>((T)2, (T)-1.5) == (T)-3, "weight term", 0, 0);
  expect(zs::cat_logmass<T>((T)1, (T)3) == (T)-2, "log-mass", 0, 0);
  expect(zs::cat_weight_logmass<T>((T)-3, (T)2, (T)0.5) == (T)-4, "weights log-mass", 0, 0);
}

int main() {
  check_gumbel<float>();
  check_gumbel<double>();
  check_running_pair<float>();
  check_running_pair<double>();
  check_lane_groups();
  check_densities<float>();
  check_densities<double>();
  return finish("cat host math ok");
}
