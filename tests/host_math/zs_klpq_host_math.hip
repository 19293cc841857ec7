// The arithmetic and the lane map of the inclusive-KL kernels (csrc/zs_klpq_math.h with zs_group_math.h: __host__ __device__)
// compiled for the HOST and run under AddressSanitizer + UndefinedBehaviorSanitizer (tests/test_klpq_host_math.py):
//     hipcc -x hip --cuda-host-only -Xarch_host -fsanitize=address,undefined ...
// (1) a datapoint's reductions in the kernel's split order -- each lane's partial over k = j, j + G, ..., then the xor butterfly --
//     against long double for every K of tests/test_klpq_kernel.py at scale 0 / 1 / 5 with offsets 0 / +80 / -80, with one -inf
//     particle and with all -inf: the (max, sum-exp) pair as the bound, the weights, the cost (both flags) and the effective
//     sample size;
// (2) the lane and row map for every (K, B) of that grid, in the launch shapes the library uses (256 threads over many
//     workgroups, and the single workgroup of 1024 threads of a launch with the batch mean): a group never crosses its wave,
//     every (k, b) is owned exactly once, w is written exactly once per element inside its exactly-sized array;
// (3) the stride addressing of the four layouts ([K, B], [B, K], shared by the batch, shared by the particles) over exactly-sized
//     arrays, forward (the left-to-right sum) and backward (every gradient element written once, the broadcast sums against
//     long double);
// (4) the batch mean in the first wave's order against long double for B of the grid and the largest B.
// Prints "klpq host math ok: N checks".
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

#include "../../zhusuan-pytorch_amd/csrc/zs_klpq_math.h"
#include "zs_host_check.h"

using namespace zs;

template <typename T> static ld unit() { return sizeof(T) == 4 ? ldexpl(1.0L, -24) : ldexpl(1.0L, -53); }

static const int Ks[] = {1, 2, 3, 5, 31, 32, 33, 50, 63, 64, 65, 130, 257};
static const int Bs[] = {1, 3, 65, 257};

template <typename T> static T* heap(size_t n, T fill) {          // exactly sized: a step outside is the sanitizer's
  T* p = (T*)malloc(sizeof(T) * (n ? n : 1));
  for (size_t i = 0; i < n; ++i) p[i] = fill;
  return p;
}
static KlpqSide side_of(const void* v, void* g, int64_t sk, int64_t sb) {
  KlpqSide s;
  memset(&s, 0, sizeof(s));
  s.n = 1;
  s.t[0].value = v; s.t[0].grad = g; s.t[0].sk = sk; s.t[0].sb = sb;
  return s;
}

// ---------------------------------------------------------------- (1)
template <typename T> struct Row { T m, s, bound, cost, sq; };
// one datapoint as its group computes it: lanes 0 .. G - 1 in turn, then the butterflies
template <typename T>
static Row<T> group_forward(const KlpqSide& p, const KlpqSide& q, int64_t b, int64_t K, bool model_grad, T* wrow) {
  const int G = group_lanes(K);
  T v[ZS_KLPQ_WAVE], c[ZS_KLPQ_WAVE];
  KlpqParticle<T> first[ZS_KLPQ_WAVE];
  for (int j = 0; j < G; ++j) {
    first[j] = KlpqParticle<T>{(T)0, (T)0, (T)0};
    if (j < K) first[j] = klpq_particle<T>(p, q, j, b);
    v[j] = klpq_lane_max<T>(p, q, b, j, G, K, first[j]);
  }
  group_butterfly_host(v, G, [](T a, T x) { return group_fmax(a, x); });
  for (int j = 1; j < G; ++j) expect(memcmp(&v[j], &v[0], sizeof(T)) == 0, "the butterfly leaves one max in every lane", (double)v[j], (double)v[0]);
  Row<T> r;
  r.m = v[0];
  for (int j = 0; j < G; ++j) v[j] = klpq_lane_sumexp<T>(p, q, b, j, G, K, first[j], r.m);
  group_butterfly_host(v, G, [](T a, T x) { return a + x; });
  for (int j = 1; j < G; ++j) expect(memcmp(&v[j], &v[0], sizeof(T)) == 0, "the butterfly leaves one sum in every lane", (double)v[j], (double)v[0]);
  r.s = v[0];
  r.bound = klpq_bound(r.m, r.s, (T)log((double)K));
  for (int j = 0; j < G; ++j) {
    const KlpqSums<T> a = klpq_lane_weights<T>(p, q, b, j, G, K, first[j], r.m, r.s, model_grad, wrow);
    v[j] = a.cost;
    c[j] = a.sq;
  }
  group_butterfly_host(v, G, [](T a, T x) { return a + x; });
  group_butterfly_host(c, G, [](T a, T x) { return a + x; });
  r.cost = -v[0];
  r.sq = c[0];
  return r;
}

template <typename T>
static void check_reductions() {
  const ld u = unit<T>();
  const double scales[] = {0.0, 1.0, 5.0}, offsets[] = {0.0, 80.0, -80.0};
  for (int K : Ks) for (double scale : scales) for (double off : offsets) for (int variant = 0; variant < 3; ++variant) {
    T* lp = heap<T>(K, 0);
    T* lq = heap<T>(K, 0);
    T* w = heap<T>(K, (T)NAN);
    for (int k = 0; k < K; ++k) {
      lp[k] = (T)(off + scale * normal01() - 3.0);
      lq[k] = (T)(scale * normal01() - 2.0);
    }
    if (variant == 1) lp[K / 2] = (T)-INFINITY;
    if (variant == 2) for (int k = 0; k < K; ++k) lp[k] = (T)-INFINITY;
    const KlpqSide p = side_of(lp, nullptr, 1, 0), q = side_of(lq, nullptr, 1, 0);
    for (int mg = 0; mg < 2; ++mg) {
      const Row<T> r = group_forward<T>(p, q, 0, K, mg != 0, w);
      const bool none = variant == 2 || (variant == 1 && K == 1);
      if (none) {
        expect(isnan((double)r.bound) && isnan((double)r.cost) && isnan((double)r.sq) && isnan((double)w[0]), "all -inf gives NaN", (double)r.bound, NAN);
        continue;
      }
      // long double on the T-rounded log-weights
      ld m = -INFINITY, s = 0, maxd = 0, cost = 0, acost = 0, sq = 0;
      std::vector<ld> lw(K);
      for (int k = 0; k < K; ++k) { lw[k] = (ld)(T)(lp[k] - lq[k]); if (lw[k] > m) m = lw[k]; }
      for (int k = 0; k < K; ++k) { s += expl(lw[k] - m); if (isfinite((double)lw[k]) && m - lw[k] > maxd) maxd = m - lw[k]; }
      const ld bound = m + logl(s) - logl((ld)K);
      const ld rel_w = (maxd + K + 8) * u;          // the rounded exponent, the K-term sum, exp, divide
      expect(fabsl((ld)r.bound - bound) <= rel_w + 4 * u * (fabsl(m) + fabsl(logl(s)) + logl((ld)K)), "bound against long double", (double)r.bound, (double)bound);
      for (int k = 0; k < K; ++k) {
        const ld wk = expl(lw[k] - m) / s, x = (ld)lq[k] + (mg ? (ld)lp[k] : 0);
        expect(fabsl((ld)w[k] - wk) <= rel_w * wk, "weight against long double", (double)w[k], (double)wk);
        if (!isfinite((double)lw[k])) expect(w[k] == (T)0, "a -inf particle has weight exactly 0", (double)w[k], 0.0);
        if (wk > 0) { cost -= wk * x; acost += wk * fabsl(x); }
        sq += wk * wk;
      }
      expect(isfinite((double)r.cost) && fabsl((ld)r.cost - cost) <= (rel_w + (K + 4) * u) * acost, "cost against long double", (double)r.cost, (double)cost);
      expect(fabsl((ld)r.sq - sq) <= (2 * rel_w + (K + 4) * u) * sq, "sum of squared weights against long double", (double)r.sq, (double)sq);
      if (K == 1) expect(w[0] == (T)1 && r.bound == (T)(lp[0] - lq[0]) && r.sq == (T)1, "K = 1: w = 1, bound = lw, ess = 1", (double)r.bound, (double)lw[0]);
    }
    free(lp); free(lq); free(w);
  }
}

// ---------------------------------------------------------------- (2)
static void walk_map(int64_t K, int64_t B, int threads, int blocks) {
  const int G = group_lanes(K);
  int* own = heap<int>((size_t)(K * B), 0);
  expect(G >= 1 && G <= ZS_KLPQ_WAVE && (G & (G - 1)) == 0 && (K <= G || G == ZS_KLPQ_WAVE) && (G < 2 * K), "group lanes", G, (double)K);
  for (int blk = 0; blk < blocks; ++blk) for (int th = 0; th < threads; ++th) {
    const GroupPlace pl = group_place(th, threads, G);
    if (blk == 0) expect((th - pl.lane) / ZS_KLPQ_WAVE == (th - pl.lane + G - 1) / ZS_KLPQ_WAVE && pl.grp < pl.groups, "a group inside its wave", th, G);
    for (int64_t rb = group_row_first(blk, pl); rb < B; rb += group_row_step(blocks, pl)) {
      const int64_t b = rb + pl.grp;
      if (b >= B) continue;
      for (int64_t k = pl.lane; k < K; k += G) ++own[b * K + k];
    }
  }
  bool once = true;
  for (int64_t i = 0; i < K * B; ++i) once = once && own[i] == 1;
  expect(once, "every (k, b) owned exactly once", (double)K, (double)B);
  free(own);
}
static void check_map() {
  for (int K : Ks) for (int B : Bs) {
    const int groups = ZS_KLPQ_THREADS / group_lanes(K);
    int blocks = (B + groups - 1) / groups;
    walk_map(K, B, ZS_KLPQ_THREADS, blocks);
    walk_map(K, B, ZS_KLPQ_THREADS, blocks > 1 ? blocks / 2 : 1);          // fewer workgroups than steps: the stride loop
    walk_map(K, B, ZS_KLPQ_MEAN_THREADS, 1);
  }
  walk_map(3, 4097, ZS_KLPQ_THREADS, 17);
  walk_map(3, ZS_KLPQ_MEAN_MAX_B, ZS_KLPQ_MEAN_THREADS, 1);
}

// ---------------------------------------------------------------- (3)
template <typename T>
static void check_layouts(int64_t K, int64_t B) {
  const ld u = unit<T>();
  // the same term in the four layouts, exactly sized
  T* kb = heap<T>((size_t)(K * B), 0);
  T* bk = heap<T>((size_t)(K * B), 0);
  T* konly = heap<T>((size_t)K, 0);
  T* bonly = heap<T>((size_t)B, 0);
  for (int64_t k = 0; k < K; ++k) for (int64_t b = 0; b < B; ++b) {
    kb[k * B + b] = bk[b * K + k] = (T)(k * 1024 + b);
    konly[k] = (T)(k * 1024);
    bonly[b] = (T)b;
  }
  T* gkb = heap<T>((size_t)(K * B), (T)NAN);
  T* gbk = heap<T>((size_t)(K * B), (T)NAN);
  T* gk = heap<T>((size_t)K, (T)NAN);
  T* gb = heap<T>((size_t)B, (T)NAN);
  T* g1 = heap<T>(1, (T)NAN);
  T one = (T)0.25;
  KlpqSide q;
  memset(&q, 0, sizeof(q));
  q.n = 4;
  q.t[0] = zs_klpq_term{kb, gkb, B, 1};
  q.t[1] = zs_klpq_term{bk, gbk, 1, K};
  q.t[2] = zs_klpq_term{konly, gk, 1, 0};
  q.t[3] = zs_klpq_term{bonly, gb, 0, 1};
  const KlpqSide p = side_of(&one, g1, 0, 0);
  bool ok = true;
  for (int64_t k = 0; k < K; ++k) for (int64_t b = 0; b < B; ++b) {
    const T want = (((T)(k * 1024 + b) + (T)(k * 1024 + b)) + (T)(k * 1024)) + (T)b;
    ok = ok && klpq_side_sum<T>(q, k, b) == want && klpq_side_sum<T>(p, k, b) == one;
  }
  expect(ok, "the four layouts address element (k, b), added left to right", (double)K, (double)B);
  // backward over the same tables: w, gcost and gbound exactly sized
  T* w = heap<T>((size_t)(K * B), 0);
  T* gc = heap<T>((size_t)B, 0);
  T* gbd = heap<T>((size_t)B, 0);
  for (int64_t i = 0; i < K * B; ++i) w[i] = (T)uniform01();
  for (int64_t b = 0; b < B; ++b) { gc[b] = (T)normal01(); gbd[b] = (T)normal01(); }
  const int64_t nth = 96;
  for (int mode = 0; mode < 3; ++mode) {          // gcost per datapoint + gbound, gcost alone, gcost of the mean
    const bool mg = mode != 1, mean = mode == 2;
    for (int64_t tid = 0; tid < nth; ++tid) klpq_backward_thread<T>(p, q, K, B, mg, mean, w, gc, mode == 0 ? gbd : nullptr, tid, nth);
    std::vector<ld> sk(K, 0), ak(K, 0), sb(B, 0), ab(B, 0);
    ld sall = 0, aall = 0;
    bool full = true;
    for (int64_t b = 0; b < B; ++b) for (int64_t k = 0; k < K; ++k) {
      const ld c = mean ? (ld)(T)(gc[0] / (T)B) : (ld)gc[b], d = mode == 0 ? (ld)gbd[b] : 0, wk = w[b * K + k];
      const ld cq = -c * wk - d * wk, cp = mg ? -c * wk + d * wk : d * wk, mag = (fabsl(c) + fabsl(d)) * wk;
      full = full && fabsl((ld)gkb[k * B + b] - cq) <= 3 * u * mag && gkb[k * B + b] == gbk[b * K + k];
      sk[k] += cq; ak[k] += mag; sb[b] += cq; ab[b] += mag; sall += cp; aall += mag;
    }
    expect(full, "a full term receives its coefficient in its own layout", (double)K, (double)B);
    bool sums = true;
    for (int64_t k = 0; k < K; ++k) sums = sums && fabsl((ld)gk[k] - sk[k]) <= (B + 3) * u * ak[k];
    for (int64_t b = 0; b < B; ++b) sums = sums && fabsl((ld)gb[b] - sb[b]) <= (K + 3) * u * ab[b];
    sums = sums && fabsl((ld)g1[0] - sall) <= (K + B + 3) * u * aall;
    expect(sums, "a shared term receives the sum over its broadcast axis", (double)K, (double)B);
  }
  free(kb); free(bk); free(konly); free(bonly); free(gkb); free(gbk); free(gk); free(gb); free(g1); free(w); free(gc); free(gbd);
}

// ---------------------------------------------------------------- (4)
template <typename T>
static void check_mean(int64_t B) {
  const ld u = unit<T>();
  T* costs = heap<T>((size_t)B, 0);
  ld sum = 0, asum = 0;
  for (int64_t b = 0; b < B; ++b) { costs[b] = (T)(10.0 * normal01() + 30.0); sum += costs[b]; asum += fabsl((ld)costs[b]); }
  T v[ZS_KLPQ_WAVE];
  for (int l = 0; l < ZS_KLPQ_WAVE; ++l) v[l] = klpq_mean_lane<T>(costs, B, l);
  group_butterfly_host(v, ZS_KLPQ_WAVE, [](T a, T x) { return a + x; });
  const T mean = v[0] / (T)B;
  expect(fabsl((ld)mean - sum / B) <= ((B + 63) / 64 + 8) * u * asum / B, "batch mean against long double", (double)mean, (double)(sum / B));
  free(costs);
}

int main() {
  check_reductions<float>();
  check_reductions<double>();
  check_map();
  for (int K : Ks) for (int B : Bs) if (K <= 65 || B <= 65) { check_layouts<float>(K, B); check_layouts<double>(K, B); }
  for (int B : Bs) { check_mean<float>(B); check_mean<double>(B); }
  check_mean<float>(ZS_KLPQ_MEAN_MAX_B);
  check_mean<double>(ZS_KLPQ_MEAN_MAX_B);
  return finish("klpq host math ok");
}
