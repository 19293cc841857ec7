// C1 - C4: the categorical families (include/zs_cat.h; its own library, ../lib/libzs_cat.so, `make cat`).
//
// A torch composition of a categorical node costs 8 - 12 launches per direction (Gumbel noise, add, argmax, one_hot, log_softmax,
// gather ...); here a node is one launch each way.  A row of N categories is cut into chunks of four; a group of
// G = cat_group_lanes(N) consecutive lanes owns a row and lane g its chunks g, g + G, ... (zs_cat_math.h), so a wave holds 64 / G
// rows and every reduction of a row -- the running (max, sum-exp) pair, the sums, the (value, index) pairs of the argmax -- is a
// butterfly of log2(G) exchanges inside the lane group.  The (max, sum-exp) merge is not symmetric in its operands in the last
// bit, so the group takes the pair of its first lane.  No LDS, no atomics; sums over the particles are made by the lane that owns
// the element in ascending k.  VEC: N is a multiple of 4 and every pointer 16-byte aligned -- a chunk is one wide access; the
// element form reads and writes the same chunks with the same arithmetic.
#include "zs_common.h"
#include "zs_cat_math.h"
#include "../../include/zs_hip.h"
#include "../../include/zs_cat.h"

#pragma clang fp contract(off)

using namespace zs;

namespace {

constexpr int THREADS = ZS_CAT_THREADS;

template <typename T, bool VEC>
__device__ __forceinline__ void load4(const T* __restrict__ row, int64_t j0, int64_t N, T fill, T out[4]) {
  if (VEC) {
    const Vec4<T> v = *reinterpret_cast<const Vec4<T>*>(row + j0);
#pragma unroll
    for (int c = 0; c < 4; ++c) out[c] = v.v[c];
  } else {
#pragma unroll
    for (int c = 0; c < 4; ++c) out[c] = j0 + c < N ? row[j0 + c] : fill;
  }
}
template <typename T, bool VEC>
__device__ __forceinline__ void store4(T* __restrict__ row, int64_t j0, int64_t N, const T in[4]) {
  if (VEC) {
    Vec4<T> v;
#pragma unroll
    for (int c = 0; c < 4; ++c) v.v[c] = in[c];
    *reinterpret_cast<Vec4<T>*>(row + j0) = v;
  } else {
#pragma unroll
    for (int c = 0; c < 4; ++c)
      if (j0 + c < N) row[j0 + c] = in[c];
  }
}

// the uniforms of flat elements i0 .. i0 + 3 of the launch's stream: element i is word i % 4 of Philox group i / 4
template <typename T>
__device__ __forceinline__ void uniform4(int64_t i0, const PhiloxCall& pc, T out[4]) {
  const uint64_t g0 = (uint64_t)i0 >> 2;
  const int o = (int)(i0 & 3);
  const Philox4 a = philox4x32_10(g0, pc);
  Philox4 b = a;
  if (o) b = philox4x32_10(g0 + 1, pc);
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int i = o + c;
    const uint32_t w = i == 0 ? a.x : i == 1 ? a.y : i == 2 ? a.z : i == 3 ? a.w : i == 4 ? b.x : i == 5 ? b.y : b.z;
    out[c] = (T)u01(w);
  }
}

// the merged pair of the group, the same bits in all of its lanes (`first`: the group's first lane within the wave)
template <typename T>
__device__ __forceinline__ CatMS<T> group_ms(CatMS<T> a, int G, int first) {
  for (int o = G >> 1; o > 0; o >>= 1) {
    CatMS<T> b;
    b.m = __shfl_xor(a.m, o, ZS_WAVE);
    b.s = __shfl_xor(a.s, o, ZS_WAVE);
    a = cat_ms_merge(a, b);
  }
  a.m = __shfl(a.m, first, ZS_WAVE);
  a.s = __shfl(a.s, first, ZS_WAVE);
  return a;
}

// ---------------------------------------------------------------- C1
template <typename T, bool VEC>
__global__ __launch_bounds__(THREADS) void k_cat_sample(const T* __restrict__ logits, const T* __restrict__ u,
                                                        int64_t* __restrict__ idx, T* __restrict__ onehot, T* __restrict__ lp,
                                                        int64_t items, int64_t R, int64_t N, int G, uint64_t seed, uint64_t call,
                                                        const uint64_t* __restrict__ rs) {
  if (rs) { seed = rs[0]; call += rs[1]; }
  const PhiloxCall pc = philox_call(call, seed);
  const int block = (int)blockIdx.x, blocks = (int)gridDim.x;
  const GroupPlace pl = group_place((int)threadIdx.x, THREADS, G);
  const int64_t item0 = cat_item_first(block, pl), stride = cat_item_step(blocks, pl), step = cat_chunk_step(G);
  for (int64_t it = item0; it < items; it += stride) {
    const int64_t r = mod_fast(it, R);
    const T* lrow = logits + r * N;
    const int64_t base = it * N;
    CatMS<T> ms = cat_ms_empty<T>();
    T bv = cat_neg_inf<T>();
    int32_t bj = INT32_MAX;
    for (int64_t j0 = cat_chunk_first(pl.lane); j0 < N; j0 += step) {
      T l[4], uu[4];
      load4<T, VEC>(lrow, j0, N, cat_neg_inf<T>(), l);
      if (u) load4<T, VEC>(u + base, j0, N, (T)0.5, uu);
      else uniform4<T>(base + j0, pc, uu);
      cat_ms_push4(ms, l);
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        T v = cat_perturbed(l[c], uu[c]);
        if (!(v == v)) v = cat_neg_inf<T>();          // a NaN logit is never preferred, and the index stays inside the row
        const int32_t j = (int32_t)(j0 + c);
        if (j0 + c < N && cat_better(v, j, bv, bj)) { bv = v; bj = j; }
      }
    }
    for (int o = G >> 1; o > 0; o >>= 1) {
      const T ov = __shfl_xor(bv, o, ZS_WAVE);
      const int32_t oj = __shfl_xor(bj, o, ZS_WAVE);
      if (cat_better(ov, oj, bv, bj)) { bv = ov; bj = oj; }
    }
    ms = group_ms(ms, G, pl.first);
    if (pl.lane == 0) {
      if (idx) idx[it] = (int64_t)bj;
      if (lp) lp[it] = bj < N ? cat_logmass(lrow[bj], cat_lse(ms)) : cat_nan<T>();
    }
    if (onehot) {
      for (int64_t j0 = cat_chunk_first(pl.lane); j0 < N; j0 += step) {
        T h[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) h[c] = j0 + c == (int64_t)bj ? (T)1 : (T)0;
        store4<T, VEC>(onehot + base, j0, N, h);
      }
    }
  }
}

// ---------------------------------------------------------------- C2
template <typename T, bool VEC>
__global__ __launch_bounds__(THREADS) void k_cat_logprob(const T* __restrict__ logits, const int64_t* __restrict__ idx,
                                                         const T* __restrict__ x, int64_t prow, T* __restrict__ lp, int64_t items,
                                                         int64_t R, int64_t N, int G) {
  const int block = (int)blockIdx.x, blocks = (int)gridDim.x;
  const GroupPlace pl = group_place((int)threadIdx.x, THREADS, G);
  const int64_t item0 = cat_item_first(block, pl), stride = cat_item_step(blocks, pl), step = cat_chunk_step(G);
  for (int64_t it = item0; it < items; it += stride) {
    const int64_t r = mod_fast(it, R);
    const int64_t xr = mod_fast(it, prow);
    const T* lrow = logits + r * N;
    CatMS<T> ms = cat_ms_empty<T>();
    T sxl = (T)0, sx = (T)0;
    for (int64_t j0 = cat_chunk_first(pl.lane); j0 < N; j0 += step) {
      T l[4];
      load4<T, VEC>(lrow, j0, N, cat_neg_inf<T>(), l);
      cat_ms_push4(ms, l);
      if (x) {
        T xx[4];
        load4<T, VEC>(x + xr * N, j0, N, (T)0, xx);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          sxl += cat_weight_term(xx[c], l[c]);
          sx += xx[c];
        }
      }
    }
    ms = group_ms(ms, G, pl.first);
    const T lse = cat_lse(ms);
    if (x) {
      sxl = group_sum(sxl, G);
      sx = group_sum(sx, G);
      if (pl.lane == 0) lp[it] = cat_weight_logmass(sxl, sx, lse);
    } else if (pl.lane == 0) {
      const int64_t j = idx[xr];
      lp[it] = j >= 0 && j < N ? cat_logmass(lrow[j], lse) : cat_nan<T>();
    }
  }
}

// One group per ROW r: first pass A_j = sum_k g_k x_kj (parked in glogits, by the lane that reads it back), W = sum_j A_j
// (= sum_k g_k sx_k) and the row's (max, sum-exp); second pass glogits_j = A_j - W softmax_j and gx.
template <typename T, bool VEC>
__global__ __launch_bounds__(THREADS) void k_cat_logprob_bwd(const T* __restrict__ logits, const int64_t* __restrict__ idx,
                                                             const T* __restrict__ x, int64_t prow, const T* __restrict__ glp,
                                                             T* glogits, T* __restrict__ gx, int64_t K, int64_t R, int64_t N, int G) {
  const int block = (int)blockIdx.x, blocks = (int)gridDim.x;
  const GroupPlace pl = group_place((int)threadIdx.x, THREADS, G);
  const int64_t item0 = cat_item_first(block, pl), stride = cat_item_step(blocks, pl), step = cat_chunk_step(G);
  const bool shared = prow == R;          // the value has no particle axis
  for (int64_t r = item0; r < R; r += stride) {
    const T* lrow = logits + r * N;
    CatMS<T> ms = cat_ms_empty<T>();
    T W = (T)0;
    for (int64_t j0 = cat_chunk_first(pl.lane); j0 < N; j0 += step) {
      T l[4], A[4] = {(T)0, (T)0, (T)0, (T)0};
      load4<T, VEC>(lrow, j0, N, cat_neg_inf<T>(), l);
      cat_ms_push4(ms, l);
      if (glogits) {
        for (int64_t k = 0; k < K; ++k) {
          const T gk = glp[k * R + r];
          const int64_t xr = shared ? r : k * R + r;
          if (x) {
            T xx[4];
            load4<T, VEC>(x + xr * N, j0, N, (T)0, xx);
#pragma unroll
            for (int c = 0; c < 4; ++c) A[c] = flat_fma(gk, xx[c], A[c]);
          } else {
            const int64_t j = idx[xr];
#pragma unroll
            for (int c = 0; c < 4; ++c)
              if (j == j0 + c && j < N) A[c] += gk;
          }
        }
        store4<T, VEC>(glogits + r * N, j0, N, A);
        W += (A[0] + A[1]) + (A[2] + A[3]);
      }
    }
    ms = group_ms(ms, G, pl.first);
    W = group_sum(W, G);
    const T lse = cat_lse(ms);
    for (int64_t j0 = cat_chunk_first(pl.lane); j0 < N; j0 += step) {
      T l[4];
      load4<T, VEC>(lrow, j0, N, cat_neg_inf<T>(), l);
      if (glogits) {
        T A[4];
        load4<T, VEC>(glogits + r * N, j0, N, (T)0, A);
#pragma unroll
        for (int c = 0; c < 4; ++c) A[c] = flat_fma(-W, cat_exp(l[c] - lse), A[c]);
        store4<T, VEC>(glogits + r * N, j0, N, A);
      }
      if (gx) {
        for (int64_t k = 0; k < K; ++k) {
          const T gk = glp[k * R + r];
          T o[4];
#pragma unroll
          for (int c = 0; c < 4; ++c) o[c] = gk * (l[c] - lse);
          store4<T, VEC>(gx + (k * R + r) * N, j0, N, o);
        }
      }
    }
  }
}

// ---------------------------------------------------------------- C3
template <typename T, bool VEC>
__global__ __launch_bounds__(THREADS) void k_cat_relaxed_sample(const T* __restrict__ logits, const T* __restrict__ u,
                                                                T* __restrict__ y, T* __restrict__ ey, T* __restrict__ lp,
                                                                int64_t items, int64_t R, int64_t N, int G, T tau, T c0,
                                                                int exp_space, uint64_t seed, uint64_t call,
                                                                const uint64_t* __restrict__ rs) {
  if (rs) { seed = rs[0]; call += rs[1]; }
  const PhiloxCall pc = philox_call(call, seed);
  const int block = (int)blockIdx.x, blocks = (int)gridDim.x;
  const GroupPlace pl = group_place((int)threadIdx.x, THREADS, G);
  const int64_t item0 = cat_item_first(block, pl), stride = cat_item_step(blocks, pl), step = cat_chunk_step(G);
  for (int64_t it = item0; it < items; it += stride) {
    const int64_t r = mod_fast(it, R);
    const T* lrow = logits + r * N;
    const int64_t base = it * N;
    CatMS<T> ma = cat_ms_empty<T>();
    for (int64_t j0 = cat_chunk_first(pl.lane); j0 < N; j0 += step) {
      T l[4], uu[4], a[4];
      load4<T, VEC>(lrow, j0, N, cat_neg_inf<T>(), l);
      if (u) load4<T, VEC>(u + base, j0, N, (T)0.5, uu);
      else uniform4<T>(base + j0, pc, uu);
#pragma unroll
      for (int c = 0; c < 4; ++c) a[c] = cat_relaxed_a(l[c], uu[c], tau);
      cat_ms_push4(ma, a);
    }
    ma = group_ms(ma, G, pl.first);
    const T lse_a = cat_lse(ma);
    // second walk over the lane's own chunks (the row is still in the cache; the draw is recomputed, not stored)
    CatMS<T> mt = cat_ms_empty<T>();
    T sum_t = (T)0, sum_y = (T)0;
    for (int64_t j0 = cat_chunk_first(pl.lane); j0 < N; j0 += step) {
      T l[4], uu[4], yy[4], t[4];
      load4<T, VEC>(lrow, j0, N, cat_neg_inf<T>(), l);
      if (u) load4<T, VEC>(u + base, j0, N, (T)0.5, uu);
      else uniform4<T>(base + j0, pc, uu);
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        yy[c] = cat_relaxed_a(l[c], uu[c], tau) - lse_a;
        const bool live = j0 + c < N;
        t[c] = live ? cat_relaxed_t(l[c], yy[c], tau) : cat_neg_inf<T>();
        sum_t += live ? t[c] : (T)0;
        sum_y += live ? yy[c] : (T)0;
      }
      cat_ms_push4(mt, t);
      if (y) store4<T, VEC>(y + base, j0, N, yy);
      if (ey) {
#pragma unroll
        for (int c = 0; c < 4; ++c) yy[c] = cat_exp(yy[c]);
        store4<T, VEC>(ey + base, j0, N, yy);
      }
    }
    if (lp) {
      mt = group_ms(mt, G, pl.first);
      sum_t = group_sum(sum_t, G);
      sum_y = group_sum(sum_y, G);
      if (pl.lane == 0) lp[it] = cat_relaxed_lp(c0, sum_t, (T)N, cat_lse(mt), sum_y, exp_space != 0);
    }
  }
}

// One group per ROW r, particle after particle; the lane that owns an element adds the particle's term to glogits.
// MODE 0: backward of C3 (reads gy / gey / glp, writes glogits).  MODE 1: backward of C4 (reads glp, writes gy_out and glogits).
template <typename T, bool VEC, int MODE>
__global__ __launch_bounds__(THREADS) void k_cat_relaxed_bwd(const T* __restrict__ logits, const T* __restrict__ y, int64_t prow,
                                                             const T* __restrict__ gy, const T* __restrict__ gey,
                                                             const T* __restrict__ glp, T* __restrict__ gy_out, T* glogits,
                                                             int64_t K, int64_t R, int64_t N, int G, T tau, int exp_space) {
  const int block = (int)blockIdx.x, blocks = (int)gridDim.x;
  const GroupPlace pl = group_place((int)threadIdx.x, THREADS, G);
  const int64_t item0 = cat_item_first(block, pl), stride = cat_item_step(blocks, pl), step = cat_chunk_step(G);
  const T e = exp_space ? (T)1 : (T)0, n = (T)N;
  const bool shared = prow == R;
  for (int64_t r = item0; r < R; r += stride) {
    const T* lrow = logits + r * N;
    for (int64_t k = 0; k < K; ++k) {
      const int64_t it = k * R + r, base = it * N;
      const T* yrow = y + (shared ? r : it) * N;
      const T gk = glp ? glp[it] : (T)0;
      CatMS<T> mt = cat_ms_empty<T>();
      T sg = (T)0;
      for (int64_t j0 = cat_chunk_first(pl.lane); j0 < N; j0 += step) {
        T l[4], yy[4], t[4];
        load4<T, VEC>(lrow, j0, N, cat_neg_inf<T>(), l);
        load4<T, VEC>(yrow, j0, N, (T)0, yy);
#pragma unroll
        for (int c = 0; c < 4; ++c) t[c] = j0 + c < N ? cat_relaxed_t(l[c], yy[c], tau) : cat_neg_inf<T>();
        cat_ms_push4(mt, t);
        if (MODE == 0) {
          T a[4] = {(T)0, (T)0, (T)0, (T)0}, b[4] = {(T)0, (T)0, (T)0, (T)0};
          if (gy) load4<T, VEC>(gy + base, j0, N, (T)0, a);
          if (gey) load4<T, VEC>(gey + base, j0, N, (T)0, b);
#pragma unroll
          for (int c = 0; c < 4; ++c) sg += gey ? flat_fma(b[c], cat_exp(yy[c]), a[c]) : a[c];
        }
      }
      mt = group_ms(mt, G, pl.first);
      const T lse_t = cat_lse(mt);
      T S = (T)0;
      if (MODE == 0) S = flat_fma(-gk * e, n, group_sum(sg, G));
      for (int64_t j0 = cat_chunk_first(pl.lane); j0 < N; j0 += step) {
        T l[4], yy[4], acc[4] = {(T)0, (T)0, (T)0, (T)0}, go[4];
        load4<T, VEC>(lrow, j0, N, cat_neg_inf<T>(), l);
        load4<T, VEC>(yrow, j0, N, (T)0, yy);
        if (glogits && k > 0) load4<T, VEC>(glogits + r * N, j0, N, (T)0, acc);
        T a[4] = {(T)0, (T)0, (T)0, (T)0}, b[4] = {(T)0, (T)0, (T)0, (T)0};
        if (MODE == 0) {
          if (gy) load4<T, VEC>(gy + base, j0, N, (T)0, a);
          if (gey) load4<T, VEC>(gey + base, j0, N, (T)0, b);
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const T q = cat_relaxed_q(cat_relaxed_t(l[c], yy[c], tau), lse_t, n);
          const T dy = gk * (flat_fma(-tau, q, -e));          // glp (-tau q - e)
          if (MODE == 0) {
            const T ex = cat_exp(yy[c]);
            const T Gy = (gey ? flat_fma(b[c], ex, a[c]) : a[c]) + dy;
            acc[c] += flat_fma(-ex, S, Gy) / tau + gk * q;
          } else {
            go[c] = dy;
            acc[c] += gk * q;
          }
        }
        if (MODE == 1 && gy_out) store4<T, VEC>(gy_out + base, j0, N, go);
        if (glogits) store4<T, VEC>(glogits + r * N, j0, N, acc);
      }
    }
  }
}

// ---------------------------------------------------------------- C4
template <typename T, bool VEC>
__global__ __launch_bounds__(THREADS) void k_cat_relaxed_logprob(const T* __restrict__ logits, const T* __restrict__ y, int64_t prow,
                                                                 T* __restrict__ lp, int64_t items, int64_t R, int64_t N, int G, T tau,
                                                                 T c0, int exp_space) {
  const int block = (int)blockIdx.x, blocks = (int)gridDim.x;
  const GroupPlace pl = group_place((int)threadIdx.x, THREADS, G);
  const int64_t item0 = cat_item_first(block, pl), stride = cat_item_step(blocks, pl), step = cat_chunk_step(G);
  for (int64_t it = item0; it < items; it += stride) {
    const T* lrow = logits + mod_fast(it, R) * N;
    const T* yrow = y + mod_fast(it, prow) * N;
    CatMS<T> mt = cat_ms_empty<T>();
    T sum_t = (T)0, sum_y = (T)0;
    for (int64_t j0 = cat_chunk_first(pl.lane); j0 < N; j0 += step) {
      T l[4], yy[4], t[4];
      load4<T, VEC>(lrow, j0, N, cat_neg_inf<T>(), l);
      load4<T, VEC>(yrow, j0, N, (T)0, yy);
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const bool live = j0 + c < N;
        t[c] = live ? cat_relaxed_t(l[c], yy[c], tau) : cat_neg_inf<T>();
        sum_t += live ? t[c] : (T)0;
        sum_y += live ? yy[c] : (T)0;
      }
      cat_ms_push4(mt, t);
    }
    mt = group_ms(mt, G, pl.first);
    sum_t = group_sum(sum_t, G);
    sum_y = group_sum(sum_y, G);
    if (pl.lane == 0) lp[it] = cat_relaxed_lp(c0, sum_t, (T)N, cat_lse(mt), sum_y, exp_space != 0);
  }
}

template <typename T>
__global__ __launch_bounds__(THREADS) void k_cat_exp(const T* __restrict__ x, T* __restrict__ out, int64_t n) {
  const int64_t stride = (int64_t)gridDim.x * THREADS;
  for (int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x; i < n; i += stride) out[i] = cat_exp(x[i]);
}

// ---------------------------------------------------------------- host side
bool aligned_all(std::initializer_list<const void*> ps) {
  uintptr_t bits = 0;
  for (const void* p : ps) bits |= (uintptr_t)p;
  return (bits & 15u) == 0;
}
int check_shape(const void* logits, int64_t K, int64_t R, int64_t N) {
  if (!logits || N < 1 || K < 0 || R < 0) return ZS_EINVAL;
  if (N > (int64_t)INT32_MAX) return ZS_ENOTSUP;
  return 0;
}
// rows of a value with period P elements of `width` each: K R or R, else -1
int64_t period_rows(int64_t P, int64_t width, int64_t K, int64_t R) {
  if (P == K * R * width) return K * R;
  if (P == R * width) return R;
  return -1;
}
unsigned grid_of(int64_t items, int G) { return grid_for(items, THREADS / G, 256u * 16u); }
double relaxed_c0(int64_t N, double tau) { return lgamma((double)N) + (double)(N - 1) * log(tau); }

#define ZS_CAT_LAUNCH(vec, kern, targs, grid, st, ...)                                              \
  do {                                                                                              \
    if (vec) hipLaunchKernelGGL((kern<T, true targs>), dim3(grid), dim3(THREADS), 0, st, __VA_ARGS__);   \
    else hipLaunchKernelGGL((kern<T, false targs>), dim3(grid), dim3(THREADS), 0, st, __VA_ARGS__);      \
  } while (0)
#define ZS_NOARG

template <typename T>
int cat_sample(const void* logits, const void* u, int64_t* idx, void* onehot, void* lp, int64_t K, int64_t R, int64_t N,
               uint64_t seed, uint64_t call, const uint64_t* rs, void* stream) {
  const int rc = check_shape(logits, K, R, N);
  if (rc) return rc;
  if (K == 0 || R == 0) return 0;
  if (!idx && !onehot && !lp) return ZS_EINVAL;
  const int G = cat_group_lanes(N);
  const bool vec = (N & 3) == 0 && aligned_all({logits, u, onehot});
  ZS_CAT_LAUNCH(vec, k_cat_sample, ZS_NOARG, grid_of(K * R, G), (hipStream_t)stream, (const T*)logits, (const T*)u, idx, (T*)onehot,
                (T*)lp, K * R, R, N, G, seed, call, rs);
  ZS_CHECK_LAUNCH();
  return 0;
}

template <typename T>
int cat_logprob(const void* logits, const int64_t* idx, const void* x, int64_t Px, void* lp, int64_t K, int64_t R, int64_t N,
                void* stream) {
  const int rc = check_shape(logits, K, R, N);
  if (rc) return rc;
  if (K == 0 || R == 0) return 0;
  if ((idx != nullptr) == (x != nullptr) || !lp) return ZS_EINVAL;
  const int64_t prow = period_rows(Px, x ? N : 1, K, R);
  if (prow < 0) return ZS_EINVAL;
  const int G = cat_group_lanes(N);
  const bool vec = (N & 3) == 0 && aligned_all({logits, x});
  ZS_CAT_LAUNCH(vec, k_cat_logprob, ZS_NOARG, grid_of(K * R, G), (hipStream_t)stream, (const T*)logits, idx, (const T*)x, prow, (T*)lp,
                K * R, R, N, G);
  ZS_CHECK_LAUNCH();
  return 0;
}

template <typename T>
int cat_logprob_bwd(const void* logits, const int64_t* idx, const void* x, int64_t Px, const void* glp, void* glogits, void* gx,
                    int64_t K, int64_t R, int64_t N, void* stream) {
  const int rc = check_shape(logits, K, R, N);
  if (rc) return rc;
  if (K == 0 || R == 0) return 0;
  if ((idx != nullptr) == (x != nullptr) || !glp || (!glogits && !gx) || (gx && !x)) return ZS_EINVAL;
  const int64_t prow = period_rows(Px, x ? N : 1, K, R);
  if (prow < 0) return ZS_EINVAL;
  const int G = cat_group_lanes(N);
  const bool vec = (N & 3) == 0 && aligned_all({logits, x, glogits, gx});
  ZS_CAT_LAUNCH(vec, k_cat_logprob_bwd, ZS_NOARG, grid_of(R, G), (hipStream_t)stream, (const T*)logits, idx, (const T*)x, prow,
                (const T*)glp, (T*)glogits, (T*)gx, K, R, N, G);
  ZS_CHECK_LAUNCH();
  return 0;
}

template <typename T>
int relaxed_sample(const void* logits, const void* u, double tau, int exp_space, void* y, void* ey, void* lp, int64_t K, int64_t R,
                   int64_t N, uint64_t seed, uint64_t call, const uint64_t* rs, void* stream) {
  const int rc = check_shape(logits, K, R, N);
  if (rc) return rc;
  if (!(tau > 0.0) || !(tau < INFINITY)) return ZS_EINVAL;
  if (K == 0 || R == 0) return 0;
  if (!exp_space) ey = nullptr;
  if (!y && !ey && !lp) return ZS_EINVAL;
  const int G = cat_group_lanes(N);
  const bool vec = (N & 3) == 0 && aligned_all({logits, u, y, ey});
  ZS_CAT_LAUNCH(vec, k_cat_relaxed_sample, ZS_NOARG, grid_of(K * R, G), (hipStream_t)stream, (const T*)logits, (const T*)u, (T*)y,
                (T*)ey, (T*)lp, K * R, R, N, G, (T)tau, (T)relaxed_c0(N, tau), exp_space, seed, call, rs);
  ZS_CHECK_LAUNCH();
  return 0;
}

template <typename T>
int relaxed_sample_bwd(const void* logits, const void* y, double tau, int exp_space, const void* gy, const void* gey, const void* glp,
                       void* glogits, int64_t K, int64_t R, int64_t N, void* stream) {
  const int rc = check_shape(logits, K, R, N);
  if (rc) return rc;
  if (!(tau > 0.0) || !(tau < INFINITY)) return ZS_EINVAL;
  if (K == 0 || R == 0) return 0;
  if (!exp_space) gey = nullptr;
  if (!y || !glogits || (!gy && !gey && !glp)) return ZS_EINVAL;
  const int G = cat_group_lanes(N);
  const bool vec = (N & 3) == 0 && aligned_all({logits, y, gy, gey, glogits});
#define ZS_MODE0 , 0
  ZS_CAT_LAUNCH(vec, k_cat_relaxed_bwd, ZS_MODE0, grid_of(R, G), (hipStream_t)stream, (const T*)logits, (const T*)y, K * R,
                (const T*)gy, (const T*)gey, (const T*)glp, (T*)nullptr, (T*)glogits, K, R, N, G, (T)tau, exp_space);
  ZS_CHECK_LAUNCH();
  return 0;
}

template <typename T>
int relaxed_logprob(const void* logits, const void* y, int64_t Py, double tau, int exp_space, void* lp, int64_t K, int64_t R,
                    int64_t N, void* stream) {
  const int rc = check_shape(logits, K, R, N);
  if (rc) return rc;
  if (!(tau > 0.0) || !(tau < INFINITY)) return ZS_EINVAL;
  if (K == 0 || R == 0) return 0;
  if (!y || !lp) return ZS_EINVAL;
  const int64_t prow = period_rows(Py, N, K, R);
  if (prow < 0) return ZS_EINVAL;
  const int G = cat_group_lanes(N);
  const bool vec = (N & 3) == 0 && aligned_all({logits, y});
  ZS_CAT_LAUNCH(vec, k_cat_relaxed_logprob, ZS_NOARG, grid_of(K * R, G), (hipStream_t)stream, (const T*)logits, (const T*)y, prow,
                (T*)lp, K * R, R, N, G, (T)tau, (T)relaxed_c0(N, tau), exp_space);
  ZS_CHECK_LAUNCH();
  return 0;
}

template <typename T>
int relaxed_logprob_bwd(const void* logits, const void* y, int64_t Py, double tau, int exp_space, const void* glp, void* gy,
                        void* glogits, int64_t K, int64_t R, int64_t N, void* stream) {
  const int rc = check_shape(logits, K, R, N);
  if (rc) return rc;
  if (!(tau > 0.0) || !(tau < INFINITY)) return ZS_EINVAL;
  if (K == 0 || R == 0) return 0;
  if (!y || !glp || (!gy && !glogits)) return ZS_EINVAL;
  const int64_t prow = period_rows(Py, N, K, R);
  if (prow < 0) return ZS_EINVAL;
  const int G = cat_group_lanes(N);
  const bool vec = (N & 3) == 0 && aligned_all({logits, y, gy, glogits});
#define ZS_MODE1 , 1
  ZS_CAT_LAUNCH(vec, k_cat_relaxed_bwd, ZS_MODE1, grid_of(R, G), (hipStream_t)stream, (const T*)logits, (const T*)y, prow,
                (const T*)nullptr, (const T*)nullptr, (const T*)glp, (T*)gy, (T*)glogits, K, R, N, G, (T)tau, exp_space);
  ZS_CHECK_LAUNCH();
  return 0;
}

}  // namespace

extern "C" int zs_cat_abi_version(void) { return ZS_CAT_ABI_VERSION; }
extern "C" int zs_cat_group_lanes(int64_t N) { return N < 1 ? 0 : cat_group_lanes(N); }

template <typename T>
int cat_exp_of(const void* x, void* out, int64_t n, void* stream) {
  if (n < 0) return ZS_EINVAL;
  if (n == 0) return 0;
  if (!x || !out) return ZS_EINVAL;
  hipLaunchKernelGGL((k_cat_exp<T>), dim3(grid_for(n, THREADS)), dim3(THREADS), 0, (hipStream_t)stream, (const T*)x, (T*)out, n);
  ZS_CHECK_LAUNCH();
  return 0;
}

#define ZS_CAT_ENTRY(SFX, T)                                                                                                         \
  extern "C" int zs_cat_exp##SFX(const void* x, void* out, int64_t n, void* stream) { return cat_exp_of<T>(x, out, n, stream); }    \
  extern "C" int zs_cat_sample_logprob##SFX(const void* logits, const void* u, int64_t* idx, void* onehot, void* lp, int64_t K,      \
                                            int64_t R, int64_t N, uint64_t seed, uint64_t call, const uint64_t* rng_state,          \
                                            void* stream) {                                                                          \
    return cat_sample<T>(logits, u, idx, onehot, lp, K, R, N, seed, call, rng_state, stream);                                        \
  }                                                                                                                                  \
  extern "C" int zs_cat_logprob##SFX(const void* logits, const int64_t* idx, const void* x, int64_t Px, void* lp, int64_t K,         \
                                     int64_t R, int64_t N, void* stream) {                                                           \
    return cat_logprob<T>(logits, idx, x, Px, lp, K, R, N, stream);                                                                  \
  }                                                                                                                                  \
  extern "C" int zs_cat_logprob_bwd##SFX(const void* logits, const int64_t* idx, const void* x, int64_t Px, const void* glp,         \
                                         void* glogits, void* gx, int64_t K, int64_t R, int64_t N, void* stream) {                   \
    return cat_logprob_bwd<T>(logits, idx, x, Px, glp, glogits, gx, K, R, N, stream);                                                \
  }                                                                                                                                  \
  extern "C" int zs_cat_expconcrete_sample_logprob##SFX(const void* logits, const void* u, double tau, int exp_space, void* y,       \
                                                        void* ey, void* lp, int64_t K, int64_t R, int64_t N, uint64_t seed,          \
                                                        uint64_t call, const uint64_t* rng_state, void* stream) {                    \
    return relaxed_sample<T>(logits, u, tau, exp_space, y, ey, lp, K, R, N, seed, call, rng_state, stream);                          \
  }                                                                                                                                  \
  extern "C" int zs_cat_expconcrete_sample_logprob_bwd##SFX(const void* logits, const void* y, double tau, int exp_space,            \
                                                            const void* gy, const void* gey, const void* glp, void* glogits,        \
                                                            int64_t K, int64_t R, int64_t N, void* stream) {                         \
    return relaxed_sample_bwd<T>(logits, y, tau, exp_space, gy, gey, glp, glogits, K, R, N, stream);                                 \
  }                                                                                                                                  \
  extern "C" int zs_cat_expconcrete_logprob##SFX(const void* logits, const void* y, int64_t Py, double tau, int exp_space, void* lp, \
                                                 int64_t K, int64_t R, int64_t N, void* stream) {                                    \
    return relaxed_logprob<T>(logits, y, Py, tau, exp_space, lp, K, R, N, stream);                                                   \
  }                                                                                                                                  \
  extern "C" int zs_cat_expconcrete_logprob_bwd##SFX(const void* logits, const void* y, int64_t Py, double tau, int exp_space,       \
                                                     const void* glp, void* gy, void* glogits, int64_t K, int64_t R, int64_t N,      \
                                                     void* stream) {                                                                 \
    return relaxed_logprob_bwd<T>(logits, y, Py, tau, exp_space, glp, gy, glogits, K, R, N, stream);                                 \
  }

ZS_CAT_ENTRY(_f32, float)
ZS_CAT_ENTRY(_f64, double)
