// The admixture (topic-model) likelihood: lp = sum_v X log(softmax(H) @ softmax(B)) and its gradients for H and B
// (include/zs_topic.h; its own library, ../lib/libzs_topic.so, `make topic`).
//
// The first kernels of this package on the matrix cores.  A torch composition writes the [R, V] product, takes its logarithm in
// a second pass, multiplies by the counts in a third and keeps [R, V] temporaries for the backward; here the product lives in
// the accumulator registers of v_mfma_{f32,f64}_16x16x4 tile by tile and only row sums and two thin gradients reach memory.
// Operands are shifted to (0, 1] (zs_topic.h) so that the matrix instructions multiply plain numbers.  One template over the
// element type: the two instructions have the same operand layout and differ in the row map of the accumulator
// (MfmaTile<T>::acc_row) and in the width of a panel.
//
// A lane l = 16 q + m of a wave holds, for the step s of a 16 x 16 tile, E[row m][4 s + q] and Bs[4 s + q][column m] -- the
// same two values serve the tile and its transpose, by the order of the instruction's operands:
//   run(e, b)   acc[v] = pred[row acc_row(q, v)][column m]        (grad_topic: the second product contracts over ROWS)
//   run(b, e)   acc[v] = pred[column acc_row(q, v)][row m]        (logprob, grad_doc: the second product contracts over COLUMNS)
// In both backwards the weights g x / acc, left where the accumulator has them, are the B operand of the second product: the
// contraction index of step v is acc_row(q, v), and the A operand is read from LDS (the panel) or memory (E) at that index.
#include "zs_common.h"
#include "zs_topic_math.h"
#include "../../include/zs_hip.h"
#include "../../include/zs_topic.h"

#pragma clang fp contract(off)

using namespace zs;

namespace {

constexpr int TOPIC_THREADS = 256;

// ---------------------------------------------------------------- the prologue
// blocks [0, K): lse of a row of B;  then a wave per row of H: E, Z, log Z;  then a wave per row of X: N
template <typename T>
__global__ __launch_bounds__(TOPIC_THREADS) void k_topic_prepare(const T* __restrict__ H, const T* __restrict__ B, const T* __restrict__ X,
                                                                 T* __restrict__ prep, int64_t R, int64_t K, int64_t V, int64_t Dx) {
  __shared__ T sh[4];
  const TopicPrep<T> w = topic_prep(prep, R, K, Dx);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t b = blockIdx.x, row_blocks = (R + 3) / 4;
  if (b < K) {
    const T* row = B + b * V;
    T m = neg_inf<T>();
    for (int64_t v = tid; v < V; v += TOPIC_THREADS) m = max_of(m, row[v]);
    m = block_max_256(m, sh);
    T s = 0;
    for (int64_t v = tid; v < V; v += TOPIC_THREADS) s += topic_exp(row[v] - m);
    s = block_sum_256(s, sh);
    if (tid == 0) w.lse[b] = m + topic_log(s);
  } else if (b < K + row_blocks) {
    const int64_t r = (b - K) * 4 + wave;
    if (r >= R) return;
    const int64_t K16 = topic_k16(K);
    const int k0 = lane, k1 = lane + 64;
    const T h0 = k0 < K ? H[r * K + k0] : neg_inf<T>(), h1 = k1 < K ? H[r * K + k1] : neg_inf<T>();
    const T m = wave_max(max_of(h0, h1));
    const T e0 = k0 < K ? topic_exp(h0 - m) : (T)0, e1 = k1 < K ? topic_exp(h1 - m) : (T)0;
    const T z = wave_sum(e0 + e1);
    if (k0 < K16) w.e[r * K16 + k0] = e0;
    if (k1 < K16) w.e[r * K16 + k1] = e1;
    if (lane == 0) {
      w.z[r] = z;
      w.logz[r] = topic_log(z);
    }
  } else {
    const int64_t d = (b - K - row_blocks) * 4 + wave;
    if (d >= Dx) return;
    T s = 0;
    for (int64_t v = lane; v < V; v += 64) {
      const T x = X[d * V + v];
      s += x > (T)0 ? x : (T)0;
    }
    s = wave_sum(s);
    if (lane == 0) w.n[d] = s;
  }
}

// ---------------------------------------------------------------- staging (the tile product is zs_tile_math.h's panel_tile)
// Bs[k][j] = exp(B[k, col0 + j] - lse_k - c_j) for k < K16 (zero for k >= K and past the last column), cs[j] = c_j.
// Every thread of the workgroup calls it; the panel is ready when it returns.
template <typename T>
__device__ __forceinline__ void topic_stage_panel(const T* __restrict__ B, const T* __restrict__ lse, int64_t V, int K, int K16,
                                                  int64_t col0, T* Bs, T* cs) {
  constexpr int P = MfmaPanel<T>::PANEL, LD = MfmaPanel<T>::LD;
  const int n = K16 * P, threads = blockDim.x;
  __syncthreads();          // the previous panel's readers are done
  for (int i = threadIdx.x; i < n; i += threads) {
    const int k = i / P, j = i % P;
    const int64_t v = col0 + j;
    Bs[k * LD + j] = (k < K && v < V) ? B[(int64_t)k * V + v] - lse[k] : neg_inf<T>();
  }
  __syncthreads();
  if ((int)threadIdx.x < P) {
    const int j = threadIdx.x;
    T m = neg_inf<T>();
    for (int k = 0; k < K; ++k) m = max_of(m, Bs[k * LD + j]);
    cs[j] = col0 + j < V ? m : (T)0;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < n; i += threads) {
    const int k = i / P, j = i % P;
    const T s = Bs[k * LD + j];
    Bs[k * LD + j] = (k < K && col0 + j < V) ? topic_exp(s - cs[j]) : (T)0;
  }
  __syncthreads();
}

// the lane's share of E for the 16 rows of a tile: a[s] = E[row][4 s + q]
template <typename T>
__device__ __forceinline__ void topic_load_rows(const T* __restrict__ E, int K16, int64_t row, int q, int steps, T (&a)[ZS_TOPIC_MAX_STEPS]) {
#pragma unroll
  for (int s = 0; s < ZS_TOPIC_MAX_STEPS; ++s) a[s] = s < steps ? E[row * K16 + 4 * s + q] : (T)0;
}

template <typename T>
size_t topic_lds_bytes_for(int64_t K16, int extra) {
  return sizeof(T) * (size_t)(K16 * MfmaPanel<T>::LD + MfmaPanel<T>::PANEL + extra);
}

// ---------------------------------------------------------------- lp
template <typename T>
__global__ __launch_bounds__(TOPIC_THREADS) void k_topic_logprob(const T* __restrict__ B, const T* __restrict__ X, const T* __restrict__ prep,
                                                                 T* __restrict__ part, int64_t R, int K, int64_t V, int64_t Dx) {
  constexpr int P = MfmaPanel<T>::PANEL, LD = MfmaPanel<T>::LD;
  const int K16 = (int)topic_k16(K), steps = topic_steps(K);
  const TopicPrep<T> w = topic_prep(const_cast<T*>(prep), R, K, Dx);
  T* Bs = tile_lds<T>();
  T* cs = Bs + K16 * LD;
  const int64_t panel = blockIdx.x, col0 = panel * P;
  topic_stage_panel(B, w.lse, V, K, K16, col0, Bs, cs);
  const int wave = mfma_wave(threadIdx.x), waves = blockDim.x >> 6, m = mfma_m(threadIdx.x), q = mfma_q(threadIdx.x);
  const int64_t tiles = blocks16(R);
  T a[ZS_TOPIC_MAX_STEPS];
  for (int64_t rt = wave; rt < tiles; rt += waves) {
    const int64_t r = rt * 16 + m;
    const bool live = r < R;
    const int64_t rc = live ? r : R - 1;
    topic_load_rows(w.e, K16, rc, q, steps, a);
    const T* xr = X + mod_fast(rc, Dx) * V;
    T sum = 0;
#pragma unroll
    for (int ct = 0; ct < P / 16; ++ct) {
      if (col0 + ct * 16 < V) {
        const typename Mfma<T>::Acc acc = panel_tile<T, false>(a, Bs + ct * 16, q, m, steps);
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          const int j = ct * 16 + MfmaTile<T>::acc_row(q, v);
          const T x = (live && col0 + j < V) ? xr[col0 + j] : (T)0;
          sum += topic_term(x, cs[j], acc[v]);
        }
      }
    }
    sum += __shfl_xor(sum, 16, ZS_WAVE);          // the four lanes of a row: q = 0 .. 3
    sum += __shfl_xor(sum, 32, ZS_WAVE);
    if (q == 0 && live) part[panel * R + r] = sum;
  }
}

template <typename T>
__global__ __launch_bounds__(TOPIC_THREADS) void k_topic_logprob_finish(const T* __restrict__ part, const T* __restrict__ prep,
                                                                        T* __restrict__ lp, int64_t R, int64_t K, int64_t Dx, int64_t panels) {
  const TopicPrep<T> w = topic_prep(const_cast<T*>(prep), R, K, Dx);
  const int64_t r = (int64_t)blockIdx.x * TOPIC_THREADS + threadIdx.x;
  if (r >= R) return;
  T s = 0;
  for (int64_t p = 0; p < panels; ++p) s += part[p * R + r];
  lp[r] = s - w.n[mod_fast(r, Dx)] * w.logz[r];
}

// ---------------------------------------------------------------- dH
template <typename T>
__global__ __launch_bounds__(TOPIC_THREADS) void k_topic_grad_doc(const T* __restrict__ B, const T* __restrict__ X, const T* __restrict__ g,
                                                                  const T* __restrict__ prep, T* __restrict__ part, int64_t R, int K,
                                                                  int64_t V, int64_t Dx, int64_t panels) {
  constexpr int P = MfmaPanel<T>::PANEL, LD = MfmaPanel<T>::LD;
  typedef typename Mfma<T>::Acc Acc;
  const int K16 = (int)topic_k16(K), steps = topic_steps(K), ktiles = K16 / 16;
  const TopicPrep<T> w = topic_prep(const_cast<T*>(prep), R, K, Dx);
  T* Bs = tile_lds<T>();
  T* cs = Bs + K16 * LD;
  const int wave = mfma_wave(threadIdx.x), waves = blockDim.x >> 6, m = mfma_m(threadIdx.x), q = mfma_q(threadIdx.x);
  const int64_t r = ((int64_t)blockIdx.x * waves + wave) * 16 + m;
  const bool live = r < R;
  const int64_t rc = live ? r : R - 1;
  T a[ZS_TOPIC_MAX_STEPS];
  topic_load_rows(w.e, K16, rc, q, steps, a);
  const T* xr = X + mod_fast(rc, Dx) * V;
  const T gr = live ? g[rc] : (T)0;
  Acc d[ZS_TOPIC_MAX_KTILES];          // d[kt][v] = sum_v' W'[row m][v'] Bs[16 kt + acc_row(q, v)][v']
#pragma unroll
  for (int kt = 0; kt < ZS_TOPIC_MAX_KTILES; ++kt) d[kt] = Acc{0, 0, 0, 0};
  const int64_t splits = gridDim.y;
  for (int64_t panel = blockIdx.y; panel < panels; panel += splits) {
    const int64_t col0 = panel * P;
    topic_stage_panel(B, w.lse, V, K, K16, col0, Bs, cs);
#pragma unroll
    for (int ct = 0; ct < P / 16; ++ct) {
      if (col0 + ct * 16 < V) {
        const Acc acc = panel_tile<T, false>(a, Bs + ct * 16, q, m, steps);
        T wgt[4];
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          const int64_t col = col0 + ct * 16 + MfmaTile<T>::acc_row(q, v);
          const T x = (live && col < V) ? xr[col] : (T)0;
          wgt[v] = topic_weight(gr, x, acc[v]);
        }
#pragma unroll
        for (int kt = 0; kt < ZS_TOPIC_MAX_KTILES; ++kt) {
          if (kt < ktiles) {
#pragma unroll
            for (int v = 0; v < 4; ++v)
              d[kt] = Mfma<T>::run(Bs[(kt * 16 + m) * LD + ct * 16 + MfmaTile<T>::acc_row(q, v)], wgt[v], d[kt]);
          }
        }
      }
    }
  }
  if (!live) return;
  T* out = part + ((int64_t)blockIdx.y * R + r) * K16;
#pragma unroll
  for (int kt = 0; kt < ZS_TOPIC_MAX_KTILES; ++kt) {
    if (kt < ktiles) {
#pragma unroll
      for (int v = 0; v < 4; ++v) out[kt * 16 + MfmaTile<T>::acc_row(q, v)] = d[kt][v];
    }
  }
}

// dH[r, k] = E[r, k] (sum over the splits - g_r N_r / Z_r)  ( = theta (dtheta - g N), with theta = E / Z and dtheta = Z sum )
template <typename T>
__global__ __launch_bounds__(TOPIC_THREADS) void k_topic_grad_doc_finish(const T* __restrict__ part, const T* __restrict__ g,
                                                                         const T* __restrict__ prep, T* __restrict__ dH, int64_t R,
                                                                         int64_t K, int64_t Dx, int64_t splits) {
  const TopicPrep<T> w = topic_prep(const_cast<T*>(prep), R, K, Dx);
  const int64_t i = (int64_t)blockIdx.x * TOPIC_THREADS + threadIdx.x, K16 = topic_k16(K);
  if (i >= R * K) return;
  int64_t r, k;
  divmod(i, K, r, k);
  T s = 0;
  for (int64_t sp = 0; sp < splits; ++sp) s += part[(sp * R + r) * K16 + k];
  dH[i] = w.e[r * K16 + k] * (s - g[r] * w.n[mod_fast(r, Dx)] / w.z[r]);
}

// ---------------------------------------------------------------- dB
// a wave per 16 columns of the panel (blockDim = 64 P / 16); G[k][column] = sum_r E[r, k] W'[r, column] over ALL rows
template <typename T>
__global__ __launch_bounds__(TOPIC_THREADS) void k_topic_grad_topic(const T* __restrict__ B, const T* __restrict__ X, const T* __restrict__ g,
                                                                    const T* __restrict__ prep, T* __restrict__ part, T* __restrict__ dB,
                                                                    int64_t R, int K, int64_t V, int64_t Dx) {
  constexpr int P = MfmaPanel<T>::PANEL, LD = MfmaPanel<T>::LD;
  typedef typename Mfma<T>::Acc Acc;
  const int K16 = (int)topic_k16(K), steps = topic_steps(K), ktiles = K16 / 16;
  const TopicPrep<T> w = topic_prep(const_cast<T*>(prep), R, K, Dx);
  T* Bs = tile_lds<T>();
  T* cs = Bs + K16 * LD;
  T* ss = cs + P;          // [waves][K16]: the waves' sums of T over their 16 columns
  const int64_t panel = blockIdx.x, col0 = panel * P;
  topic_stage_panel(B, w.lse, V, K, K16, col0, Bs, cs);
  const int wave = mfma_wave(threadIdx.x), waves = blockDim.x >> 6, m = mfma_m(threadIdx.x), q = mfma_q(threadIdx.x);
  const int64_t col = col0 + wave * 16 + m, tiles = blocks16(R);
  const bool col_live = col < V;
  const T* Bc = Bs + wave * 16;
  Acc G[ZS_TOPIC_MAX_KTILES];
#pragma unroll
  for (int kt = 0; kt < ZS_TOPIC_MAX_KTILES; ++kt) G[kt] = Acc{0, 0, 0, 0};
  T a[ZS_TOPIC_MAX_STEPS];
  if (col0 + wave * 16 < V) {
    for (int64_t rt = 0; rt < tiles; ++rt) {
      const int64_t ra = rt * 16 + m;
      topic_load_rows(w.e, K16, ra < R ? ra : R - 1, q, steps, a);
      const Acc acc = panel_tile<T, true>(a, Bc, q, m, steps);
      T wgt[4];
      int64_t rows[4];
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int64_t r = rt * 16 + MfmaTile<T>::acc_row(q, v);
        const bool live = r < R && col_live;
        rows[v] = r < R ? r : R - 1;
        const T x = live ? X[mod_fast(rows[v], Dx) * V + col] : (T)0;
        wgt[v] = topic_weight(live ? g[rows[v]] : (T)0, x, acc[v]);
      }
#pragma unroll
      for (int kt = 0; kt < ZS_TOPIC_MAX_KTILES; ++kt) {
        if (kt < ktiles) {
#pragma unroll
          for (int v = 0; v < 4; ++v) G[kt] = Mfma<T>::run(w.e[rows[v] * K16 + kt * 16 + m], wgt[v], G[kt]);
        }
      }
    }
  }
  // T[k, column] = Bs[k][column] G[k][column]  ( = phi dphi: the column scale exp(c_v) of phi cancels that of W )
#pragma unroll
  for (int kt = 0; kt < ZS_TOPIC_MAX_KTILES; ++kt) {
    if (kt < ktiles) {
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int k = kt * 16 + MfmaTile<T>::acc_row(q, v);
        const T t = Bc[k * LD + m] * G[kt][v];
        if (k < K && col_live) dB[(int64_t)k * V + col] = t;
        const T row = group_sum(t, 16);          // over the wave's 16 columns
        if (m == 0) ss[wave * K16 + k] = row;
      }
    }
  }
  __syncthreads();
  for (int k = threadIdx.x; k < K16; k += blockDim.x) {
    T s = 0;
    for (int wv = 0; wv < waves; ++wv) s += ss[wv * K16 + k];
    part[panel * K16 + k] = s;
  }
}

// dB[k, v] = T[k, v] - phi[k, v] s_k, s_k the sum of the panels' partials; grid (column chunks of 1024, K)
template <typename T>
__global__ __launch_bounds__(TOPIC_THREADS) void k_topic_grad_topic_finish(const T* __restrict__ B, const T* __restrict__ prep,
                                                                           const T* __restrict__ part, T* __restrict__ dB, int64_t R,
                                                                           int64_t K, int64_t V, int64_t Dx, int64_t panels) {
  __shared__ T sh[4];
  const TopicPrep<T> w = topic_prep(const_cast<T*>(prep), R, K, Dx);
  const int64_t k = blockIdx.y, K16 = topic_k16(K);
  T s = 0;
  for (int64_t p = threadIdx.x; p < panels; p += TOPIC_THREADS) s += part[p * K16 + k];
  s = block_sum_256(s, sh);
  const T lse = w.lse[k];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int64_t v = ((int64_t)blockIdx.x * 4 + i) * TOPIC_THREADS + threadIdx.x;
    if (v < V) dB[k * V + v] = dB[k * V + v] - topic_exp(B[k * V + v] - lse) * s;
  }
}

// ---------------------------------------------------------------- the entry points
// 0 = go on, 1 = nothing to do, else the code to return
int topic_check(bool pointers, int64_t R, int64_t K, int64_t V, int64_t Dx) {
  if (!pointers || R < 0 || K < 1 || V < 1 || Dx < 1 || R % Dx != 0) return ZS_EINVAL;
  if (K > ZS_TOPIC_MAX_TOPICS || R >= ((int64_t)1 << 31) || V >= ((int64_t)1 << 31)) return ZS_ENOTSUP;
  return R == 0 ? 1 : 0;
}
unsigned topic_blocks(int64_t n) { return (unsigned)((n + TOPIC_THREADS - 1) / TOPIC_THREADS); }

template <typename T>
int topic_prepare(const void* H, const void* B, const void* X, void* prep, int64_t R, int64_t K, int64_t V, int64_t Dx, void* stream) {
  const int rc = topic_check(H && B && X && prep, R, K, V, Dx);
  if (rc) return rc == 1 ? 0 : rc;
  const int64_t blocks = K + (R + 3) / 4 + (Dx + 3) / 4;
  hipLaunchKernelGGL((k_topic_prepare<T>), dim3((unsigned)blocks), dim3(TOPIC_THREADS), 0, (hipStream_t)stream, (const T*)H, (const T*)B,
                     (const T*)X, (T*)prep, R, K, V, Dx);
  ZS_CHECK_LAUNCH();
  return 0;
}

template <typename T>
int topic_logprob(const void* B, const void* X, const void* prep, void* part, void* lp, int64_t R, int64_t K, int64_t V, int64_t Dx,
                  void* stream) {
  const int rc = topic_check(B && X && prep && part && lp, R, K, V, Dx);
  if (rc) return rc == 1 ? 0 : rc;
  const int64_t panels = zs::panels(sizeof(T), V);
  hipLaunchKernelGGL((k_topic_logprob<T>), dim3((unsigned)panels), dim3(TOPIC_THREADS), topic_lds_bytes_for<T>(topic_k16(K), 0),
                     (hipStream_t)stream, (const T*)B, (const T*)X, (const T*)prep, (T*)part, R, (int)K, V, Dx);
  ZS_CHECK_LAUNCH();
  hipLaunchKernelGGL((k_topic_logprob_finish<T>), dim3(topic_blocks(R)), dim3(TOPIC_THREADS), 0, (hipStream_t)stream, (const T*)part,
                     (const T*)prep, (T*)lp, R, K, Dx, panels);
  ZS_CHECK_LAUNCH();
  return 0;
}

template <typename T>
int topic_grad_doc(const void* B, const void* X, const void* g, const void* prep, void* part, void* dH, int64_t R, int64_t K, int64_t V,
                   int64_t Dx, int64_t splits, void* stream) {
  const int rc = topic_check(B && X && g && prep && part && dH, R, K, V, Dx);
  if (rc) return rc == 1 ? 0 : rc;          // (R == 0 before the splits: zs_topic_doc_splits has none to offer for no rows)
  const int64_t panels = zs::panels(sizeof(T), V);
  if (splits < 1 || splits > panels || splits > 65535) return ZS_EINVAL;
  const int64_t row_blocks = (R + ZS_TOPIC_ROWS_PER_BLOCK - 1) / ZS_TOPIC_ROWS_PER_BLOCK;
  hipLaunchKernelGGL((k_topic_grad_doc<T>), dim3((unsigned)row_blocks, (unsigned)splits), dim3(TOPIC_THREADS),
                     topic_lds_bytes_for<T>(topic_k16(K), 0), (hipStream_t)stream, (const T*)B, (const T*)X, (const T*)g, (const T*)prep,
                     (T*)part, R, (int)K, V, Dx, panels);
  ZS_CHECK_LAUNCH();
  hipLaunchKernelGGL((k_topic_grad_doc_finish<T>), dim3(topic_blocks(R * K)), dim3(TOPIC_THREADS), 0, (hipStream_t)stream, (const T*)part,
                     (const T*)g, (const T*)prep, (T*)dH, R, K, Dx, splits);
  ZS_CHECK_LAUNCH();
  return 0;
}

template <typename T>
int topic_grad_topic(const void* B, const void* X, const void* g, const void* prep, void* part, void* dB, int64_t R, int64_t K, int64_t V,
                     int64_t Dx, void* stream) {
  const int rc = topic_check(B && X && g && prep && part && dB, R, K, V, Dx);
  if (rc) return rc == 1 ? 0 : rc;
  const int64_t panels = zs::panels(sizeof(T), V), K16 = topic_k16(K);
  const int waves = MfmaPanel<T>::PANEL / 16;
  hipLaunchKernelGGL((k_topic_grad_topic<T>), dim3((unsigned)panels), dim3(64 * waves), topic_lds_bytes_for<T>(K16, waves * (int)K16),
                     (hipStream_t)stream, (const T*)B, (const T*)X, (const T*)g, (const T*)prep, (T*)part, (T*)dB, R, (int)K, V, Dx);
  ZS_CHECK_LAUNCH();
  hipLaunchKernelGGL((k_topic_grad_topic_finish<T>), dim3((unsigned)((V + 4 * TOPIC_THREADS - 1) / (4 * TOPIC_THREADS)), (unsigned)K),
                     dim3(TOPIC_THREADS), 0, (hipStream_t)stream, (const T*)B, (const T*)prep, (const T*)part, (T*)dB, R, K, V, Dx, panels);
  ZS_CHECK_LAUNCH();
  return 0;
}

}  // namespace

extern "C" int zs_topic_abi_version(void) { return ZS_TOPIC_ABI_VERSION; }
extern "C" int zs_topic_max_topics(void) { return ZS_TOPIC_MAX_TOPICS; }
extern "C" int64_t zs_topic_panels(int elem_bytes, int64_t V) { return panels(elem_bytes, V); }
extern "C" int64_t zs_topic_doc_splits(int elem_bytes, int64_t R, int64_t V) { return topic_doc_splits(elem_bytes, R, V); }
extern "C" int64_t zs_topic_workspace_elems(int which, int elem_bytes, int64_t R, int64_t K, int64_t V, int64_t Dx, int64_t splits) {
  const int64_t panels = zs::panels(elem_bytes, V);
  if (panels == 0 || R < 0 || K < 1 || K > ZS_TOPIC_MAX_TOPICS || Dx < 1) return -1;
  switch (which) {
    case ZS_TOPIC_WS_PREP: return topic_prep_elems(R, K, Dx);
    case ZS_TOPIC_WS_LOGPROB: return panels * R;
    case ZS_TOPIC_WS_GRAD_DOC: return splits < 1 ? -1 : splits * R * topic_k16(K);
    case ZS_TOPIC_WS_GRAD_TOPIC: return panels * topic_k16(K);
    default: return -1;
  }
}

#define ZS_TOPIC_ENTRY(SFX, T)                                                                                                       \
  extern "C" int zs_topic_prepare##SFX(const void* H, const void* B, const void* X, void* prep, int64_t R, int64_t K, int64_t V,     \
                                       int64_t Dx, void* stream) {                                                                   \
    return topic_prepare<T>(H, B, X, prep, R, K, V, Dx, stream);                                                                     \
  }                                                                                                                                  \
  extern "C" int zs_topic_logprob##SFX(const void* B, const void* X, const void* prep, void* part, void* lp, int64_t R, int64_t K,   \
                                       int64_t V, int64_t Dx, void* stream) {                                                        \
    return topic_logprob<T>(B, X, prep, part, lp, R, K, V, Dx, stream);                                                              \
  }                                                                                                                                  \
  extern "C" int zs_topic_grad_doc##SFX(const void* B, const void* X, const void* g, const void* prep, void* part, void* dH,         \
                                        int64_t R, int64_t K, int64_t V, int64_t Dx, int64_t splits, void* stream) {                 \
    return topic_grad_doc<T>(B, X, g, prep, part, dH, R, K, V, Dx, splits, stream);                                                  \
  }                                                                                                                                  \
  extern "C" int zs_topic_grad_topic##SFX(const void* B, const void* X, const void* g, const void* prep, void* part, void* dB,       \
                                          int64_t R, int64_t K, int64_t V, int64_t Dx, void* stream) {                               \
    return topic_grad_topic<T>(B, X, g, prep, part, dB, R, K, V, Dx, stream);                                                        \
  }

ZS_TOPIC_ENTRY(_f32, float)
ZS_TOPIC_ENTRY(_f64, double)
