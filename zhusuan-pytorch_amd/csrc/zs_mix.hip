// The mixture-of-Gaussians density: lp = logsumexp_c ( log pi_c + log N(x; mean_c, diag sigma_c^2) ) and its gradients for x,
// logits, mean and logstd (include/zs_mix.h; its own library, ../lib/libzs_mix.so, `make mix`).
//
// The fourth user of the matrix cores after zs_topic, zs_matvar and zs_svgd.  A torch composition writes the [R, C] scores (the
// broadcast form even [R, C, D]), reduces them in a second pass and keeps them for the backward; here a score tile lives in the
// accumulator registers of v_mfma_{f32,f64}_16x16x4 and only lp, dx and partials of the thin parameter gradients reach memory.
// One template over the element type: the two instructions have the same operand layout and differ in the row map of the
// accumulator (MfmaTile<T>::acc_row), in where the odd neighbour of an even output row lives (mix_odd_row) and in the panel width.
//
// A lane l = 16 q + m of a wave holds, for the step s of a 16 x 16 tile, YY[row m][4 s + q] and Ws[4 s + q][component m] -- the
// same two values serve the tile and its transpose, by the order of the instruction's operands:
//   run(a, w)   acc[v] = score[row acc_row(q, v)][component m]        (grad_params: the second product contracts over ROWS)
//   run(w, a)   acc[v] = score[component acc_row(q, v)][row m]        (logprob, grad_x: the second product contracts over COMPONENTS)
// In both backwards the weights G = g exp(s - lp), left where the accumulator has them, are the B operand of the second product:
// the contraction index of step v is acc_row(q, v), and the A operand is read from LDS (the panel) or memory (x) at that index.
#include "zs_common.h"
#include "zs_mix_math.h"
#include "../../include/zs_hip.h"
#include "../../include/zs_mix.h"

#pragma clang fp contract(off)

using namespace zs;

namespace {

constexpr int MIX_THREADS = 256;

// out[n + 1] for the holder of an even output row n = 16 nt + acc_row(q, v) -- f32: the next register of the same lane; f64: the
// same register of the lane q ^ 1 (every lane of the wave makes the exchange)
__device__ __forceinline__ float mix_odd_row(const Mfma<float>::Acc& d, int v) { return d[v | 1]; }
__device__ __forceinline__ double mix_odd_row(const Mfma<double>::Acc& d, int v) { return __shfl_xor(d[v], 16, ZS_WAVE); }
template <typename T>
__device__ __forceinline__ bool mix_holds_even(int q, int v) { return (MfmaTile<T>::acc_row(q, v) & 1) == 0; }

// ---------------------------------------------------------------- the prologue
// blocks [0, D): the centre of a dimension;  block D: the log-sum-exp of the logits
template <typename T>
__global__ __launch_bounds__(MIX_THREADS) void k_mix_centre(const T* __restrict__ logits, const T* __restrict__ mean, T* __restrict__ prep,
                                                            int64_t C, int64_t D) {
  __shared__ T sh[4];
  const MixPrep<T> w = mix_prep(prep, C, D);
  const int tid = threadIdx.x;
  const int64_t d = blockIdx.x;
  if (d < D) {
    T s = 0;
    for (int64_t c = tid; c < C; c += MIX_THREADS) s += mean[c * D + d];
    s = block_sum_256(s, sh);
    if (tid == 0) w.cen[d] = s / (T)C;
  } else {
    T m = neg_inf<T>();
    for (int64_t c = tid; c < C; c += MIX_THREADS) m = max_of(m, logits[c]);
    m = block_max_256(m, sh);
    T s = 0;
    for (int64_t c = tid; c < C; c += MIX_THREADS) s += mix_exp(logits[c] - m);
    s = block_sum_256(s, sh);
    if (tid == 0) w.lse[0] = m + mix_log(s);
  }
}

// a thread per (padded) component: log_softmax, b and the column of the packed operand
template <typename T>
__global__ __launch_bounds__(MIX_THREADS) void k_mix_pack(const T* __restrict__ logits, const T* __restrict__ mean, const T* __restrict__ logstd,
                                                          T* __restrict__ prep, int64_t C, int D) {
  const MixPrep<T> w = mix_prep(prep, C, D);
  const int64_t c = (int64_t)blockIdx.x * MIX_THREADS + threadIdx.x;
  if (c >= w.cpad) return;
  const int K16 = mix_k16(D);
  const bool live = c < C;
  T sum_ls = 0, sum_q = 0;
  for (int d = 0; d < D; ++d) {
    T wnu = 0, mhw = 0;
    if (live) {
      const T ls = logstd[c * D + d], nu = mean[c * D + d] - w.cen[d];
      const T wt = mix_exp((T)-2 * ls);
      wnu = wt * nu;
      mhw = (T)-0.5 * wt;
      sum_ls += ls;
      sum_q += wnu * nu;
    }
    w.w[(int64_t)(2 * d) * w.cpad + c] = wnu;
    w.w[(int64_t)(2 * d + 1) * w.cpad + c] = mhw;
  }
  for (int k = 2 * D; k < K16; ++k) w.w[(int64_t)k * w.cpad + c] = (T)0;
  const T lsm = live ? logits[c] - w.lse[0] : neg_inf<T>();
  w.lsm[c] = lsm;
  w.b[c] = live ? ((lsm - sum_ls) - (T)(0.5 * ZS_MIX_LOG_2PI) * (T)D) - (T)0.5 * sum_q : neg_inf<T>();
}

// ---------------------------------------------------------------- staging (the tile product is zs_tile_math.h's panel_tile)
// Ws[k][j] = W[k, col0 + j] for k < K16, bs[j] = b[col0 + j] (-inf past the last component).  Every thread of the workgroup
// calls it; the panel is ready when it returns.
template <typename T>
__device__ __forceinline__ void mix_stage_panel(const MixPrep<T>& w, int K16, int64_t col0, T* Ws, T* bs) {
  constexpr int P = MfmaPanel<T>::PANEL, LD = MfmaPanel<T>::LD;
  const int n = K16 * P, threads = blockDim.x;
  __syncthreads();          // the previous panel's readers are done
  for (int i = threadIdx.x; i < n; i += threads) {
    const int k = i / P, j = i % P;
    Ws[k * LD + j] = w.w[(int64_t)k * w.cpad + col0 + j];
  }
  if ((int)threadIdx.x < P) bs[threadIdx.x] = w.b[col0 + threadIdx.x];
  __syncthreads();
}

// the lane's share of [y | y^2] (interleaved) for the 16 rows of a tile: a[s] = YY[row][4 s + q]
template <typename T>
__device__ __forceinline__ void mix_load_rows(const T* __restrict__ x, const T* __restrict__ cen, int D, int64_t row, int q,
                                              T (&a)[ZS_MIX_MAX_STEPS]) {
#pragma unroll
  for (int s = 0; s < ZS_MIX_MAX_STEPS; ++s) {
    const int k = 4 * s + q, d = k >> 1;
    a[s] = d < D ? mix_row_elem(x[row * D + d] - cen[d], k) : (T)0;
  }
}

template <typename T>
size_t mix_lds_bytes_for(int K16) { return sizeof(T) * (size_t)(K16 * MfmaPanel<T>::LD + MfmaPanel<T>::PANEL); }

// ---------------------------------------------------------------- lp
template <typename T>
__global__ __launch_bounds__(MIX_THREADS) void k_mix_logprob(const T* __restrict__ x, const T* __restrict__ prep, T* __restrict__ lp,
                                                             int64_t R, int64_t C, int D) {
  constexpr int P = MfmaPanel<T>::PANEL;
  const int K16 = mix_k16(D), steps = mix_steps(D);
  const MixPrep<T> w = mix_prep(const_cast<T*>(prep), C, D);
  T* Ws = tile_lds<T>();
  T* bs = Ws + K16 * MfmaPanel<T>::LD;
  const int wave = mfma_wave(threadIdx.x), waves = blockDim.x >> 6, m = mfma_m(threadIdx.x), q = mfma_q(threadIdx.x);
  const int64_t r = ((int64_t)blockIdx.x * waves + wave) * 16 + m;
  const bool live = r < R;
  T a[ZS_MIX_MAX_STEPS];
  mix_load_rows(x, w.cen, D, live ? r : R - 1, q, a);
  T mx = neg_inf<T>(), sm = 0;          // of the components this lane has seen: 4 per tile
  const int64_t panels = w.cpad / P;
  for (int64_t panel = 0; panel < panels; ++panel) {
    const int64_t col0 = panel * P;
    mix_stage_panel(w, K16, col0, Ws, bs);
#pragma unroll
    for (int ct = 0; ct < P / 16; ++ct) {
      if (col0 + ct * 16 < C) {
        const typename Mfma<T>::Acc acc = panel_tile<T, false>(a, Ws + ct * 16, q, m, steps);
        T s[4], tm = neg_inf<T>();
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          s[v] = acc[v] + bs[ct * 16 + MfmaTile<T>::acc_row(q, v)];
          tm = max_of(tm, s[v]);
        }
        mix_fold(mx, sm, s, tm);
      }
    }
  }
  T M = max_of(mx, __shfl_xor(mx, 16, ZS_WAVE));          // the four lanes of a row: q = 0 .. 3
  M = max_of(M, __shfl_xor(M, 32, ZS_WAVE));
  T sum = mix_rescale(mx, sm, M);
  sum += __shfl_xor(sum, 16, ZS_WAVE);
  sum += __shfl_xor(sum, 32, ZS_WAVE);
  if (q == 0 && live) lp[r] = M + mix_log(sum);
}

// ---------------------------------------------------------------- dx
template <typename T>
__global__ __launch_bounds__(MIX_THREADS) void k_mix_grad_x(const T* __restrict__ x, const T* __restrict__ g, const T* __restrict__ lp,
                                                            const T* __restrict__ prep, T* __restrict__ dx, int64_t R, int64_t C, int D) {
  constexpr int P = MfmaPanel<T>::PANEL, LD = MfmaPanel<T>::LD;
  typedef typename Mfma<T>::Acc Acc;
  const int K16 = mix_k16(D), steps = mix_steps(D), ntiles = K16 / 16;
  const MixPrep<T> w = mix_prep(const_cast<T*>(prep), C, D);
  T* Ws = tile_lds<T>();
  T* bs = Ws + K16 * LD;
  const int wave = mfma_wave(threadIdx.x), waves = blockDim.x >> 6, m = mfma_m(threadIdx.x), q = mfma_q(threadIdx.x);
  const int64_t r = ((int64_t)blockIdx.x * waves + wave) * 16 + m;
  const bool live = r < R;
  const int64_t rc = live ? r : R - 1;
  T a[ZS_MIX_MAX_STEPS];
  mix_load_rows(x, w.cen, D, rc, q, a);
  const T gr = g[rc], lpr = lp[rc];
  Acc d[ZS_MIX_MAX_NTILES];          // d[nt][v] = sum_c Ws[16 nt + acc_row(q, v)][c] G[c][row m]
#pragma unroll
  for (int nt = 0; nt < ZS_MIX_MAX_NTILES; ++nt) d[nt] = Acc{0, 0, 0, 0};
  const int64_t panels = w.cpad / P;
  for (int64_t panel = 0; panel < panels; ++panel) {
    const int64_t col0 = panel * P;
    mix_stage_panel(w, K16, col0, Ws, bs);
#pragma unroll
    for (int ct = 0; ct < P / 16; ++ct) {
      if (col0 + ct * 16 < C) {
        const Acc acc = panel_tile<T, false>(a, Ws + ct * 16, q, m, steps);
        T G[4];
#pragma unroll
        for (int v = 0; v < 4; ++v) G[v] = mix_weight(live, gr, acc[v] + bs[ct * 16 + MfmaTile<T>::acc_row(q, v)], lpr);
#pragma unroll
        for (int nt = 0; nt < ZS_MIX_MAX_NTILES; ++nt) {
          if (nt < ntiles) {
#pragma unroll
            for (int v = 0; v < 4; ++v)
              d[nt] = Mfma<T>::run(Ws[(nt * 16 + m) * LD + ct * 16 + MfmaTile<T>::acc_row(q, v)], G[v], d[nt]);
          }
        }
      }
    }
  }
  // row 2 d of the output is sum_c G (w nu), row 2 d + 1 is sum_c G (-w / 2):  dx = even + 2 y odd
#pragma unroll
  for (int nt = 0; nt < ZS_MIX_MAX_NTILES; ++nt) {
    if (nt < ntiles) {
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const T odd = mix_odd_row(d[nt], v);
        const int dim = (nt * 16 + MfmaTile<T>::acc_row(q, v)) >> 1;
        if (mix_holds_even<T>(q, v) && live && dim < D) {
          const T y = x[r * D + dim] - w.cen[dim];
          dx[r * D + dim] = d[nt][v] + (T)2 * y * odd;
        }
      }
    }
  }
}

// ---------------------------------------------------------------- dlogits, dmean, dlogstd
// grid (panels, shares); a wave per 16 components of the panel (blockDim = 64 P / 16) walks the row tiles share, share + shares, ...
template <typename T>
__global__ __launch_bounds__(MIX_THREADS) void k_mix_grad_params(const T* __restrict__ x, const T* __restrict__ g, const T* __restrict__ lp,
                                                                 const T* __restrict__ prep, T* __restrict__ part, int64_t R, int64_t C, int D) {
  constexpr int P = MfmaPanel<T>::PANEL, LD = MfmaPanel<T>::LD;
  typedef typename Mfma<T>::Acc Acc;
  const int K16 = mix_k16(D), steps = mix_steps(D), ntiles = K16 / 16;
  const MixPrep<T> w = mix_prep(const_cast<T*>(prep), C, D);
  T* Ws = tile_lds<T>();
  T* bs = Ws + K16 * LD;
  const int64_t col0 = (int64_t)blockIdx.x * P, share = blockIdx.y, shares = gridDim.y;
  mix_stage_panel(w, K16, col0, Ws, bs);
  const int wave = mfma_wave(threadIdx.x), m = mfma_m(threadIdx.x), q = mfma_q(threadIdx.x);
  const int64_t col = col0 + wave * 16 + m, tiles = blocks16(R);
  const T* Wc = Ws + wave * 16;
  const T bc = bs[wave * 16 + m];
  Acc acc_out[ZS_MIX_MAX_NTILES];          // acc_out[nt][v] = sum_r YY[r][16 nt + acc_row(q, v)] G[r][component m]
#pragma unroll
  for (int nt = 0; nt < ZS_MIX_MAX_NTILES; ++nt) acc_out[nt] = Acc{0, 0, 0, 0};
  T nsum = 0, gsum = 0;
  T a[ZS_MIX_MAX_STEPS];
  if (col0 + wave * 16 < C) {
    for (int64_t rt = share; rt < tiles; rt += shares) {
      const int64_t ra = rt * 16 + m;
      mix_load_rows(x, w.cen, D, ra < R ? ra : R - 1, q, a);
      const Acc acc = panel_tile<T, true>(a, Wc, q, m, steps);
      T G[4];
      int64_t rows[4];
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int64_t r = rt * 16 + MfmaTile<T>::acc_row(q, v);
        const bool live = r < R;
        rows[v] = live ? r : R - 1;
        const T gr = live ? g[rows[v]] : (T)0;
        G[v] = mix_weight(live, gr, acc[v] + bc, lp[rows[v]]);
        nsum += G[v];
        gsum += gr;
      }
#pragma unroll
      for (int nt = 0; nt < ZS_MIX_MAX_NTILES; ++nt) {
        if (nt < ntiles) {
          const int k = nt * 16 + m, dim = k >> 1;
#pragma unroll
          for (int v = 0; v < 4; ++v) {
            const T yy = dim < D ? mix_row_elem(x[rows[v] * D + dim] - w.cen[dim], k) : (T)0;
            acc_out[nt] = Mfma<T>::run(yy, G[v], acc_out[nt]);
          }
        }
      }
    }
  }
  T* out = part + share * ((int64_t)(K16 + 1) * w.cpad);
#pragma unroll
  for (int nt = 0; nt < ZS_MIX_MAX_NTILES; ++nt) {
    if (nt < ntiles) {
#pragma unroll
      for (int v = 0; v < 4; ++v) out[(int64_t)(nt * 16 + MfmaTile<T>::acc_row(q, v)) * w.cpad + col] = acc_out[nt][v];
    }
  }
  nsum += __shfl_xor(nsum, 16, ZS_WAVE);          // over the 16 rows of the tiles: q = 0 .. 3
  nsum += __shfl_xor(nsum, 32, ZS_WAVE);
  gsum += __shfl_xor(gsum, 16, ZS_WAVE);
  gsum += __shfl_xor(gsum, 32, ZS_WAVE);
  if (q == 0) out[(int64_t)K16 * w.cpad + col] = nsum;
  if (blockIdx.x == 0 && threadIdx.x == 0) part[shares * ((int64_t)(K16 + 1) * w.cpad) + share] = gsum;          // (component 0 is live)
}

// a thread per element of mean: the shares in order, then the closed forms; the threads of dimension 0 also give dlogits
template <typename T>
__global__ __launch_bounds__(MIX_THREADS) void k_mix_grad_params_finish(const T* __restrict__ mean, const T* __restrict__ logstd,
                                                                        const T* __restrict__ prep, const T* __restrict__ part,
                                                                        T* __restrict__ dlogits, T* __restrict__ dmean, T* __restrict__ dlogstd,
                                                                        int64_t C, int64_t D, int64_t shares) {
  const MixPrep<T> w = mix_prep(const_cast<T*>(prep), C, D);
  const int64_t i = (int64_t)blockIdx.x * MIX_THREADS + threadIdx.x;
  if (i >= C * D) return;
  int64_t c, d;
  divmod(i, D, c, d);
  const int64_t K16 = mix_k16(D), stride = (K16 + 1) * w.cpad;
  T gy = 0, gy2 = 0, n = 0;
  for (int64_t sh = 0; sh < shares; ++sh) {
    const T* p = part + sh * stride;
    gy += p[(2 * d) * w.cpad + c];
    gy2 += p[(2 * d + 1) * w.cpad + c];
    n += p[K16 * w.cpad + c];
  }
  const T wt = mix_exp((T)-2 * logstd[i]), nu = mean[i] - w.cen[d];
  dmean[i] = mix_dmean(wt, nu, gy, n);
  dlogstd[i] = mix_dlogstd(wt, nu, gy, gy2, n);
  if (d == 0) {
    T sumg = 0;
    for (int64_t sh = 0; sh < shares; ++sh) sumg += part[shares * stride + sh];
    dlogits[c] = mix_dlogits(n, w.lsm[c], sumg);
  }
}

// ---------------------------------------------------------------- the entry points
// 0 = go on, 1 = nothing to do, else the code to return
int mix_check(bool pointers, int64_t R, int64_t C, int64_t D) {
  if (!pointers || R < 0 || C < 1 || D < 1) return ZS_EINVAL;
  if (D > ZS_MIX_MAX_DIM || C > ZS_MIX_MAX_COMPONENTS || R >= ((int64_t)1 << 31)) return ZS_ENOTSUP;
  return R == 0 ? 1 : 0;
}
unsigned mix_blocks(int64_t n) { return (unsigned)((n + MIX_THREADS - 1) / MIX_THREADS); }

template <typename T>
int mix_prepare(const void* logits, const void* mean, const void* logstd, void* prep, int64_t C, int64_t D, void* stream) {
  const int rc = mix_check(logits && mean && logstd && prep, 1, C, D);
  if (rc) return rc;
  hipLaunchKernelGGL((k_mix_centre<T>), dim3((unsigned)(D + 1)), dim3(MIX_THREADS), 0, (hipStream_t)stream, (const T*)logits, (const T*)mean,
                     (T*)prep, C, D);
  ZS_CHECK_LAUNCH();
  hipLaunchKernelGGL((k_mix_pack<T>), dim3(mix_blocks(mix_cpad(sizeof(T), C))), dim3(MIX_THREADS), 0, (hipStream_t)stream, (const T*)logits,
                     (const T*)mean, (const T*)logstd, (T*)prep, C, (int)D);
  ZS_CHECK_LAUNCH();
  return 0;
}

template <typename T>
int mix_logprob(const void* x, const void* prep, void* lp, int64_t R, int64_t C, int64_t D, void* stream) {
  const int rc = mix_check(x && prep && lp, R, C, D);
  if (rc) return rc == 1 ? 0 : rc;
  const int64_t blocks = (R + ZS_MIX_ROWS_PER_BLOCK - 1) / ZS_MIX_ROWS_PER_BLOCK;
  hipLaunchKernelGGL((k_mix_logprob<T>), dim3((unsigned)blocks), dim3(MIX_THREADS), mix_lds_bytes_for<T>(mix_k16(D)), (hipStream_t)stream,
                     (const T*)x, (const T*)prep, (T*)lp, R, C, (int)D);
  ZS_CHECK_LAUNCH();
  return 0;
}

template <typename T>
int mix_grad_x(const void* x, const void* g, const void* lp, const void* prep, void* dx, int64_t R, int64_t C, int64_t D, void* stream) {
  const int rc = mix_check(x && g && lp && prep && dx, R, C, D);
  if (rc) return rc == 1 ? 0 : rc;
  const int64_t blocks = (R + ZS_MIX_ROWS_PER_BLOCK - 1) / ZS_MIX_ROWS_PER_BLOCK;
  hipLaunchKernelGGL((k_mix_grad_x<T>), dim3((unsigned)blocks), dim3(MIX_THREADS), mix_lds_bytes_for<T>(mix_k16(D)), (hipStream_t)stream,
                     (const T*)x, (const T*)g, (const T*)lp, (const T*)prep, (T*)dx, R, C, (int)D);
  ZS_CHECK_LAUNCH();
  return 0;
}

template <typename T>
int mix_grad_params(const void* x, const void* g, const void* lp, const void* mean, const void* logstd, const void* prep, void* part,
                    void* dlogits, void* dmean, void* dlogstd, int64_t R, int64_t C, int64_t D, int64_t shares, void* stream) {
  const int rc = mix_check(x && g && lp && mean && logstd && prep && part && dlogits && dmean && dlogstd, R, C, D);
  if (rc) return rc == 1 ? 0 : rc;          // (R == 0 before the shares: zs_mix_row_shares has none to offer for no rows)
  if (shares < 1 || shares > blocks16(R) || shares > 65535) return ZS_EINVAL;
  const int waves = MfmaPanel<T>::PANEL / 16;
  hipLaunchKernelGGL((k_mix_grad_params<T>), dim3((unsigned)panels(sizeof(T), C), (unsigned)shares), dim3(64 * waves),
                     mix_lds_bytes_for<T>(mix_k16(D)), (hipStream_t)stream, (const T*)x, (const T*)g, (const T*)lp, (const T*)prep, (T*)part,
                     R, C, (int)D);
  ZS_CHECK_LAUNCH();
  hipLaunchKernelGGL((k_mix_grad_params_finish<T>), dim3(mix_blocks(C * D)), dim3(MIX_THREADS), 0, (hipStream_t)stream, (const T*)mean,
                     (const T*)logstd, (const T*)prep, (const T*)part, (T*)dlogits, (T*)dmean, (T*)dlogstd, C, D, shares);
  ZS_CHECK_LAUNCH();
  return 0;
}

}  // namespace

extern "C" int zs_mix_abi_version(void) { return ZS_MIX_ABI_VERSION; }
extern "C" int zs_mix_max_dim(void) { return ZS_MIX_MAX_DIM; }
extern "C" int zs_mix_max_components(void) { return ZS_MIX_MAX_COMPONENTS; }
extern "C" int64_t zs_mix_panels(int elem_bytes, int64_t C) { return panels(elem_bytes, C); }
extern "C" int64_t zs_mix_row_shares(int elem_bytes, int64_t R, int64_t C) { return mix_row_shares(elem_bytes, R, C); }
extern "C" int64_t zs_mix_workspace_elems(int which, int elem_bytes, int64_t C, int64_t D, int64_t shares) {
  if (panels(elem_bytes, C) == 0 || C > ZS_MIX_MAX_COMPONENTS || D < 1 || D > ZS_MIX_MAX_DIM) return -1;
  switch (which) {
    case ZS_MIX_WS_PREP: return mix_prep_elems(elem_bytes, C, D);
    case ZS_MIX_WS_GRAD_PARAMS: return shares < 1 ? -1 : mix_part_elems(elem_bytes, C, D, shares);
    default: return -1;
  }
}

#define ZS_MIX_ENTRY(SFX, T)                                                                                                           \
  extern "C" int zs_mix_prepare##SFX(const void* logits, const void* mean, const void* logstd, void* prep, int64_t C, int64_t D,       \
                                     void* stream) {                                                                                   \
    return mix_prepare<T>(logits, mean, logstd, prep, C, D, stream);                                                                   \
  }                                                                                                                                    \
  extern "C" int zs_mix_logprob##SFX(const void* x, const void* prep, void* lp, int64_t R, int64_t C, int64_t D, void* stream) {       \
    return mix_logprob<T>(x, prep, lp, R, C, D, stream);                                                                               \
  }                                                                                                                                    \
  extern "C" int zs_mix_grad_x##SFX(const void* x, const void* g, const void* lp, const void* prep, void* dx, int64_t R, int64_t C,    \
                                    int64_t D, void* stream) {                                                                         \
    return mix_grad_x<T>(x, g, lp, prep, dx, R, C, D, stream);                                                                         \
  }                                                                                                                                    \
  extern "C" int zs_mix_grad_params##SFX(const void* x, const void* g, const void* lp, const void* mean, const void* logstd,           \
                                         const void* prep, void* part, void* dlogits, void* dmean, void* dlogstd, int64_t R,           \
                                         int64_t C, int64_t D, int64_t shares, void* stream) {                                         \
    return mix_grad_params<T>(x, g, lp, mean, logstd, prep, part, dlogits, dmean, dlogstd, R, C, D, shares, stream);                   \
  }

ZS_MIX_ENTRY(_f32, float)
ZS_MIX_ENTRY(_f64, double)
