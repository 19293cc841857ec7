// S1, S2, S3: Stein variational gradient descent over K interacting particles (include/zs_svgd.h; its own library,
// ../lib/libzs_svgd.so, `make svgd`).
//
// A torch composition of one step is a chain of mean, sub, matmul, diagonal, quantile, exp, sum and two more matmul launches with
// [K, K] and [K, D] temporaries.  Here a step over one table of latents is three launches.  The latents form one flat column
// space (pointer table by value, a column finds its tensor by bisection); a workgroup owns slabs of 32 columns and holds ALL K
// particles of a slab in LDS, so the column means cost no extra pass, and both heavy pieces run on v_mfma_{f32,f64}_16x16x4:
//
//   gram    G += C C^T over the slab, C the centred slab: lane 16 q + m reads A = C[16 bi + m][4 s + q] and B = C[16 bj + m][4 s + q]
//           for tile pair (bi, bj) -- both along a row of the tile, LD = 36 keeps the 64 lanes in 64 banks.  The pairs are dealt
//           over eight waves, the accumulators stay in registers across all slabs of the persistent workgroup (17 pairs x 4 values
//           a wave at K = 256) and leave once, as one double partial per workgroup in its own slot.
//   finish  one workgroup: partials in slot order, d, the median by exact bit-pattern selection, h, k = exp(-d / h), the row sums.
//   update  U = G - (2/h) C staged in LDS (LD = 48: the B operand is read down a column, the four k-rows 16 banks apart); wave b
//           keeps rows 16 b .. 16 b + 15 of k as A operands in registers for every slab it walks and forms k U for the slab's two
//           column blocks; the epilogue is the step itself.
//
// A kernel is compiled per register tier (accumulators a wave / strip length), so that every register array is indexed
// statically; the host picks the smallest tier that holds K.  No atomics, no scratch.
#include "zs_common.h"
#include "zs_svgd_math.h"
#include "../../include/zs_hip.h"
#include "../../include/zs_svgd.h"

#pragma clang fp contract(off)

using namespace zs;

namespace {

constexpr int SLAB = ZS_SVGD_SLAB;
constexpr int LDG = ZS_SVGD_LD_GRAM;
constexpr int LDU = ZS_SVGD_LD_UPDATE;

template <typename T>
struct Table {
  const T* q[ZS_SVGD_MAX_TENSORS];
  const T* grad[ZS_SVGD_MAX_TENSORS];
  T* out[ZS_SVGD_MAX_TENSORS];
  T* h[ZS_SVGD_MAX_TENSORS];
  int64_t col[ZS_SVGD_MAX_TENSORS + 1];          // first column of tensor t; col[n_tensors] = D
  int n_tensors;
};

// where column j of the flat space lives: its tensor, that tensor's width, and the offset of (row 0, j) in it
struct Column {
  int t;
  int64_t width, off;
};
template <typename T>
__device__ __forceinline__ Column column_of(const Table<T>& ts, int64_t j) {
  Column c;
  c.t = flat_tensor_of(ts.col, ts.n_tensors, j);
  c.width = ts.col[c.t + 1] - ts.col[c.t];
  c.off = j - ts.col[c.t];
  return c;
}

// mean[c] = the mean over the K particles of column c0 + c (0 past D): thread (part, c) adds the rows part, part + PARTS, ... in
// ascending order, thread c the PARTS partials in ascending order.  Begins and ends synchronised.
template <typename T, int THREADS>
__device__ __forceinline__ void column_means(const Table<T>& ts, int64_t c0, int64_t D, int K, T* red, T* mean) {
  constexpr int PARTS = THREADS / SLAB;
  const int c = threadIdx.x % SLAB, part = threadIdx.x / SLAB;
  const int64_t j = c0 + c;
  T s = (T)0;
  if (j < D) {
    const Column w = column_of(ts, j);
    const T* p = ts.q[w.t] + w.off;
    for (int k = part; k < K; k += PARTS) s += p[(int64_t)k * w.width];
  }
  red[part * SLAB + c] = s;
  __syncthreads();
  if (threadIdx.x < SLAB) {
    T a = (T)0;
    for (int p = 0; p < PARTS; ++p) a += red[p * SLAB + threadIdx.x];
    mean[threadIdx.x] = a / (T)K;
  }
  __syncthreads();
}

// ---------------------------------------------------------------- S1
template <typename T, int PPW>
__global__ __launch_bounds__(ZS_SVGD_GRAM_THREADS) void k_svgd_gram(const Table<T> ts, int64_t D, int K, int64_t slabs,
                                                                    double* partials) {
  typedef typename Mfma<T>::Acc Acc;
  constexpr int THREADS = ZS_SVGD_GRAM_THREADS, PARTS = THREADS / SLAB;
  __shared__ T tile[SvgdCap<T>::MAX_K * LDG];
  __shared__ T red[PARTS * SLAB];
  __shared__ T mean[SLAB];
  const int nb = svgd_blocks(K), npairs = svgd_pairs(nb), k16 = 16 * nb;
  const int m = mfma_m(threadIdx.x), q = mfma_q(threadIdx.x), wave = mfma_wave(threadIdx.x);
  const int c = threadIdx.x % SLAB, part = threadIdx.x / SLAB;
  int bi[PPW], bj[PPW];
  Acc acc[PPW];
#pragma unroll
  for (int t = 0; t < PPW; ++t) {
    const int p = svgd_pair_index(wave, t);
    bi[t] = bj[t] = 0;
    if (p < npairs) svgd_pair_of(p, bi[t], bj[t]);
    acc[t] = Acc{0, 0, 0, 0};
  }
  for (int64_t slab = blockIdx.x; slab < slabs; slab += gridDim.x) {
    const int64_t c0 = slab * SLAB, j = c0 + c;
    column_means<T, THREADS>(ts, c0, D, K, red, mean);
    {
      const bool live = j < D;
      Column w = {0, 0, 0};
      if (live) w = column_of(ts, j);
      const T* p = ts.q[w.t] + w.off;
      const T mu = mean[c];
      for (int row = part; row < k16; row += PARTS)
        tile[row * LDG + c] = (live && svgd_row_live(row, K)) ? p[(int64_t)row * w.width] - mu : (T)0;
    }
    __syncthreads();
    const int64_t left = D - c0;
    const int steps = left < SLAB ? (int)((left + 3) >> 2) : SLAB / 4;          // (columns past D are zero)
#pragma unroll
    for (int t = 0; t < PPW; ++t) {
      if (svgd_pair_index(wave, t) < npairs) {
        const T* a = tile + (16 * bi[t] + m) * LDG + q;
        const T* b = tile + (16 * bj[t] + m) * LDG + q;
        for (int s = 0; s < steps; ++s) acc[t] = Mfma<T>::run(a[4 * s], b[4 * s], acc[t]);
      }
    }
    __syncthreads();          // the next slab is staged over this one
  }
  double* out = partials + (int64_t)blockIdx.x * K * K;
#pragma unroll
  for (int t = 0; t < PPW; ++t) {
    if (svgd_pair_index(wave, t) < npairs) {
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int r = 16 * bi[t] + MfmaTile<T>::acc_row(q, v), cc = 16 * bj[t] + m;
        if (r < K && cc < K) {
          out[r * K + cc] = (double)acc[t][v];
          if (bi[t] != bj[t]) out[cc * K + r] = (double)acc[t][v];
        }
      }
    }
  }
}

// ---------------------------------------------------------------- S2
// the sum over the workgroup of a packed pair of counts, in every thread (integers: any order); begins and ends synchronised
__device__ __forceinline__ long long block_count(long long v, long long* sh) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, ZS_WAVE);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  long long s = 0;
  for (int w = 0; w < ZS_SVGD_FINISH_THREADS / 64; ++w) s += sh[w];
  return s;
}

__global__ __launch_bounds__(ZS_SVGD_FINISH_THREADS) void k_svgd_finish(const double* __restrict__ partials, int64_t n_slots, int K,
                                                                        int median, double bandwidth, double* state) {
  constexpr int THREADS = ZS_SVGD_FINISH_THREADS;
  __shared__ double gd[ZS_SVGD_MAX_PARTICLES];
  __shared__ long long counts[THREADS / 64];
  const int tid = threadIdx.x, kk = K * K;
  double* rowsum = state + ZS_SVGD_STATE_HEADER;
  double* kern = rowsum + K;
  if (tid < K) {
    double a = 0.0;
    for (int64_t s = 0; s < n_slots; ++s) a += partials[s * kk + tid * K + tid];
    gd[tid] = a;
  }
  __syncthreads();
  // every element of d (and later of k) belongs to ONE thread through all phases: e = tid, tid + THREADS, ...; (i, j) and (j, i)
  // add the same partials, those of the lower triangle, in the same order
  for (int e = tid; e < kk; e += THREADS) {
    const int i = e / K, j = e % K, hi = i > j ? i : j, lo = i > j ? j : i;
    double g = 0.0;
    for (int64_t s = 0; s < n_slots; ++s) g += partials[s * kk + hi * K + lo];
    kern[e] = svgd_dist(gd[i], gd[j], g, i == j);
  }
  double h = bandwidth, med = -1.0;
  if (median) {
    const int64_t r0 = svgd_rank_lo(kk), r1 = svgd_rank_hi(kk);
    uint64_t a0 = 0, a1 = 0;
    for (int bit = 62; bit >= 0; --bit) {
      const uint64_t c0 = svgd_candidate(a0, bit), c1 = svgd_candidate(a1, bit);
      long long n = 0;
      for (int e = tid; e < kk; e += THREADS) {
        const uint64_t x = svgd_bits(kern[e]);
        n += (x < c0 ? 1LL : 0LL) + (x < c1 ? (1LL << 32) : 0LL);
      }
      n = block_count(n, counts);
      a0 = svgd_select_step(a0, bit, n & 0xFFFFFFFFLL, r0);
      a1 = svgd_select_step(a1, bit, n >> 32, r1);
    }
    med = svgd_median_of(svgd_from_bits(a0), svgd_from_bits(a1));
    h = svgd_bandwidth(med, K);
  }
  for (int e = tid; e < kk; e += THREADS) kern[e] = exp(-kern[e] / h);
  __syncthreads();
  if (tid < K) {
    double s = 0.0;
    for (int j = 0; j < K; ++j) s += kern[tid * K + j];
    rowsum[tid] = s;
  }
  if (tid == 0) {
    state[0] = h;
    state[1] = 2.0 / h;
    state[2] = med;
    state[3] = (double)K;
  }
}

// ---------------------------------------------------------------- S3
// NB: blocks of 16 particles the strip registers hold (K <= 16 NB); WAVES >= NB, wave b < blocks(K) owns strip b
template <typename T, int NB, int WAVES>
__global__ __launch_bounds__(64 * WAVES) void k_svgd_update(const Table<T> ts, int64_t D, int K, int64_t slabs,
                                                            const double* __restrict__ state, const SvgdStep<T> st0) {
  typedef typename Mfma<T>::Acc Acc;
  constexpr int THREADS = 64 * WAVES, PARTS = THREADS / SLAB;
  __shared__ T tile[16 * NB * LDU];
  __shared__ T red[PARTS * SLAB];
  __shared__ T mean[SLAB];
  __shared__ T rowsum[16 * NB];
  const int nb = svgd_blocks(K), k16 = 16 * nb, ksteps = 4 * nb;
  const int m = mfma_m(threadIdx.x), q = mfma_q(threadIdx.x), wave = mfma_wave(threadIdx.x);
  const int c = threadIdx.x % SLAB, part = threadIdx.x / SLAB;
  const bool owner = wave < nb;
  SvgdStep<T> st = st0;
  st.two_over_h = (T)state[1];
  const double* kern = state + ZS_SVGD_STATE_HEADER + K;
  T a[4 * NB];
#pragma unroll
  for (int s = 0; s < 4 * NB; ++s) {
    const int row = 16 * wave + m, kc = 4 * s + q;
    a[s] = (owner && row < K && kc < K) ? (T)kern[row * K + kc] : (T)0;
  }
  for (int i = threadIdx.x; i < 16 * NB; i += THREADS) rowsum[i] = i < K ? (T)state[ZS_SVGD_STATE_HEADER + i] : (T)0;
  for (int64_t slab = blockIdx.x; slab < slabs; slab += gridDim.x) {
    const int64_t c0 = slab * SLAB, j = c0 + c;
    column_means<T, THREADS>(ts, c0, D, K, red, mean);
    {
      const bool live = j < D;
      Column w = {0, 0, 0};
      if (live) w = column_of(ts, j);
      const T* p = ts.q[w.t] + w.off;
      const T* g = ts.grad[w.t] + w.off;
      const T mu = mean[c];
      for (int row = part; row < k16; row += PARTS) {
        T u = (T)0;
        if (live && svgd_row_live(row, K)) u = g[(int64_t)row * w.width] - st.two_over_h * (p[(int64_t)row * w.width] - mu);
        tile[row * LDU + c] = u;
      }
    }
    __syncthreads();
    if (owner) {
#pragma unroll
      for (int cb = 0; cb < SLAB / 16; ++cb) {
        const T* b = tile + q * LDU + 16 * cb + m;
        Acc acc = {0, 0, 0, 0};
#pragma unroll
        for (int s = 0; s < 4 * NB; ++s)
          if (s < ksteps) acc = Mfma<T>::run(a[s], b[4 * s * LDU], acc);
        const int cc = 16 * cb + m;
        const int64_t jj = c0 + cc;
        if (jj < D) {
          const Column w = column_of(ts, jj);
          const T mu = mean[cc];
#pragma unroll
          for (int v = 0; v < 4; ++v) {
            const int r = 16 * wave + MfmaTile<T>::acc_row(q, v);
            if (r < K) {
              const int64_t at = (int64_t)r * w.width + w.off;
              const T theta = ts.q[w.t][at];
              const T phi = svgd_phi(acc[v], rowsum[r], theta - mu, st);
              ts.out[w.t][at] = svgd_move(theta, phi, st.adagrad ? ts.h[w.t] + at : nullptr, st);
            }
          }
        }
      }
    }
    __syncthreads();          // the next slab is staged over this one
  }
}

// ---------------------------------------------------------------- the entry points
// validates a table and fills the kernel's; 0, ZS_EINVAL or ZS_ENOTSUP
template <typename T>
int fill_table(bool update, bool adagrad, const zs_svgd_tensor* tensors, int n_tensors, int64_t n, int64_t K, Table<T>& ts) {
  if (!tensors || n_tensors < 1 || K < 1 || n < 0) return ZS_EINVAL;
  if (n_tensors > ZS_SVGD_MAX_TENSORS || K > SvgdCap<T>::MAX_K) return ZS_ENOTSUP;
  memset(&ts, 0, sizeof(ts));
  ts.n_tensors = n_tensors;
  int64_t col = 0;
  for (int i = 0; i < n_tensors; ++i) {
    const zs_svgd_tensor& t = tensors[i];
    if (t.row < 1 || t.start != K * col || !t.q_in) return ZS_EINVAL;
    if (update && (!t.grad || !t.q_out || (adagrad && !t.h))) return ZS_EINVAL;
    ts.q[i] = (const T*)t.q_in;
    ts.grad[i] = (const T*)t.grad;
    ts.out[i] = (T*)t.q_out;
    ts.h[i] = (T*)t.h;
    ts.col[i] = col;
    col += t.row;
    if (col > INT64_MAX / (2 * K)) return ZS_ENOTSUP;
  }
  ts.col[n_tensors] = col;
  return n == K * col ? 0 : ZS_EINVAL;
}

template <typename T, int PPW>
void launch_gram(unsigned grid, hipStream_t st, const Table<T>& ts, int64_t D, int K, int64_t slabs, double* partials) {
  hipLaunchKernelGGL((k_svgd_gram<T, PPW>), dim3(grid), dim3(ZS_SVGD_GRAM_THREADS), 0, st, ts, D, K, slabs, partials);
}
template <typename T>
int svgd_gram(const zs_svgd_tensor* tensors, int n_tensors, int64_t n, int64_t K, double* partials, void* stream) {
  Table<T> ts;
  const int rc = fill_table<T>(false, false, tensors, n_tensors, n, K, ts);
  if (rc) return rc;
  if (!partials) return ZS_EINVAL;
  const int64_t D = ts.col[n_tensors], slabs = svgd_slabs(D);
  const unsigned grid = (unsigned)svgd_gram_slots(D);
  const int ppw = svgd_pairs_per_wave(svgd_blocks((int)K));
  hipStream_t st = (hipStream_t)stream;
  if (ppw <= 1) launch_gram<T, 1>(grid, st, ts, D, (int)K, slabs, partials);
  else if (ppw <= 5) launch_gram<T, 5>(grid, st, ts, D, (int)K, slabs, partials);
  else if constexpr (SvgdCap<T>::MAX_K > 128) launch_gram<T, 17>(grid, st, ts, D, (int)K, slabs, partials);
  ZS_CHECK_LAUNCH();
  return 0;
}

int svgd_finish(const double* partials, int64_t n_slots, int64_t K, int median, double bandwidth, double* state, void* stream) {
  if (!partials || !state || n_slots < 1 || K < 1) return ZS_EINVAL;
  if (!median && !(bandwidth > 0.0)) return ZS_EINVAL;
  if (K > ZS_SVGD_MAX_PARTICLES) return ZS_ENOTSUP;
  hipLaunchKernelGGL(k_svgd_finish, dim3(1), dim3(ZS_SVGD_FINISH_THREADS), 0, (hipStream_t)stream, partials, n_slots, (int)K,
                     median ? 1 : 0, bandwidth, state);
  ZS_CHECK_LAUNCH();
  return 0;
}

template <typename T, int NB, int WAVES>
void launch_update(hipStream_t st, const Table<T>& ts, int64_t D, int K, const double* state, const SvgdStep<T>& step) {
  const int64_t slabs = svgd_slabs(D);
  hipLaunchKernelGGL((k_svgd_update<T, NB, WAVES>), dim3(grid_for(slabs, 1, 1024u)), dim3(64 * WAVES), 0, st, ts, D, K, slabs, state,
                     step);
}
template <typename T>
int svgd_update(const zs_svgd_tensor* tensors, int n_tensors, int64_t n, int64_t K, const double* state, double step_size,
                int adagrad, int first, double alpha, double fudge, void* stream) {
  Table<T> ts;
  const int rc = fill_table<T>(true, adagrad != 0, tensors, n_tensors, n, K, ts);
  if (rc) return rc;
  if (!state || step_size != step_size || alpha != alpha || fudge != fudge) return ZS_EINVAL;
  SvgdStep<T> step;
  step.step = (T)step_size, step.alpha = (T)alpha, step.one_minus_alpha = (T)(1.0 - alpha), step.fudge = (T)fudge;
  step.two_over_h = (T)0, step.inv_k = (T)(1.0 / (double)K), step.adagrad = adagrad ? 1 : 0, step.first = first ? 1 : 0;
  const int64_t D = ts.col[n_tensors];
  const int nb = svgd_blocks((int)K);
  hipStream_t st = (hipStream_t)stream;
  if (nb <= 2) launch_update<T, 2, 4>(st, ts, D, (int)K, state, step);
  else if (nb <= 8) launch_update<T, 8, 8>(st, ts, D, (int)K, state, step);
  else if constexpr (SvgdCap<T>::MAX_K > 128) launch_update<T, 16, 16>(st, ts, D, (int)K, state, step);
  ZS_CHECK_LAUNCH();
  return 0;
}

}  // namespace

extern "C" int zs_svgd_abi_version(void) { return ZS_SVGD_ABI_VERSION; }
extern "C" int zs_svgd_max_particles(void) { return ZS_SVGD_MAX_PARTICLES; }
extern "C" int zs_svgd_max_particles_of(int elem_bytes) { return svgd_max_particles_of(elem_bytes); }
extern "C" int zs_svgd_slab(void) { return ZS_SVGD_SLAB; }
extern "C" int zs_svgd_grid_cap(void) { return ZS_SVGD_GRID_CAP; }
extern "C" int64_t zs_svgd_gram_slots(int64_t D) { return D < 1 ? -1 : svgd_gram_slots(D); }
extern "C" int64_t zs_svgd_partial_doubles(int64_t K) { return (K < 1 || K > ZS_SVGD_MAX_PARTICLES) ? -1 : K * K; }
extern "C" int64_t zs_svgd_state_doubles(int64_t K) {
  return (K < 1 || K > ZS_SVGD_MAX_PARTICLES) ? -1 : ZS_SVGD_STATE_HEADER + K + K * K;
}
extern "C" int zs_svgd_finish(const double* partials, int64_t n_slots, int64_t K, int median, double bandwidth, double* state,
                              void* stream) {
  return svgd_finish(partials, n_slots, K, median, bandwidth, state, stream);
}

#define ZS_SVGD_ENTRY(SFX, T)                                                                                                      \
  extern "C" int zs_svgd_gram##SFX(const struct zs_svgd_tensor* tensors, int n_tensors, int64_t n, int64_t K, double* partials,    \
                                   void* stream) {                                                                                 \
    return svgd_gram<T>(tensors, n_tensors, n, K, partials, stream);                                                               \
  }                                                                                                                                \
  extern "C" int zs_svgd_update##SFX(const struct zs_svgd_tensor* tensors, int n_tensors, int64_t n, int64_t K,                    \
                                     const double* state, double step_size, int adagrad, int first, double alpha, double fudge,   \
                                     void* stream) {                                                                               \
    return svgd_update<T>(tensors, n_tensors, n, K, state, step_size, adagrad, first, alpha, fudge, stream);                       \
  }

ZS_SVGD_ENTRY(_f32, float)
ZS_SVGD_ENTRY(_f64, double)
