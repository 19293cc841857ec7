// MultivariateNormalLowRank: the density of a normal with covariance diag(d) + W W^T, its backward, the draw and its backward
// (include/zs_lowrank.h; its own library, ../lib/libzs_lowrank.so, `make lowrank`).
//
// The fifth user of the matrix cores after zs_topic, zs_matvar, zs_svgd and zs_mix.  The case is one row (or a few), D in the
// hundreds to thousands, tens of particles: every heavy step is a thin product against the factor W [D, r], r <= 64, and the D
// axis streams through LDS in panels of 64 rows, so nothing limits D but the grid.  One template over the element type; the two
// instructions differ only in the row map of the accumulator (MfmaTile<T>::acc_row).
//
// A lane l = 16 q + m of a wave gives Mfma<T>::run(a, b, acc) the elements A[m][k = q] and B[k = q][m] of a 16 x 4 by 4 x 16 step
// and holds acc[v] = out[acc_row(q, v)][m].  Three products use it:
//   direct       A = a particle operand [16][LDY] at [m][4 s + q], B = the panel at [4 s + q][16 t + m]: u = y Wd, u P
//   transposed   A likewise, B = the panel at [16 t + m][4 s + q]: the tile (v W^T)[particle acc_row][d-row 16 t + m]
//   from the accumulator   a = Sigma^-1 y stays where the transposed product left it and IS the A operand of A^T diag(g) V: the
//                contraction index of step v is the particle acc_row(q, v), and B is read from LDS at that particle's row
#include "zs_common.h"
#include "zs_lowrank_math.h"
#include "../../include/zs_hip.h"
#include "../../include/zs_lowrank.h"

#pragma clang fp contract(off)

using namespace zs;

namespace {

constexpr int LR_THREADS = 256;

template <typename T>
struct LrLds {
  T *Ws, *rds, *Ys, *Us, *misc;          // the panel, 1 / d of its rows, y of the tile, u (then v; the rank noise), small sums
};
template <typename T>
__device__ __forceinline__ LrLds<T> lr_lds() {
  T* p = tile_lds<T>();
  return LrLds<T>{p, p + LR_WS, p + LR_WS + LR_PANEL, p + LR_WS + LR_PANEL + LR_YS, p + LR_WS + LR_PANEL + 2 * LR_YS};
}
template <typename T>
constexpr size_t lr_lds_bytes() { return sizeof(T) * (size_t)LR_LDS_ELEMS; }

// element `flat` of the launch's normal stream, as zs_philox_normal_f32 numbers them
template <typename T>
__device__ __forceinline__ T lr_normal_at(int64_t flat, const PhiloxCall& pc) {
  return (T)f4_get(philox_normal4((uint64_t)flat >> 2, pc), (int)(flat & 3));
}
template <typename T>
__device__ __forceinline__ T lr_noise(const T* __restrict__ eps, int64_t flat, const PhiloxCall& pc) {
  return eps ? eps[flat] : lr_normal_at<T>(flat, pc);
}

// ---------------------------------------------------------------- staging
// Ws[dl][j] = W[d0 + dl][j] and rds[dl] = 1 / d[d0 + dl], zero past D and past r (columns up to rp).  Every thread of the
// workgroup calls the staging functions between two barriers of the caller's.
template <typename T>
__device__ __forceinline__ void lr_stage_factor(const LrLds<T>& L, const T* __restrict__ Wr, const T* __restrict__ dr, int D, int r, int rp,
                                                int d0) {
  for (int i = threadIdx.x; i < LR_PANEL * rp; i += LR_THREADS) {
    const int dl = i / rp, j = i - dl * rp, d = d0 + dl;
    L.Ws[dl * LR_LD + j] = (d < D && j < r) ? Wr[(int64_t)d * r + j] : (T)0;
  }
  if ((int)threadIdx.x < LR_PANEL) {
    const int d = d0 + (int)threadIdx.x;
    L.rds[threadIdx.x] = d < D ? (T)1 / dr[d] : (T)0;
  }
}
// Ys[p][dl] = x[particle k0 + p][d0 + dl] - mean[d0 + dl], zero past K and past D; shared != 0: x has no particle axis
template <typename T>
__device__ __forceinline__ void lr_stage_y(const LrLds<T>& L, const T* __restrict__ x, bool shared, const T* __restrict__ mr, int64_t k0,
                                           int64_t K, int64_t R, int64_t row, int D, int d0) {
  for (int i = threadIdx.x; i < 16 * LR_PANEL; i += LR_THREADS) {
    const int p = i / LR_PANEL, dl = i - p * LR_PANEL, d = d0 + dl;
    const int64_t k = k0 + p;
    T y = 0;
    if (k < K && d < D) y = x[((shared ? 0 : k * R) + row) * D + d] - mr[d];
    L.Ys[p * LR_LDY + dl] = y;
  }
}

// ---------------------------------------------------------------- u = y Wd and q = sum y^2 / d of one particle tile
// Leaves Us[p][j] = u (j < rp) and misc[64 + p] = q.  The four waves take every fourth k-step of each panel; their partials are
// added in wave order.  Begins and ends with a barrier.
template <typename T>
__device__ __forceinline__ void lr_tile_u(const LrLds<T>& L, const T* __restrict__ Wr, const T* __restrict__ dr, const T* __restrict__ mr,
                                          const T* __restrict__ x, bool shared, int64_t k0, int64_t K, int64_t R, int64_t row, int D, int r) {
  typedef typename Mfma<T>::Acc Acc;
  const int rp = lr_rp(r), RT = rp / 16;
  const int wave = mfma_wave(threadIdx.x), m = mfma_m(threadIdx.x), q = mfma_q(threadIdx.x);
  Acc acc[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) acc[t] = Acc{0, 0, 0, 0};
  T sq = 0;
  for (int d0 = 0; d0 < D; d0 += LR_PANEL) {
    __syncthreads();          // the previous panel's readers are done
    lr_stage_factor(L, Wr, dr, D, r, rp, d0);
    lr_stage_y(L, x, shared, mr, k0, K, R, row, D, d0);
    __syncthreads();
#pragma unroll
    for (int n = 0; n < 4; ++n) {
      const int kk = 4 * (wave + 4 * n) + q;
      const T y = L.Ys[m * LR_LDY + kk], a = y * L.rds[kk];
      sq += a * y;
#pragma unroll
      for (int t = 0; t < 4; ++t)
        if (t < RT) acc[t] = Mfma<T>::run(a, L.Ws[kk * LR_LD + t * 16 + m], acc[t]);
    }
  }
  sq += __shfl_xor(sq, 16, ZS_WAVE);          // the four lanes of a particle: q = 0 .. 3
  sq += __shfl_xor(sq, 32, ZS_WAVE);
  __syncthreads();          // the panel is free: it takes the waves' partials [4][16][LDY]
  T* Up = L.Ws;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    if (t < RT) {
#pragma unroll
      for (int v = 0; v < 4; ++v) Up[(wave * 16 + MfmaTile<T>::acc_row(q, v)) * LR_LDY + t * 16 + m] = acc[t][v];
    }
  }
  if (q == 0) L.misc[wave * 16 + m] = sq;
  __syncthreads();
  for (int i = threadIdx.x; i < 16 * rp; i += LR_THREADS) {
    const int p = i / rp, j = i - p * rp, o = p * LR_LDY + j;
    L.Us[o] = ((Up[o] + Up[LR_YS + o]) + Up[2 * LR_YS + o]) + Up[3 * LR_YS + o];
  }
  if (threadIdx.x < 16) L.misc[64 + threadIdx.x] = ((L.misc[threadIdx.x] + L.misc[16 + threadIdx.x]) + L.misc[32 + threadIdx.x]) + L.misc[48 + threadIdx.x];
  __syncthreads();
}

// rank tile t of Us P, P [rp, rp] row-major in memory: acc[v] = (u P)[particle acc_row(q, v)][16 t + m]
template <typename T>
__device__ __forceinline__ typename Mfma<T>::Acc lr_times(const T* Us, const T* __restrict__ P, int rp, int t, int q, int m) {
  typename Mfma<T>::Acc acc = {0, 0, 0, 0};
  for (int s = 0; s < rp / 4; ++s) acc = Mfma<T>::run(Us[m * LR_LDY + 4 * s + q], P[(4 * s + q) * rp + t * 16 + m], acc);
  return acc;
}
// the tile (Us W^T)[particle acc_row(q, v)][d-row dl] of the staged panel
template <typename T>
__device__ __forceinline__ typename Mfma<T>::Acc lr_times_panel_t(const LrLds<T>& L, int rp, int dl, int q, int m) {
  typename Mfma<T>::Acc acc = {0, 0, 0, 0};
  for (int s = 0; s < rp / 4; ++s) acc = Mfma<T>::run(L.Us[m * LR_LDY + 4 * s + q], L.Ws[dl * LR_LD + 4 * s + q], acc);
  return acc;
}

// ---------------------------------------------------------------- prepare
// grid = splits * R; one partial C[rp, rp] and one partial sum log d per (row, split)
template <typename T>
__global__ __launch_bounds__(LR_THREADS) void k_lr_cap_partial(const T* __restrict__ factor, const T* __restrict__ diag, T* __restrict__ part,
                                                               int64_t R, int D, int r, int64_t splits) {
  typedef typename Mfma<T>::Acc Acc;
  __shared__ T sh[4];
  const LrLds<T> L = lr_lds<T>();
  const int rp = lr_rp(r), RT = rp / 16;
  const int64_t row = blockIdx.x % R, split = blockIdx.x / R;
  const T* Wr = factor + row * D * r;
  const T* dr = diag + row * D;
  const int64_t npan = lr_panels(D), pps = (npan + splits - 1) / splits;
  const int64_t p0 = split * pps, p1 = p0 + pps < npan ? p0 + pps : npan;
  const int wave = mfma_wave(threadIdx.x), m = mfma_m(threadIdx.x), q = mfma_q(threadIdx.x);
  Acc acc[4];
#pragma unroll
  for (int n = 0; n < 4; ++n) acc[n] = Acc{0, 0, 0, 0};
  T ls = 0;
  for (int64_t pn = p0; pn < p1; ++pn) {
    const int d0 = (int)pn * LR_PANEL;
    __syncthreads();
    lr_stage_factor(L, Wr, dr, D, r, rp, d0);
    if ((int)threadIdx.x < LR_PANEL && d0 + (int)threadIdx.x < D) ls += lr_log(dr[d0 + threadIdx.x]);
    __syncthreads();
#pragma unroll
    for (int n = 0; n < 4; ++n) {
      const int t = wave + 4 * n;
      if (t < RT * RT) {
        const int ti = t / RT, tj = t - ti * RT;
        for (int s = 0; s < LR_PANEL / 4; ++s) {
          const int kk = 4 * s + q;
          acc[n] = Mfma<T>::run(L.Ws[kk * LR_LD + ti * 16 + m] * L.rds[kk], L.Ws[kk * LR_LD + tj * 16 + m], acc[n]);
        }
      }
    }
  }
  T* out = part + (row * splits + split) * lr_cap_part(r);
#pragma unroll
  for (int n = 0; n < 4; ++n) {
    const int t = wave + 4 * n;
    if (t < RT * RT) {
      const int ti = t / RT, tj = t - ti * RT;
#pragma unroll
      for (int v = 0; v < 4; ++v) out[(ti * 16 + MfmaTile<T>::acc_row(q, v)) * rp + tj * 16 + m] = acc[n][v];
    }
  }
  ls = block_sum_256(ls, sh);
  if (threadIdx.x == 0) out[rp * rp] = ls;
}

// M[k][i] of L^-1 for k >= i: the strict lower triangle of M is kept transposed in the upper triangle of Cs, 1 / L_ii in Ds
template <typename T>
__device__ __forceinline__ T lr_minv(const T* Cs, const T* Ds, int k, int i) { return k > i ? Cs[i * LR_CLD + k] : Ds[i]; }

// a workgroup per row: the partials in split order, + I, Cholesky, the inverse of the factor, prep
template <typename T>
__global__ __launch_bounds__(LR_THREADS) void k_lr_cap_finish(const T* __restrict__ part, T* __restrict__ prep, int r, int64_t splits) {
  __shared__ T Cs[64 * LR_CLD];
  __shared__ T Ds[64];
  const int rp = lr_rp(r), tid = threadIdx.x;
  const int64_t row = blockIdx.x;
  const T* pr = part + row * splits * lr_cap_part(r);
  T* out = prep + row * lr_prep_row(r);
  for (int i = tid; i < rp * rp; i += LR_THREADS) {
    const int a = i / rp, b = i - a * rp;
    T s = 0;
    for (int64_t sp = 0; sp < splits; ++sp) s += pr[sp * lr_cap_part(r) + i];
    Cs[a * LR_CLD + b] = a == b ? s + (T)1 : s;
  }
  if (tid == 0) {
    T s = 0;
    for (int64_t sp = 0; sp < splits; ++sp) s += pr[sp * lr_cap_part(r) + rp * rp];
    out[2 * rp * rp + 1] = s;
  }
  for (int k = 0; k < r; ++k) {          // right-looking, on the lower triangle
    __syncthreads();
    const T piv = lr_sqrt(Cs[k * LR_CLD + k]);
    __syncthreads();          // every thread has read the pivot
    if (tid == 0) {
      Cs[k * LR_CLD + k] = piv;
      Ds[k] = (T)1 / piv;
    }
    for (int i = k + 1 + tid; i < r; i += LR_THREADS) Cs[i * LR_CLD + k] = Cs[i * LR_CLD + k] / piv;
    __syncthreads();
    const int n = r - k - 1;
    for (int idx = tid; idx < n * n; idx += LR_THREADS) {
      const int i = k + 1 + idx / n, j = k + 1 + idx % n;
      if (j <= i) Cs[i * LR_CLD + j] -= Cs[i * LR_CLD + k] * Cs[j * LR_CLD + k];
    }
  }
  __syncthreads();
  if (tid < r) {          // column tid of M = L^-1 by forward substitution, into row tid of the upper triangle
    const int j = tid;
    for (int i = j + 1; i < r; ++i) {
      T s = Cs[i * LR_CLD + j] * Ds[j];
      for (int k = j + 1; k < i; ++k) s += Cs[i * LR_CLD + k] * Cs[j * LR_CLD + k];
      Cs[j * LR_CLD + i] = -s * Ds[i];
    }
  }
  __syncthreads();
  for (int idx = tid; idx < rp * rp; idx += LR_THREADS) {
    const int i = idx / rp, j = idx - i * rp;
    T mt = 0, ci = 0;
    if (i < r && j < r) {
      if (j >= i) mt = lr_minv(Cs, Ds, j, i);          // Mt[i][j] = M[j][i]
      for (int k = i > j ? i : j; k < r; ++k) ci += lr_minv(Cs, Ds, k, i) * lr_minv(Cs, Ds, k, j);
    }
    out[idx] = mt;
    out[rp * rp + idx] = ci;
  }
  if (tid == 0) {
    T s = 0;
    for (int i = 0; i < r; ++i) s += lr_log(Cs[i * LR_CLD + i]);
    out[2 * rp * rp] = (T)2 * s;
  }
}

// ---------------------------------------------------------------- lp
// grid = particle tiles * R
template <typename T>
__global__ __launch_bounds__(LR_THREADS) void k_lr_logprob(const T* __restrict__ mean, const T* __restrict__ factor, const T* __restrict__ diag,
                                                           const T* __restrict__ prep, const T* __restrict__ x, int shared, T* __restrict__ lp,
                                                           int64_t K, int64_t R, int D, int r, T c0) {
  const LrLds<T> L = lr_lds<T>();
  const int rp = lr_rp(r), RT = rp / 16;
  const int64_t row = blockIdx.x % R, k0 = (blockIdx.x / R) * 16;
  const T* pr = prep + row * lr_prep_row(r);
  lr_tile_u(L, factor + row * D * r, diag + row * D, mean + row * D, x, shared != 0, k0, K, R, row, D, r);
  const int wave = mfma_wave(threadIdx.x), m = mfma_m(threadIdx.x), q = mfma_q(threadIdx.x);
  if (wave < RT) {          // |L^-1 u|^2, rank tile `wave`
    const typename Mfma<T>::Acc t = lr_times(L.Us, pr, rp, wave, q, m);
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      T s = t[v] * t[v];
      s += __shfl_xor(s, 1, ZS_WAVE);
      s += __shfl_xor(s, 2, ZS_WAVE);
      s += __shfl_xor(s, 4, ZS_WAVE);
      s += __shfl_xor(s, 8, ZS_WAVE);
      if (m == 0) L.misc[80 + wave * 16 + MfmaTile<T>::acc_row(q, v)] = s;
    }
  }
  __syncthreads();
  if (threadIdx.x < 16 && k0 + threadIdx.x < K) {
    T quad = 0;
    for (int t = 0; t < RT; ++t) quad += L.misc[80 + t * 16 + threadIdx.x];
    lp[(k0 + threadIdx.x) * R + row] = lr_lp(L.misc[64 + threadIdx.x], quad, pr[2 * rp * rp + 1], pr[2 * rp * rp], c0);
  }
}

// ---------------------------------------------------------------- the density's backward
// grid = shares * R; share s walks the particle tiles s, s + shares, ... and adds them into its partial [gW[D, r] | gmean[D] | ga2[D]]
template <typename T>
__global__ __launch_bounds__(LR_THREADS) void k_lr_logprob_bwd(const T* __restrict__ mean, const T* __restrict__ factor, const T* __restrict__ diag,
                                                               const T* __restrict__ prep, const T* __restrict__ x, int shared,
                                                               const T* __restrict__ glp, T* __restrict__ part, T* __restrict__ gx, int64_t K,
                                                               int64_t R, int D, int r, int64_t shares) {
  typedef typename Mfma<T>::Acc Acc;
  const LrLds<T> L = lr_lds<T>();
  const int rp = lr_rp(r), RT = rp / 16;
  const int64_t row = blockIdx.x % R, share = blockIdx.x / R, tiles = blocks16(K);
  const T* Wr = factor + row * D * r;
  const T* dr = diag + row * D;
  const T* mr = mean + row * D;
  const T* Cinv = prep + row * lr_prep_row(r) + rp * rp;
  T* pW = part + (row * shares + share) * lr_bwd_part(D, r);
  T* pm = pW + (int64_t)D * r;
  T* pa = pm + D;
  const int wave = mfma_wave(threadIdx.x), m = mfma_m(threadIdx.x), q = mfma_q(threadIdx.x);
  const int dl = wave * 16 + m;          // this lane's d-row of a panel
  for (int64_t pt = share; pt < tiles; pt += shares) {
    const bool first = pt == share;
    const int64_t k0 = pt * 16;
    lr_tile_u(L, Wr, dr, mr, x, shared != 0, k0, K, R, row, D, r);
    Acc av = {0, 0, 0, 0};
    if (wave < RT) av = lr_times(L.Us, Cinv, rp, wave, q, m);
    __syncthreads();          // u has been read: v takes its place
    if (wave < RT) {
#pragma unroll
      for (int v = 0; v < 4; ++v) L.Us[MfmaTile<T>::acc_row(q, v) * LR_LDY + wave * 16 + m] = av[v];
    }
    T gq[4];
    int64_t kq[4];
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      kq[v] = k0 + MfmaTile<T>::acc_row(q, v);
      gq[v] = kq[v] < K ? glp[kq[v] * R + row] : (T)0;
    }
    for (int d0 = 0; d0 < D; d0 += LR_PANEL) {
      __syncthreads();          // v is written; the previous panel's readers are done
      lr_stage_factor(L, Wr, dr, D, r, rp, d0);
      lr_stage_y(L, x, shared != 0, mr, k0, K, R, row, D, d0);
      __syncthreads();
      const Acc vw = lr_times_panel_t(L, rp, dl, q, m);
      const int d = d0 + dl;
      const T rd = L.rds[dl];
      T a[4], gm = 0, ga = 0;
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        a[v] = lr_a(L.Ys[MfmaTile<T>::acc_row(q, v) * LR_LDY + dl], vw[v], rd);
        const T t = gq[v] * a[v];
        gm += t;
        ga += t * a[v];
        if (gx && kq[v] < K && d < D) gx[(kq[v] * R + row) * D + d] = -t;
      }
      gm += __shfl_xor(gm, 16, ZS_WAVE);          // over the tile's 16 particles: q = 0 .. 3
      gm += __shfl_xor(gm, 32, ZS_WAVE);
      ga += __shfl_xor(ga, 16, ZS_WAVE);
      ga += __shfl_xor(ga, 32, ZS_WAVE);
      if (q == 0 && d < D) {
        pm[d] = first ? gm : pm[d] + gm;
        pa[d] = first ? ga : pa[d] + ga;
      }
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        if (t < RT) {
          Acc w = {0, 0, 0, 0};
#pragma unroll
          for (int v = 0; v < 4; ++v) w = Mfma<T>::run(a[v], gq[v] * L.Us[MfmaTile<T>::acc_row(q, v) * LR_LDY + t * 16 + m], w);
          const int j = t * 16 + m;
#pragma unroll
          for (int v = 0; v < 4; ++v) {
            const int dd = d0 + wave * 16 + MfmaTile<T>::acc_row(q, v);
            if (dd < D && j < r) {
              T* o = pW + (int64_t)dd * r + j;
              *o = first ? w[v] : *o + w[v];
            }
          }
        }
      }
    }
  }
}

// grid = panels * R, a wave per d-row (16 rows in turn): the shares in order, then the closed forms
template <typename T>
__global__ __launch_bounds__(LR_THREADS) void k_lr_logprob_bwd_finish(const T* __restrict__ factor, const T* __restrict__ diag,
                                                                      const T* __restrict__ prep, const T* __restrict__ glp,
                                                                      const T* __restrict__ part, T* __restrict__ gmean, T* __restrict__ gfactor,
                                                                      T* __restrict__ gdiag, int64_t K, int64_t R, int D, int r, int64_t shares) {
  __shared__ T Ci[64 * LR_CLD];
  __shared__ T sh[4];
  const int rp = lr_rp(r), tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int64_t row = blockIdx.x % R, pn = blockIdx.x / R;
  const T* Cinv = prep + row * lr_prep_row(r) + rp * rp;
  for (int i = tid; i < rp * rp; i += LR_THREADS) Ci[(i / rp) * LR_CLD + i % rp] = Cinv[i];
  T sg = 0;
  for (int64_t k = tid; k < K; k += LR_THREADS) sg += glp[k * R + row];
  const T sumg = block_sum_256(sg, sh);          // (its barriers also publish Ci)
  const int64_t stride = lr_bwd_part(D, r);
  const T* p0 = part + row * shares * stride;
  const bool live = lane < r;
  const int jc = live ? lane : 0;
  for (int n = 0; n < 16; ++n) {
    const int d = (int)pn * LR_PANEL + wave * 16 + n;
    if (d >= D) break;          // (uniform over the wave)
    const T wj = live ? factor[(row * D + d) * r + lane] : (T)0;
    const T rd = (T)1 / diag[row * D + d];
    T s = 0;
    for (int i = 0; i < r; ++i) s += __shfl(wj, i, ZS_WAVE) * Ci[i * LR_CLD + jc];
    const T e = live ? s * rd : (T)0;
    if (live) {
      T acc = 0;
      for (int64_t sp = 0; sp < shares; ++sp) acc += p0[sp * stride + (int64_t)d * r + lane];
      gfactor[(row * D + d) * r + lane] = lr_gfactor(acc, sumg, e);
    }
    const T h = wave_sum(e * wj * rd);
    if (lane == 0) {
      T gm = 0, ga = 0;
      for (int64_t sp = 0; sp < shares; ++sp) {
        gm += p0[sp * stride + (int64_t)D * r + d];
        ga += p0[sp * stride + (int64_t)D * r + D + d];
      }
      gmean[row * D + d] = gm;
      gdiag[row * D + d] = lr_gdiag(ga, sumg, rd, h);
    }
  }
}

// ---------------------------------------------------------------- the draw
// grid = (particle tiles * R, panels)
template <typename T>
__global__ __launch_bounds__(LR_THREADS) void k_lr_sample(const T* __restrict__ mean, const T* __restrict__ factor, const T* __restrict__ diag,
                                                          const T* __restrict__ eps, T* __restrict__ z, int64_t K, int64_t R, int D, int r,
                                                          uint64_t seed, uint64_t call, const uint64_t* __restrict__ rs) {
  typedef typename Mfma<T>::Acc Acc;
  if (rs) { seed = rs[0]; call += rs[1]; }
  const PhiloxCall pc = philox_call(call, seed);
  const LrLds<T> L = lr_lds<T>();
  const int rp = lr_rp(r);
  const int64_t row = blockIdx.x % R, k0 = (blockIdx.x / R) * 16, wide = (int64_t)D + r;
  const int d0 = (int)blockIdx.y * LR_PANEL;
  lr_stage_factor(L, factor + row * D * r, diag + row * D, D, r, rp, d0);
  for (int i = threadIdx.x; i < 16 * rp; i += LR_THREADS) {          // the rank noise of the tile
    const int p = i / rp, j = i - p * rp;
    const int64_t k = k0 + p;
    L.Us[p * LR_LDY + j] = (k < K && j < r) ? lr_noise(eps, (k * R + row) * wide + D + j, pc) : (T)0;
  }
  __syncthreads();
  const int wave = mfma_wave(threadIdx.x), m = mfma_m(threadIdx.x), q = mfma_q(threadIdx.x);
  const int dl = wave * 16 + m, d = d0 + dl;
  const Acc ew = lr_times_panel_t(L, rp, dl, q, m);
  if (d < D) {
    const T mu = mean[row * D + d], dd = diag[row * D + d];
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int64_t k = k0 + MfmaTile<T>::acc_row(q, v);
      if (k < K) z[(k * R + row) * D + d] = lr_draw(mu, dd, lr_noise(eps, (k * R + row) * wide + d, pc), ew[v]);
    }
  }
}

// grid = panels * R; wave t owns the d-rows 16 t .. 16 t + 15 of the panel and walks all particles
template <typename T>
__global__ __launch_bounds__(LR_THREADS) void k_lr_sample_bwd(const T* __restrict__ diag, const T* __restrict__ eps, const T* __restrict__ gz,
                                                              T* __restrict__ gmean, T* __restrict__ gfactor, T* __restrict__ gdiag, int64_t K,
                                                              int64_t R, int D, int r, uint64_t seed, uint64_t call,
                                                              const uint64_t* __restrict__ rs) {
  typedef typename Mfma<T>::Acc Acc;
  if (rs) { seed = rs[0]; call += rs[1]; }
  const PhiloxCall pc = philox_call(call, seed);
  const int RT = lr_rp(r) / 16;
  const int64_t row = blockIdx.x % R, pn = blockIdx.x / R, wide = (int64_t)D + r;
  const int wave = mfma_wave(threadIdx.x), m = mfma_m(threadIdx.x), q = mfma_q(threadIdx.x);
  const int dbase = (int)pn * LR_PANEL + wave * 16, d = dbase + m;
  Acc acc[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) acc[t] = Acc{0, 0, 0, 0};
  T gm = 0, ge = 0;
  if (dbase < D) {          // (uniform over the wave)
    for (int64_t k4 = 0; k4 < K; k4 += 4) {
      const int64_t k = k4 + q, base = k * R + row;
      const bool live = k < K && d < D;
      const T g = live ? gz[base * D + d] : (T)0;
      const T e = live ? lr_noise(eps, base * wide + d, pc) : (T)0;
      gm += g;
      ge += g * e;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        if (t < RT) {
          const int j = t * 16 + m;
          acc[t] = Mfma<T>::run(g, (k < K && j < r) ? lr_noise(eps, base * wide + D + j, pc) : (T)0, acc[t]);
        }
      }
    }
  }
  gm += __shfl_xor(gm, 16, ZS_WAVE);          // the four lanes of a d-row: q = 0 .. 3
  gm += __shfl_xor(gm, 32, ZS_WAVE);
  ge += __shfl_xor(ge, 16, ZS_WAVE);
  ge += __shfl_xor(ge, 32, ZS_WAVE);
  if (q == 0 && d < D) {
    gmean[row * D + d] = gm;
    gdiag[row * D + d] = lr_draw_gdiag(ge, diag[row * D + d]);
  }
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    if (t < RT) {
      const int j = t * 16 + m;
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int dd = dbase + MfmaTile<T>::acc_row(q, v);
        if (dd < D && j < r) gfactor[(row * D + dd) * r + j] = acc[t][v];
      }
    }
  }
}

// ---------------------------------------------------------------- the entry points
// 0 = go on, 1 = nothing to do, else the code to return; `groups`: workgroups per row of the launch's x axis
int lr_check(bool pointers, int64_t K, int64_t R, int64_t D, int64_t r) {
  if (!pointers || K < 0 || R < 0 || D < 1 || r < 1) return ZS_EINVAL;
  if (D > ZS_LOWRANK_MAX_DIM || r > ZS_LOWRANK_MAX_RANK) return ZS_ENOTSUP;
  return (K == 0 || R == 0) ? 1 : 0;
}
bool lr_grid_fits(int64_t groups, int64_t R) { return groups <= (((int64_t)1 << 31) - 1) / R; }
// 1: x has no particle axis, 0: it has one, -1: neither
int lr_shared(int64_t Px, int64_t K, int64_t R, int64_t D) { return Px == K * R * D ? 0 : (Px == R * D ? 1 : -1); }
double lr_c0(int64_t D) { return -0.5 * (double)D * ZS_LOWRANK_LOG_2PI; }

template <typename T>
int lr_prepare(const void* factor, const void* diag, void* part, void* prep, int64_t R, int64_t D, int64_t r, int64_t splits, void* stream) {
  const int rc = lr_check(factor && diag && part && prep, 1, R, D, r);
  if (rc) return rc == 1 ? 0 : rc;
  if (splits < 1 || splits > lr_panels(D)) return ZS_EINVAL;
  if (!lr_grid_fits(splits, R)) return ZS_ENOTSUP;
  hipLaunchKernelGGL((k_lr_cap_partial<T>), dim3((unsigned)(splits * R)), dim3(LR_THREADS), lr_lds_bytes<T>(), (hipStream_t)stream,
                     (const T*)factor, (const T*)diag, (T*)part, R, (int)D, (int)r, splits);
  ZS_CHECK_LAUNCH();
  hipLaunchKernelGGL((k_lr_cap_finish<T>), dim3((unsigned)R), dim3(LR_THREADS), 0, (hipStream_t)stream, (const T*)part, (T*)prep, (int)r,
                     splits);
  ZS_CHECK_LAUNCH();
  return 0;
}

template <typename T>
int lr_logprob(const void* mean, const void* factor, const void* diag, const void* prep, const void* x, int64_t Px, void* lp, int64_t K,
               int64_t R, int64_t D, int64_t r, void* stream) {
  const int rc = lr_check(mean && factor && diag && prep && x && lp, K, R, D, r);
  if (rc) return rc == 1 ? 0 : rc;
  const int shared = lr_shared(Px, K, R, D);
  if (shared < 0) return ZS_EINVAL;
  if (!lr_grid_fits(blocks16(K), R)) return ZS_ENOTSUP;
  hipLaunchKernelGGL((k_lr_logprob<T>), dim3((unsigned)(blocks16(K) * R)), dim3(LR_THREADS), lr_lds_bytes<T>(), (hipStream_t)stream,
                     (const T*)mean, (const T*)factor, (const T*)diag, (const T*)prep, (const T*)x, shared, (T*)lp, K, R, (int)D, (int)r,
                     (T)lr_c0(D));
  ZS_CHECK_LAUNCH();
  return 0;
}

template <typename T>
int lr_logprob_bwd(const void* mean, const void* factor, const void* diag, const void* prep, const void* x, int64_t Px, const void* glp,
                   void* part, void* gx, void* gmean, void* gfactor, void* gdiag, int64_t K, int64_t R, int64_t D, int64_t r, int64_t shares,
                   void* stream) {
  const int rc = lr_check(mean && factor && diag && prep && x && glp && part && gmean && gfactor && gdiag, K, R, D, r);
  if (rc) return rc == 1 ? 0 : rc;
  const int shared = lr_shared(Px, K, R, D);
  if (shared < 0 || shares < 1 || shares > blocks16(K)) return ZS_EINVAL;
  if (!lr_grid_fits(shares, R) || !lr_grid_fits(lr_panels(D), R)) return ZS_ENOTSUP;
  hipLaunchKernelGGL((k_lr_logprob_bwd<T>), dim3((unsigned)(shares * R)), dim3(LR_THREADS), lr_lds_bytes<T>(), (hipStream_t)stream,
                     (const T*)mean, (const T*)factor, (const T*)diag, (const T*)prep, (const T*)x, shared, (const T*)glp, (T*)part, (T*)gx,
                     K, R, (int)D, (int)r, shares);
  ZS_CHECK_LAUNCH();
  hipLaunchKernelGGL((k_lr_logprob_bwd_finish<T>), dim3((unsigned)(lr_panels(D) * R)), dim3(LR_THREADS), 0, (hipStream_t)stream,
                     (const T*)factor, (const T*)diag, (const T*)prep, (const T*)glp, (const T*)part, (T*)gmean, (T*)gfactor, (T*)gdiag, K, R,
                     (int)D, (int)r, shares);
  ZS_CHECK_LAUNCH();
  return 0;
}

template <typename T>
int lr_sample(const void* mean, const void* factor, const void* diag, const void* eps, void* z, int64_t K, int64_t R, int64_t D, int64_t r,
              uint64_t seed, uint64_t call, const uint64_t* rs, void* stream) {
  const int rc = lr_check(mean && factor && diag && z, K, R, D, r);
  if (rc) return rc == 1 ? 0 : rc;
  if (!lr_grid_fits(blocks16(K), R)) return ZS_ENOTSUP;
  hipLaunchKernelGGL((k_lr_sample<T>), dim3((unsigned)(blocks16(K) * R), (unsigned)lr_panels(D)), dim3(LR_THREADS), lr_lds_bytes<T>(),
                     (hipStream_t)stream, (const T*)mean, (const T*)factor, (const T*)diag, (const T*)eps, (T*)z, K, R, (int)D, (int)r, seed,
                     call, rs);
  ZS_CHECK_LAUNCH();
  return 0;
}

template <typename T>
int lr_sample_bwd(const void* diag, const void* eps, const void* gz, void* gmean, void* gfactor, void* gdiag, int64_t K, int64_t R, int64_t D,
                  int64_t r, uint64_t seed, uint64_t call, const uint64_t* rs, void* stream) {
  const int rc = lr_check(diag && gz && gmean && gfactor && gdiag, K, R, D, r);
  if (rc) return rc == 1 ? 0 : rc;
  if (!lr_grid_fits(lr_panels(D), R)) return ZS_ENOTSUP;
  hipLaunchKernelGGL((k_lr_sample_bwd<T>), dim3((unsigned)(lr_panels(D) * R)), dim3(LR_THREADS), 0, (hipStream_t)stream, (const T*)diag,
                     (const T*)eps, (const T*)gz, (T*)gmean, (T*)gfactor, (T*)gdiag, K, R, (int)D, (int)r, seed, call, rs);
  ZS_CHECK_LAUNCH();
  return 0;
}

}  // namespace

extern "C" int zs_lowrank_abi_version(void) { return ZS_LOWRANK_ABI_VERSION; }
extern "C" int zs_lowrank_max_dim(void) { return ZS_LOWRANK_MAX_DIM; }
extern "C" int zs_lowrank_max_rank(void) { return ZS_LOWRANK_MAX_RANK; }
extern "C" int64_t zs_lowrank_splits(int which, int64_t K, int64_t R, int64_t D) {
  if (D > ZS_LOWRANK_MAX_DIM) return 0;
  switch (which) {
    case ZS_LOWRANK_WS_PREPARE: return lr_splits(R, D);
    case ZS_LOWRANK_WS_LOGPROB_BWD: return D < 1 ? 0 : lr_shares(K, R);
    default: return 0;
  }
}
extern "C" int64_t zs_lowrank_workspace_elems(int which, int64_t R, int64_t D, int64_t r, int64_t n) {
  if (R < 0 || D < 1 || D > ZS_LOWRANK_MAX_DIM || r < 1 || r > ZS_LOWRANK_MAX_RANK) return -1;
  switch (which) {
    case ZS_LOWRANK_WS_PREP: return R * lr_prep_row(r);
    case ZS_LOWRANK_WS_PREPARE: return n < 1 ? -1 : R * n * lr_cap_part(r);
    case ZS_LOWRANK_WS_LOGPROB_BWD: return n < 1 ? -1 : R * n * lr_bwd_part(D, r);
    default: return -1;
  }
}

#define ZS_LOWRANK_ENTRY(SFX, T)                                                                                                       \
  extern "C" int zs_lowrank_prepare##SFX(const void* factor, const void* diag, void* part, void* prep, int64_t R, int64_t D, int64_t r, \
                                         int64_t splits, void* stream) {                                                               \
    return lr_prepare<T>(factor, diag, part, prep, R, D, r, splits, stream);                                                           \
  }                                                                                                                                    \
  extern "C" int zs_lowrank_logprob##SFX(const void* mean, const void* factor, const void* diag, const void* prep, const void* x,      \
                                         int64_t Px, void* lp, int64_t K, int64_t R, int64_t D, int64_t r, void* stream) {             \
    return lr_logprob<T>(mean, factor, diag, prep, x, Px, lp, K, R, D, r, stream);                                                     \
  }                                                                                                                                    \
  extern "C" int zs_lowrank_logprob_bwd##SFX(const void* mean, const void* factor, const void* diag, const void* prep, const void* x,  \
                                             int64_t Px, const void* glp, void* part, void* gx, void* gmean, void* gfactor,            \
                                             void* gdiag, int64_t K, int64_t R, int64_t D, int64_t r, int64_t shares, void* stream) {  \
    return lr_logprob_bwd<T>(mean, factor, diag, prep, x, Px, glp, part, gx, gmean, gfactor, gdiag, K, R, D, r, shares, stream);       \
  }                                                                                                                                    \
  extern "C" int zs_lowrank_sample##SFX(const void* mean, const void* factor, const void* diag, const void* eps, void* z, int64_t K,   \
                                        int64_t R, int64_t D, int64_t r, uint64_t seed, uint64_t call, const uint64_t* rng_state,      \
                                        void* stream) {                                                                                \
    return lr_sample<T>(mean, factor, diag, eps, z, K, R, D, r, seed, call, rng_state, stream);                                        \
  }                                                                                                                                    \
  extern "C" int zs_lowrank_sample_bwd##SFX(const void* diag, const void* eps, const void* gz, void* gmean, void* gfactor,             \
                                            void* gdiag, int64_t K, int64_t R, int64_t D, int64_t r, uint64_t seed, uint64_t call,     \
                                            const uint64_t* rng_state, void* stream) {                                                 \
    return lr_sample_bwd<T>(diag, eps, gz, gmean, gfactor, gdiag, K, R, D, r, seed, call, rng_state, stream);                          \
  }

ZS_LOWRANK_ENTRY(_f32, float)
ZS_LOWRANK_ENTRY(_f64, double)
