// GPConditional: the predictive moments of a sparse Gaussian process with an ARD squared-exponential kernel, and their backward
// (include/zs_gp.h; its own library, ../lib/libzs_gp.so, `make gp`).
//
// The sixth user of the matrix cores after zs_topic, zs_matvar, zs_svgd, zs_mix and zs_lowrank.  The case is many inputs x
// [N, d] against few inducing inputs Z [M, d], M <= 128: the cross-covariance K_xz [N, M] is formed 16 rows at a time in the
// accumulators of a wave, exponentiated there, and kept as a [16, M] strip in LDS, where it is the row operand of every product
// that follows.  Nothing of size [N, M] reaches memory.  One template over the element type.
//
// A lane l = 16 q + m of a wave gives Mfma<T>::run(a, b, acc) the elements A[m][k = q] and B[k = q][m] of a 16 x 4 by 4 x 16 step
// and holds acc[v] = out[acc_row(q, v)][m].  Three products use it:
//   rows first    a = a strip at [m][4 s + q], b = an operand at [4 s + q][16 t + m]: acc[v] = out[row acc_row][column 16 t + m]
//   columns first the same two values in the other order: acc[v] = out[column 16 t + acc_row][row m] -- the moments are written
//                 with the 16 lanes of a q along n
//   over the rows a = a strip at [4 s + q][16 t + m]: the contraction runs over the 64 rows of the workgroup's block (the
//                 backward's sums over n); the output tiles are dealt to the four waves
#include "zs_common.h"
#include "zs_gp_math.h"
#include "../../include/zs_hip.h"
#include "../../include/zs_gp.h"

#pragma clang fp contract(off)

using namespace zs;

namespace {

template <typename T>
struct GpCap {
  static constexpr int MAX_INDUCING = sizeof(T) == 4 ? ZS_GP_MAX_INDUCING_F32 : ZS_GP_MAX_INDUCING_F64;
};

// ---------------------------------------------------------------- staging
// Zt[j][i] = Z[i][j] / l[j] - cen[j], cen[j] the mean over the inducing inputs of Z[:, j] / l[j]; zero past d and past M;
// zn[i] = |row i|^2.  Every thread of the workgroup calls it; it ends with a barrier.
template <typename T>
__device__ __forceinline__ void gp_stage_z(T* Zt, T* cen, T* zn, const T* __restrict__ Z, const T* __restrict__ len, int M, int d, int Mp,
                                           int d16) {
  const int ldb = gp_ldb(Mp), tid = threadIdx.x;
  for (int i = tid; i < d16 * Mp; i += GP_THREADS) {
    const int j = i / Mp, c = i - j * Mp;
    Zt[j * ldb + c] = (j < d && c < M) ? Z[(int64_t)c * d + j] / len[j] : (T)0;
  }
  __syncthreads();
  if (tid < 64) {
    T s = 0;
    if (tid < d)
      for (int c = 0; c < M; ++c) s += Zt[tid * ldb + c];
    cen[tid] = s / (T)M;
  }
  __syncthreads();
  for (int i = tid; i < d * Mp; i += GP_THREADS) {
    const int j = i / Mp, c = i - j * Mp;
    if (c < M) Zt[j * ldb + c] -= cen[j];
  }
  __syncthreads();
  if (tid < Mp) {
    T s = 0;
    for (int j = 0; j < d; ++j) s += Zt[j * ldb + tid] * Zt[j * ldb + tid];
    zn[tid] = s;
  }
  __syncthreads();
}

// The [16, Mp] strip of K_xz of one wave: a[s] is the lane's element [row m][4 s + q] of the centred x / l.  The score tile
// x~ . z~ is formed on the matrix cores, -1/2 (|x~|^2 + |z~|^2) is added and the tile exponentiated in the accumulator;
// Kw[row][column] takes it, zero past M and for the rows past `rows`.
template <typename T>
__device__ __forceinline__ void gp_strip(const T (&a)[16], int steps, const T* Zt, const T* zn, T* Kw, int Mp, int M, int64_t rows, T amp2,
                                         int q, int m) {
  typedef typename Mfma<T>::Acc Acc;
  const int ldb = gp_ldb(Mp), lda = gp_lda(Mp);
  T xn = 0;
#pragma unroll
  for (int s = 0; s < 16; ++s) xn += a[s] * a[s];
  xn += __shfl_xor(xn, 16, ZS_WAVE);          // the four lanes of a row: q = 0 .. 3
  xn += __shfl_xor(xn, 32, ZS_WAVE);
  T xr[4];
#pragma unroll
  for (int v = 0; v < 4; ++v) xr[v] = __shfl(xn, MfmaTile<T>::acc_row(q, v), ZS_WAVE);
  for (int t = 0; t < Mp / 16; ++t) {
    Acc acc = {0, 0, 0, 0};
#pragma unroll
    for (int s = 0; s < 16; ++s)
      if (s < steps) acc = Mfma<T>::run(a[s], Zt[(4 * s + q) * ldb + 16 * t + m], acc);
    const int c = 16 * t + m;
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int r = MfmaTile<T>::acc_row(q, v);
      Kw[r * lda + c] = (c < M && r < rows) ? gp_kernel(acc[v], xr[v], zn[c], amp2) : (T)0;
    }
  }
}

// ---------------------------------------------------------------- prepare
// one workgroup: (L^-1)^T by forward substitution (a thread per column), w = L^-1 fz^T, c = L^-T w.  w is written to the
// workspace and read back by other threads of the workgroup after a barrier, which is what makes it visible to them: ws is
// not __restrict__.
template <typename T>
__global__ __launch_bounds__(GP_THREADS) void k_gp_prepare(const T* __restrict__ L, const T* __restrict__ fz, int shared, T* ws,
                                                           int M, int K) {
  const int Mp = gp_p16(M), Kp = gp_p16(K), LDP = Mp + 1, tid = threadIdx.x;
  T* Ls = tile_lds<T>();
  T* Xt = Ls + Mp * LDP;
  for (int i = tid; i < Mp * Mp; i += GP_THREADS) {
    const int r = i / Mp, c = i - r * Mp;
    Ls[r * LDP + c] = (r < M && c <= r) ? L[(int64_t)r * M + c] : (T)0;          // only i >= j is read
    Xt[r * LDP + c] = 0;
  }
  __syncthreads();
  if (tid < M) {          // column j of X = L^-1, kept as row j of Xt
    const int j = tid;
    Xt[j * LDP + j] = (T)1 / Ls[j * LDP + j];
    for (int i = j + 1; i < M; ++i) {
      T s = 0;
      for (int k = j; k < i; ++k) s += Ls[i * LDP + k] * Xt[j * LDP + k];
      Xt[j * LDP + i] = -s / Ls[i * LDP + i];
    }
  }
  __syncthreads();
  T* wv = ws + (int64_t)Mp * Mp + (int64_t)Mp * Kp;
  T* cv = ws + (int64_t)Mp * Mp;
  for (int i = tid; i < Mp * Mp; i += GP_THREADS) ws[i] = Xt[(i / Mp) * LDP + i % Mp];
  for (int idx = tid; idx < Mp * Kp; idx += GP_THREADS) {
    const int i = idx / Kp, k = idx - i * Kp;
    T s = 0;
    if (i < M && k < K) {
      const T* f = fz + (shared ? 0 : (int64_t)k * M);
      for (int j = 0; j <= i; ++j) s += Xt[j * LDP + i] * f[j];
    }
    wv[idx] = s;
  }
  __syncthreads();          // w is visible to the workgroup
  for (int idx = tid; idx < Mp * Kp; idx += GP_THREADS) {
    const int j = idx / Kp, k = idx - j * Kp;
    T s = 0;
    if (j < M && k < K)
      for (int i = j; i < M; ++i) s += Xt[j * LDP + i] * wv[i * Kp + k];
    cv[idx] = s;
  }
}

// ---------------------------------------------------------------- the moments
// grid = 64-row blocks of x; a wave owns 16 rows
template <typename T>
__global__ __launch_bounds__(GP_THREADS) void k_gp_moments(const T* __restrict__ x, const T* __restrict__ Z, const T* __restrict__ len,
                                                           const T* __restrict__ amp, const T* __restrict__ ws, T* __restrict__ mean,
                                                           T* __restrict__ var, int64_t N, int M, int d, int K) {
  typedef typename Mfma<T>::Acc Acc;
  const int Mp = gp_p16(M), d16 = gp_p16(d), Kp = gp_p16(K), ldb = gp_ldb(Mp), lda = gp_lda(Mp), tid = threadIdx.x;
  T* Lt = tile_lds<T>();
  T* Zt = Lt + Mp * ldb;
  T* Ks = Zt + d16 * ldb;
  T* cen = Ks + GP_ROWS * lda;
  T* zn = cen + 64;
  for (int i = tid; i < Mp * Mp; i += GP_THREADS) Lt[(i / Mp) * ldb + i % Mp] = ws[i];
  gp_stage_z(Zt, cen, zn, Z, len, M, d, Mp, d16);
  const int wave = mfma_wave(tid), m = mfma_m(tid), q = mfma_q(tid), steps = (d + 3) / 4;
  const int64_t n0 = (int64_t)blockIdx.x * GP_ROWS + wave * 16, n = n0 + m;
  const T amp2 = amp[0] * amp[0];
  T a[16];          // the wave's row operand stays in registers
#pragma unroll
  for (int s = 0; s < 16; ++s) {
    const int j = 4 * s + q;
    a[s] = (j < d && n < N) ? x[n * d + j] / len[j] - cen[j] : (T)0;
  }
  T* Kw = Ks + wave * 16 * lda;
  gp_strip(a, steps, Zt, zn, Kw, Mp, M, N - n0, amp2, q, m);
  __syncthreads();
  // A = K_xz L^-T, columns first: acc[v] = A[n0 + m][16 t + acc_row]; column block t needs the k-steps up to its diagonal block
  T sq = 0;
  for (int t = 0; t < Mp / 16; ++t) {
    Acc acc = {0, 0, 0, 0};
    for (int s = 0; s < 4 * (t + 1); ++s) acc = Mfma<T>::run(Lt[(4 * s + q) * ldb + 16 * t + m], Kw[m * lda + 4 * s + q], acc);
#pragma unroll
    for (int v = 0; v < 4; ++v) sq += acc[v] * acc[v];
  }
  sq += __shfl_xor(sq, 16, ZS_WAVE);
  sq += __shfl_xor(sq, 32, ZS_WAVE);
  if (q == 0 && n < N) var[n] = gp_var(amp2, sq);
  // mean = K_xz c, columns first, the particles in tiles of 16
  const T* cv = ws + (int64_t)Mp * Mp;
  for (int kt = 0; kt < Kp / 16; ++kt) {
    Acc acc = {0, 0, 0, 0};
    for (int s = 0; s < Mp / 4; ++s) acc = Mfma<T>::run(cv[(4 * s + q) * Kp + 16 * kt + m], Kw[m * lda + 4 * s + q], acc);
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int k = 16 * kt + MfmaTile<T>::acc_row(q, v);
      if (k < K && n < N) mean[(int64_t)k * N + n] = acc[v];
    }
  }
}

// ---------------------------------------------------------------- the backward
// this thread's element of a share's partial: the first block writes it, the later ones add (the same thread, in block order)
template <typename T>
__device__ __forceinline__ void gp_add(T* o, T v, bool first) { *o = first ? v : *o + v; }

// grid = shares; share s walks the 64-row blocks s, s + shares, ...
template <typename T>
__global__ __launch_bounds__(GP_THREADS) void k_gp_moments_bwd(const T* __restrict__ x, const T* __restrict__ Z, const T* __restrict__ len,
                                                               const T* __restrict__ amp, const T* __restrict__ ws,
                                                               const T* __restrict__ gmean, const T* __restrict__ gvar, T* __restrict__ part,
                                                               T* __restrict__ gx, int64_t N, int M, int d, int K, int64_t shares) {
  typedef typename Mfma<T>::Acc Acc;
  const int Mp = gp_p16(M), d16 = gp_p16(d), Kp = gp_p16(K), ldb = gp_ldb(Mp), lda = gp_lda(Mp), ldx = gp_lda(d16), tid = threadIdx.x;
  const int MT = Mp / 16, DT = d16 / 16, KT = Kp / 16;
  T* Zt = tile_lds<T>();
  T* Ks = Zt + d16 * ldb;
  T* As = Ks + GP_ROWS * lda;
  T* Xs = As + GP_ROWS * lda;
  T* cen = Xs + GP_ROWS * ldx;
  T* zn = cen + 64;
  T* rowP = zn + Mp;
  T* gvs = rowP + GP_ROWS;
  gp_stage_z(Zt, cen, zn, Z, len, M, d, Mp, d16);
  const int wave = mfma_wave(tid), m = mfma_m(tid), q = mfma_q(tid), steps = (d + 3) / 4;
  const T amp2 = amp[0] * amp[0];
  const T* Lt = ws;          // (L^-1)^T [Mp, Mp], read from memory
  const T* cv = ws + (int64_t)Mp * Mp;
  const GpPart P = gp_part(M, d, K);
  T* mine = part + (int64_t)blockIdx.x * P.stride;
  T* Kw = Ks + wave * 16 * lda;
  T* Aw = As + wave * 16 * lda;
  const T* Xw = Xs + wave * 16 * ldx;
  T ls[4] = {0, 0, 0, 0}, pa = 0, pg = 0;
  const int64_t nb = gp_row_blocks(N);
  for (int64_t b = blockIdx.x; b < nb; b += shares) {
    const bool first = b == (int64_t)blockIdx.x;
    const int64_t nb0 = b * GP_ROWS, n0 = nb0 + wave * 16, n = n0 + m;
    __syncthreads();          // the previous block's readers are done
    for (int i = tid; i < GP_ROWS * d16; i += GP_THREADS) {
      const int r = i / d16, j = i - r * d16;
      Xs[r * ldx + j] = (nb0 + r < N && j < d) ? x[(nb0 + r) * d + j] / len[j] - cen[j] : (T)0;
    }
    if (tid < GP_ROWS) gvs[tid] = (gvar && nb0 + tid < N) ? gvar[nb0 + tid] : (T)0;
    __syncthreads();
    T a[16];
#pragma unroll
    for (int s = 0; s < 16; ++s) a[s] = s < steps ? Xw[m * ldx + 4 * s + q] : (T)0;
    gp_strip(a, steps, Zt, zn, Kw, Mp, M, N - n0, amp2, q, m);
    __syncthreads();
    if (gvar) {          // A = K_xz L^-T of the wave's rows, rows first
      for (int t = 0; t < MT; ++t) {
        Acc acc = {0, 0, 0, 0};
        for (int s = 0; s < 4 * (t + 1); ++s) acc = Mfma<T>::run(Kw[m * lda + 4 * s + q], Lt[(4 * s + q) * Mp + 16 * t + m], acc);
#pragma unroll
        for (int v = 0; v < 4; ++v) Aw[MfmaTile<T>::acc_row(q, v) * lda + 16 * t + m] = acc[v];
      }
    }
    if (gmean) {          // K_xz^T gmean^T [Mp, Kp] over the block's rows
      for (int tt = wave; tt < MT * KT; tt += 4) {
        const int mt = tt / KT, kt = tt - mt * KT, kk = 16 * kt + m;
        Acc acc = {0, 0, 0, 0};
#pragma unroll 4
        for (int s = 0; s < 16; ++s) {
          const int64_t nn = nb0 + 4 * s + q;
          acc = Mfma<T>::run(Ks[(4 * s + q) * lda + 16 * mt + m], (nn < N && kk < K) ? gmean[(int64_t)kk * N + nn] : (T)0, acc);
        }
#pragma unroll
        for (int v = 0; v < 4; ++v) gp_add(mine + P.B + (int64_t)(16 * mt + MfmaTile<T>::acc_row(q, v)) * Kp + kk, acc[v], first);
      }
    }
    __syncthreads();          // K_xz has been read by every wave: P takes its place
    // G_K = gmean^T c^T + G_A L^-1 with G_A = -2 gvar A, then P = G_K o K_xz in place
    T rp[4] = {0, 0, 0, 0};
    for (int t = 0; t < MT; ++t) {
      Acc acc = {0, 0, 0, 0};
      if (gmean) {
        for (int s = 0; s < Kp / 4; ++s) {
          const int kk = 4 * s + q;
          acc = Mfma<T>::run((kk < K && n < N) ? gmean[(int64_t)kk * N + n] : (T)0, cv[(16 * t + m) * Kp + kk], acc);
        }
      }
      if (gvar) {
        const T g2 = (T)-2 * gvs[wave * 16 + m];
        for (int s = 4 * t; s < Mp / 4; ++s) acc = Mfma<T>::run(g2 * Aw[m * lda + 4 * s + q], Lt[(16 * t + m) * Mp + 4 * s + q], acc);
      }
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int o = MfmaTile<T>::acc_row(q, v) * lda + 16 * t + m;
        const T pv = acc[v] * Kw[o];
        Kw[o] = pv;
        rp[v] += pv;
      }
    }
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      T s = rp[v];
      s += __shfl_xor(s, 1, ZS_WAVE);
      s += __shfl_xor(s, 2, ZS_WAVE);
      s += __shfl_xor(s, 4, ZS_WAVE);
      s += __shfl_xor(s, 8, ZS_WAVE);
      if (m == 0) rowP[wave * 16 + MfmaTile<T>::acc_row(q, v)] = s;
    }
    __syncthreads();
    if (tid < GP_ROWS) {
      pa += rowP[tid];
      pg += gvs[tid];
    }
    // gx~ = P z~ - rowsum(P) x~ of the wave's rows, rows first; its product with x~ is the rows' part of the lengthscale sum
#pragma unroll
    for (int jt = 0; jt < 4; ++jt) {
      if (jt < DT) {
        Acc acc = {0, 0, 0, 0};
        for (int s = 0; s < Mp / 4; ++s) acc = Mfma<T>::run(Kw[m * lda + 4 * s + q], Zt[(16 * jt + m) * ldb + 4 * s + q], acc);
        const int j = 16 * jt + m;
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          const int r = MfmaTile<T>::acc_row(q, v);
          const T xv = Xw[r * ldx + j], g = gp_gscaled(acc[v], rowP[wave * 16 + r], xv);
          ls[jt] += xv * g;
          if (gx && j < d && n0 + r < N) gx[(n0 + r) * d + j] = g / len[j];
        }
      }
    }
    // P^T x~ [Mp, d16] and colsum P over the block's rows
    for (int tt = wave; tt < MT * DT; tt += 4) {
      const int mt = tt / DT, jt = tt - mt * DT;
      Acc acc = {0, 0, 0, 0};
#pragma unroll 4
      for (int s = 0; s < 16; ++s) acc = Mfma<T>::run(Ks[(4 * s + q) * lda + 16 * mt + m], Xs[(4 * s + q) * ldx + 16 * jt + m], acc);
#pragma unroll
      for (int v = 0; v < 4; ++v) gp_add(mine + P.PtX + (int64_t)(16 * mt + MfmaTile<T>::acc_row(q, v)) * d16 + 16 * jt + m, acc[v], first);
    }
    if (tid < Mp) {
      T s = 0;
      for (int r = 0; r < GP_ROWS; ++r) s += Ks[r * lda + tid];
      gp_add(mine + P.colP + tid, s, first);
    }
    if (gvar) {          // A^T diag(gvar) A, the tiles on and below the diagonal
      for (int tt = wave; tt < MT * (MT + 1) / 2; tt += 4) {
        int ti = 0;
        while ((ti + 1) * (ti + 2) / 2 <= tt) ++ti;
        const int tj = tt - ti * (ti + 1) / 2;
        Acc acc = {0, 0, 0, 0};
#pragma unroll 4
        for (int s = 0; s < 16; ++s) {
          const int r = 4 * s + q;
          acc = Mfma<T>::run(gvs[r] * As[r * lda + 16 * ti + m], As[r * lda + 16 * tj + m], acc);
        }
#pragma unroll
        for (int v = 0; v < 4; ++v) gp_add(mine + P.Q + (int64_t)(16 * ti + MfmaTile<T>::acc_row(q, v)) * Mp + 16 * tj + m, acc[v], first);
      }
    }
  }
  // the sums the lanes carried over the blocks: the four waves' lengthscale sums in wave order, sum P and sum gvar
  __syncthreads();
#pragma unroll
  for (int jt = 0; jt < 4; ++jt) {
    T s = ls[jt];
    s += __shfl_xor(s, 16, ZS_WAVE);
    s += __shfl_xor(s, 32, ZS_WAVE);
    if (q == 0 && jt < DT) Xs[wave * 64 + 16 * jt + m] = s;
  }
  __syncthreads();
  if (tid < d16) mine[P.lsum + tid] = ((Xs[tid] + Xs[64 + tid]) + Xs[128 + tid]) + Xs[192 + tid];
  if (tid < GP_ROWS) {
    pa = wave_sum(pa);
    pg = wave_sum(pg);
    if (tid == 0) {
      mine[P.sums] = pa;
      mine[P.sums + 1] = pg;
    }
  }
}

// one workgroup: the shares in order, the closed forms of gZ, gl and ga, and the prepare's backward to gfz and gL.  The summed
// partial, h and e live in `part` and are read by other threads of the workgroup than wrote them, after a barrier, which is
// what makes them visible: part is not __restrict__.
template <typename T>
__global__ __launch_bounds__(GP_THREADS) void k_gp_bwd_finish(const T* __restrict__ Z, const T* __restrict__ len, const T* __restrict__ amp,
                                                              const T* __restrict__ ws, T* part, int64_t shares, int has_gmean,
                                                              int has_gvar, int shared, T* __restrict__ gZ, T* __restrict__ glen,
                                                              T* __restrict__ gamp, T* __restrict__ gL, T* __restrict__ gfz, int M, int d,
                                                              int K) {
  const int Mp = gp_p16(M), d16 = gp_p16(d), Kp = gp_p16(K), ldb = gp_ldb(Mp), tid = threadIdx.x;
  const GpPart P = gp_part(M, d, K);
  T* S = part + shares * P.stride;          // the summed partial
  T* h = S + P.stride;
  T* e = h + (int64_t)Mp * Kp;
  const T* Lt = ws;
  const T* cv = ws + (int64_t)Mp * Mp;
  const T* wv = cv + (int64_t)Mp * Kp;
  T* Zt = tile_lds<T>();
  T* cen = Zt + d16 * ldb;
  T* zn = cen + 64;
  for (int64_t idx = tid; idx < P.stride; idx += GP_THREADS) {
    int64_t src = idx;
    bool live = true;
    if (idx < P.PtX) {
      live = has_gmean != 0;
    } else if (idx >= P.Q && idx < P.colP) {          // the tiles above the diagonal are those below, transposed
      const int64_t o = idx - P.Q, i = o / Mp, j = o - i * Mp;
      live = has_gvar != 0;
      if (i / 16 < j / 16) src = P.Q + j * Mp + i;
    }
    T s = 0;
    if (live)
      for (int64_t sp = 0; sp < shares; ++sp) s += part[sp * P.stride + src];
    S[idx] = s;
  }
  gp_stage_z(Zt, cen, zn, Z, len, M, d, Mp, d16);          // (its barriers also publish S)
  if (gZ) {
    for (int idx = tid; idx < M * d; idx += GP_THREADS) {
      const int i = idx / d, j = idx - i * d;
      gZ[idx] = gp_gscaled(S[P.PtX + (int64_t)i * d16 + j], S[P.colP + i], Zt[j * ldb + i]) / len[j];
    }
  }
  if (glen && tid < d) {
    T sz = 0;
    for (int i = 0; i < M; ++i) sz += Zt[tid * ldb + i] * gp_gscaled(S[P.PtX + (int64_t)i * d16 + tid], S[P.colP + i], Zt[tid * ldb + i]);
    glen[tid] = gp_glength(S[P.lsum + tid], sz, len[tid]);
  }
  if (gamp && tid == 0) gamp[0] = gp_gamp(S[P.sums], S[P.sums + 1], amp[0]);
  if (!gL && !gfz) return;
  // through the prepare: G_c = S.B; h = L^-1 G_c, e = L^-T h = gfz^T; gL = tril(2 L^-T Q - c h^T - e w^T)
  for (int idx = tid; idx < Mp * Kp; idx += GP_THREADS) {
    const int i = idx / Kp, k = idx - i * Kp;
    T s = 0;
    if (i < M)
      for (int j = 0; j <= i; ++j) s += Lt[j * Mp + i] * S[P.B + (int64_t)j * Kp + k];
    h[idx] = s;
  }
  __syncthreads();
  for (int idx = tid; idx < Mp * Kp; idx += GP_THREADS) {
    const int j = idx / Kp, k = idx - j * Kp;
    T s = 0;
    for (int i = j; i < M; ++i) s += Lt[j * Mp + i] * h[i * Kp + k];
    e[idx] = s;
  }
  __syncthreads();
  if (gfz) {
    if (shared) {
      for (int j = tid; j < M; j += GP_THREADS) {
        T s = 0;
        for (int k = 0; k < K; ++k) s += e[j * Kp + k];
        gfz[j] = s;
      }
    } else {
      for (int idx = tid; idx < K * M; idx += GP_THREADS) {
        const int k = idx / M, j = idx - k * M;
        gfz[idx] = e[j * Kp + k];
      }
    }
  }
  if (gL) {
    for (int idx = tid; idx < M * M; idx += GP_THREADS) {
      const int i = idx / M, j = idx - i * M;
      T val = 0;
      if (i >= j) {
        T s1 = 0, s2 = 0;
        for (int k = 0; k < K; ++k) s1 += cv[i * Kp + k] * h[j * Kp + k] + e[i * Kp + k] * wv[j * Kp + k];
        if (has_gvar)
          for (int r = i; r < M; ++r) s2 += Lt[i * Mp + r] * S[P.Q + (int64_t)r * Mp + j];
        val = (T)2 * s2 - s1;
      }
      gL[idx] = val;          // the upper triangle is written as zeros
    }
  }
}

// ---------------------------------------------------------------- the entry points
// a launch may ask for more dynamic LDS than the default limit of a kernel: raise the kernel's limit to the device's, once per
// kernel (host-side bookkeeping of the runtime; nothing is enqueued).  A failure here shows as the launch's own error.
template <typename F>
hipError_t gp_raise_lds_limit(F kernel) {
  return hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, ZS_GP_LDS_BYTES);
}
#define ZS_GP_ALLOW_LDS(KERNEL)                                 \
  do {                                                          \
    static const hipError_t once = gp_raise_lds_limit(KERNEL);  \
    (void)once;                                                 \
  } while (0)

template <typename T>
int gp_check(bool pointers, int64_t N, int64_t M, int64_t d, int64_t K) {
  if (!pointers || N < 0 || M < 1 || d < 1 || K < 1) return ZS_EINVAL;
  if (M > GpCap<T>::MAX_INDUCING || d > ZS_GP_MAX_INPUT_DIM || K > ZS_GP_MAX_PARTICLES || gp_row_blocks(N) > (((int64_t)1 << 31) - 1)) return ZS_ENOTSUP;
  return 0;
}
// 1: fz has no particle axis, 0: it has one, -1: neither
int gp_shared(int64_t Pf, int64_t M, int64_t K) { return Pf == K * M ? 0 : (Pf == M ? 1 : -1); }

template <typename T>
int gp_prepare(const void* L, const void* fz, int64_t Pf, void* ws, int64_t M, int64_t K, void* stream) {
  const int rc = gp_check<T>(L && fz && ws, 0, M, 1, K);
  if (rc) return rc;
  const int shared = gp_shared(Pf, M, K);
  if (shared < 0) return ZS_EINVAL;
  ZS_GP_ALLOW_LDS(k_gp_prepare<T>);
  hipLaunchKernelGGL((k_gp_prepare<T>), dim3(1), dim3(GP_THREADS), sizeof(T) * (size_t)gp_prep_lds_elems(gp_p16(M)), (hipStream_t)stream,
                     (const T*)L, (const T*)fz, shared, (T*)ws, (int)M, (int)K);
  ZS_CHECK_LAUNCH();
  return 0;
}

template <typename T>
int gp_moments(const void* x, const void* Z, const void* len, const void* amp, const void* ws, void* mean, void* var, int64_t N, int64_t M,
               int64_t d, int64_t K, void* stream) {
  const int rc = gp_check<T>(x && Z && len && amp && ws && mean && var, N, M, d, K);
  if (rc) return rc;
  if (N == 0) return 0;
  ZS_GP_ALLOW_LDS(k_gp_moments<T>);
  hipLaunchKernelGGL((k_gp_moments<T>), dim3((unsigned)gp_row_blocks(N)), dim3(GP_THREADS),
                     sizeof(T) * (size_t)gp_fwd_lds_elems(gp_p16(M), gp_p16(d)), (hipStream_t)stream, (const T*)x, (const T*)Z, (const T*)len,
                     (const T*)amp, (const T*)ws, (T*)mean, (T*)var, N, (int)M, (int)d, (int)K);
  ZS_CHECK_LAUNCH();
  return 0;
}

template <typename T>
int gp_moments_bwd(const void* x, const void* Z, const void* len, const void* amp, int64_t Pf, const void* ws, const void* gmean,
                   const void* gvar, void* part, void* gx, void* gZ, void* glen, void* gamp, void* gL, void* gfz, int64_t N, int64_t M,
                   int64_t d, int64_t K, int64_t shares, void* stream) {
  const int rc = gp_check<T>(x && Z && len && amp && ws && part, N, M, d, K);
  if (rc) return rc;
  const int shared = gp_shared(Pf, M, K);
  if (shared < 0 || N < 1 || shares < 1 || shares > gp_row_blocks(N)) return ZS_EINVAL;
  ZS_GP_ALLOW_LDS(k_gp_moments_bwd<T>);
  hipLaunchKernelGGL((k_gp_moments_bwd<T>), dim3((unsigned)shares), dim3(GP_THREADS),
                     sizeof(T) * (size_t)gp_bwd_lds_elems(gp_p16(M), gp_p16(d)), (hipStream_t)stream, (const T*)x, (const T*)Z, (const T*)len,
                     (const T*)amp, (const T*)ws, (const T*)gmean, (const T*)gvar, (T*)part, (T*)gx, N, (int)M, (int)d, (int)K, shares);
  ZS_CHECK_LAUNCH();
  const int Mp = gp_p16(M);
  hipLaunchKernelGGL((k_gp_bwd_finish<T>), dim3(1), dim3(GP_THREADS), sizeof(T) * (size_t)(gp_p16(d) * gp_ldb(Mp) + 64 + Mp),
                     (hipStream_t)stream, (const T*)Z, (const T*)len, (const T*)amp, (const T*)ws, (T*)part, shares, gmean ? 1 : 0,
                     gvar ? 1 : 0, shared, (T*)gZ, (T*)glen, (T*)gamp, (T*)gL, (T*)gfz, (int)M, (int)d, (int)K);
  ZS_CHECK_LAUNCH();
  return 0;
}

}  // namespace

extern "C" int zs_gp_abi_version(void) { return ZS_GP_ABI_VERSION; }
extern "C" int zs_gp_max_inducing(int elem_bytes) { return gp_max_inducing(elem_bytes); }
extern "C" int zs_gp_max_input_dim(void) { return ZS_GP_MAX_INPUT_DIM; }
extern "C" int64_t zs_gp_row_shares(int64_t N) { return gp_shares(N); }
extern "C" int64_t zs_gp_workspace_elems(int which, int64_t M, int64_t d, int64_t K, int64_t n) {
  if (M < 1 || M > ZS_GP_MAX_INDUCING_F32 || d < 1 || d > ZS_GP_MAX_INPUT_DIM || K < 1 || K > ZS_GP_MAX_PARTICLES) return -1;
  switch (which) {
    case ZS_GP_WS_PREP: return gp_prep_elems(M, K);
    case ZS_GP_WS_BWD: return n < 1 ? -1 : gp_bwd_elems(M, d, K, n);
    default: return -1;
  }
}

#define ZS_GP_ENTRY(SFX, T)                                                                                                             \
  extern "C" int zs_gp_prepare##SFX(const void* kzz_tril, const void* fz, int64_t Pf, void* prep, int64_t M, int64_t K, void* stream) { \
    return gp_prepare<T>(kzz_tril, fz, Pf, prep, M, K, stream);                                                                         \
  }                                                                                                                                     \
  extern "C" int zs_gp_moments##SFX(const void* x, const void* inducing, const void* lengthscale, const void* amplitude,                \
                                    const void* prep, void* mean, void* var, int64_t N, int64_t M, int64_t d, int64_t K, void* stream) { \
    return gp_moments<T>(x, inducing, lengthscale, amplitude, prep, mean, var, N, M, d, K, stream);                                     \
  }                                                                                                                                     \
  extern "C" int zs_gp_moments_bwd##SFX(const void* x, const void* inducing, const void* lengthscale, const void* amplitude,            \
                                        int64_t Pf, const void* prep, const void* gmean, const void* gvar, void* part, void* gx,        \
                                        void* ginducing, void* glengthscale, void* gamplitude, void* gtril, void* gfz, int64_t N,       \
                                        int64_t M, int64_t d, int64_t K, int64_t shares, void* stream) {                                \
    return gp_moments_bwd<T>(x, inducing, lengthscale, amplitude, Pf, prep, gmean, gvar, part, gx, ginducing, glengthscale, gamplitude, \
                             gtril, gfz, N, M, d, K, shares, stream);                                                                   \
  }

ZS_GP_ENTRY(_f32, float)
ZS_GP_ENTRY(_f64, double)
