// M1, M2 and their backwards: MatrixVariateNormalCholesky (include/zs_matvar.h; its own library, ../lib/libzs_matvar.so,
// `make matvar`).
//
// A torch composition of the node is a chain of tril, expand, matmul, solve_triangular, diagonal, log and sum launches that
// materialises [K, R, n, n] and [K, R, p, p] expansions of the factors and keeps them for the backward.  Here an event lives in
// LDS as a tile of 16 x 16 blocks (zs_matvar_math.h: the padding, the budget) and every product and every substitution step runs on
// v_mfma_{f32,f64}_16x16x4; the factors are read from memory block by block as operands (all particles of a row read the same
// factor: it stays in L2), blocks above the diagonal are never read and never multiplied.
//
// A lane l = 16 q + m of a wave holds, for step s of a 16 x 16 block product, A[m][4 s + q] and B[4 s + q][m], and leaves with
// D[acc_row(q, v)][m], v = 0..3 (zs_tile_math.h).  Two things follow, and the whole file is built on them:
//   * an accumulator can be the B operand of the next product as it stands, with the contraction index of step v taken as
//     acc_row(q, v) and the A operand read at that index (the order of a sum's terms is free).  The substitution step
//     Y_i = inv(L_ii) (D_i - sum_j L_ij Y_j) is two chained products with the difference formed in registers.
//   * a tile is addressed by two strides (sa along the axis that is solved, sb along the free one), so the solve from the right,
//     A V^T = Y, is the same routine as the solve from the left on the transposed view: no transposition goes through LDS.
// The free axis is cut over the four waves, a wave owns its blocks through every step of a solve.
//
// The k-sums of the backwards: a workgroup walks a contiguous share of a row's particles in ascending k and adds each particle's
// tiles to its own partial in the workspace (one owner per element, plain loads and stores, no atomics); a finish launch adds the
// shares in share order, adds the diagonal terms and writes the zeros above the diagonal.
#include "zs_common.h"
#include "zs_matvar_math.h"
#include "../../include/zs_hip.h"
#include "../../include/zs_matvar.h"

#pragma clang fp contract(off)

using namespace zs;

namespace {

constexpr int THREADS = ZS_MATVAR_THREADS;

// what a kernel knows about its event and its place
template <typename T>
struct Geo {
  int n, p, nbn, nbp, ld;          // the event, its blocks, the leading dimension of a tile
  int m, q, wave;                  // the lane's place in the matrix instruction, its wave
  T *s0, *s1, *inv, *red;          // two tiles, the inverses of the diagonal blocks (U's, then V's), four reduction slots
};

template <typename T>
__device__ __forceinline__ Geo<T> geo_of(int n, int p) {
  Geo<T> g;
  g.n = n, g.p = p, g.nbn = blocks16(n), g.nbp = blocks16(p), g.ld = matvar_ld(p);
  g.m = mfma_m(threadIdx.x), g.q = mfma_q(threadIdx.x), g.wave = mfma_wave(threadIdx.x);
  g.s0 = tile_lds<T>();
  g.s1 = g.s0 + 16 * g.nbn * g.ld;
  g.inv = g.s1 + 16 * g.nbn * g.ld;
  g.red = g.inv + 256 * (g.nbn + g.nbp);
  return g;
}

// L[row][col] of a dim x dim lower-triangular factor; zero, and no read, outside the matrix and above the diagonal
template <typename T>
__device__ __forceinline__ T fac(const T* __restrict__ L, int dim, int row, int col) {
  return (row < dim && col <= row) ? L[row * dim + col] : (T)0;
}

// ---------------------------------------------------------------- staging
// tile <- src[n, p] - sub[n, p] (sub may be NULL), zeros in the ragged edge; the caller synchronises
template <typename T>
__device__ __forceinline__ void stage(const Geo<T>& g, T* tile, const T* __restrict__ src, const T* __restrict__ sub) {
  const int p16 = 16 * g.nbp, total = 16 * g.nbn * p16;
  for (int i = threadIdx.x; i < total; i += THREADS) {
    const int row = i / p16, col = i % p16;
    T v = (T)0;
    if (row < g.n && col < g.p) {
      v = src[row * g.p + col];
      if (sub) v -= sub[row * g.p + col];
    }
    tile[row * g.ld + col] = v;
  }
}
// tile <- elements [base, base + n p) of the launch's normal stream, as zs_philox_normal_f32 numbers them; zeros in the ragged edge
template <typename T>
__device__ __forceinline__ void stage_noise(const Geo<T>& g, T* tile, int64_t base, const PhiloxCall& pc) {
  const int p16 = 16 * g.nbp, total = 16 * g.nbn * p16;
  for (int i = threadIdx.x; i < total; i += THREADS) {
    const int row = i / p16, col = i % p16;
    if (row >= g.n || col >= g.p) tile[row * g.ld + col] = (T)0;
  }
  const int64_t np = (int64_t)g.n * g.p, g0 = base >> 2, g1 = (base + np - 1) >> 2;
  for (int64_t grp = g0 + threadIdx.x; grp <= g1; grp += THREADS) {
    const float4 v = philox_normal4((uint64_t)grp, pc);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int64_t e = 4 * grp + c - base;
      if (e >= 0 && e < np) {
        const int row = (int)(e / g.p), col = (int)(e % g.p);
        tile[row * g.ld + col] = (T)f4_get(v, c);
      }
    }
  }
}
template <typename T>
__device__ __forceinline__ void copy_tile(const Geo<T>& g, T* dst, const T* src) {
  const int p16 = 16 * g.nbp, total = 16 * g.nbn * p16;
  for (int i = threadIdx.x; i < total; i += THREADS) {
    const int at = (i / p16) * g.ld + i % p16;
    dst[at] = src[at];
  }
}
// the sum of squares of a tile, in every thread (a fixed order: the thread's elements in turn, the lanes of a wave by butterfly,
// the four waves pairwise)
template <typename T>
__device__ __forceinline__ T sum_squares(const Geo<T>& g, const T* tile) {
  const int p16 = 16 * g.nbp, total = 16 * g.nbn * p16;
  T s = (T)0;
  for (int i = threadIdx.x; i < total; i += THREADS) {
    const T v = tile[(i / p16) * g.ld + i % p16];
    s += v * v;
  }
  return block_sum_256(s, g.red);
}
// sum_i log L_ii of a dim x dim factor (dim <= 128 < THREADS), in every thread
template <typename T>
__device__ __forceinline__ T sum_log_diag(const Geo<T>& g, const T* __restrict__ L, int dim) {
  const int i = threadIdx.x;
  return block_sum_256(i < dim ? matvar_log(L[i * dim + i]) : (T)0, g.red);
}

// The inverses of the 16 x 16 diagonal blocks of U and V by scalar substitution, one column per thread (at most 8 + 8 blocks of 16
// columns = 256 threads); a block that runs past the matrix is continued by the identity.  inv[b][i][c] = (L_bb^-1)[i][c].
template <typename T>
__device__ __forceinline__ void invert_diagonal_blocks(const Geo<T>& g, const T* __restrict__ U, const T* __restrict__ V) {
  const int b = threadIdx.x >> 4, c = threadIdx.x & 15;
  if (b < g.nbn + g.nbp) {
    const bool isu = b < g.nbn;
    const T* __restrict__ L = isu ? U : V;
    const int dim = isu ? g.n : g.p, r0 = 16 * (isu ? b : b - g.nbn);
    T* x = g.inv + 256 * b;
    for (int i = 0; i < 16; ++i) {
      const int row = r0 + i;
      T s = i == c ? (T)1 : (T)0;
      if (row < dim) {
        for (int j = 0; j < i; ++j) s -= L[row * dim + r0 + j] * x[j * 16 + c];
        s = s / L[row * dim + row];
      }
      x[i * 16 + c] = s;
    }
  }
}

// ---------------------------------------------------------------- blocked substitution
// Orders the LDS writes of a wave's lanes before the LDS reads of its other lanes (a fence at wavefront scope; the wave's LDS
// operations are issued in order, so no workgroup barrier is needed where a wave only re-reads its own blocks).
__device__ __forceinline__ void wave_lds_order() {
#if ZS_ON_DEVICE
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#endif
}
// Solves L W = C (TRANS false, block rows ascending) or L^T W = C (TRANS true, descending) in place on a tile view: element
// (a, f) of the view is S[a sa + f sb], a along the solved axis (nba blocks, the factor's dimension), f along the free one
// (nbf blocks, cut over the waves).  `inv` holds the inverses of L's diagonal blocks.  A wave owns its free-axis blocks through
// every step, so the block rows are ordered inside the wave only; one workgroup barrier at the end.  Ends synchronised.
template <typename T, bool TRANS>
__device__ __forceinline__ void solve(const Geo<T>& g, T* S, int sa, int sb, int nba, int nbf, const T* __restrict__ L, int dim,
                                      const T* inv) {
  typedef typename Mfma<T>::Acc Acc;
  for (int step = 0; step < nba; ++step) {
    const int i = TRANS ? nba - 1 - step : step;
    for (int jb = g.wave; jb < nbf; jb += ZS_MATVAR_WAVES) {
      T* col = S + (16 * jb + g.m) * sb;
      Acc acc = {0, 0, 0, 0};
      for (int kb = TRANS ? i + 1 : 0; kb < (TRANS ? nba : i); ++kb) {
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          const int k = 16 * kb + 4 * s + g.q;
          const T a = TRANS ? fac(L, dim, k, 16 * i + g.m) : fac(L, dim, 16 * i + g.m, k);
          acc = Mfma<T>::run(a, col[k * sa], acc);
        }
      }
      Acc y = {0, 0, 0, 0};
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int k = MfmaTile<T>::acc_row(g.q, v);
        const T r = col[(16 * i + k) * sa] - acc[v];
        const T a = TRANS ? inv[256 * i + k * 16 + g.m] : inv[256 * i + g.m * 16 + k];
        y = Mfma<T>::run(a, r, y);
      }
#pragma unroll
      for (int v = 0; v < 4; ++v) col[(16 * i + MfmaTile<T>::acc_row(g.q, v)) * sa] = y[v];
    }
    wave_lds_order();          // the next block row reads what OTHER LANES OF THIS WAVE wrote: no other wave's blocks
  }
  __syncthreads();
}

// A = U^-1 (S0) V^-T in place: the two forward substitutions of M2
template <typename T>
__device__ __forceinline__ void whiten(const Geo<T>& g, const T* __restrict__ U, const T* __restrict__ V) {
  solve<T, false>(g, g.s0, g.ld, 1, g.nbn, g.nbp, U, g.n, g.inv);
  solve<T, false>(g, g.s0, 1, g.ld, g.nbp, g.nbn, V, g.p, g.inv + 256 * g.nbn);
}

// ---------------------------------------------------------------- products
// S1 <- U S1 (the tile holds E): block rows descending, so that a block row is overwritten after its last reader; a wave owns its
// block columns.  Ends synchronised.
template <typename T>
__device__ __forceinline__ void left_multiply(const Geo<T>& g, T* S, const T* __restrict__ U) {
  typedef typename Mfma<T>::Acc Acc;
  for (int jb = g.wave; jb < g.nbp; jb += ZS_MATVAR_WAVES) {
    T* col = S + 16 * jb + g.m;
    for (int ib = g.nbn - 1; ib >= 0; --ib) {
      Acc acc = {0, 0, 0, 0};
      for (int kb = 0; kb <= ib; ++kb) {
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          const int k = 16 * kb + 4 * s + g.q;
          acc = Mfma<T>::run(fac(U, g.n, 16 * ib + g.m, k), col[k * g.ld], acc);
        }
      }
#pragma unroll
      for (int v = 0; v < 4; ++v) col[(16 * ib + MfmaTile<T>::acc_row(g.q, v)) * g.ld] = acc[v];
    }
  }
  __syncthreads();
}
// S <- S V (V_NOT_VT) or, into memory, out = mean + S V^T (the draw).  A wave owns its block rows; S V runs block columns ascending
// in place (block column jb reads the block columns kb >= jb).  V^T's blocks are read as the B operand from V's rows.
template <typename T, bool DRAW>
__device__ __forceinline__ void right_multiply(const Geo<T>& g, T* S, const T* __restrict__ V, const T* __restrict__ mean, T* __restrict__ out) {
  typedef typename Mfma<T>::Acc Acc;
  for (int ib = g.wave; ib < g.nbn; ib += ZS_MATVAR_WAVES) {
    T* row = S + (16 * ib + g.m) * g.ld;
    for (int jb = 0; jb < g.nbp; ++jb) {
      Acc acc = {0, 0, 0, 0};
      for (int kb = DRAW ? 0 : jb; kb < (DRAW ? jb + 1 : g.nbp); ++kb) {
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          const int k = 16 * kb + 4 * s + g.q;
          const T b = DRAW ? fac(V, g.p, 16 * jb + g.m, k) : fac(V, g.p, k, 16 * jb + g.m);
          acc = Mfma<T>::run(row[k], b, acc);
        }
      }
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int r = 16 * ib + MfmaTile<T>::acc_row(g.q, v), c = 16 * jb + g.m;
        if (DRAW) {
          if (r < g.n && c < g.p) out[r * g.p + c] = mean[r * g.p + c] + acc[v];
        } else {
          S[r * g.ld + c] = acc[v];
        }
      }
    }
  }
  __syncthreads();
}

// part[a, b] (+)= w sum_c X(a, c) Y(b, c) for the block-lower-triangular tiles of a dim x dim output, X(a, c) = Sx[a sa + c sc]
// and Y likewise: w B A^T (sa = ld, sc = 1) and w C^T A (sa = 1, sc = ld).  The tiles are dealt to the waves in turn; every element
// has one owner, the same for every particle.
template <typename T>
__device__ __forceinline__ void gram_lower(const Geo<T>& g, const T* Sx, const T* Sy, int sa, int sc, int nbo, int nbc, int dim, T w,
                                           bool first, T* part) {
  typedef typename Mfma<T>::Acc Acc;
  int t = 0;
  for (int bi = 0; bi < nbo; ++bi) {
    for (int bj = 0; bj <= bi; ++bj, ++t) {
      if ((t & (ZS_MATVAR_WAVES - 1)) != g.wave) continue;
      const T* x = Sx + (16 * bi + g.m) * sa;
      const T* y = Sy + (16 * bj + g.m) * sa;
      Acc acc = {0, 0, 0, 0};
      for (int cb = 0; cb < nbc; ++cb) {
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          const int c = (16 * cb + 4 * s + g.q) * sc;
          acc = Mfma<T>::run(x[c], y[c], acc);
        }
      }
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int r = 16 * bi + MfmaTile<T>::acc_row(g.q, v), c = 16 * bj + g.m;
        if (r < dim && c < dim) {
          const T val = w * acc[v];
          part[r * dim + c] = first ? val : part[r * dim + c] + val;
        }
      }
    }
  }
}

// ---------------------------------------------------------------- M1
template <typename T>
__global__ __launch_bounds__(THREADS) void k_matvar_sample(const T* __restrict__ mean, const T* __restrict__ U, const T* __restrict__ V,
                                                           const T* __restrict__ eps, T* __restrict__ z, T* __restrict__ lp, int64_t R,
                                                           int n, int p, uint64_t seed, uint64_t call, const uint64_t* __restrict__ rs) {
  const Geo<T> g = geo_of<T>(n, p);
  if (rs) { seed = rs[0]; call += rs[1]; }
  const PhiloxCall pc = philox_call(call, seed);
  const int64_t it = blockIdx.x, r = it % R, np = (int64_t)n * p;
  U += r * n * n, V += r * p * p;
  if (eps) stage<T>(g, g.s1, eps + it * np, nullptr);
  else stage_noise<T>(g, g.s1, it * np, pc);
  __syncthreads();
  if (lp) {
    const T ss = sum_squares(g, g.s1);
    const T su = sum_log_diag(g, U, n), sv = sum_log_diag(g, V, p);
    if (threadIdx.x == 0) lp[it] = matvar_lp(n, p, su, sv, ss);
  }
  if (z) {
    left_multiply(g, g.s1, U);
    right_multiply<T, true>(g, g.s1, V, mean + r * np, z + it * np);
  }
}

// the backward of M1: gmean, gU and gV partials of a share of a row's particles
template <typename T>
__global__ __launch_bounds__(THREADS) void k_matvar_sample_bwd(const T* __restrict__ U, const T* __restrict__ V, const T* __restrict__ eps,
                                                               const T* __restrict__ gz, T* part, int want, int64_t K, int64_t R, int n,
                                                               int p, int64_t per, uint64_t seed, uint64_t call,
                                                               const uint64_t* __restrict__ rs) {
  const Geo<T> g = geo_of<T>(n, p);
  if (rs) { seed = rs[0]; call += rs[1]; }
  const PhiloxCall pc = philox_call(call, seed);
  const int64_t r = blockIdx.x % R, share = blockIdx.x / R, np = (int64_t)n * p;
  const int64_t k0 = share * per, k1 = k0 + per < K ? k0 + per : K;
  U += r * n * n, V += r * p * p;
  T* pm = part + (share * R + r) * matvar_part_stride(n, p);
  T* pu = pm + np;
  T* pv = pu + n * n;
  for (int64_t k = k0; k < k1; ++k) {
    const int64_t it = k * R + r;
    const bool first = k == k0;
    const T* gzk = gz + it * np;
    if (want & 1) {
      for (int i = threadIdx.x; i < (int)np; i += THREADS) pm[i] = first ? gzk[i] : pm[i] + gzk[i];
    }
    if (want & 6) {
      stage<T>(g, g.s0, gzk, nullptr);
      if (eps) stage<T>(g, g.s1, eps + it * np, nullptr);
      else stage_noise<T>(g, g.s1, it * np, pc);
      __syncthreads();
    }
    if (want & 2) {          // gU += (gZ V) E^T
      right_multiply<T, false>(g, g.s0, V, nullptr, nullptr);
      gram_lower<T>(g, g.s0, g.s1, g.ld, 1, g.nbn, g.nbp, n, (T)1, first, pu);
      __syncthreads();
      if (want & 4) {
        stage<T>(g, g.s0, gzk, nullptr);
        __syncthreads();
      }
    }
    if (want & 4) {          // gV += gZ^T (U E)
      left_multiply(g, g.s1, U);
      gram_lower<T>(g, g.s0, g.s1, 1, g.ld, g.nbp, g.nbn, p, (T)1, first, pv);
      __syncthreads();
    }
  }
}

// ---------------------------------------------------------------- M2
template <typename T>
__global__ __launch_bounds__(THREADS) void k_matvar_logprob(const T* __restrict__ mean, const T* __restrict__ U, const T* __restrict__ V,
                                                            const T* __restrict__ x, int shared_x, T* __restrict__ lp, int64_t R, int n,
                                                            int p) {
  const Geo<T> g = geo_of<T>(n, p);
  const int64_t it = blockIdx.x, r = it % R, np = (int64_t)n * p;
  U += r * n * n, V += r * p * p;
  invert_diagonal_blocks(g, U, V);
  stage<T>(g, g.s0, x + (shared_x ? r : it) * np, mean + r * np);
  __syncthreads();
  whiten(g, U, V);
  const T ss = sum_squares(g, g.s0);
  const T su = sum_log_diag(g, U, n), sv = sum_log_diag(g, V, p);
  if (threadIdx.x == 0) lp[it] = matvar_lp(n, p, su, sv, ss);
}

// the backward of M2: gx, and the gmean, gU and gV partials of a share of a row's particles
template <typename T>
__global__ __launch_bounds__(THREADS) void k_matvar_logprob_bwd(const T* __restrict__ mean, const T* __restrict__ U, const T* __restrict__ V,
                                                                const T* __restrict__ x, int shared_x, const T* __restrict__ glp,
                                                                T* __restrict__ gx, T* part, int want, int64_t K, int64_t R, int n, int p,
                                                                int64_t per) {
  const Geo<T> g = geo_of<T>(n, p);
  const int64_t r = blockIdx.x % R, share = blockIdx.x / R, np = (int64_t)n * p;
  const int64_t k0 = share * per, k1 = k0 + per < K ? k0 + per : K;
  U += r * n * n, V += r * p * p;
  T* pm = part ? part + (share * R + r) * matvar_part_stride(n, p) : nullptr;          // (NULL when only gx is asked for: want == 0)
  T* pu = part ? pm + np : nullptr;
  T* pv = part ? pu + n * n : nullptr;
  const T* invv = g.inv + 256 * g.nbn;
  const int p16 = 16 * g.nbp, total = 16 * g.nbn * p16;
  invert_diagonal_blocks(g, U, V);
  for (int64_t k = k0; k < k1; ++k) {
    const int64_t it = k * R + r;
    const bool first = k == k0;
    const T w = glp[it];
    stage<T>(g, g.s0, x + (shared_x ? r : it) * np, mean + r * np);
    __syncthreads();
    whiten(g, U, V);                                                       // S0 = A
    if ((want & 3) || gx) {
      copy_tile(g, g.s1, g.s0);
      __syncthreads();
      solve<T, true>(g, g.s1, g.ld, 1, g.nbn, g.nbp, U, n, g.inv);         // S1 = B = U^-T A
      if (want & 2) {
        gram_lower<T>(g, g.s1, g.s0, g.ld, 1, g.nbn, g.nbp, n, w, first, pu);          // gU += w B A^T
        __syncthreads();
      }
      if ((want & 1) || gx) {
        solve<T, true>(g, g.s1, 1, g.ld, g.nbp, g.nbn, V, p, invv);        // S1 = S = B V^-1
        for (int i = threadIdx.x; i < total; i += THREADS) {
          const int row = i / p16, col = i % p16;
          if (row < n && col < p) {
            const T ws = w * g.s1[row * g.ld + col];
            if (gx) gx[it * np + row * p + col] = -ws;
            if (want & 1) pm[row * p + col] = first ? ws : pm[row * p + col] + ws;
          }
        }
        __syncthreads();
      }
    }
    if (want & 4) {
      copy_tile(g, g.s1, g.s0);
      __syncthreads();
      solve<T, true>(g, g.s1, 1, g.ld, g.nbp, g.nbn, V, p, invv);          // S1 = C = A V^-1
      gram_lower<T>(g, g.s1, g.s0, 1, g.ld, g.nbp, g.nbn, p, w, first, pv);          // gV += w C^T A
      __syncthreads();
    }
  }
}

// ---------------------------------------------------------------- the finish of both backwards
// One thread per element of (gmean, gU, gV) of a row: the shares in share order; on the diagonals -p (sum_k glp) / U_ii and
// -n (sum_k glp) / V_jj, the k-sum in ascending k by the element's owner; zeros above the diagonals.
template <typename T>
__global__ __launch_bounds__(THREADS) void k_matvar_finish(const T* __restrict__ part, const T* __restrict__ U, const T* __restrict__ V,
                                                           const T* __restrict__ glp, T* __restrict__ gmean, T* __restrict__ gU,
                                                           T* __restrict__ gV, int64_t shares, int64_t K, int64_t R, int64_t n, int64_t p) {
  const int64_t stride = matvar_part_stride(n, p), i = (int64_t)blockIdx.x * THREADS + threadIdx.x;
  if (i >= R * stride) return;
  const int64_t r = i / stride, e = i % stride, np = n * p;
  T* out;
  int64_t dim, row, col, at;
  const T* L;
  T scale;
  if (e < np) {
    out = gmean, at = r * np + e, dim = 0, row = 1, col = 0, L = nullptr, scale = (T)0;
  } else if (e < np + n * n) {
    out = gU, dim = n, row = (e - np) / n, col = (e - np) % n, at = r * n * n + (e - np), L = U + r * n * n, scale = (T)p;
  } else {
    const int64_t f = e - np - n * n;
    out = gV, dim = p, row = f / p, col = f % p, at = r * p * p + f, L = V + r * p * p, scale = (T)n;
  }
  if (!out) return;
  T s = (T)0;
  if (col <= row) {
    for (int64_t sh = 0; sh < shares; ++sh) s += part[(sh * R + r) * stride + e];
    if (dim && row == col && glp) {
      T sg = (T)0;
      for (int64_t k = 0; k < K; ++k) sg += glp[k * R + r];
      s = s - scale * sg / L[row * dim + row];
    }
  }
  out[at] = s;
}

// ---------------------------------------------------------------- the entry points
template <typename T>
int check_shape(bool pointers, int64_t K, int64_t R, int64_t n, int64_t p) {
  if (!pointers || n < 1 || p < 1 || K < 0 || R < 0) return ZS_EINVAL;
  if (n > MatvarCap<T>::MAX_DIM || p > MatvarCap<T>::MAX_DIM) return ZS_ENOTSUP;
  const int64_t grid_max = ((int64_t)1 << 31) - 1;
  if (K > 0 && R > 0 && K > grid_max / R) return ZS_ENOTSUP;                                   // a workgroup per event
  if (R > grid_max / matvar_part_stride(n, p) * ZS_MATVAR_THREADS) return ZS_ENOTSUP;          // the finish: a thread per element of a row's gradients
  return 0;
}
// 1: the value has the particle axis, 0: it is shared by the particles, -1: neither
int period_kind(int64_t P, int64_t K, int64_t R, int64_t n, int64_t p) {
  if (P == K * R * n * p) return 1;
  if (P == R * n * p) return 0;
  return -1;
}
template <typename T>
size_t lds_bytes(int64_t n, int64_t p) { return sizeof(T) * (size_t)matvar_lds_elems((int)n, (int)p); }
// a launch may ask for more dynamic LDS than the default limit of a kernel: raise the kernel's limit to the device's, once per
// kernel (host-side bookkeeping of the runtime; nothing is enqueued).  A failure here shows as the launch's own error.
template <typename F>
hipError_t raise_lds_limit(F kernel) {
  return hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, ZS_MATVAR_LDS_BYTES);
}
#define ZS_MATVAR_ALLOW_LDS(KERNEL)                            \
  do {                                                         \
    static const hipError_t once = raise_lds_limit(KERNEL);    \
    (void)once;                                                \
  } while (0)

template <typename T>
int launch_finish(const void* part, const void* U, const void* V, const void* glp, void* gmean, void* gU, void* gV, int64_t shares,
                  int64_t K, int64_t R, int64_t n, int64_t p, void* stream) {
  const int64_t total = R * matvar_part_stride(n, p);
  hipLaunchKernelGGL((k_matvar_finish<T>), dim3((unsigned)((total + THREADS - 1) / THREADS)), dim3(THREADS), 0, (hipStream_t)stream,
                     (const T*)part, (const T*)U, (const T*)V, (const T*)glp, (T*)gmean, (T*)gU, (T*)gV, shares, K, R, n, p);
  ZS_CHECK_LAUNCH();
  return 0;
}

template <typename T>
int matvar_sample(const void* mean, const void* U, const void* V, const void* eps, void* z, void* lp, int64_t K, int64_t R, int64_t n,
                  int64_t p, uint64_t seed, uint64_t call, const uint64_t* rs, void* stream) {
  const int rc = check_shape<T>(mean && U && V, K, R, n, p);
  if (rc) return rc;
  if (K == 0 || R == 0) return 0;
  if (!z && !lp) return ZS_EINVAL;
  ZS_MATVAR_ALLOW_LDS(k_matvar_sample<T>);
  hipLaunchKernelGGL((k_matvar_sample<T>), dim3((unsigned)(K * R)), dim3(THREADS), lds_bytes<T>(n, p), (hipStream_t)stream, (const T*)mean,
                     (const T*)U, (const T*)V, (const T*)eps, (T*)z, (T*)lp, R, (int)n, (int)p, seed, call, rs);
  ZS_CHECK_LAUNCH();
  return 0;
}

template <typename T>
int matvar_sample_bwd(const void* U, const void* V, const void* eps, const void* gz, const void* glp, void* part, void* gmean, void* gU,
                      void* gV, int64_t K, int64_t R, int64_t n, int64_t p, uint64_t seed, uint64_t call, const uint64_t* rs,
                      void* stream) {
  const int rc = check_shape<T>(U && V, K, R, n, p);
  if (rc) return rc;
  if (K == 0 || R == 0) return 0;
  if ((!gmean && !gU && !gV) || (!gz && !glp) || (gz && !part)) return ZS_EINVAL;
  int64_t shares = 0;
  if (gz) {          // (without gz the sums over the shares are empty: the finish alone writes the diagonal terms)
    shares = matvar_shares(K, R);
    const int want = (gmean ? 1 : 0) | (gU ? 2 : 0) | (gV ? 4 : 0);
    ZS_MATVAR_ALLOW_LDS(k_matvar_sample_bwd<T>);
    hipLaunchKernelGGL((k_matvar_sample_bwd<T>), dim3((unsigned)(shares * R)), dim3(THREADS), lds_bytes<T>(n, p), (hipStream_t)stream,
                       (const T*)U, (const T*)V, (const T*)eps, (const T*)gz, (T*)part, want, K, R, (int)n, (int)p,
                       matvar_share_len(K, shares), seed, call, rs);
    ZS_CHECK_LAUNCH();
  }
  return launch_finish<T>(part, U, V, glp, gmean, gU, gV, shares, K, R, n, p, stream);
}

template <typename T>
int matvar_logprob(const void* mean, const void* U, const void* V, const void* x, int64_t Px, void* lp, int64_t K, int64_t R, int64_t n,
                   int64_t p, void* stream) {
  const int rc = check_shape<T>(mean && U && V, K, R, n, p);
  if (rc) return rc;
  if (K == 0 || R == 0) return 0;
  const int kind = period_kind(Px, K, R, n, p);
  if (!x || !lp || kind < 0) return ZS_EINVAL;
  ZS_MATVAR_ALLOW_LDS(k_matvar_logprob<T>);
  hipLaunchKernelGGL((k_matvar_logprob<T>), dim3((unsigned)(K * R)), dim3(THREADS), lds_bytes<T>(n, p), (hipStream_t)stream, (const T*)mean,
                     (const T*)U, (const T*)V, (const T*)x, kind == 0 ? 1 : 0, (T*)lp, R, (int)n, (int)p);
  ZS_CHECK_LAUNCH();
  return 0;
}

template <typename T>
int matvar_logprob_bwd(const void* mean, const void* U, const void* V, const void* x, int64_t Px, const void* glp, void* part, void* gx,
                       void* gmean, void* gU, void* gV, int64_t K, int64_t R, int64_t n, int64_t p, void* stream) {
  const int rc = check_shape<T>(mean && U && V, K, R, n, p);
  if (rc) return rc;
  if (K == 0 || R == 0) return 0;
  const int kind = period_kind(Px, K, R, n, p);
  const bool sums = gmean || gU || gV;
  if (!x || !glp || kind < 0 || (!gx && !sums) || (sums && !part)) return ZS_EINVAL;
  const int64_t shares = matvar_shares(K, R);
  const int want = (gmean ? 1 : 0) | (gU ? 2 : 0) | (gV ? 4 : 0);
  ZS_MATVAR_ALLOW_LDS(k_matvar_logprob_bwd<T>);
  hipLaunchKernelGGL((k_matvar_logprob_bwd<T>), dim3((unsigned)(shares * R)), dim3(THREADS), lds_bytes<T>(n, p), (hipStream_t)stream,
                     (const T*)mean, (const T*)U, (const T*)V, (const T*)x, kind == 0 ? 1 : 0, (const T*)glp, (T*)gx, (T*)part, want, K, R,
                     (int)n, (int)p, matvar_share_len(K, shares));
  ZS_CHECK_LAUNCH();
  if (!sums) return 0;
  return launch_finish<T>(part, U, V, glp, gmean, gU, gV, shares, K, R, n, p, stream);
}

}  // namespace

extern "C" int zs_matvar_abi_version(void) { return ZS_MATVAR_ABI_VERSION; }
extern "C" int zs_matvar_max_dim(int elem_bytes) { return matvar_max_dim(elem_bytes); }
extern "C" int64_t zs_matvar_shares(int64_t K, int64_t R) { return matvar_shares(K, R); }
extern "C" int64_t zs_matvar_workspace_elems(int which, int elem_bytes, int64_t K, int64_t R, int64_t n, int64_t p) {
  const int cap = matvar_max_dim(elem_bytes);
  if (cap == 0 || K < 0 || R < 0 || n < 1 || p < 1 || n > cap || p > cap) return -1;
  if (which != ZS_MATVAR_WS_SAMPLE_BWD && which != ZS_MATVAR_WS_LOGPROB_BWD) return -1;
  return matvar_part_elems(K, R, n, p);
}

#define ZS_MATVAR_ENTRY(SFX, T)                                                                                                       \
  extern "C" int zs_matvar_sample_logprob##SFX(const void* mean, const void* u_tril, const void* v_tril, const void* eps, void* z,    \
                                               void* lp, int64_t K, int64_t R, int64_t n, int64_t p, uint64_t seed, uint64_t call,   \
                                               const uint64_t* rng_state, void* stream) {                                            \
    return matvar_sample<T>(mean, u_tril, v_tril, eps, z, lp, K, R, n, p, seed, call, rng_state, stream);                             \
  }                                                                                                                                   \
  extern "C" int zs_matvar_sample_logprob_bwd##SFX(const void* u_tril, const void* v_tril, const void* eps, const void* gz,           \
                                                   const void* glp, void* part, void* gmean, void* gu, void* gv, int64_t K,          \
                                                   int64_t R, int64_t n, int64_t p, uint64_t seed, uint64_t call,                    \
                                                   const uint64_t* rng_state, void* stream) {                                        \
    return matvar_sample_bwd<T>(u_tril, v_tril, eps, gz, glp, part, gmean, gu, gv, K, R, n, p, seed, call, rng_state, stream);        \
  }                                                                                                                                   \
  extern "C" int zs_matvar_logprob##SFX(const void* mean, const void* u_tril, const void* v_tril, const void* x, int64_t Px,          \
                                        void* lp, int64_t K, int64_t R, int64_t n, int64_t p, void* stream) {                         \
    return matvar_logprob<T>(mean, u_tril, v_tril, x, Px, lp, K, R, n, p, stream);                                                    \
  }                                                                                                                                   \
  extern "C" int zs_matvar_logprob_bwd##SFX(const void* mean, const void* u_tril, const void* v_tril, const void* x, int64_t Px,      \
                                            const void* glp, void* part, void* gx, void* gmean, void* gu, void* gv, int64_t K,       \
                                            int64_t R, int64_t n, int64_t p, void* stream) {                                         \
    return matvar_logprob_bwd<T>(mean, u_tril, v_tril, x, Px, glp, part, gx, gmean, gu, gv, K, R, n, p, stream);                      \
  }

ZS_MATVAR_ENTRY(_f32, float)
ZS_MATVAR_ENTRY(_f64, double)
