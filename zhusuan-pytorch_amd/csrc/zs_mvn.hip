// V1, V2 and their backwards: MultivariateNormalCholesky (include/zs_mvn.h; its own library, ../lib/libzs_mvn.so, `make mvn`).
//
// A torch composition of the node costs about a dozen launches each way (noise, batched matmul, add, solve_triangular, square,
// sum, diagonal, log, sum ...); here it is one launch each way.  A group of G = next_pow2(D) lanes owns a row of the batch, lane
// i its component i (zs_mvn_math.h); a workgroup is one wave of 64 / G rows.  L of those rows is copied once into LDS (lower
// triangle only, odd row stride) and reused by all the particles the workgroup walks; vectors stay in registers, one element per
// lane, and are exchanged by shuffles inside the group: the matvec and the column-oriented substitutions broadcast one solved
// component per step, the row sums are butterflies.  No atomics, no scratch: the only per-lane array -- row i of the gtril
// accumulator -- is indexed by a loop unrolled over the template parameter G.  Every access is one element wide, so the bits do
// not depend on the alignment of the operands.
#include "zs_common.h"
#include "zs_mvn_math.h"
#include "../../include/zs_hip.h"
#include "../../include/zs_mvn.h"

#pragma clang fp contract(off)

using namespace zs;

namespace {

constexpr int THREADS = ZS_MVN_THREADS;

// the lower triangle of L[r] into the group's tile (the upper triangle is never read, neither here nor from the tile)
template <typename T, int G>
__device__ __forceinline__ void tile_load(T* tile, const T* __restrict__ Lr, const GroupPlace& pl, int D) {
  for (MvnWalk w = mvn_walk_first(pl.lane, D); w.i < D; mvn_walk_next(w, G, D))
    if (w.j <= w.i) tile[mvn_tile_index(pl.grp, w.i, w.j, G)] = Lr[w.i * D + w.j];
}
// the group's tile out to a D x D matrix, zeros above the diagonal
template <typename T, int G>
__device__ __forceinline__ void tile_store(const T* tile, T* __restrict__ out, const GroupPlace& pl, int D) {
  for (MvnWalk w = mvn_walk_first(pl.lane, D); w.i < D; mvn_walk_next(w, G, D))
    out[w.i * D + w.j] = w.j <= w.i ? tile[mvn_tile_index(pl.grp, w.i, w.j, G)] : (T)0;
}

// element `flat` of the launch's normal stream, as zs_philox_normal_f32 numbers them
template <typename T>
__device__ __forceinline__ T normal_at(int64_t flat, const PhiloxCall& pc) {
  return (T)f4_get(philox_normal4((uint64_t)flat >> 2, pc), (int)(flat & 3));
}

// y = L^-1 b over the group: lane i enters with b_i and leaves with y_i (zs_mvn_math.h: mvn_forward_row)
template <typename T, int G>
__device__ __forceinline__ T forward_subst(const T* tile, const GroupPlace& pl, int D, T b, T rdiag) {
  for (int j = 0; j < D; ++j) {
    const T t = __shfl(mvn_solved(b, rdiag), pl.first + j, ZS_WAVE);
    if (pl.lane > j && pl.lane < D) b = mvn_subst_step(b, tile[mvn_tile_index(pl.grp, pl.lane, j, G)], t);
  }
  return mvn_solved(b, rdiag);
}
// w = L^-T c over the group (mvn_backward_row)
template <typename T, int G>
__device__ __forceinline__ T backward_subst(const T* tile, const GroupPlace& pl, int D, T c, T rdiag) {
  for (int j = D - 1; j >= 0; --j) {
    const T t = __shfl(mvn_solved(c, rdiag), pl.first + j, ZS_WAVE);
    if (pl.lane < j) c = mvn_subst_step(c, tile[mvn_tile_index(pl.grp, j, pl.lane, G)], t);
  }
  return mvn_solved(c, rdiag);
}

// ---------------------------------------------------------------- V1 and V2
// SAMPLE: z = mean + L eps and the density of that draw (y = eps, no solve).  Otherwise: the density of a given x (y = L^-1 (x - mean)).
// blockIdx.y cuts the particles into contiguous shares of `kshare` (no sum runs over k here, so the cut changes no bit).
template <typename T, int G, bool SAMPLE>
__global__ __launch_bounds__(THREADS) void k_mvn_forward(const T* __restrict__ mean, const T* __restrict__ tril,
                                                         const T* __restrict__ in, int64_t prow, T* __restrict__ z, T* __restrict__ lp,
                                                         int64_t K, int64_t R, int D, int64_t kshare, T c0, uint64_t seed,
                                                         uint64_t call, const uint64_t* __restrict__ rs) {
  __shared__ T tile[THREADS * (G + 1)];
  if (rs) { seed = rs[0]; call += rs[1]; }
  const PhiloxCall pc = philox_call(call, seed);
  const GroupPlace pl = group_place((int)threadIdx.x, THREADS, G);
  const int64_t k0 = (int64_t)blockIdx.y * kshare, k1 = k0 + kshare < K ? k0 + kshare : K;
  for (int64_t rb = group_row_first((int)blockIdx.x, pl); rb < R; rb += group_row_step((int)gridDim.x, pl)) {
    const int64_t r = rb + pl.grp;
    const bool valid = r < R, act = valid && pl.lane < D;
    __syncthreads();
    if (valid) tile_load<T, G>(tile, tril + r * D * D, pl, D);
    __syncthreads();
    const T m = act ? mean[r * D + pl.lane] : (T)0;
    const T diag = act ? tile[mvn_tile_index(pl.grp, pl.lane, pl.lane, G)] : (T)1;
    const T rdiag = mvn_rdiag(diag);
    const T slog = group_sum(act ? mvn_log(diag) : (T)0, G);
    for (int64_t k = k0; k < k1; ++k) {
      const int64_t it = k * R + r;
      T y;
      if (SAMPLE) {
        y = (T)0;
        if (act) y = in ? in[it * D + pl.lane] : normal_at<T>(it * D + pl.lane, pc);
        T acc = m;
        for (int j = 0; j < D; ++j) {
          const T ej = __shfl(y, pl.first + j, ZS_WAVE);
          if (act && j <= pl.lane) acc = mvn_matvec_step(acc, tile[mvn_tile_index(pl.grp, pl.lane, j, G)], ej);
        }
        if (act && z) z[it * D + pl.lane] = acc;
      } else {
        const int64_t xr = prow == R ? r : it;
        const T b = act ? in[xr * D + pl.lane] - m : (T)0;
        y = forward_subst<T, G>(tile, pl, D, b, rdiag);
      }
      if (lp) {
        const T ss = group_sum(act ? y * y : (T)0, G);
        if (valid && pl.lane == 0) lp[it] = mvn_lp(c0, slog, ss);
      }
    }
  }
}

// ---------------------------------------------------------------- the backwards
// One group per ROW, its particles in ascending k; lane i keeps gmean_i and row i of gtril in registers.
//   MODE 0  reparameterised draw: gmean = sum_k gz, gtril_ij = sum_k gz_i eps_j - delta_ij (sum_k glp) / L_ii
//   MODE 1  detached draw, the density's direct dependence: y = eps, w = L^-T y, gmean = sum_k glp w, gtril_ij = sum_k glp (w_i y_j - delta_ij / L_ii)
//   MODE 2  density of a given x: y = L^-1 (x - mean), then as MODE 1, and gx = -glp w
template <typename T, int G, int MODE>
__global__ __launch_bounds__(THREADS) void k_mvn_backward(const T* __restrict__ mean, const T* __restrict__ tril,
                                                          const T* __restrict__ in, int64_t prow, const T* __restrict__ gz,
                                                          const T* __restrict__ glp, T* __restrict__ gx, T* __restrict__ gmean,
                                                          T* __restrict__ gtril, int64_t K, int64_t R, int D, uint64_t seed,
                                                          uint64_t call, const uint64_t* __restrict__ rs) {
  __shared__ T tile[THREADS * (G + 1)];
  if (rs) { seed = rs[0]; call += rs[1]; }
  const PhiloxCall pc = philox_call(call, seed);
  const GroupPlace pl = group_place((int)threadIdx.x, THREADS, G);
  for (int64_t rb = group_row_first((int)blockIdx.x, pl); rb < R; rb += group_row_step((int)gridDim.x, pl)) {
    const int64_t r = rb + pl.grp;
    const bool valid = r < R, act = valid && pl.lane < D;
    const T* Lr = tril + r * D * D;
    __syncthreads();
    if (MODE != 0 && valid) tile_load<T, G>(tile, Lr, pl, D);
    __syncthreads();
    const T m = (MODE == 2 && act) ? mean[r * D + pl.lane] : (T)0;
    const T rdiag = mvn_rdiag(act ? Lr[pl.lane * D + pl.lane] : (T)1);
    T gm = (T)0, sg = (T)0, acc[G];
#pragma unroll
    for (int j = 0; j < G; ++j) acc[j] = (T)0;
    for (int64_t k = 0; k < K; ++k) {
      const int64_t it = k * R + r;
      const T g = (glp && valid) ? glp[it] : (T)0;
      T y = (T)0, w;
      if (MODE == 2) {
        const int64_t xr = prow == R ? r : it;
        y = forward_subst<T, G>(tile, pl, D, act ? in[xr * D + pl.lane] - m : (T)0, rdiag);
      } else if (act) {
        y = in ? in[it * D + pl.lane] : normal_at<T>(it * D + pl.lane, pc);
      }
      if (MODE == 0) {
        w = (gz && act) ? gz[it * D + pl.lane] : (T)0;
        gm += w;
        sg += g;
#pragma unroll
        for (int j = 0; j < G; ++j)
          if (j < D) acc[j] = flat_fma(w, __shfl(y, pl.first + j, ZS_WAVE), acc[j]);
      } else {
        w = backward_subst<T, G>(tile, pl, D, y, rdiag);
        gm = flat_fma(g, w, gm);
        if (MODE == 2 && gx && act) gx[it * D + pl.lane] = -g * w;
#pragma unroll
        for (int j = 0; j < G; ++j)
          if (j < D) acc[j] = mvn_gtril_step(acc[j], g, w, __shfl(y, pl.first + j, ZS_WAVE), j == pl.lane, rdiag);
      }
    }
    if (gmean && act) gmean[r * D + pl.lane] = gm;
    if (gtril) {
      __syncthreads();          // the substitutions have finished with the tile
#pragma unroll
      for (int j = 0; j < G; ++j)
        if (act && j <= pl.lane) tile[mvn_tile_index(pl.grp, pl.lane, j, G)] = (MODE == 0 && j == pl.lane) ? flat_fma(-sg, rdiag, acc[j]) : acc[j];
      __syncthreads();
      if (valid) tile_store<T, G>(tile, gtril + r * D * D, pl, D);
    }
  }
}

// ---------------------------------------------------------------- host side
int check_shape(const void* mean, const void* tril, int64_t K, int64_t R, int64_t D) {
  if (!mean || !tril || D < 1 || K < 0 || R < 0) return ZS_EINVAL;
  if (D > ZS_MVN_MAX_DIM) return ZS_ENOTSUP;
  return 0;
}
// rows of a value with period P elements: K R or R, else -1
int64_t period_rows(int64_t P, int64_t D, int64_t K, int64_t R) {
  if (P == K * R * D) return K * R;
  if (P == R * D) return R;
  return -1;
}
unsigned row_blocks(int64_t R, int G) { return grid_for(R, THREADS / G, 256u * 16u); }
double lp_c0(int64_t D) { return -0.5 * (double)D * 1.8378770664093454835606594728112; }

#define ZS_MVN_BY_G(G_, CALL)                     \
  switch (G_) {                                   \
    case 1: { constexpr int GG = 1; CALL; } break;   \
    case 2: { constexpr int GG = 2; CALL; } break;   \
    case 4: { constexpr int GG = 4; CALL; } break;   \
    case 8: { constexpr int GG = 8; CALL; } break;   \
    case 16: { constexpr int GG = 16; CALL; } break; \
    case 32: { constexpr int GG = 32; CALL; } break; \
    default: { constexpr int GG = 64; CALL; } break; \
  }

template <typename T, bool SAMPLE>
int forward(const void* mean, const void* tril, const void* in, int64_t prow, void* z, void* lp, int64_t K, int64_t R, int64_t D,
            uint64_t seed, uint64_t call, const uint64_t* rs, void* stream) {
  const int G = group_lanes(D);
  const unsigned gx = row_blocks(R, G);
  // enough workgroups to fill the chip when the rows alone do not: the particles are cut into contiguous shares
  int64_t shares = (2048 + gx - 1) / gx;
  if (shares > K) shares = K;
  if (shares > 65535) shares = 65535;
  const int64_t kshare = (K + shares - 1) / shares;
  const unsigned gy = (unsigned)((K + kshare - 1) / kshare);
  ZS_MVN_BY_G(G, hipLaunchKernelGGL((k_mvn_forward<T, GG, SAMPLE>), dim3(gx, gy), dim3(THREADS), 0, (hipStream_t)stream,
                                    (const T*)mean, (const T*)tril, (const T*)in, prow, (T*)z, (T*)lp, K, R, (int)D, kshare,
                                    (T)lp_c0(D), seed, call, rs));
  ZS_CHECK_LAUNCH();
  return 0;
}

template <typename T, int MODE>
int backward(const void* mean, const void* tril, const void* in, int64_t prow, const void* gz, const void* glp, void* gx, void* gmean,
             void* gtril, int64_t K, int64_t R, int64_t D, uint64_t seed, uint64_t call, const uint64_t* rs, void* stream) {
  const int G = group_lanes(D);
  ZS_MVN_BY_G(G, hipLaunchKernelGGL((k_mvn_backward<T, GG, MODE>), dim3(row_blocks(R, G)), dim3(THREADS), 0, (hipStream_t)stream,
                                    (const T*)mean, (const T*)tril, (const T*)in, prow, (const T*)gz, (const T*)glp, (T*)gx,
                                    (T*)gmean, (T*)gtril, K, R, (int)D, seed, call, rs));
  ZS_CHECK_LAUNCH();
  return 0;
}

template <typename T>
int mvn_sample(const void* mean, const void* tril, const void* eps, void* z, void* lp, int64_t K, int64_t R, int64_t D, uint64_t seed,
               uint64_t call, const uint64_t* rs, void* stream) {
  const int rc = check_shape(mean, tril, K, R, D);
  if (rc) return rc;
  if (K == 0 || R == 0) return 0;
  if (!z && !lp) return ZS_EINVAL;
  return forward<T, true>(mean, tril, eps, K * R, z, lp, K, R, D, seed, call, rs, stream);
}

template <typename T>
int mvn_sample_bwd(const void* tril, const void* eps, const void* gz, const void* glp, int reparameterized, void* gmean, void* gtril,
                   int64_t K, int64_t R, int64_t D, uint64_t seed, uint64_t call, const uint64_t* rs, void* stream) {
  const int rc = check_shape(tril, tril, K, R, D);
  if (rc) return rc;
  if (K == 0 || R == 0) return 0;
  if ((!gmean && !gtril) || (!gz && !glp) || (!reparameterized && !glp)) return ZS_EINVAL;
  if (reparameterized)
    return backward<T, 0>(nullptr, tril, eps, K * R, gz, glp, nullptr, gmean, gtril, K, R, D, seed, call, rs, stream);
  return backward<T, 1>(nullptr, tril, eps, K * R, nullptr, glp, nullptr, gmean, gtril, K, R, D, seed, call, rs, stream);
}

template <typename T>
int mvn_logprob(const void* mean, const void* tril, const void* x, int64_t Px, void* lp, int64_t K, int64_t R, int64_t D, void* stream) {
  const int rc = check_shape(mean, tril, K, R, D);
  if (rc) return rc;
  if (K == 0 || R == 0) return 0;
  if (!x || !lp) return ZS_EINVAL;
  const int64_t prow = period_rows(Px, D, K, R);
  if (prow < 0) return ZS_EINVAL;
  return forward<T, false>(mean, tril, x, prow, nullptr, lp, K, R, D, 0, 0, nullptr, stream);
}

template <typename T>
int mvn_logprob_bwd(const void* mean, const void* tril, const void* x, int64_t Px, const void* glp, void* gx, void* gmean, void* gtril,
                    int64_t K, int64_t R, int64_t D, void* stream) {
  const int rc = check_shape(mean, tril, K, R, D);
  if (rc) return rc;
  if (K == 0 || R == 0) return 0;
  if (!x || !glp || (!gx && !gmean && !gtril)) return ZS_EINVAL;
  const int64_t prow = period_rows(Px, D, K, R);
  if (prow < 0) return ZS_EINVAL;
  return backward<T, 2>(mean, tril, x, prow, nullptr, glp, gx, gmean, gtril, K, R, D, 0, 0, nullptr, stream);
}

}  // namespace

extern "C" int zs_mvn_abi_version(void) { return ZS_MVN_ABI_VERSION; }
extern "C" int zs_mvn_max_dim(void) { return ZS_MVN_MAX_DIM; }
extern "C" int zs_mvn_group_lanes(int64_t D) { return (D < 1 || D > ZS_MVN_MAX_DIM) ? 0 : group_lanes(D); }

#define ZS_MVN_ENTRY(SFX, T)                                                                                                        \
  extern "C" int zs_mvn_sample_logprob##SFX(const void* mean, const void* tril, const void* eps, void* z, void* lp, int64_t K,      \
                                            int64_t R, int64_t D, uint64_t seed, uint64_t call, const uint64_t* rng_state,         \
                                            void* stream) {                                                                         \
    return mvn_sample<T>(mean, tril, eps, z, lp, K, R, D, seed, call, rng_state, stream);                                           \
  }                                                                                                                                 \
  extern "C" int zs_mvn_sample_logprob_bwd##SFX(const void* tril, const void* eps, const void* gz, const void* glp,                 \
                                                int reparameterized, void* gmean, void* gtril, int64_t K, int64_t R, int64_t D,    \
                                                uint64_t seed, uint64_t call, const uint64_t* rng_state, void* stream) {            \
    return mvn_sample_bwd<T>(tril, eps, gz, glp, reparameterized, gmean, gtril, K, R, D, seed, call, rng_state, stream);            \
  }                                                                                                                                 \
  extern "C" int zs_mvn_logprob##SFX(const void* mean, const void* tril, const void* x, int64_t Px, void* lp, int64_t K, int64_t R, \
                                     int64_t D, void* stream) {                                                                     \
    return mvn_logprob<T>(mean, tril, x, Px, lp, K, R, D, stream);                                                                  \
  }                                                                                                                                 \
  extern "C" int zs_mvn_logprob_bwd##SFX(const void* mean, const void* tril, const void* x, int64_t Px, const void* glp, void* gx,  \
                                         void* gmean, void* gtril, int64_t K, int64_t R, int64_t D, void* stream) {                 \
    return mvn_logprob_bwd<T>(mean, tril, x, Px, glp, gx, gmean, gtril, K, R, D, stream);                                           \
  }

ZS_MVN_ENTRY(_f32, float)
ZS_MVN_ENTRY(_f64, double)
