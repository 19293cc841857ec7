// H1: Hamiltonian Monte Carlo with a Metropolis correction (include/zs_hmc.h; its own library, ../lib/libzs_hmc.so, `make hmc`).
//
// One HMC iteration of L leapfrog steps is L + 1 gradients of the log joint through the existing kernels; around them a torch
// restatement runs, per latent, a draw, a square-and-sum, several axpys and a where.  Here the latents of a chunk form ONE flat
// index space as in zs_mcmc.hip (pointer table by value, a thread owns four consecutive elements -- one Philox group -- and
// finds their tensor by bisection), and an iteration is L + 3 launches: BEGIN (draw, K0, half kick, drift), L - 1 STEP (kick,
// drift), END (half kick, K1), decide (per-chain accept, step-size update on the device) and select.
//
// Kinetic sums: a workgroup of 256 threads owns a tile of 1024 consecutive flat elements.  The squares go to LDS with a key per
// element -- the offset in the tile at which the element's (tensor, chain) row begins, -1 for a row that began in an earlier
// tile -- and ten rounds of a segmented inclusive scan (Hillis-Steele, double-buffered) leave, at the last element of every row
// inside the tile, that row's sum over the tile.  That element's thread stores it into the slot of (chain, tensor, tile) of the
// caller's workspace.  The tree's shape depends on the flat indices only: no atomics, the same bits on every run and on both
// access paths.  One chain over many workgroups gives one slot per tile; row = 1 gives 1024 rows per tile, one slot each.
// decide (one workgroup) adds a chain's slots in double.
#include "zs_common.h"
#include "zs_hmc_math.h"
#include "../../include/zs_hip.h"
#include "../../include/zs_hmc.h"

using namespace zs;

namespace {

constexpr int TILE = ZS_HMC_TILE;
constexpr int THREADS = TILE / 4;
constexpr int DECIDE_THREADS = 1024;
constexpr int DEAD_KEY = 1 << 30;

template <typename T>
struct Table {
  const T* q0[ZS_HMC_MAX_TENSORS];
  T* q[ZS_HMC_MAX_TENSORS];
  T* p[ZS_HMC_MAX_TENSORS];
  const T* grad[ZS_HMC_MAX_TENSORS];
  const T* z[ZS_HMC_MAX_TENSORS];
  T* p0[ZS_HMC_MAX_TENSORS];                 // (select: q_out)
  int64_t start[ZS_HMC_MAX_TENSORS + 1];     // start[n_tensors] = n
  int64_t row[ZS_HMC_MAX_TENSORS];
  int32_t poff[ZS_HMC_MAX_TENSORS + 1];      // first slot of tensor s within a chain's slots; poff[n_tensors] = slots
  uint32_t has_z, has_p0;
  int n_tensors;
};

template <typename T, int KIND, bool VEC>
__global__ __launch_bounds__(THREADS) void k_hmc_move(const Table<T> ts, int64_t n, int64_t tiles, const double* __restrict__ state,
                                                      T* __restrict__ ksum, uint64_t seed, uint64_t call,
                                                      const uint64_t* __restrict__ rs) {
  constexpr bool SUM = KIND != ZS_HMC_STEP;
  __shared__ T sv[2][SUM ? TILE : 1];
  __shared__ int skey[SUM ? TILE : 1];
  const HmcStep<T> st = hmc_step_of<T>(state[HMC_EPS]);
  if (KIND == ZS_HMC_BEGIN && rs) { seed = rs[0]; call += rs[1]; }
  const PhiloxCall pc = philox_call(call, seed);
  const int tid = threadIdx.x;
  const int64_t slots = ts.poff[ts.n_tensors];
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t gi = tile * THREADS + tid, i0 = gi << 2;
    T sq[4] = {(T)0, (T)0, (T)0, (T)0};
    int key[4] = {DEAD_KEY, DEAD_KEY, DEAD_KEY, DEAD_KEY};
    if (i0 < n) {
      if (VEC) {
        // every start and row is a multiple of 4 and every pointer aligned (checked on the host): one tensor, one chain
        const HmcLoc l = hmc_locate(ts.start, ts.row, ts.n_tensors, i0);
        const int s = l.s;
        Vec4<T> q, p, zz;
        const Vec4<T> g = *reinterpret_cast<const Vec4<T>*>(ts.grad[s] + l.off);
        if (KIND == ZS_HMC_BEGIN) {
          q = *reinterpret_cast<const Vec4<T>*>(ts.q0[s] + l.off);
          if ((ts.has_z >> s) & 1u) {
            zz = *reinterpret_cast<const Vec4<T>*>(ts.z[s] + l.off);
          } else {
            const float4 nrm = philox_normal4((uint64_t)gi, pc);
            zz.v[0] = (T)nrm.x; zz.v[1] = (T)nrm.y; zz.v[2] = (T)nrm.z; zz.v[3] = (T)nrm.w;
          }
        } else {
          p = *reinterpret_cast<const Vec4<T>*>(ts.p[s] + l.off);
          if (KIND == ZS_HMC_STEP) q = *reinterpret_cast<const Vec4<T>*>(ts.q[s] + l.off);
        }
        const int k = hmc_key(l.run_start, tile);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if (KIND == ZS_HMC_BEGIN) sq[j] = hmc_begin(q.v[j], g.v[j], zz.v[j], st, q.v[j], p.v[j]);
          else if (KIND == ZS_HMC_STEP) hmc_step(q.v[j], p.v[j], g.v[j], st);
          else sq[j] = hmc_end(p.v[j], g.v[j], st);
          key[j] = k;
        }
        if (KIND != ZS_HMC_END) {
          *reinterpret_cast<Vec4<T>*>(ts.q[s] + l.off) = q;
          *reinterpret_cast<Vec4<T>*>(ts.p[s] + l.off) = p;
        }
        if (KIND == ZS_HMC_BEGIN && ((ts.has_p0 >> s) & 1u)) *reinterpret_cast<Vec4<T>*>(ts.p0[s] + l.off) = zz;
      } else {
        // element form: each of the four elements finds its own tensor and chain; those past n are clamped onto the group's
        // first one, so the loads are unconditional and only the stores and the kinetic terms are not
        T q[4], p[4], g[4], zz[4];
        int sj[4];
        int64_t off[4];
        bool inj[4], all_inj = true;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int64_t i = flat_clamped_index(gi, j, n);
          const HmcLoc l = hmc_locate(ts.start, ts.row, ts.n_tensors, i);
          sj[j] = l.s;
          off[j] = l.off;
          if (flat_element_live(gi, j, n)) key[j] = hmc_key(l.run_start, tile);
          g[j] = ts.grad[l.s][l.off];
          inj[j] = (ts.has_z >> l.s) & 1u;
          all_inj = all_inj && inj[j];
          if (KIND == ZS_HMC_BEGIN) {
            q[j] = ts.q0[l.s][l.off];
            zz[j] = inj[j] ? ts.z[l.s][l.off] : (T)0;
          } else {
            p[j] = ts.p[l.s][l.off];
            q[j] = KIND == ZS_HMC_STEP ? ts.q[l.s][l.off] : (T)0;
          }
        }
        if (KIND == ZS_HMC_BEGIN && !all_inj) {
          const float4 nrm = philox_normal4((uint64_t)gi, pc);
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (!inj[j]) zz[j] = (T)f4_get(nrm, j);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          T t;
          if (KIND == ZS_HMC_BEGIN) t = hmc_begin(q[j], g[j], zz[j], st, q[j], p[j]);
          else if (KIND == ZS_HMC_STEP) { hmc_step(q[j], p[j], g[j], st); t = (T)0; }
          else t = hmc_end(p[j], g[j], st);
          if (flat_element_live(gi, j, n)) {
            sq[j] = t;
            if (KIND != ZS_HMC_END) {
              ts.q[sj[j]][off[j]] = q[j];
              ts.p[sj[j]][off[j]] = p[j];
            }
            if (KIND == ZS_HMC_BEGIN && ((ts.has_p0 >> sj[j]) & 1u)) ts.p0[sj[j]][off[j]] = zz[j];
          }
        }
      }
    }
    if (SUM) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        sv[0][4 * tid + j] = sq[j];
        skey[4 * tid + j] = key[j];
      }
      __syncthreads();
      int b = 0;
      for (int d = 1; d < TILE; d <<= 1) {
        T x[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int e = j * THREADS + tid;
          x[j] = sv[b][e];
          if (e >= d && skey[e - d] == skey[e]) x[j] += sv[b][e - d];
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) sv[b ^ 1][j * THREADS + tid] = x[j];
        b ^= 1;
        __syncthreads();
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int e = j * THREADS + tid;
        const int64_t i = tile * TILE + e;
        if (i < n && (e == TILE - 1 || i + 1 >= n || skey[e + 1] != skey[e])) {
          // the last element of its row inside this tile: sv holds the row's sum over the tile
          const HmcLoc l = hmc_locate(ts.start, ts.row, ts.n_tensors, i);
          const int64_t slot = hmc_slot(l.chain, slots, ts.poff[l.s], l.run_start, tile);
          ksum[slot] = sv[b][e];
          const int64_t r = ts.row[l.s];
          if (i == l.run_start + r - 1 && hmc_pieces_of(l.run_start, r) < hmc_pieces(r)) ksum[slot + 1] = (T)0;
        }
      }
      __syncthreads();
    }
  }
}

template <typename T, bool VEC>
__global__ __launch_bounds__(THREADS) void k_hmc_select(const Table<T> ts, int64_t n, int64_t groups, const int32_t* __restrict__ accept) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t gi = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; gi < groups; gi += stride) {
    if (VEC) {
      const HmcLoc l = hmc_locate(ts.start, ts.row, ts.n_tensors, gi << 2);
      const T* src = accept[l.chain] ? ts.q[l.s] : ts.q0[l.s];
      *reinterpret_cast<Vec4<T>*>(ts.p0[l.s] + l.off) = *reinterpret_cast<const Vec4<T>*>(src + l.off);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (!flat_element_live(gi, j, n)) continue;
        const HmcLoc l = hmc_locate(ts.start, ts.row, ts.n_tensors, (gi << 2) + j);
        ts.p0[l.s][l.off] = accept[l.chain] ? ts.q[l.s][l.off] : ts.q0[l.s][l.off];
      }
    }
  }
}

struct Chunks {
  const void* k0[ZS_HMC_MAX_CHUNKS];
  const void* k1[ZS_HMC_MAX_CHUNKS];
  int64_t slots[ZS_HMC_MAX_CHUNKS];
  uint32_t f64_mask;
  int n_chunks;
};

__device__ __forceinline__ double chain_sum(const void* k, bool f64, int64_t c, int64_t slots) {
  double s = 0.0;
  if (f64) {
    const double* p = (const double*)k + c * slots;
    for (int64_t j = 0; j < slots; ++j) s += p[j];
  } else {
    const float* p = (const float*)k + c * slots;
    for (int64_t j = 0; j < slots; ++j) s += (double)p[j];
  }
  return s;
}

template <typename T>
__global__ __launch_bounds__(DECIDE_THREADS) void k_hmc_decide(const Chunks ch, int64_t C, const T* __restrict__ logp0,
                                                             const T* __restrict__ logp1, const T* __restrict__ u,
                                                             double* __restrict__ state, double* __restrict__ out,
                                                             int32_t* __restrict__ accept, int adapting, double delta, double gamma,
                                                             double t0, double kappa, uint64_t seed, uint64_t call,
                                                             const uint64_t* __restrict__ rs) {
  __shared__ double sa[DECIDE_THREADS];
  __shared__ double sn[DECIDE_THREADS];
  if (rs) { seed = rs[0]; call += rs[1]; }
  const PhiloxCall pc = philox_call(call, seed);
  const int tid = threadIdx.x;
  double asum = 0.0, nacc = 0.0;
  for (int64_t c = tid; c < C; c += DECIDE_THREADS) {
    double k0 = 0.0, k1 = 0.0;
    for (int k = 0; k < ch.n_chunks; ++k) {
      const bool f64 = (ch.f64_mask >> k) & 1u;
      k0 += chain_sum(ch.k0[k], f64, c, ch.slots[k]);
      k1 += chain_sum(ch.k1[k], f64, c, ch.slots[k]);
    }
    k0 *= 0.5;
    k1 *= 0.5;
    double uc;
    if (u) {
      uc = (double)u[c];
    } else {
      const Philox4 r = philox4x32_10((uint64_t)(c >> 2), pc);
      const int w = (int)(c & 3);
      uc = (double)u01(w == 0 ? r.x : (w == 1 ? r.y : (w == 2 ? r.z : r.w)));
    }
    const double l0 = (double)logp0[c], l1 = (double)logp1[c];
    const double dh = hmc_delta_h(l0, l1, k0, k1);
    const double a = hmc_accept_prob(dh);
    const bool acc = hmc_accept(dh, uc);
    accept[c] = acc ? 1 : 0;
    out[c] = a;
    out[C + c] = k0 - l0;
    out[2 * C + c] = k1 - l1;
    out[3 * C + c] = dh;
    out[4 * C + c] = acc ? l1 : l0;
    asum += a;
    nacc += acc ? 1.0 : 0.0;
  }
  sa[tid] = asum;
  sn[tid] = nacc;
  __syncthreads();
  for (int d = DECIDE_THREADS / 2; d > 0; d >>= 1) {
    if (tid < d) {
      sa[tid] += sa[tid + d];
      sn[tid] += sn[tid + d];
    }
    __syncthreads();
  }
  if (tid == 0) {
    const double abar = sa[0] / (double)C;
    hmc_adapt(state, abar, adapting, delta, gamma, t0, kappa);
    state[HMC_ABAR] = abar;
    state[HMC_NACC] = sn[0];
  }
}

// validates a move / select table and fills the kernel's; returns 0, ZS_EINVAL or ZS_ENOTSUP; *vec: the 16-byte path applies
template <typename T>
int fill_table(int kind, bool select, const zs_hmc_tensor* tensors, int n_tensors, int64_t n, int64_t C, Table<T>& ts, bool* vec) {
  if (n_tensors < 1 || !tensors || tensors[0].start != 0) return ZS_EINVAL;
  const size_t A = sizeof(T) * 4;
  memset(&ts, 0, sizeof(ts));
  ts.n_tensors = n_tensors;
  *vec = true;
  int64_t poff = 0;
  for (int i = 0; i < n_tensors; ++i) {
    const zs_hmc_tensor& t = tensors[i];
    const int64_t end = i + 1 < n_tensors ? tensors[i + 1].start : n;
    if (t.row < 1 || end <= t.start || (end - t.start) / C != t.row || (end - t.start) % C != 0) return ZS_EINVAL;
    uintptr_t bits = 0;
    if (select) {
      if (!t.q0 || !t.q || !t.q_out) return ZS_EINVAL;
      ts.q0[i] = (const T*)t.q0;
      ts.q[i] = (T*)t.q;
      ts.p0[i] = (T*)t.q_out;
    } else {
      const bool begin = kind == ZS_HMC_BEGIN;
      if (!t.grad || !t.p || (begin && !t.q0) || (kind != ZS_HMC_END && !t.q)) return ZS_EINVAL;
      ts.grad[i] = (const T*)t.grad;
      ts.p[i] = (T*)t.p;
      ts.q0[i] = begin ? (const T*)t.q0 : nullptr;
      ts.q[i] = kind != ZS_HMC_END ? (T*)t.q : nullptr;
      ts.z[i] = begin ? (const T*)t.z : nullptr;
      ts.p0[i] = begin ? (T*)t.p0 : nullptr;
      if (ts.z[i]) ts.has_z |= 1u << i;
      if (ts.p0[i]) ts.has_p0 |= 1u << i;
    }
    bits = (uintptr_t)ts.q0[i] | (uintptr_t)ts.q[i] | (uintptr_t)ts.p[i] | (uintptr_t)ts.grad[i] | (uintptr_t)ts.z[i] | (uintptr_t)ts.p0[i];
    *vec = *vec && (t.start & 3) == 0 && (t.row & 3) == 0 && !(bits & (A - 1));
    ts.start[i] = t.start;
    ts.row[i] = t.row;
    ts.poff[i] = (int32_t)poff;
    poff += hmc_pieces(t.row);
    if (poff > INT32_MAX) return ZS_ENOTSUP;
  }
  ts.start[n_tensors] = n;
  ts.poff[n_tensors] = (int32_t)poff;
  return 0;
}

template <typename T, int KIND>
void launch_move(bool vec, unsigned grid, hipStream_t st, const Table<T>& ts, int64_t n, int64_t tiles, const double* state, T* ksum,
                 uint64_t seed, uint64_t call, const uint64_t* rs) {
  if (vec)
    hipLaunchKernelGGL((k_hmc_move<T, KIND, true>), dim3(grid), dim3(THREADS), 0, st, ts, n, tiles, state, ksum, seed, call, rs);
  else
    hipLaunchKernelGGL((k_hmc_move<T, KIND, false>), dim3(grid), dim3(THREADS), 0, st, ts, n, tiles, state, ksum, seed, call, rs);
}

template <typename T>
int hmc_move(int kind, const zs_hmc_tensor* tensors, int n_tensors, int64_t n, int64_t C, const double* state, void* ksum,
             uint64_t seed, uint64_t call, const uint64_t* rng_state, void* stream) {
  if (kind < ZS_HMC_BEGIN || kind > ZS_HMC_END) return ZS_EINVAL;
  if (n < 0 || C < 0 || n_tensors < 0) return ZS_EINVAL;
  if (n_tensors > ZS_HMC_MAX_TENSORS) return ZS_ENOTSUP;
  if (n == 0 || C == 0) return 0;
  if (!state || (kind != ZS_HMC_STEP && !ksum)) return ZS_EINVAL;
  Table<T> ts;
  bool vec;
  const int rc = fill_table<T>(kind, false, tensors, n_tensors, n, C, ts, &vec);
  if (rc) return rc;
  const int64_t tiles = (n + TILE - 1) / TILE;
  const unsigned grid = grid_for(tiles, 1, 256u * 64u);
  hipStream_t st = (hipStream_t)stream;
  T* ks = (T*)ksum;
  switch (kind) {
    case ZS_HMC_BEGIN: launch_move<T, ZS_HMC_BEGIN>(vec, grid, st, ts, n, tiles, state, ks, seed, call, rng_state); break;
    case ZS_HMC_STEP: launch_move<T, ZS_HMC_STEP>(vec, grid, st, ts, n, tiles, state, ks, seed, call, rng_state); break;
    default: launch_move<T, ZS_HMC_END>(vec, grid, st, ts, n, tiles, state, ks, seed, call, rng_state); break;
  }
  ZS_CHECK_LAUNCH();
  return 0;
}

template <typename T>
int hmc_select(const zs_hmc_tensor* tensors, int n_tensors, int64_t n, int64_t C, const int32_t* accept, void* stream) {
  if (n < 0 || C < 0 || n_tensors < 0) return ZS_EINVAL;
  if (n_tensors > ZS_HMC_MAX_TENSORS) return ZS_ENOTSUP;
  if (n == 0 || C == 0) return 0;
  if (!accept) return ZS_EINVAL;
  Table<T> ts;
  bool vec;
  const int rc = fill_table<T>(0, true, tensors, n_tensors, n, C, ts, &vec);
  if (rc) return rc;
  const int64_t groups = (n + 3) / 4;
  const unsigned grid = grid_for(groups, THREADS, 256u * 16u);
  if (vec)
    hipLaunchKernelGGL((k_hmc_select<T, true>), dim3(grid), dim3(THREADS), 0, (hipStream_t)stream, ts, n, groups, accept);
  else
    hipLaunchKernelGGL((k_hmc_select<T, false>), dim3(grid), dim3(THREADS), 0, (hipStream_t)stream, ts, n, groups, accept);
  ZS_CHECK_LAUNCH();
  return 0;
}

template <typename T>
int hmc_decide(const zs_hmc_chunk* chunks, int n_chunks, int64_t C, const void* logp0, const void* logp1, const void* u,
               double* state, double* out, int32_t* accept, int adapting, double delta, double gamma, double t0, double kappa,
               uint64_t seed, uint64_t call, const uint64_t* rng_state, void* stream) {
  if (C < 0 || n_chunks < 0) return ZS_EINVAL;
  if (n_chunks > ZS_HMC_MAX_CHUNKS) return ZS_ENOTSUP;
  if (C == 0) return 0;
  if (n_chunks < 1 || !chunks || !logp0 || !logp1 || !state || !out || !accept) return ZS_EINVAL;
  if (adapting && (!(delta > 0.0 && delta < 1.0) || !(gamma > 0.0) || !(t0 >= 0.0) || !(kappa > 0.5 && kappa <= 1.0))) return ZS_EINVAL;
  Chunks ch;
  memset(&ch, 0, sizeof(ch));
  ch.n_chunks = n_chunks;
  for (int k = 0; k < n_chunks; ++k) {
    if (!chunks[k].k0 || !chunks[k].k1 || chunks[k].slots < 1) return ZS_EINVAL;
    ch.k0[k] = chunks[k].k0;
    ch.k1[k] = chunks[k].k1;
    ch.slots[k] = chunks[k].slots;
    if (chunks[k].is_f64) ch.f64_mask |= 1u << k;
  }
  hipLaunchKernelGGL((k_hmc_decide<T>), dim3(1), dim3(DECIDE_THREADS), 0, (hipStream_t)stream, ch, C, (const T*)logp0, (const T*)logp1,
                     (const T*)u, state, out, accept, adapting, delta, gamma, t0, kappa, seed, call, rng_state);
  ZS_CHECK_LAUNCH();
  return 0;
}

}  // namespace

extern "C" int zs_hmc_abi_version(void) { return ZS_HMC_ABI_VERSION; }

extern "C" int64_t zs_hmc_ksum_slots(const int64_t* rows, int n_tensors) {
  if (!rows || n_tensors < 0) return -1;
  int64_t s = 0;
  for (int i = 0; i < n_tensors; ++i) {
    if (rows[i] < 1) return -1;
    s += hmc_pieces(rows[i]);
  }
  return s;
}

#define ZS_HMC_ENTRY(SFX, T)                                                                                                        \
  extern "C" int zs_hmc_move##SFX(int kind, const struct zs_hmc_tensor* tensors, int n_tensors, int64_t n, int64_t C,               \
                                  const double* state, void* ksum, uint64_t seed, uint64_t call, const uint64_t* rng_state,        \
                                  void* stream) {                                                                                   \
    return hmc_move<T>(kind, tensors, n_tensors, n, C, state, ksum, seed, call, rng_state, stream);                                 \
  }                                                                                                                                 \
  extern "C" int zs_hmc_decide##SFX(const struct zs_hmc_chunk* chunks, int n_chunks, int64_t C, const void* logp0,                  \
                                    const void* logp1, const void* u, double* state, double* out, int32_t* accept, int adapting,   \
                                    double delta, double gamma, double t0, double kappa, uint64_t seed, uint64_t call,              \
                                    const uint64_t* rng_state, void* stream) {                                                      \
    return hmc_decide<T>(chunks, n_chunks, C, logp0, logp1, u, state, out, accept, adapting, delta, gamma, t0, kappa, seed, call,   \
                         rng_state, stream);                                                                                        \
  }                                                                                                                                 \
  extern "C" int zs_hmc_select##SFX(const struct zs_hmc_tensor* tensors, int n_tensors, int64_t n, int64_t C,                       \
                                    const int32_t* accept, void* stream) {                                                          \
    return hmc_select<T>(tensors, n_tensors, n, C, accept, stream);                                                                 \
  }

ZS_HMC_ENTRY(_f32, float)
ZS_HMC_ENTRY(_f64, double)
