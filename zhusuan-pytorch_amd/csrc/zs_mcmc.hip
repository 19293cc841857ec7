// M1: the stochastic-gradient MCMC update (SGLD, PSGLD, SGHMC) of up to 32 latent tensors in one launch
// (include/zs_mcmc.h; built as its own library, ../lib/libzs_mcmc.so, by `make mcmc`).
//
// The reference's samplers (zhusuan/mcmc/SGLD.py:42-54,67-82, SGHMC.py:25-56) update latent by latent: a torch.normal on the
// host, three to six element-wise kernels and a detach each, around a log joint that costs a handful of launches.  Here the
// latents of a step form ONE flat index space [start[s], start[s+1]) as the parameters do in k_adam_step (zs_adam.hip): values,
// gradients, state and injected noise are read where they live through a pointer table passed by value, a thread owns four
// consecutive elements -- one Philox group, so the noise of flat element i is element i of zs_philox_normal_f32's stream for
// the same (seed, call) -- and finds their tensor by bisection.  Purely element-wise: no hand-off between workgroups, no LDS,
// no atomics.  HBM traffic per element (fp32): SGLD 12 B (q, g in; q out), PSGLD and SGHMC post 20 B (q, g, state in; q,
// state out), SGHMC pre 8 to 16 B.
//
// Launch geometry: k_adam_step's (at most 256 workgroups of 1024 threads, one per CU, grid-stride) as the starting point; it
// was measured for Adam's 28 B per element and a ticket at the end, not for this kernel, whose launches at the sizes of the
// BNN callers (1.5 K to 15 K elements) are a single partial wave of workgroups either way.
#include "zs_common.h"
#include "zs_mcmc_math.h"
#include "../../include/zs_hip.h"
#include "../../include/zs_mcmc.h"

using namespace zs;

namespace {

template <typename T>
struct Table {
  const T* q_in[ZS_MCMC_MAX_TENSORS];
  T* q_out[ZS_MCMC_MAX_TENSORS];
  const T* grad[ZS_MCMC_MAX_TENSORS];       // (a kind that does not read an operand never dereferences its pointer)
  T* state[ZS_MCMC_MAX_TENSORS];
  const T* z[ZS_MCMC_MAX_TENSORS];
  int64_t start[ZS_MCMC_MAX_TENSORS + 1];   // start[n_tensors] = n
  uint32_t has_z;                           // bit s: tensor s brings its own standard normals
  int n_tensors;
};

template <typename T, int KIND, bool VEC>
__global__ __launch_bounds__(1024) void k_mcmc_update(const Table<T> ts, const McmcCoef<T> c, int64_t n, int draws, uint64_t seed,
                                                      uint64_t call, const uint64_t* __restrict__ rs) {
  constexpr bool GRAD = KIND != ZS_MCMC_SGHMC_PRE, STATE = KIND != ZS_MCMC_SGLD;
  if (rs) { seed = rs[0]; call += rs[1]; }
  const PhiloxCall pc = philox_call(call, seed);
  const int64_t groups = (n + 3) >> 2;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  // draws: the kind uses noise at all (SGHMC_PRE without a velocity resample does not); the generator runs for a group only
  // where one of its elements has no injected value
  for (int64_t gi = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; gi < groups; gi += stride) {
    if (VEC) {
      // every tensor starts at a multiple of 4 and is aligned for one wide access per operand (checked on the host)
      const int64_t i0 = gi << 2;
      const int s = flat_tensor_of(ts.start, ts.n_tensors, i0);
      const int64_t off = i0 - ts.start[s];
      const bool inj = (ts.has_z >> s) & 1u;
      Vec4<T> q = *reinterpret_cast<const Vec4<T>*>(ts.q_in[s] + off), g, st, zz;
      if (GRAD) g = *reinterpret_cast<const Vec4<T>*>(ts.grad[s] + off);
      if (STATE) st = *reinterpret_cast<const Vec4<T>*>(ts.state[s] + off);
      if (draws) {
        if (inj) {
          zz = *reinterpret_cast<const Vec4<T>*>(ts.z[s] + off);
        } else {
          const float4 nrm = philox_normal4((uint64_t)gi, pc);
          zz.v[0] = (T)nrm.x; zz.v[1] = (T)nrm.y; zz.v[2] = (T)nrm.z; zz.v[3] = (T)nrm.w;
        }
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        T sj = STATE ? st.v[j] : (T)0;
        mcmc_apply<T, KIND>(q.v[j], sj, GRAD ? g.v[j] : (T)0, draws ? zz.v[j] : (T)0, c);
        if (STATE) st.v[j] = sj;
      }
      *reinterpret_cast<Vec4<T>*>(ts.q_out[s] + off) = q;
      if (STATE) *reinterpret_cast<Vec4<T>*>(ts.state[s] + off) = st;
    } else {
      // element form (tensors of any length and alignment): four consecutive elements, each finds its own tensor; the
      // elements past n are clamped onto the group's first one, so the loads are unconditional and only the stores are not
      T q[4], g[4], st[4], zz[4];
      T* qd[4];
      T* sd[4];
      bool inj[4], all_inj = true;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int64_t i = flat_clamped_index(gi, j, n);
        const int s = flat_tensor_of(ts.start, ts.n_tensors, i);
        const int64_t off = i - ts.start[s];
        inj[j] = (ts.has_z >> s) & 1u;
        all_inj = all_inj && inj[j];
        q[j] = ts.q_in[s][off];
        qd[j] = ts.q_out[s] + off;
        g[j] = GRAD ? ts.grad[s][off] : (T)0;
        sd[j] = STATE ? ts.state[s] + off : nullptr;
        st[j] = STATE ? *sd[j] : (T)0;
        zz[j] = (draws && inj[j]) ? ts.z[s][off] : (T)0;
      }
      if (draws && !all_inj) {
        const float4 nrm = philox_normal4((uint64_t)gi, pc);
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (!inj[j]) zz[j] = (T)f4_get(nrm, j);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        mcmc_apply<T, KIND>(q[j], st[j], g[j], zz[j], c);
        if (flat_element_live(gi, j, n)) {
          *qd[j] = q[j];
          if (STATE) *sd[j] = st[j];
        }
      }
    }
  }
}

template <typename T, int KIND>
void launch(bool vec, unsigned grid, hipStream_t st, const Table<T>& ts, const McmcCoef<T>& c, int64_t n, int draws, uint64_t seed,
            uint64_t call, const uint64_t* rs) {
  if (vec)
    hipLaunchKernelGGL((k_mcmc_update<T, KIND, true>), dim3(grid), dim3(1024), 0, st, ts, c, n, draws, seed, call, rs);
  else
    hipLaunchKernelGGL((k_mcmc_update<T, KIND, false>), dim3(grid), dim3(1024), 0, st, ts, c, n, draws, seed, call, rs);
}

template <typename T>
int mcmc_update(int kind, const zs_mcmc_tensor* tensors, int n_tensors, int64_t n, double lr, double decay, double epsilon,
                double alpha, double beta, int flags, uint64_t seed, uint64_t call, const uint64_t* rng_state, void* stream) {
  if (kind < ZS_MCMC_SGLD || kind > ZS_MCMC_SGHMC_POST) return ZS_EINVAL;
  if (flags & ~(ZS_MCMC_SECOND_ORDER | ZS_MCMC_RESAMPLE_V)) return ZS_EINVAL;
  if (n < 0 || n_tensors < 0 || !(lr >= 0.0)) return ZS_EINVAL;
  if (kind == ZS_MCMC_PSGLD && (!(decay >= 0.0 && decay < 1.0) || !(epsilon >= 0.0))) return ZS_EINVAL;
  if (kind == ZS_MCMC_SGHMC_POST && !(alpha >= beta)) return ZS_EINVAL;
  if (n_tensors > ZS_MCMC_MAX_TENSORS) return ZS_ENOTSUP;
  if (n == 0) return 0;
  if (n_tensors < 1 || !tensors || tensors[0].start != 0) return ZS_EINVAL;
  const size_t A = sizeof(T) * 4;
  const bool need_g = mcmc_reads_grad(kind), need_s = mcmc_has_state(kind), draws = mcmc_draws(kind, flags);
  bool vec = (n & 3) == 0;
  Table<T> ts;
  memset(&ts, 0, sizeof(ts));
  ts.n_tensors = n_tensors;
  for (int i = 0; i < n_tensors; ++i) {
    const zs_mcmc_tensor& t = tensors[i];
    const int64_t end = i + 1 < n_tensors ? tensors[i + 1].start : n;
    if (end <= t.start) return ZS_EINVAL;                  // non-empty, ascending
    if (!t.q_in || !t.q_out || (need_g && !t.grad) || (need_s && !t.state)) return ZS_EINVAL;
    ts.q_in[i] = (const T*)t.q_in;
    ts.q_out[i] = (T*)t.q_out;
    ts.grad[i] = need_g ? (const T*)t.grad : nullptr;
    ts.state[i] = need_s ? (T*)t.state : nullptr;
    ts.z[i] = draws ? (const T*)t.z : nullptr;
    ts.start[i] = t.start;
    if (ts.z[i]) ts.has_z |= 1u << i;
    const uintptr_t bits = (uintptr_t)ts.q_in[i] | (uintptr_t)ts.q_out[i] | (uintptr_t)ts.grad[i] | (uintptr_t)ts.state[i] | (uintptr_t)ts.z[i];
    vec = vec && (t.start & 3) == 0 && !(bits & (A - 1));
  }
  ts.start[n_tensors] = n;
  const McmcCoef<T> c = mcmc_coef<T>(kind, flags, lr, decay, epsilon, alpha, beta);
  const unsigned grid = grid_for((n + 3) / 4, 1024, 256u);
  hipStream_t st = (hipStream_t)stream;
  switch (kind) {
    case ZS_MCMC_SGLD: launch<T, ZS_MCMC_SGLD>(vec, grid, st, ts, c, n, draws, seed, call, rng_state); break;
    case ZS_MCMC_PSGLD: launch<T, ZS_MCMC_PSGLD>(vec, grid, st, ts, c, n, draws, seed, call, rng_state); break;
    case ZS_MCMC_SGHMC_PRE: launch<T, ZS_MCMC_SGHMC_PRE>(vec, grid, st, ts, c, n, draws, seed, call, rng_state); break;
    default: launch<T, ZS_MCMC_SGHMC_POST>(vec, grid, st, ts, c, n, draws, seed, call, rng_state); break;
  }
  ZS_CHECK_LAUNCH();
  return 0;
}

}  // namespace

extern "C" int zs_mcmc_abi_version(void) { return ZS_MCMC_ABI_VERSION; }

extern "C" int zs_mcmc_update_f32(int kind, const struct zs_mcmc_tensor* tensors, int n_tensors, int64_t n, double lr, double decay,
                                  double epsilon, double alpha, double beta, int flags, uint64_t seed, uint64_t call,
                                  const uint64_t* rng_state, void* stream) {
  return mcmc_update<float>(kind, tensors, n_tensors, n, lr, decay, epsilon, alpha, beta, flags, seed, call, rng_state, stream);
}
extern "C" int zs_mcmc_update_f64(int kind, const struct zs_mcmc_tensor* tensors, int n_tensors, int64_t n, double lr, double decay,
                                  double epsilon, double alpha, double beta, int flags, uint64_t seed, uint64_t call,
                                  const uint64_t* rng_state, void* stream) {
  return mcmc_update<double>(kind, tensors, n_tensors, n, lr, decay, epsilon, alpha, beta, flags, seed, call, rng_state, stream);
}
