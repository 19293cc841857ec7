// P1, P1b, P1f, H1, H1b: the planar and Householder flow stacks (include/zs_nf.h; its own library, ../lib/libzs_nf.so, `make nf`).
//
// A torch composition of one planar layer is about fifteen launches each way on a [B, D] tensor, once per layer; here the whole
// stack is one launch each way (plus the small finish of the parameter gradients).  A group of G = next_pow2(D) lanes owns a row,
// lane i its component i (zs_nf_math.h); a workgroup is one wave of 64 / G rows.  z stays in a register through all L layers, dots
// are butterflies inside the group.  The planar kernels first form uh_l and c_l of every layer in LDS (each workgroup on its own:
// no workgroup waits for another).  The backwards recompute the forward and keep every layer's input z_l in LDS, one element per
// lane and layer, read back by the lane that wrote it.  No atomics, no scratch: nothing per lane is indexed by a run-time value.
// Every access is one element wide, so the bits do not depend on the alignment of the operands.
#include "zs_common.h"
#include "zs_nf_math.h"
#include "../../include/zs_hip.h"
#include "../../include/zs_nf.h"

#pragma clang fp contract(off)

using namespace zs;

namespace {

constexpr int THREADS = ZS_NF_THREADS;

extern __shared__ __align__(16) unsigned char nf_lds_raw[];

// The parameter quantities of layer l over one wave: lane d < D holds u_l[d], w_l[d], uh_l[d]; s, n, k, c are the same in all lanes.
template <typename T>
struct NfLayer { T u, w, s, n, k, uh, c; };
template <typename T>
__device__ __forceinline__ NfLayer<T> planar_layer(const T* __restrict__ u, const T* __restrict__ w, int l, int D, int lane) {
  NfLayer<T> p;
  const bool on = lane < D;
  p.u = on ? u[l * D + lane] : (T)0;
  p.w = on ? w[l * D + lane] : (T)0;
  p.s = group_sum(p.w * p.u, ZS_WAVE);
  p.n = group_sum(p.w * p.w, ZS_WAVE);
  p.k = nf_planar_k(p.s);
  p.uh = on ? nf_planar_uhat(p.u, p.w, p.k, p.n) : (T)0;
  p.c = group_sum(p.w * p.uh, ZS_WAVE);
  return p;
}
// uh[L D] and c[L] of the stack into LDS (the caller's barrier follows)
template <typename T>
__device__ __forceinline__ void planar_stack_to_lds(const T* __restrict__ u, const T* __restrict__ w, T* uh, T* cc, int D, int L) {
  const int lane = (int)threadIdx.x;
  for (int l = 0; l < L; ++l) {
    const NfLayer<T> p = planar_layer(u, w, l, D, lane);
    if (lane < D) uh[l * D + lane] = p.uh;
    if (lane == 0) cc[l] = p.c;
  }
}

// ---------------------------------------------------------------- P1
template <typename T>
__global__ __launch_bounds__(THREADS) void k_planar_fwd(const T* __restrict__ u, const T* __restrict__ w, const T* __restrict__ b,
                                                        const T* x, T* y, T* __restrict__ logdet, int64_t R, int D, int L, int G) {
  T* uh = reinterpret_cast<T*>(nf_lds_raw);
  T* cc = uh + L * D;
  planar_stack_to_lds(u, w, uh, cc, D, L);
  __syncthreads();
  const GroupPlace pl = group_place((int)threadIdx.x, THREADS, G);
  for (int64_t rb = group_row_first((int)blockIdx.x, pl); rb < R; rb += group_row_step((int)gridDim.x, pl)) {
    const int64_t r = rb + pl.grp;
    const bool valid = r < R, act = valid && pl.lane < D;
    T z = act ? x[r * D + pl.lane] : (T)0, ld = (T)0;
    for (int l = 0; l < L; ++l) {
      const T wd = act ? w[l * D + pl.lane] : (T)0;
      const T t = nf_planar_t(group_sum(wd * z, G), b[l]);
      if (act) z = nf_planar_z(z, uh[l * D + pl.lane], t);
      ld = nf_planar_logdet(ld, t, cc[l]);
    }
    if (act && y) y[r * D + pl.lane] = z;
    if (valid && pl.lane == 0 && logdet) logdet[r] = ld;
  }
}

// ---------------------------------------------------------------- P1b
// this tile's sum of `v` over the groups of the wave in ascending group (= row) order, for component pl.lane
template <typename T>
__device__ __forceinline__ T tile_sum(T v, const GroupPlace& pl, int G) {
  T s = __shfl(v, pl.lane, ZS_WAVE);
  for (int gi = 1; gi < pl.groups; ++gi) s += __shfl(v, gi * G + pl.lane, ZS_WAVE);
  return s;
}

template <typename T>
__global__ __launch_bounds__(THREADS) void k_planar_bwd(const T* __restrict__ u, const T* __restrict__ w, const T* __restrict__ b,
                                                        const T* __restrict__ x, const T* __restrict__ gy, const T* __restrict__ gld,
                                                        T* __restrict__ gx, T* partials, int64_t R, int D, int L, int G) {
  const int lane = (int)threadIdx.x;
  const GroupPlace pl = group_place(lane, THREADS, G);
  T* uh = reinterpret_cast<T*>(nf_lds_raw);
  T* cc = uh + L * D;
  T* ts = cc + L;
  T* zin = ts + L * pl.groups;
  planar_stack_to_lds(u, w, uh, cc, D, L);
  const int64_t rb0 = group_row_first((int)blockIdx.x, pl);
  for (int64_t rb = rb0; rb < R; rb += group_row_step((int)gridDim.x, pl)) {
    const int64_t r = rb + pl.grp;
    const bool valid = r < R, act = valid && pl.lane < D;
    __syncthreads();          // uh, c are in place; the previous tile has finished with ts
    // the forward again, with the forward's own device functions: the same a_l, z_l bit for bit
    T z = act ? x[r * D + pl.lane] : (T)0;
    for (int l = 0; l < L; ++l) {
      zin[nf_z_index(l, lane)] = z;
      const T wd = act ? w[l * D + pl.lane] : (T)0;
      const T t = nf_planar_t(group_sum(wd * z, G), b[l]);
      if (pl.lane == 0) ts[nf_t_index(l, pl.grp, pl.groups)] = t;
      if (act) z = nf_planar_z(z, uh[l * D + pl.lane], t);
    }
    __syncthreads();
    T g = (gy && act) ? gy[r * D + pl.lane] : (T)0;
    const T gl = (gld && valid) ? gld[r] : (T)0;
    for (int l = L - 1; l >= 0; --l) {
      const T t = ts[nf_t_index(l, pl.grp, pl.groups)], c = cc[l];
      const T uhd = act ? uh[l * D + pl.lane] : (T)0, wd = act ? w[l * D + pl.lane] : (T)0;
      const T zl = zin[nf_z_index(l, lane)];
      const T h = nf_planar_h(t), m = nf_planar_m(h, c);
      const T ga = nf_planar_gt(group_sum(g * uhd, G), gl, c, m, t) * h;
      if (partials) {
        const T su = tile_sum(act ? g * t : (T)0, pl, G);
        const T sw = tile_sum(act ? ga * zl : (T)0, pl, G);
        const T sb = tile_sum(valid ? ga : (T)0, pl, G);
        const T sc = tile_sum(valid ? nf_planar_gc(gl, h, m) : (T)0, pl, G);
        T* P = partials + nf_partial_row((int64_t)blockIdx.x, l, D, L);
        if (pl.grp == 0 && pl.lane < D) {
          T* pu = P + nf_partial_guh(pl.lane);
          T* pw = P + nf_partial_gw(pl.lane, D);
          *pu = rb == rb0 ? su : *pu + su;
          *pw = rb == rb0 ? sw : *pw + sw;
        }
        if (lane == 0) {
          T* pb = P + nf_partial_gb(D);
          T* pc = P + nf_partial_gc(D);
          *pb = rb == rb0 ? sb : *pb + sb;
          *pc = rb == rb0 ? sc : *pc + sc;
        }
      }
      if (act) g = nf_planar_g(g, ga, wd);
    }
    if (gx && act) gx[r * D + pl.lane] = g;
  }
}

// ---------------------------------------------------------------- P1f
// One workgroup; wave j takes the layers j, j + waves, ...: lane d adds the partials of (l, d) in ascending workgroup order, then
// the parameter chain with the quantities planar_layer gives (the backward's own).
template <typename T>
__global__ __launch_bounds__(ZS_NF_FINISH_THREADS) void k_planar_finish(const T* __restrict__ u, const T* __restrict__ w,
                                                                         const T* __restrict__ partials, int64_t n_wg,
                                                                         T* __restrict__ gu, T* __restrict__ gw, T* __restrict__ gb,
                                                                         int D, int L) {
  const int lane = (int)threadIdx.x & (ZS_WAVE - 1), wave = (int)threadIdx.x / ZS_WAVE, waves = (int)blockDim.x / ZS_WAVE;
  const bool on = lane < D;
  const int d = on ? lane : 0;
  for (int l = wave; l < L; l += waves) {
    const NfLayer<T> p = planar_layer(u, w, l, D, lane);
    const T* P = partials + nf_partial_row(0, l, D, L);
    const int64_t step = nf_partial_row(1, 0, D, L);
    T Gu = P[nf_partial_guh(d)], Gw = P[nf_partial_gw(d, D)], Gb = P[nf_partial_gb(D)], Gc = P[nf_partial_gc(D)];
    // the loads of U workgroups are requested together, the additions stay in ascending order: one wave alone would otherwise
    // wait a memory latency per workgroup (4096 of them at B = 4096, D = 40)
    constexpr int U = 64 / (int)sizeof(T);
    int64_t g = 1;
    for (; g + U <= n_wg; g += U) {
      T a[U], b[U], c[U], e[U];
#pragma unroll
      for (int j = 0; j < U; ++j) {
        const T* Pj = P + (g + j) * step;
        a[j] = Pj[nf_partial_guh(d)];
        b[j] = Pj[nf_partial_gw(d, D)];
        c[j] = Pj[nf_partial_gb(D)];
        e[j] = Pj[nf_partial_gc(D)];
      }
#pragma unroll
      for (int j = 0; j < U; ++j) {
        Gu += a[j];
        Gw += b[j];
        Gb += c[j];
        Gc += e[j];
      }
    }
    for (; g < n_wg; ++g) {
      const T* Pj = P + g * step;
      Gu += Pj[nf_partial_guh(d)];
      Gw += Pj[nf_partial_gw(d, D)];
      Gb += Pj[nf_partial_gb(D)];
      Gc += Pj[nf_partial_gc(D)];
    }
    const T Gu1 = on ? nf_finish_guh(Gu, Gc, p.w) : (T)0;
    const T Gw1 = nf_finish_gw0(Gw, Gc, p.uh);
    const T pp = group_sum(Gu1 * p.w, ZS_WAVE), dk = nf_planar_dk(p.s);
    if (on && gu) gu[l * D + lane] = nf_finish_gu(Gu1, pp, p.n, dk, p.w);
    if (on && gw) gw[l * D + lane] = nf_finish_gw(Gw1, Gu1, pp, p.n, p.k, dk, p.u, p.w);
    if (lane == 0 && gb) gb[l] = Gb;
  }
}

// ---------------------------------------------------------------- H1, H1b
template <typename T>
__global__ __launch_bounds__(THREADS) void k_householder_fwd(const T* __restrict__ v, const T* x, T* y, int64_t R, int D, int L, int G) {
  const GroupPlace pl = group_place((int)threadIdx.x, THREADS, G);
  for (int64_t rb = group_row_first((int)blockIdx.x, pl); rb < R; rb += group_row_step((int)gridDim.x, pl)) {
    const int64_t r = rb + pl.grp;
    const bool act = r < R && pl.lane < D;
    T z = act ? x[r * D + pl.lane] : (T)0;
    for (int l = 0; l < L; ++l) {
      const T vd = act ? v[((int64_t)l * R + r) * D + pl.lane] : (T)0;
      const T n = group_sum(vd * vd, G), p = group_sum(vd * z, G);
      if (act) z = nf_householder_z(z, vd, p, n);
    }
    if (act) y[r * D + pl.lane] = z;
  }
}

template <typename T>
__global__ __launch_bounds__(THREADS) void k_householder_bwd(const T* __restrict__ v, const T* __restrict__ x, const T* __restrict__ gy,
                                                             T* __restrict__ gx, T* __restrict__ gv, int64_t R, int D, int L, int G) {
  T* zin = reinterpret_cast<T*>(nf_lds_raw);
  const int lane = (int)threadIdx.x;
  const GroupPlace pl = group_place(lane, THREADS, G);
  for (int64_t rb = group_row_first((int)blockIdx.x, pl); rb < R; rb += group_row_step((int)gridDim.x, pl)) {
    const int64_t r = rb + pl.grp;
    const bool act = r < R && pl.lane < D;
    T z = act ? x[r * D + pl.lane] : (T)0;
    for (int l = 0; l < L; ++l) {
      zin[nf_z_index(l, lane)] = z;          // read back below by this lane only
      const T vd = act ? v[((int64_t)l * R + r) * D + pl.lane] : (T)0;
      const T n = group_sum(vd * vd, G), p = group_sum(vd * z, G);
      if (act) z = nf_householder_z(z, vd, p, n);
    }
    T g = act ? gy[r * D + pl.lane] : (T)0;
    for (int l = L - 1; l >= 0; --l) {
      const int64_t at = ((int64_t)l * R + r) * D + pl.lane;
      const T vd = act ? v[at] : (T)0;
      const T zl = zin[nf_z_index(l, lane)];
      const T n = group_sum(vd * vd, G), p = group_sum(vd * zl, G), q = group_sum(vd * g, G);
      if (act && gv) gv[at] = nf_householder_gv(g, zl, vd, p, q, n);
      if (act) g = nf_householder_z(g, vd, q, n);
    }
    if (act && gx) gx[r * D + pl.lane] = g;
  }
}

// ---------------------------------------------------------------- host side
int check_shape(int64_t R, int64_t D, int64_t L) {
  if (D < 1 || R < 0 || L < 0) return ZS_EINVAL;
  if (D > ZS_NF_MAX_DIM || L > ZS_NF_MAX_LAYERS) return ZS_ENOTSUP;
  return 0;
}

template <typename T>
int planar_fwd(const void* u, const void* w, const void* b, const void* x, void* y, void* logdet, int64_t R, int64_t D, int64_t L,
               void* stream) {
  if (!u || !w || !b || !x) return ZS_EINVAL;
  const int rc = check_shape(R, D, L);
  if (rc) return rc;
  if (R == 0 || L == 0) return 0;
  if (!y && !logdet) return ZS_EINVAL;
  const int G = group_lanes(D);
  hipLaunchKernelGGL((k_planar_fwd<T>), dim3(nf_workgroups(R, G)), dim3(THREADS), (size_t)nf_planar_fwd_lds(D, L) * sizeof(T),
                     (hipStream_t)stream, (const T*)u, (const T*)w, (const T*)b, (const T*)x, (T*)y, (T*)logdet, R, (int)D, (int)L, G);
  ZS_CHECK_LAUNCH();
  return 0;
}

template <typename T>
int planar_bwd(const void* u, const void* w, const void* b, const void* x, const void* gy, const void* gld, void* gx, void* partials,
               int64_t R, int64_t D, int64_t L, void* stream) {
  if (!u || !w || !b || !x) return ZS_EINVAL;
  const int rc = check_shape(R, D, L);
  if (rc) return rc;
  if (R == 0 || L == 0) return 0;
  if ((!gy && !gld) || (!gx && !partials)) return ZS_EINVAL;
  const int G = group_lanes(D);
  hipLaunchKernelGGL((k_planar_bwd<T>), dim3(nf_workgroups(R, G)), dim3(THREADS), (size_t)nf_planar_bwd_lds(D, L, G) * sizeof(T),
                     (hipStream_t)stream, (const T*)u, (const T*)w, (const T*)b, (const T*)x, (const T*)gy, (const T*)gld, (T*)gx,
                     (T*)partials, R, (int)D, (int)L, G);
  ZS_CHECK_LAUNCH();
  return 0;
}

template <typename T>
int planar_finish(const void* u, const void* w, const void* partials, int64_t n_wg, void* gu, void* gw, void* gb, int64_t D, int64_t L,
                  void* stream) {
  if (!u || !w || !partials) return ZS_EINVAL;
  const int rc = check_shape(0, D, L);
  if (rc) return rc;
  if (L == 0) return 0;
  if (n_wg < 1 || n_wg > ZS_NF_MAX_WORKGROUPS || (!gu && !gw && !gb)) return ZS_EINVAL;
  hipLaunchKernelGGL((k_planar_finish<T>), dim3(1), dim3(ZS_NF_FINISH_THREADS), 0, (hipStream_t)stream, (const T*)u, (const T*)w,
                     (const T*)partials, n_wg, (T*)gu, (T*)gw, (T*)gb, (int)D, (int)L);
  ZS_CHECK_LAUNCH();
  return 0;
}

template <typename T>
int householder_fwd(const void* v, const void* x, void* y, int64_t R, int64_t D, int64_t L, void* stream) {
  if (!v || !x) return ZS_EINVAL;
  const int rc = check_shape(R, D, L);
  if (rc) return rc;
  if (R == 0 || L == 0) return 0;
  if (!y) return ZS_EINVAL;
  const int G = group_lanes(D);
  hipLaunchKernelGGL((k_householder_fwd<T>), dim3(nf_workgroups(R, G)), dim3(THREADS), 0, (hipStream_t)stream, (const T*)v,
                     (const T*)x, (T*)y, R, (int)D, (int)L, G);
  ZS_CHECK_LAUNCH();
  return 0;
}

template <typename T>
int householder_bwd(const void* v, const void* x, const void* gy, void* gx, void* gv, int64_t R, int64_t D, int64_t L, void* stream) {
  if (!v || !x || !gy) return ZS_EINVAL;
  const int rc = check_shape(R, D, L);
  if (rc) return rc;
  if (R == 0 || L == 0) return 0;
  if (!gx && !gv) return ZS_EINVAL;
  const int G = group_lanes(D);
  hipLaunchKernelGGL((k_householder_bwd<T>), dim3(nf_workgroups(R, G)), dim3(THREADS), (size_t)nf_householder_bwd_lds(L) * sizeof(T),
                     (hipStream_t)stream, (const T*)v, (const T*)x, (const T*)gy, (T*)gx, (T*)gv, R, (int)D, (int)L, G);
  ZS_CHECK_LAUNCH();
  return 0;
}

}  // namespace

extern "C" int zs_nf_abi_version(void) { return ZS_NF_ABI_VERSION; }
extern "C" int zs_nf_max_dim(void) { return ZS_NF_MAX_DIM; }
extern "C" int zs_nf_max_layers(void) { return ZS_NF_MAX_LAYERS; }
extern "C" int zs_nf_max_workgroups(void) { return ZS_NF_MAX_WORKGROUPS; }
extern "C" int zs_nf_group_lanes(int64_t D) { return (D < 1 || D > ZS_NF_MAX_DIM) ? 0 : group_lanes(D); }
extern "C" int zs_nf_planar_workgroups(int64_t R, int64_t D) {
  return (R < 1 || D < 1 || D > ZS_NF_MAX_DIM) ? 0 : nf_workgroups(R, group_lanes(D));
}

#define ZS_NF_ENTRY(SFX, T)                                                                                                          \
  extern "C" int zs_nf_planar_fwd##SFX(const void* u, const void* w, const void* b, const void* x, void* y, void* logdet, int64_t R, \
                                       int64_t D, int64_t L, void* stream) {                                                         \
    return planar_fwd<T>(u, w, b, x, y, logdet, R, D, L, stream);                                                                    \
  }                                                                                                                                  \
  extern "C" int zs_nf_planar_bwd##SFX(const void* u, const void* w, const void* b, const void* x, const void* gy, const void* gld,  \
                                       void* gx, void* partials, int64_t R, int64_t D, int64_t L, void* stream) {                    \
    return planar_bwd<T>(u, w, b, x, gy, gld, gx, partials, R, D, L, stream);                                                        \
  }                                                                                                                                  \
  extern "C" int zs_nf_planar_finish##SFX(const void* u, const void* w, const void* partials, int64_t n_wg, void* gu, void* gw,      \
                                          void* gb, int64_t D, int64_t L, void* stream) {                                            \
    return planar_finish<T>(u, w, partials, n_wg, gu, gw, gb, D, L, stream);                                                         \
  }                                                                                                                                  \
  extern "C" int zs_nf_householder_fwd##SFX(const void* v, const void* x, void* y, int64_t R, int64_t D, int64_t L, void* stream) {  \
    return householder_fwd<T>(v, x, y, R, D, L, stream);                                                                             \
  }                                                                                                                                  \
  extern "C" int zs_nf_householder_bwd##SFX(const void* v, const void* x, const void* gy, void* gx, void* gv, int64_t R, int64_t D,  \
                                            int64_t L, void* stream) {                                                               \
    return householder_bwd<T>(v, x, gy, gx, gv, R, D, L, stream);                                                                    \
  }

ZS_NF_ENTRY(_f32, float)
ZS_NF_ENTRY(_f64, double)
