// F1: the element-wise work of the normalising-flow layers around their inner networks, one launch per entry
// (include/zs_flow.h; built as its own library, ../lib/libzs_flow.so, by `make flow`).
//
// The reference's flow layers (zhusuan/invertible/coupling.py, scaling.py, made.py, distributions/flow_distribution.py) issue
// a string of tiny element-wise launches around every inner network, each with its own backward: two mask multiplies, two
// `1 - mask`, a masked shift and two adds per additive coupling; exp, multiply and sum per Scaling; chunk, subtract, exp,
// multiply, negate per MADE; log-density, row sum and add per FlowDistribution.log_prob.  At the sizes of the reference's flow
// VAE (B = 64, z = 40, ten couplings) the step is bound by launches, not bytes: every entry here is ONE launch.
//
// Three kernel shapes, all memory-streaming, no inline assembly, LDS only as reduction scratch:
//   * flat element-wise (split, merge, MADE, tail backward): grid-stride over B*D elements, W = 4 elements per thread with
//     one wide access per operand when D % 4 == 0 and every operand is aligned to 4 T (a group of four then never straddles a
//     row), W = 1 otherwise;
//   * column tiles (Scaling): a workgroup owns 64 consecutive columns and all B rows, 16 row lanes per column; the column sums
//     of the backward are combined through LDS in a fixed order; workgroup 0 also sums log_scale in the forward;
//   * one wavefront per row (tail forward): lane-strided terms, butterfly, the row's log-det added by lane 0.
// No reduction crosses a workgroup, so none needs an atomic or a hand-off: results are bit-reproducible.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "zs_flow_math.h"
#include "zs_group_math.h"         // group_sum; Vec4 (zs_flat_math.h)
#include "../../include/zs_hip.h"
#include "../../include/zs_flow.h"

using namespace zs;

#define ZS_FLOW_CHECK_LAUNCH()                      \
  do {                                              \
    hipError_t e__ = hipGetLastError();             \
    if (e__ != hipSuccess) return (int)e__;         \
  } while (0)

namespace {

constexpr int kBlock = 256;
constexpr unsigned kMaxGrid = 2048;

template <typename T, int W>
__device__ __forceinline__ void ld(const T* p, int64_t i, T (&r)[W]) {
  if (W == 4) {
    const Vec4<T> t = *reinterpret_cast<const Vec4<T>*>(p + i);
#pragma unroll
    for (int j = 0; j < W; ++j) r[j] = t.v[j];
  } else {
    r[0] = p[i];
  }
}
template <typename T, int W>
__device__ __forceinline__ void st(T* p, int64_t i, const T (&r)[W]) {
  if (W == 4) {
    Vec4<T> t;
#pragma unroll
    for (int j = 0; j < W; ++j) t.v[j] = r[j];
    *reinterpret_cast<Vec4<T>*>(p + i) = t;
  } else {
    p[i] = r[0];
  }
}

unsigned flat_grid(int64_t items) {
  int64_t b = (items + kBlock - 1) / kBlock;
  if (b < 1) b = 1;
  if (b > (int64_t)kMaxGrid) b = kMaxGrid;
  return (unsigned)b;
}

template <typename T>
bool aligned4(const void* p) { return (((uintptr_t)p) & (sizeof(T) * 4 - 1)) == 0; }

// ---------------------------------------------------------------------------------------------- coupling, MASK
// OP 0: out = mask * a   (split and its backward: the same expression)
template <typename T, int W>
__global__ __launch_bounds__(kBlock) void k_mask_mul(const T* __restrict__ a, const T* __restrict__ mask, T* __restrict__ out,
                                                     int64_t n, int64_t D) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x * W;
  for (int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * W; i < n; i += stride) {
    const int64_t d = i % D;
    T av[W], mv[W], ov[W];
    ld<T, W>(a, i, av);
    ld<T, W>(mask, d, mv);
#pragma unroll
    for (int j = 0; j < W; ++j) ov[j] = flow_split_mask(mv[j], av[j]);
    st<T, W>(out, i, ov);
  }
}

template <typename T, int W>
__global__ __launch_bounds__(kBlock) void k_merge_mask(const T* __restrict__ x, const T* __restrict__ mask,
                                                       const T* __restrict__ shift, T sign, T* __restrict__ y, int64_t n, int64_t D) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x * W;
  for (int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * W; i < n; i += stride) {
    const int64_t d = i % D;
    T xv[W], mv[W], sv[W], yv[W];
    ld<T, W>(x, i, xv);
    ld<T, W>(mask, d, mv);
    ld<T, W>(shift, i, sv);
#pragma unroll
    for (int j = 0; j < W; ++j) yv[j] = flow_merge_mask(mv[j], xv[j], sv[j], sign);
    st<T, W>(y, i, yv);
  }
}

template <typename T, int W>
__global__ __launch_bounds__(kBlock) void k_merge_mask_bwd(const T* __restrict__ gy, const T* __restrict__ mask, T sign,
                                                           T* __restrict__ gx, T* __restrict__ gshift, int64_t n, int64_t D) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x * W;
  for (int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * W; i < n; i += stride) {
    const int64_t d = i % D;
    T gv[W], mv[W], xv[W], sv[W];
    ld<T, W>(gy, i, gv);
    ld<T, W>(mask, d, mv);
#pragma unroll
    for (int j = 0; j < W; ++j) flow_merge_mask_bwd(mv[j], gv[j], sign, xv[j], sv[j]);
    st<T, W>(gx, i, xv);
    st<T, W>(gshift, i, sv);
  }
}

// ---------------------------------------------------------------------------------------------- coupling, INTERLEAVE
// One thread per PAIR of columns (b, j): n = B * D/2 pairs; the pair of x is two consecutive elements.
template <typename T>
__global__ __launch_bounds__(kBlock) void k_split_pairs(const T* __restrict__ x, T* __restrict__ out, int64_t n, int sel) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += stride) out[p] = x[flow_pair_column(p, sel)];
}
template <typename T>
__global__ __launch_bounds__(kBlock) void k_split_pairs_bwd(const T* __restrict__ g, T* __restrict__ gx, int64_t n, int sel) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += stride) {
    gx[flow_pair_column(p, sel)] = g[p];
    gx[flow_pair_column(p, 1 - sel)] = (T)0;
  }
}
template <typename T>
__global__ __launch_bounds__(kBlock) void k_merge_pairs(const T* __restrict__ x, const T* __restrict__ shift, T sign,
                                                        T* __restrict__ y, int64_t n, int sel) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += stride) {
    const int64_t off = flow_pair_column(p, sel), on = flow_pair_column(p, 1 - sel);
    const T xo = x[off], xn = x[on];
    y[off] = xo;
    y[on] = flow_shift_add(xn, shift[p], sign);
  }
}
template <typename T>
__global__ __launch_bounds__(kBlock) void k_merge_pairs_bwd(const T* __restrict__ gy, T sign, T* __restrict__ gx,
                                                            T* __restrict__ gshift, int64_t n, int sel) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += stride) {
    const int64_t off = flow_pair_column(p, sel), on = flow_pair_column(p, 1 - sel);
    const T go = gy[off], gn = gy[on];
    gx[off] = go;
    gx[on] = gn;
    gshift[p] = sign * gn;
  }
}

// ---------------------------------------------------------------------------------------------- Scaling (column tiles)
// blockDim = (ZS_FLOW_COL_TILE, ZS_FLOW_ROW_LANES); workgroup t owns columns [64 t, 64 t + 64).
template <typename T>
__global__ __launch_bounds__(ZS_FLOW_COL_TILE * ZS_FLOW_ROW_LANES) void k_scale_fwd(const T* x, const T* __restrict__ log_scale, T sign,
                                                                                    T* y, T* __restrict__ logdet, int64_t B, int64_t D) {
  __shared__ T red[ZS_FLOW_COL_TILE * ZS_FLOW_ROW_LANES];
  const int c = threadIdx.x, r = threadIdx.y;
  const int64_t d = (int64_t)blockIdx.x * ZS_FLOW_COL_TILE + c;
  if (d < D) {
    const T f = flow_scale_factor(log_scale[d], sign);
    for (int64_t b = r; b < B; b += ZS_FLOW_ROW_LANES) {
      const int64_t i = flow_at(b, d, D);
      y[i] = flow_mul(x[i], f);
    }
  }
  if (blockIdx.x == 0) {
    // logdet = sum_d log_scale[d]: thread t adds elements t, t + 1024, ... ascending; a tree over the 1024 partial sums
    const int t = r * ZS_FLOW_COL_TILE + c;
    constexpr int N = ZS_FLOW_COL_TILE * ZS_FLOW_ROW_LANES;
    T acc = (T)0;
    for (int64_t k = t; k < D; k += N) acc += log_scale[k];
    red[t] = acc;
    __syncthreads();
    for (int o = N / 2; o > 0; o >>= 1) {
      if (t < o) red[t] += red[t + o];
      __syncthreads();
    }
    if (t == 0) logdet[0] = red[0];
  }
}

template <typename T>
__global__ __launch_bounds__(ZS_FLOW_COL_TILE * ZS_FLOW_ROW_LANES) void k_scale_bwd(const T* gy, const T* __restrict__ y,
                                                                                    const T* __restrict__ log_scale,
                                                                                    const T* __restrict__ g_logdet, T sign, T* gx,
                                                                                    T* __restrict__ g_log_scale, int64_t B, int64_t D) {
  __shared__ T red[ZS_FLOW_ROW_LANES][ZS_FLOW_COL_TILE];
  const int c = threadIdx.x, r = threadIdx.y;
  const int64_t d = (int64_t)blockIdx.x * ZS_FLOW_COL_TILE + c;
  T acc = (T)0;
  if (d < D) {
    const T f = flow_scale_factor(log_scale[d], sign);
    for (int64_t b = r; b < B; b += ZS_FLOW_ROW_LANES) {
      const int64_t i = flow_at(b, d, D);
      const T g = gy[i];
      acc = flow_add(acc, flow_mul(g, y[i]));          // (no fma: zs_flow_math.h)
      gx[i] = flow_mul(g, f);
    }
  }
  red[r][c] = acc;
  __syncthreads();
  if (r == 0 && d < D) {
    T s = red[0][c];
#pragma unroll
    for (int k = 1; k < ZS_FLOW_ROW_LANES; ++k) s += red[k][c];
    g_log_scale[d] = flow_scale_gls(sign, s, g_logdet ? g_logdet[0] : (T)0);
  }
}

// ---------------------------------------------------------------------------------------------- MADE's affine
template <typename T, int W>
__global__ __launch_bounds__(kBlock) void k_made_fwd(const T* __restrict__ x, const T* __restrict__ net, T* __restrict__ u,
                                                     T* __restrict__ logdet, int64_t n, int64_t D) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x * W;
  for (int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * W; i < n; i += stride) {
    const int64_t b = i / D, d = i - b * D;
    T xv[W], mv[W], av[W], uv[W], lv[W];
    ld<T, W>(x, i, xv);
    ld<T, W>(net, flow_made_m_at(b, d, D), mv);
    ld<T, W>(net, flow_made_loga_at(b, d, D), av);
#pragma unroll
    for (int j = 0; j < W; ++j) {
      uv[j] = flow_made_u(xv[j], mv[j], av[j]);
      lv[j] = -av[j];
    }
    st<T, W>(u, i, uv);
    st<T, W>(logdet, i, lv);
  }
}

template <typename T, int W>
__global__ __launch_bounds__(kBlock) void k_made_bwd(const T* __restrict__ gu, const T* __restrict__ gld, const T* __restrict__ x,
                                                     const T* __restrict__ net, T* __restrict__ gx, T* __restrict__ gnet, int64_t n,
                                                     int64_t D) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x * W;
  for (int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * W; i < n; i += stride) {
    const int64_t b = i / D, d = i - b * D;
    const int64_t im = flow_made_m_at(b, d, D), ia = flow_made_loga_at(b, d, D);
    T guv[W], glv[W], xv[W], mv[W], av[W], gxv[W], gmv[W], gav[W];
#pragma unroll
    for (int j = 0; j < W; ++j) guv[j] = glv[j] = (T)0;
    if (gu) ld<T, W>(gu, i, guv);
    if (gld) ld<T, W>(gld, i, glv);
    ld<T, W>(x, i, xv);
    ld<T, W>(net, im, mv);
    ld<T, W>(net, ia, av);
#pragma unroll
    for (int j = 0; j < W; ++j) flow_made_bwd(guv[j], glv[j], xv[j], mv[j], av[j], gxv[j], gmv[j], gav[j]);
    st<T, W>(gx, i, gxv);
    st<T, W>(gnet, im, gmv);
    st<T, W>(gnet, ia, gav);
  }
}

template <typename T>
__global__ __launch_bounds__(kBlock) void k_made_inv_col(const T* __restrict__ u, const T* __restrict__ net, T* __restrict__ x,
                                                         int64_t B, int64_t D, int64_t col) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; b < B; b += stride) {
    const int64_t i = flow_at(b, col, D);
    x[i] = flow_made_inv(u[i], net[flow_made_m_at(b, col, D)], net[flow_made_loga_at(b, col, D)]);
  }
}

// ---------------------------------------------------------------------------------------------- FlowDistribution tail
// one wavefront per row, kBlock / 64 rows per workgroup
template <typename T>
__global__ __launch_bounds__(kBlock) void k_tail(int base, const T* __restrict__ z, const T* __restrict__ loc,
                                                 const T* __restrict__ scale, int param_rows, const T* __restrict__ logdet,
                                                 int logdet_kind, T* __restrict__ out, int64_t B, int64_t D) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t wstride = (int64_t)gridDim.x * (kBlock / 64);
  for (int64_t b = (int64_t)blockIdx.x * (kBlock / 64) + wave; b < B; b += wstride) {
    T acc = (T)0;
    for (int64_t d = lane; d < D; d += 64) {
      const int64_t i = flow_at(b, d, D), ip = param_rows ? i : d;
      acc = flow_add(acc, flow_base_lp(base, z[i], loc[ip], scale[ip]));
    }
    acc = group_sum(acc, ZS_WAVE);
    if (lane == 0) {
      if (logdet_kind == ZS_FLOW_LOGDET_SCALAR) acc += logdet[0];
      else if (logdet_kind == ZS_FLOW_LOGDET_ROWS) acc += logdet[b];
      out[b] = acc;
    }
  }
}

template <typename T, int W>
__global__ __launch_bounds__(kBlock) void k_tail_bwd(int base, const T* __restrict__ g, const T* __restrict__ z,
                                                     const T* __restrict__ loc, const T* __restrict__ scale, int param_rows,
                                                     T* __restrict__ gz, T* __restrict__ g_logdet, int64_t n, int64_t D) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x * W;
  for (int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * W; i < n; i += stride) {
    const int64_t b = i / D, d = i - b * D;
    const T gb = g[b];
    T zv[W], lv[W], sv[W], ov[W];
    ld<T, W>(z, i, zv);
    ld<T, W>(loc, param_rows ? i : d, lv);
    ld<T, W>(scale, param_rows ? i : d, sv);
#pragma unroll
    for (int j = 0; j < W; ++j) ov[j] = flow_mul(gb, flow_base_dz(base, zv[j], lv[j], sv[j]));
    st<T, W>(gz, i, ov);
    if (g_logdet && d == 0) g_logdet[b] = gb;
  }
}

// ---------------------------------------------------------------------------------------------- host side
#define ZS_FLOW_FLAT(KERN, vec, n, st, ...)                                                                      \
  do {                                                                                                           \
    if (vec)                                                                                                     \
      hipLaunchKernelGGL((KERN<T, 4>), dim3(flat_grid(((n) + 3) / 4)), dim3(kBlock), 0, st, __VA_ARGS__);        \
    else                                                                                                         \
      hipLaunchKernelGGL((KERN<T, 1>), dim3(flat_grid(n)), dim3(kBlock), 0, st, __VA_ARGS__);                    \
  } while (0)

bool bad_sizes(int64_t B, int64_t D) { return B < 0 || D < 0; }
// B * D must stay a valid flat index
bool too_large(int64_t B, int64_t D) { return B > 0 && D > 0 && D > (INT64_MAX / 4) / B; }

template <typename T>
int split(bool bwd, int mode, const void* a, const void* mask, void* out, int64_t B, int64_t D, int sel, void* stream) {
  if (mode != ZS_FLOW_MASK && mode != ZS_FLOW_INTERLEAVE) return ZS_EINVAL;
  if (bad_sizes(B, D) || !a || !out) return ZS_EINVAL;
  if (mode == ZS_FLOW_MASK && !mask) return ZS_EINVAL;
  if (mode == ZS_FLOW_INTERLEAVE && ((D & 1) || (sel != 0 && sel != 1))) return ZS_EINVAL;
  if (too_large(B, D)) return ZS_ENOTSUP;
  if (B == 0 || D == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  const int64_t n = B * D;
  if (mode == ZS_FLOW_MASK) {
    const bool vec = (D & 3) == 0 && aligned4<T>(a) && aligned4<T>(mask) && aligned4<T>(out);
    ZS_FLOW_FLAT(k_mask_mul, vec, n, st, (const T*)a, (const T*)mask, (T*)out, n, D);
  } else if (!bwd) {
    hipLaunchKernelGGL((k_split_pairs<T>), dim3(flat_grid(n / 2)), dim3(kBlock), 0, st, (const T*)a, (T*)out, n / 2, sel);
  } else {
    hipLaunchKernelGGL((k_split_pairs_bwd<T>), dim3(flat_grid(n / 2)), dim3(kBlock), 0, st, (const T*)a, (T*)out, n / 2, sel);
  }
  ZS_FLOW_CHECK_LAUNCH();
  return 0;
}

template <typename T>
int merge(int mode, const void* x, const void* mask, const void* shift, double sign, void* y, int64_t B, int64_t D, int sel,
          void* stream) {
  if (mode != ZS_FLOW_MASK && mode != ZS_FLOW_INTERLEAVE) return ZS_EINVAL;
  if (bad_sizes(B, D) || !x || !shift || !y) return ZS_EINVAL;
  if (mode == ZS_FLOW_MASK && !mask) return ZS_EINVAL;
  if (mode == ZS_FLOW_INTERLEAVE && ((D & 1) || (sel != 0 && sel != 1))) return ZS_EINVAL;
  if (too_large(B, D)) return ZS_ENOTSUP;
  if (B == 0 || D == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  const int64_t n = B * D;
  if (mode == ZS_FLOW_MASK) {
    const bool vec = (D & 3) == 0 && aligned4<T>(x) && aligned4<T>(mask) && aligned4<T>(shift) && aligned4<T>(y);
    ZS_FLOW_FLAT(k_merge_mask, vec, n, st, (const T*)x, (const T*)mask, (const T*)shift, (T)sign, (T*)y, n, D);
  } else {
    hipLaunchKernelGGL((k_merge_pairs<T>), dim3(flat_grid(n / 2)), dim3(kBlock), 0, st, (const T*)x, (const T*)shift, (T)sign,
                       (T*)y, n / 2, sel);
  }
  ZS_FLOW_CHECK_LAUNCH();
  return 0;
}

template <typename T>
int merge_bwd(int mode, const void* gy, const void* mask, double sign, void* gx, void* gshift, int64_t B, int64_t D, int sel,
              void* stream) {
  if (mode != ZS_FLOW_MASK && mode != ZS_FLOW_INTERLEAVE) return ZS_EINVAL;
  if (bad_sizes(B, D) || !gy || !gx || !gshift) return ZS_EINVAL;
  if (mode == ZS_FLOW_MASK && !mask) return ZS_EINVAL;
  if (mode == ZS_FLOW_INTERLEAVE && ((D & 1) || (sel != 0 && sel != 1))) return ZS_EINVAL;
  if (too_large(B, D)) return ZS_ENOTSUP;
  if (B == 0 || D == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  const int64_t n = B * D;
  if (mode == ZS_FLOW_MASK) {
    const bool vec = (D & 3) == 0 && aligned4<T>(gy) && aligned4<T>(mask) && aligned4<T>(gx) && aligned4<T>(gshift);
    ZS_FLOW_FLAT(k_merge_mask_bwd, vec, n, st, (const T*)gy, (const T*)mask, (T)sign, (T*)gx, (T*)gshift, n, D);
  } else {
    hipLaunchKernelGGL((k_merge_pairs_bwd<T>), dim3(flat_grid(n / 2)), dim3(kBlock), 0, st, (const T*)gy, (T)sign, (T*)gx,
                       (T*)gshift, n / 2, sel);
  }
  ZS_FLOW_CHECK_LAUNCH();
  return 0;
}

unsigned col_tiles(int64_t D) { return (unsigned)((D + ZS_FLOW_COL_TILE - 1) / ZS_FLOW_COL_TILE); }

template <typename T>
int scale_fwd(const void* x, const void* log_scale, double sign, void* y, void* logdet, int64_t B, int64_t D, void* stream) {
  if (bad_sizes(B, D) || !x || !log_scale || !y || !logdet) return ZS_EINVAL;
  if (too_large(B, D) || D > (int64_t)ZS_FLOW_COL_TILE * 0x7fffffff) return ZS_ENOTSUP;
  if (B == 0 || D == 0) return 0;
  hipLaunchKernelGGL((k_scale_fwd<T>), dim3(col_tiles(D)), dim3(ZS_FLOW_COL_TILE, ZS_FLOW_ROW_LANES), 0, (hipStream_t)stream,
                     (const T*)x, (const T*)log_scale, (T)sign, (T*)y, (T*)logdet, B, D);
  ZS_FLOW_CHECK_LAUNCH();
  return 0;
}

template <typename T>
int scale_bwd(const void* gy, const void* y, const void* log_scale, const void* g_logdet, double sign, void* gx, void* g_log_scale,
              int64_t B, int64_t D, void* stream) {
  if (bad_sizes(B, D) || !gy || !y || !log_scale || !gx || !g_log_scale) return ZS_EINVAL;
  if (too_large(B, D) || D > (int64_t)ZS_FLOW_COL_TILE * 0x7fffffff) return ZS_ENOTSUP;
  if (B == 0 || D == 0) return 0;
  hipLaunchKernelGGL((k_scale_bwd<T>), dim3(col_tiles(D)), dim3(ZS_FLOW_COL_TILE, ZS_FLOW_ROW_LANES), 0, (hipStream_t)stream,
                     (const T*)gy, (const T*)y, (const T*)log_scale, (const T*)g_logdet, (T)sign, (T*)gx, (T*)g_log_scale, B, D);
  ZS_FLOW_CHECK_LAUNCH();
  return 0;
}

template <typename T>
int made_fwd(const void* x, const void* net, void* u, void* logdet, int64_t B, int64_t D, void* stream) {
  if (bad_sizes(B, D) || !x || !net || !u || !logdet) return ZS_EINVAL;
  if (too_large(B, 2 * D)) return ZS_ENOTSUP;
  if (B == 0 || D == 0) return 0;
  const int64_t n = B * D;
  const bool vec = (D & 3) == 0 && aligned4<T>(x) && aligned4<T>(net) && aligned4<T>(u) && aligned4<T>(logdet);
  ZS_FLOW_FLAT(k_made_fwd, vec, n, (hipStream_t)stream, (const T*)x, (const T*)net, (T*)u, (T*)logdet, n, D);
  ZS_FLOW_CHECK_LAUNCH();
  return 0;
}

template <typename T>
int made_bwd(const void* gu, const void* gld, const void* x, const void* net, void* gx, void* gnet, int64_t B, int64_t D,
             void* stream) {
  if (bad_sizes(B, D) || (!gu && !gld) || !x || !net || !gx || !gnet) return ZS_EINVAL;
  if (too_large(B, 2 * D)) return ZS_ENOTSUP;
  if (B == 0 || D == 0) return 0;
  const int64_t n = B * D;
  const bool vec = (D & 3) == 0 && aligned4<T>(gu) && aligned4<T>(gld) && aligned4<T>(x) && aligned4<T>(net) && aligned4<T>(gx) &&
                   aligned4<T>(gnet);
  ZS_FLOW_FLAT(k_made_bwd, vec, n, (hipStream_t)stream, (const T*)gu, (const T*)gld, (const T*)x, (const T*)net, (T*)gx, (T*)gnet,
               n, D);
  ZS_FLOW_CHECK_LAUNCH();
  return 0;
}

template <typename T>
int made_inv_col(const void* u, const void* net, void* x, int64_t B, int64_t D, int64_t col, void* stream) {
  if (bad_sizes(B, D) || !u || !net || !x) return ZS_EINVAL;
  if (too_large(B, 2 * D)) return ZS_ENOTSUP;
  if (B == 0 || D == 0) return 0;
  if (col < 0 || col >= D) return ZS_EINVAL;
  hipLaunchKernelGGL((k_made_inv_col<T>), dim3(flat_grid(B)), dim3(kBlock), 0, (hipStream_t)stream, (const T*)u, (const T*)net,
                     (T*)x, B, D, col);
  ZS_FLOW_CHECK_LAUNCH();
  return 0;
}

bool bad_tail(int base, int param_rows) {
  return (base != ZS_FLOW_NORMAL && base != ZS_FLOW_LOGISTIC) || (param_rows != 0 && param_rows != 1);
}

template <typename T>
int tail(int base, const void* z, const void* loc, const void* scale, int param_rows, const void* logdet, int logdet_kind, void* out,
         int64_t B, int64_t D, void* stream) {
  if (bad_tail(base, param_rows) || logdet_kind < ZS_FLOW_LOGDET_NONE || logdet_kind > ZS_FLOW_LOGDET_ROWS) return ZS_EINVAL;
  if (bad_sizes(B, D) || !z || !loc || !scale || !out || (logdet_kind != ZS_FLOW_LOGDET_NONE && !logdet)) return ZS_EINVAL;
  if (too_large(B, D)) return ZS_ENOTSUP;
  if (B == 0 || D == 0) return 0;
  const int rows = kBlock / 64;
  hipLaunchKernelGGL((k_tail<T>), dim3(flat_grid((B + rows - 1) / rows * kBlock)), dim3(kBlock), 0, (hipStream_t)stream, base,
                     (const T*)z, (const T*)loc, (const T*)scale, param_rows, (const T*)logdet, logdet_kind, (T*)out, B, D);
  ZS_FLOW_CHECK_LAUNCH();
  return 0;
}

template <typename T>
int tail_bwd(int base, const void* g, const void* z, const void* loc, const void* scale, int param_rows, void* gz, void* g_logdet,
             int64_t B, int64_t D, void* stream) {
  if (bad_tail(base, param_rows)) return ZS_EINVAL;
  if (bad_sizes(B, D) || !g || !z || !loc || !scale || !gz) return ZS_EINVAL;
  if (too_large(B, D)) return ZS_ENOTSUP;
  if (B == 0 || D == 0) return 0;
  const int64_t n = B * D;
  const bool vec = (D & 3) == 0 && aligned4<T>(z) && aligned4<T>(loc) && aligned4<T>(scale) && aligned4<T>(gz);
  ZS_FLOW_FLAT(k_tail_bwd, vec, n, (hipStream_t)stream, base, (const T*)g, (const T*)z, (const T*)loc, (const T*)scale, param_rows,
               (T*)gz, (T*)g_logdet, n, D);
  ZS_FLOW_CHECK_LAUNCH();
  return 0;
}

}  // namespace

extern "C" int zs_flow_abi_version(void) { return ZS_FLOW_ABI_VERSION; }

#define ZS_FLOW_DEFINE(SFX, T)                                                                                                 \
  extern "C" int zs_flow_split_##SFX(int mode, const void* x, const void* mask, void* out, int64_t B, int64_t D, int sel,     \
                                     void* stream) {                                                                           \
    return split<T>(false, mode, x, mask, out, B, D, sel, stream);                                                             \
  }                                                                                                                            \
  extern "C" int zs_flow_split_bwd_##SFX(int mode, const void* g_out, const void* mask, void* gx, int64_t B, int64_t D,       \
                                         int sel, void* stream) {                                                              \
    return split<T>(true, mode, g_out, mask, gx, B, D, sel, stream);                                                           \
  }                                                                                                                            \
  extern "C" int zs_flow_merge_##SFX(int mode, const void* x, const void* mask, const void* shift, double sign, void* y,      \
                                     int64_t B, int64_t D, int sel, void* stream) {                                            \
    return merge<T>(mode, x, mask, shift, sign, y, B, D, sel, stream);                                                         \
  }                                                                                                                            \
  extern "C" int zs_flow_merge_bwd_##SFX(int mode, const void* gy, const void* mask, double sign, void* gx, void* gshift,     \
                                         int64_t B, int64_t D, int sel, void* stream) {                                        \
    return merge_bwd<T>(mode, gy, mask, sign, gx, gshift, B, D, sel, stream);                                                  \
  }                                                                                                                            \
  extern "C" int zs_flow_scale_fwd_##SFX(const void* x, const void* log_scale, double sign, void* y, void* logdet, int64_t B, \
                                         int64_t D, void* stream) {                                                            \
    return scale_fwd<T>(x, log_scale, sign, y, logdet, B, D, stream);                                                          \
  }                                                                                                                            \
  extern "C" int zs_flow_scale_bwd_##SFX(const void* gy, const void* y, const void* log_scale, const void* g_logdet,          \
                                         double sign, void* gx, void* g_log_scale, int64_t B, int64_t D, void* stream) {       \
    return scale_bwd<T>(gy, y, log_scale, g_logdet, sign, gx, g_log_scale, B, D, stream);                                      \
  }                                                                                                                            \
  extern "C" int zs_flow_made_fwd_##SFX(const void* x, const void* net, void* u, void* logdet, int64_t B, int64_t D,          \
                                        void* stream) {                                                                        \
    return made_fwd<T>(x, net, u, logdet, B, D, stream);                                                                       \
  }                                                                                                                            \
  extern "C" int zs_flow_made_bwd_##SFX(const void* gu, const void* gld, const void* x, const void* net, void* gx,            \
                                        void* gnet, int64_t B, int64_t D, void* stream) {                                      \
    return made_bwd<T>(gu, gld, x, net, gx, gnet, B, D, stream);                                                               \
  }                                                                                                                            \
  extern "C" int zs_flow_made_inv_col_##SFX(const void* u, const void* net, void* x, int64_t B, int64_t D, int64_t col,       \
                                            void* stream) {                                                                    \
    return made_inv_col<T>(u, net, x, B, D, col, stream);                                                                      \
  }                                                                                                                            \
  extern "C" int zs_flow_tail_##SFX(int base, const void* z, const void* loc, const void* scale, int param_rows,              \
                                    const void* logdet, int logdet_kind, void* out, int64_t B, int64_t D, void* stream) {      \
    return tail<T>(base, z, loc, scale, param_rows, logdet, logdet_kind, out, B, D, stream);                                   \
  }                                                                                                                            \
  extern "C" int zs_flow_tail_bwd_##SFX(int base, const void* g, const void* z, const void* loc, const void* scale,           \
                                        int param_rows, void* gz, void* g_logdet, int64_t B, int64_t D, void* stream) {        \
    return tail_bwd<T>(base, g, z, loc, scale, param_rows, gz, g_logdet, B, D, stream);                                        \
  }

ZS_FLOW_DEFINE(f32, float)
ZS_FLOW_DEFINE(f64, double)
