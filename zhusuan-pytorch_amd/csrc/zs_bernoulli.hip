// Bernoulli kernels (K3, K5) for gfx950.  K3 is the byte-dominant kernel of the VAE / IWAE
// objectives: it streams p[K, B, 784] once (16 B per lane, four independent loads in flight per
// lane), re-reads the observation row x[b, :] from L2, and reduces each row on the wavefront.
#include "zs_common.h"
#include "zs_iw1_args.h"
#include "zs_iwpersist.h"
#include "zs_sample_tile.h"
#include "../../include/zs_hip.h"
#include <stdlib.h>

using namespace zs;

namespace {

__device__ __forceinline__ float bern_row_terms(const float4& pv, const float4& xv) {
  return bern_lp2_term(pv.x, xv.x) + bern_lp2_term(pv.y, xv.y) + bern_lp2_term(pv.z, xv.z) +
         bern_lp2_term(pv.w, xv.w);
}

// The streamed operand read with the non-temporal hint.  Forward (read-only stream): pays at every size of the
// shared-observation kernel.  Backward (a read and a write stream): only far beyond the 256 MB Infinity Cache (6.6 GB of p:
// 63 -> 67 % of the roofline; 0.8-3.2 GB: 72 -> 65 %), so the host asks for it above 4 GB.
template <bool NTL>
__device__ __forceinline__ float4 ld_stream(const float4* __restrict__ q) {
  if (NTL) {
    const zs_f4v v = __builtin_nontemporal_load(reinterpret_cast<const zs_f4v*>(q));
    return make_float4(v.x, v.y, v.z, v.w);
  }
  return *q;
}

// ------------------------------------------------------------------------------------
// K3 forward.  One wave handles `rpw` rows per pass with G lanes per row; for long rows
// (D4 > 64, e.g. 784 pixels = 196 float4) G = 64 and the four chunk loads of a lane are issued
// back to back before any arithmetic.  LOGITS: the streamed operand holds logits and
// p = sigmoid(logit) is formed in registers (optionally stored to probs_out).
// ------------------------------------------------------------------------------------
template <bool LOGITS, bool WRITE_P>
__global__ __launch_bounds__(256) void k_bern_logprob_rows(
    const float4* __restrict__ p, const float4* __restrict__ x, int64_t xrows, float* __restrict__ lp,
    float4* __restrict__ probs_out, int64_t K, int64_t R, int D4, int G, int rpw, int p2,
    int64_t sk, int64_t sr) {
  const int lane = threadIdx.x & 63;
  const int rw = lane / G, lig = lane - rw * G;
  const bool lane_on = rw < rpw;
  const int64_t rows = K * R;
  const int64_t tiles = (rows + rpw - 1) / rpw;
  const int64_t nwaves = (int64_t)gridDim.x * (blockDim.x >> 6);
  for (int64_t t = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); t < tiles; t += nwaves) {
    const int64_t row = t * rpw + rw;
    const bool on = lane_on && row < rows;
    float acc = 0.f;
    if (on) {
      const float4* __restrict__ prow = p + row * D4;
      const float4* __restrict__ xrow = x + (xrows == rows ? row : mod_fast(row, xrows)) * D4;
      float4* __restrict__ orow = WRITE_P ? probs_out + row * D4 : nullptr;
      for (int c0 = lig; c0 < D4; c0 += 4 * G) {
        float4 pv[4], xv[4];
        bool ok[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int c = c0 + u * G;
          ok[u] = c < D4;
          if (ok[u]) {
            pv[u] = prow[c];
            xv[u] = xrow[c];
          }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          if (ok[u]) {
            if (LOGITS) {
              pv[u].x = sigmoid_fast(pv[u].x);
              pv[u].y = sigmoid_fast(pv[u].y);
              pv[u].z = sigmoid_fast(pv[u].z);
              pv[u].w = sigmoid_fast(pv[u].w);
              if (WRITE_P) orow[c0 + u * G] = pv[u];
            }
            acc += bern_row_terms(pv[u], xv[u]);
          }
        }
      }
    }
    acc = group_sum_down(acc, lig, G, p2);
    if (on && lig == 0) {
      int64_t k, r;
      divmod(row, R, k, r);
      lp[k * sk + r * sr] = acc * ZS_LN2;
    }
  }
}

// ------------------------------------------------------------------------------------
// K3 forward, long rows (D4 >= 64; the 784-pixel case is D4 = 196): one wave per row, every lane
// issues its (up to) four 16-B loads of p and of x back to back, then does the arithmetic; the row
// is reduced with a 6-step __shfl_xor butterfly.  Measured on MI355X in isolation at the config-3
// size (12800 rows, 41 MB): 7.2 us = 5.7 TB/s; a plain float4 read of the same bytes takes 6.1 us.
// ------------------------------------------------------------------------------------
template <bool LOGITS, bool WRITE_P>
__global__ __launch_bounds__(256) void k_bern_logprob_longrow(
    const float4* __restrict__ p, const float4* __restrict__ x, int64_t xrows, float* __restrict__ lp,
    float4* __restrict__ probs_out, int64_t rows, int64_t R, int D4, int64_t sk, int64_t sr) {
  const int lane = threadIdx.x & 63;
  const int64_t nwaves = (int64_t)gridDim.x * 4;
  for (int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); row < rows; row += nwaves) {
    const float4* __restrict__ prow = p + row * D4;
    const float4* __restrict__ xrow = x + (xrows == rows ? row : mod_fast(row, xrows)) * D4;
    float acc = 0.f;
    for (int c0 = lane; c0 < D4; c0 += 256) {
      float4 pv[4], xv[4];
      bool ok[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int c = c0 + 64 * u;
        ok[u] = c < D4;
        if (ok[u]) {
          pv[u] = prow[c];
          xv[u] = xrow[c];
        }
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        if (ok[u]) {
          if (LOGITS) {
            pv[u].x = sigmoid_fast(pv[u].x);
            pv[u].y = sigmoid_fast(pv[u].y);
            pv[u].z = sigmoid_fast(pv[u].z);
            pv[u].w = sigmoid_fast(pv[u].w);
            if (WRITE_P) probs_out[row * D4 + c0 + 64 * u] = pv[u];
          }
          acc += bern_row_terms(pv[u], xv[u]);
        }
      }
    }
    acc = wave_sum(acc);
    if (lane == 0) {
      int64_t k, r;
      divmod(row, R, k, r);
      lp[k * sk + r * sr] = acc * ZS_LN2;
    }
  }
}

// The same mapping with the row's coordinates taken from the block indices: grid = (ceil(R / 4), K), wave w of workgroup
// (bx, k) owns row (k, r = 4 bx + w).  The grid-stride form above keeps the row index in vector registers and divides it per
// lane -- divmod(row, R) for the output slot and mod_fast(row, xrows) for the observation row: 23 v_mul_lo_u32, 15
// v_mad_u64_u32, 10 v_mul_hi_u32, 16 conversions and two v_rcp_iflag of the kernel's 430 VALU instructions per 784-float row
// (VERDICT r03, weak 3).  Here nothing is divided: used whenever every row gets a wave of its own and the observation is
// either shared by the particles (xrows == R) or full-size.
template <bool LOGITS, bool WRITE_P>
__global__ __launch_bounds__(256) void k_bern_logprob_longrow2d(
    const float4* __restrict__ p, const float4* __restrict__ x, int x_full, float* __restrict__ lp,
    float4* __restrict__ probs_out, int64_t R, int D4, int64_t sk, int64_t sr) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int64_t k = blockIdx.y;
  if (r >= R) return;                                             // (r is wave-uniform: whole waves leave)
  const int64_t row = k * R + r;
  const float4* __restrict__ prow = p + row * D4;
  const float4* __restrict__ xrow = x + (x_full ? row : r) * D4;
  float acc = 0.f;
  float4 pv[4], xv[4];
  bool ok[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int c = lane + 64 * u;
    ok[u] = c < D4;
    if (ok[u]) {
      pv[u] = prow[c];
      xv[u] = xrow[c];
    }
  }
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    if (ok[u]) {
      if (LOGITS) {
        pv[u].x = sigmoid_fast(pv[u].x);
        pv[u].y = sigmoid_fast(pv[u].y);
        pv[u].z = sigmoid_fast(pv[u].z);
        pv[u].w = sigmoid_fast(pv[u].w);
        if (WRITE_P) probs_out[row * D4 + lane + 64 * u] = pv[u];
      }
      // (scalar arithmetic: the packed form of bern_piece_acc -- which pays in IW1, where a workgroup's share of rows is fixed --
      // was measured 0.8 us SLOWER in this kernel at the config size, 7.5 against 6.7 us: here the hardware scheduler evens out the
      // arithmetic over all SIMDs and the kernel is not bound by instruction issue)
      acc += bern_row_terms(pv[u], xv[u]);
    }
  }
  acc = wave_sum(acc);
  if (lane == 0) lp[k * sk + r * sr] = acc * ZS_LN2;
}

// K3 forward for big problems where the observation is shared by J = rows / xrows particles
// (x [B, X] against p [K, B, X]) and 64 < D <= 1024: a wave keeps its observation row in registers and
// streams JC particle rows past it (U of them in flight), which halves the load instructions per byte
// of p.  Measured: 6.1-6.3 TB/s at 321 MB and 5.8 TB/s at 2.6 GB, against 5.4 / 4.7 TB/s for one
// wave per row.
template <bool LOGITS, bool WRITE_P, int U, bool NTL>
__global__ __launch_bounds__(256) void k_bern_logprob_xreuse(
    const float4* __restrict__ p, const float4* __restrict__ x, int64_t xrows, int64_t J, int64_t JC,
    float* __restrict__ lp, float4* __restrict__ probs_out, int64_t R, int D4, int64_t sk, int64_t sr) {
  const int lane = threadIdx.x & 63;
  const int64_t jchunks = (J + JC - 1) / JC;
  const int64_t items = xrows * jchunks;
  const int64_t nwaves = (int64_t)gridDim.x * 4;
  for (int64_t it = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); it < items; it += nwaves) {
    int64_t jc, r0;
    divmod(it, xrows, jc, r0);   // neighbouring waves -> neighbouring rows of p
    const float4* __restrict__ xrow = x + r0 * D4;
    float4 xv[4];
    bool ok[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int c = lane + 64 * u;
      ok[u] = c < D4;
      xv[u] = ok[u] ? xrow[c] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    const int64_t j0 = jc * JC, j1 = (j0 + JC < J) ? j0 + JC : J;
    for (int64_t j = j0; j < j1; j += U) {
      float4 pv[U][4];
      bool live[U];
#pragma unroll
      for (int v = 0; v < U; ++v) {
        live[v] = j + v < j1;
        const float4* __restrict__ prow = p + ((j + v) * xrows + r0) * D4;
#pragma unroll
        for (int u = 0; u < 4; ++u)
          if (live[v] && ok[u]) pv[v][u] = ld_stream<NTL>(prow + lane + 64 * u);
      }
#pragma unroll
      for (int v = 0; v < U; ++v) {
        float acc = 0.f;
        const int64_t row = (j + v) * xrows + r0;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          if (live[v] && ok[u]) {
            if (LOGITS) {
              pv[v][u].x = sigmoid_fast(pv[v][u].x);
              pv[v][u].y = sigmoid_fast(pv[v][u].y);
              pv[v][u].z = sigmoid_fast(pv[v][u].z);
              pv[v][u].w = sigmoid_fast(pv[v][u].w);
              if (WRITE_P) probs_out[row * D4 + lane + 64 * u] = pv[v][u];
            }
            if (LOGITS && U == 1) {
              // the logits form with one row in flight (rows < 400 000) is the one variant of this kernel that gains from packed
              // fp32 terms: 131 k rows 57 -> 69 % of the roofline; with two rows in flight (1 M rows) it LOSES 3 points, the
              // probs form is indifferent (profiles/r04_k3_logits_packed.txt)
              zs_f2v t2 = {0.f, 0.f};
              bern_piece_acc(pv[v][u], xv[u], make_float4(1.0f - xv[u].x, 1.0f - xv[u].y, 1.0f - xv[u].z, 1.0f - xv[u].w), t2);
              acc += t2.x + t2.y;
            } else {
              acc += bern_row_terms(pv[v][u], xv[u]);
            }
          }
        }
        acc = wave_sum(acc);
        if (live[v] && lane == 0) {
          int64_t k = j + v, r = r0;                 // xrows == R: row (j + v) * R + r0 IS (k, r)
          if (xrows != R) divmod(row, R, k, r);
          lp[k * sk + r * sr] = acc * ZS_LN2;
        }
      }
    }
  }
}

template <bool LOGITS>
__global__ __launch_bounds__(256) void k_bern_logprob_serial(
    const float* __restrict__ p, const float* __restrict__ x, int64_t Px, float* __restrict__ lp,
    float* __restrict__ probs_out, int64_t K, int64_t R, int64_t D, int64_t sk, int64_t sr) {
  const int64_t rows = K * R;
  for (int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; row < rows;
       row += (int64_t)gridDim.x * blockDim.x) {
    float acc = 0.f;
    for (int64_t d = 0; d < D; ++d) {
      const int64_t i = row * D + d;
      float pv = p[i];
      if (LOGITS) {
        pv = sigmoid_fast(pv);
        if (probs_out) probs_out[i] = pv;
      }
      acc += bern_lp2_term(pv, x[mod_fast(i, Px)]);
    }
    int64_t k, r;
      divmod(row, R, k, r);
    lp[k * sk + r * sr] = acc * ZS_LN2;
  }
}

// ------------------------------------------------------------------------------------
// K3 backward: gp = glp[k, r] * (x/(p+e) - (1-x)/((1-p)+e))   [* p*(1-p) for logits]
// same row mapping as the forward; reads p and x, writes gp, 16 B per lane.
// ------------------------------------------------------------------------------------

// d/dp of the row term, x ra - (1 - x) rb, with its one fused multiply-add spelled out.  Left to the compiler (bern_dp,
// zs_elem_math.h) the two instantiations of k_bern_logprob_bwd_rows contracted different products -- the non-temporal one
// fma(-(1 - x), rb, x ra), the plain one fma(x, ra, -((1 - x) rb)) -- so a gradient changed in its last bits when the tensor
// outgrew the Infinity Cache (tests/test_size_gated_variants.py, bb-K50-R33555-D40).  This is the plain instantiation's form.
__device__ __forceinline__ float bern_dp_rows(float p, float x) {
  return fmaf(x, rcp_fast(p + ZS_BERN_EPS), -((1.0f - x) * rcp_fast((1.0f - p) + ZS_BERN_EPS)));
}

template <bool LOGITS, bool NT>
__global__ __launch_bounds__(256) void k_bern_logprob_bwd_rows(
    const float4* __restrict__ p, const float4* __restrict__ x, int64_t xrows,
    const float* __restrict__ glp, int64_t gsk, int64_t gsr, const float* __restrict__ gscale, int64_t gss,
    float4* __restrict__ gp, int64_t K, int64_t R, int D4, int G, int rpw) {
  const int lane = threadIdx.x & 63;
  const int rw = lane / G, lig = lane - rw * G;
  const bool lane_on = rw < rpw;
  const int64_t rows = K * R;
  const int64_t tiles = (rows + rpw - 1) / rpw;
  const int64_t nwaves = (int64_t)gridDim.x * (blockDim.x >> 6);
  for (int64_t t = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); t < tiles; t += nwaves) {
    const int64_t row = t * rpw + rw;
    if (!(lane_on && row < rows)) continue;
    int64_t k, r;
      divmod(row, R, k, r);
    float g = glp[k * gsk + r * gsr];
    if (gscale) g *= gscale[r * gss];
    const float4* __restrict__ prow = p + row * D4;
    const float4* __restrict__ xrow = x + (xrows == rows ? row : mod_fast(row, xrows)) * D4;
    float4* __restrict__ grow = gp + row * D4;
    for (int c0 = lig; c0 < D4; c0 += 4 * G) {
      float4 pv[4], xv[4];
      bool ok[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int c = c0 + u * G;
        ok[u] = c < D4;
        if (ok[u]) {
          pv[u] = prow[c];
          xv[u] = xrow[c];
        }
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        if (ok[u]) {
          float4 o;
          if (LOGITS) {
            const float a = sigmoid_fast(pv[u].x), b = sigmoid_fast(pv[u].y), c = sigmoid_fast(pv[u].z),
                        d = sigmoid_fast(pv[u].w);
            o.x = g * bern_dp_rows(a, xv[u].x) * a * (1.0f - a);
            o.y = g * bern_dp_rows(b, xv[u].y) * b * (1.0f - b);
            o.z = g * bern_dp_rows(c, xv[u].z) * c * (1.0f - c);
            o.w = g * bern_dp_rows(d, xv[u].w) * d * (1.0f - d);
          } else {
            o.x = g * bern_dp_rows(pv[u].x, xv[u].x);
            o.y = g * bern_dp_rows(pv[u].y, xv[u].y);
            o.z = g * bern_dp_rows(pv[u].z, xv[u].z);
            o.w = g * bern_dp_rows(pv[u].w, xv[u].w);
          }
          if (NT) {   // gradient tensors beyond the Infinity Cache: streaming (non-temporal) stores
            const zs_f4v v = {o.x, o.y, o.z, o.w};
            __builtin_nontemporal_store(v, reinterpret_cast<zs_f4v*>(&grow[c0 + u * G]));
          } else {
            grow[c0 + u * G] = o;
          }
        }
      }
    }
  }
}

// K3 backward, long rows, coordinates from the block indices (see k_bern_logprob_longrow2d): no division, the row's
// incoming gradient and its optional scale (the objective's incoming gradient, gscale[r * gss]) are scalar loads.
template <bool LOGITS, bool NT>
__global__ __launch_bounds__(256) void k_bern_logprob_bwd_longrow2d(
    const float4* __restrict__ p, const float4* __restrict__ x, int x_full,
    const float* __restrict__ glp, int64_t gsk, int64_t gsr, const float* __restrict__ gscale, int64_t gss,
    float4* __restrict__ gp, int64_t R, int D4) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int64_t k = blockIdx.y;
  if (r >= R) return;
  const int64_t row = k * R + r;
  const float4* __restrict__ prow = p + row * D4;
  const float4* __restrict__ xrow = x + (x_full ? row : r) * D4;
  float4* __restrict__ grow = gp + row * D4;
  float4 pv[4], xv[4];
  bool ok[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int c = lane + 64 * u;
    ok[u] = c < D4;
    if (ok[u]) {
      pv[u] = prow[c];
      xv[u] = xrow[c];
    }
  }
  float g = glp[k * gsk + r * gsr];
  if (gscale) g *= gscale[r * gss];
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    if (ok[u]) {
      const float4 o = bern_piece_grad<LOGITS>(pv[u], xv[u], g);          // packed fp32 (zs_elem_math.h)
      if (NT) {
        const zs_f4v v = {o.x, o.y, o.z, o.w};
        __builtin_nontemporal_store(v, reinterpret_cast<zs_f4v*>(&grow[lane + 64 * u]));
      } else {
        grow[lane + 64 * u] = o;
      }
    }
  }
}

// IW1's backward as ONE launch with two independent roles (no hand-off between them): plane y = 0 of the grid is the K-summed
// gradient of log q w.r.t. the variational node's parameters (K2's backward-ksum, 4 K-slices per workgroup: its dependent rounds
// of loads hide under the stream below -- it is dispatched first), planes y = 1 .. K are K3's backward, one wave per row with
// the row's coordinates taken from the block indices.  Both take their row gradients as coef[.][r, k] * gout[r * gss].
template <bool LOGITS, bool NT>
__global__ __launch_bounds__(256) void k_iw1_bwd(
    const float4* __restrict__ p, const float4* __restrict__ x, int x_full, const float* __restrict__ coef,
    const float* __restrict__ gout, int64_t gss, float4* __restrict__ gp, int64_t K, int64_t R, int D4,
    const float4* __restrict__ zq, const float4* __restrict__ qmu, const float4* __restrict__ qsigma, float4* __restrict__ gqmu,
    float4* __restrict__ gqsigma, int64_t Mq4, int Dq4, bool q_ls) {
  if (blockIdx.y == 0) {
    if ((int64_t)blockIdx.x * 64 < Mq4)
      logprob_bwd_ksum_body<D_NORMAL, 4>(blockIdx.x, zq, qmu, qsigma, coef + R * K, 1, K, nullptr, gqmu, gqsigma, K, Mq4, Dq4, q_ls,
                                         gout, gss);
    return;
  }
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int64_t k = blockIdx.y - 1;
  if (r >= R) return;
  const int64_t row = k * R + r;
  const float4* __restrict__ prow = p + row * D4;
  const float4* __restrict__ xrow = x + (x_full ? row : r) * D4;
  float4* __restrict__ grow = gp + row * D4;
  float4 pv[4], xv[4];
  bool ok[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int c = lane + 64 * u;
    ok[u] = c < D4;
    if (ok[u]) {
      pv[u] = prow[c];
      xv[u] = xrow[c];
    }
  }
  const float g = coef[r * K + k] * gout[r * gss];
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    if (ok[u]) {
      const float4 o = bern_piece_grad<LOGITS>(pv[u], xv[u], g);          // packed fp32 (zs_elem_math.h)
      if (NT) {
        const zs_f4v v = {o.x, o.y, o.z, o.w};
        __builtin_nontemporal_store(v, reinterpret_cast<zs_f4v*>(&grow[lane + 64 * u]));
      } else {
        grow[lane + 64 * u] = o;
      }
    }
  }
}

// K3 backward for big problems with a shared observation (same tiling as k_bern_logprob_xreuse): the wave keeps
// x[b, :] in registers, streams JC particle rows of p past it and writes the gradient rows, non-temporally when
// the tensor cannot stay in the Infinity Cache.
template <bool LOGITS, bool NT, int U, bool NTL>
__global__ __launch_bounds__(256) void k_bern_logprob_bwd_xreuse(
    const float4* __restrict__ p, const float4* __restrict__ x, int64_t xrows, int64_t J, int64_t JC,
    const float* __restrict__ glp, int64_t gsk, int64_t gsr, const float* __restrict__ gscale, int64_t gss,
    float4* __restrict__ gp, int64_t R, int D4) {
  (void)U;
  const int lane = threadIdx.x & 63;
  const int64_t jchunks = (J + JC - 1) / JC;
  const int64_t items = xrows * jchunks;
  const int64_t nwaves = (int64_t)gridDim.x * 4;
  // column of each of the lane's four 16-byte pieces, clamped into the row: every load is issued unconditionally (a
  // guarded load puts an exec-mask change -- and with it a wait for the previous load -- between two loads); only the
  // stores are predicated
  int col[4];
  bool ok[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int c = lane + 64 * u;
    ok[u] = c < D4;
    col[u] = ok[u] ? c : D4 - 1;
  }
  for (int64_t it = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); it < items; it += nwaves) {
    int64_t jc, r0;
    divmod(it, xrows, jc, r0);
    const float4* __restrict__ xrow = x + r0 * D4;
    float4 xv[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) xv[u] = xrow[col[u]];
    const int64_t j0 = jc * JC, j1 = (j0 + JC < J) ? j0 + JC : J;
    // rolling prefetch: the loads of particle row j + 1 are in flight while row j is computed and stored, so a wave
    // always has one row (3 KB at 784 pixels) outstanding
    float4 nx[4];
    float gn;
    {
      const int64_t row = j0 * xrows + r0;
      int64_t k = j0, r = r0;                       // xrows == R: row j * R + r0 IS (k, r)
      if (xrows != R) divmod(row, R, k, r);
      gn = glp[k * gsk + r * gsr];
      if (gscale) gn *= gscale[r * gss];
      const float4* __restrict__ prow = p + row * D4;
#pragma unroll
      for (int u = 0; u < 4; ++u) nx[u] = ld_stream<NTL>(prow + col[u]);
    }
    for (int64_t j = j0; j < j1; ++j) {
      float4 pv[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) pv[u] = nx[u];
      const float g = gn;
      const int64_t row = j * xrows + r0;
      {
        const int64_t jn = j + 1 < j1 ? j + 1 : j;                    // last iteration: a harmless re-read
        const int64_t rown = jn * xrows + r0;
        int64_t k = jn, r = r0;
        if (xrows != R) divmod(rown, R, k, r);
        gn = glp[k * gsk + r * gsr];
        if (gscale) gn *= gscale[r * gss];
        const float4* __restrict__ prow = p + rown * D4;
#pragma unroll
        for (int u = 0; u < 4; ++u) nx[u] = ld_stream<NTL>(prow + col[u]);
      }
      float4* __restrict__ grow = gp + row * D4;
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const float4 o = bern_piece_grad<LOGITS>(pv[u], xv[u], g);        // packed fp32 (zs_elem_math.h)
        if (ok[u]) {
          if (NT) {
            const zs_f4v vv = {o.x, o.y, o.z, o.w};
            __builtin_nontemporal_store(vv, reinterpret_cast<zs_f4v*>(&grow[lane + 64 * u]));
          } else {
            grow[lane + 64 * u] = o;
          }
        }
      }
    }
  }
}

template <bool LOGITS>
__global__ __launch_bounds__(256) void k_bern_logprob_bwd_serial(
    const float* __restrict__ p, const float* __restrict__ x, int64_t Px, const float* __restrict__ glp,
    int64_t gsk, int64_t gsr, const float* __restrict__ gscale, int64_t gss, float* __restrict__ gp, int64_t N, int64_t R,
    int64_t D) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t row = i / D;
    int64_t k, r;
      divmod(row, R, k, r);
    float g = glp[k * gsk + r * gsr];
    if (gscale) g *= gscale[r * gss];
    float pv = p[i];
    float scale = 1.0f;
    if (LOGITS) {
      pv = sigmoid_fast(pv);
      scale = pv * (1.0f - pv);
    }
    gp[i] = g * bern_dp(pv, x[mod_fast(i, Px)]) * scale;
  }
}

// K5: Bernoulli._sample -- out = (u < p), u ~ U(0,1) from Philox (bernoulli.py:80)
__global__ __launch_bounds__(256) void k_bern_sample(const float* __restrict__ p, int64_t Pp,
                                                     float* __restrict__ out, int64_t N, uint64_t seed,
                                                     uint64_t call, const uint64_t* __restrict__ rs) {
  if (rs) { seed = rs[0]; call += rs[1]; }
  const int64_t groups = (N + 3) / 4;
  for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += (int64_t)gridDim.x * blockDim.x) {
    const Philox4 r = philox4x32_10((uint64_t)g, call, seed);
    const float u[4] = {u01(r.x), u01(r.y), u01(r.z), u01(r.w)};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int64_t i = g * 4 + j;
      if (i < N) out[i] = u[j] < p[mod_fast(i, Pp)] ? 1.0f : 0.0f;
    }
  }
}

// Work items of the shared-observation kernels: (observation row, chunk of JC particles).  One item per wave and one
// wave slot per item in the grid, so the hardware dispatcher evens out the CUs (a capped grid striding over the items
// left waves with 1 or 2 of them at the 1 M-row sweep point: 64 % of the roofline instead of 67-71 %).  JC is the largest
// chunk that still gives every resident wave slot (256 CUs x 32) about sixteen items, divides J with little waste
// (equal items), and is at least 4 rows so that the observation row in registers is amortised.
inline int64_t pick_jc(int64_t J, int64_t xrows) {
  static const int jc_env = env_knob("ZS_K3_JC", 0);     // experiments only
  if (jc_env > 0) return jc_env < J ? jc_env : J;
  const int64_t target = 256ll * 32 * 16;
  for (int64_t jc = J < 4096 ? J : 4096; jc >= 1; --jc) {     // (bounded host loop; chunks beyond 4096 rows gain nothing)
    const int64_t chunks = (J + jc - 1) / jc;
    if ((chunks * jc - J) * 8 > J) continue;          // unequal last chunk: skip
    if (xrows * chunks >= target || jc <= 4) return jc;
  }
  return 1;
}
inline unsigned grid_for_items(int64_t items) {         // 4 waves per workgroup, one item per wave
  const int64_t b = (items + 3) / 4;
  return (unsigned)(b < 1 ? 1 : (b > 0x7fffffffll ? 0x7fffffffll : b));
}

template <bool LOGITS>
int launch_fwd(const float* p, const float* x, int64_t Px, float* lp, float* probs_out, int64_t K, int64_t R,
               int64_t D, int64_t sk, int64_t sr, hipStream_t st) {
  if (K < 1 || R < 0 || D < 1 || Px < 1) return ZS_EINVAL;
  const int64_t N = K * R * D;
  if (N == 0) return 0;
  if (!p || !x || !lp) return ZS_EINVAL;
  if (N % Px) return ZS_EINVAL;
  const bool vec = (D % 4 == 0) && Px >= D && (Px % D == 0) && aligned16(p) && aligned16(x) &&
                   (!probs_out || aligned16(probs_out));
  if (vec) {
    const int D4 = (int)(D / 4);
    const int64_t rows = K * R, xrows = Px / D;
    const int kid = LOGITS ? KID_BERN_LOGITS_LOGPROB : KID_BERN_LOGPROB;
    float4* po = (float4*)probs_out;
    if (D4 >= 64) {
      const int64_t J = rows / xrows;
      if (D4 <= 256 && J >= 2 && rows > 32768) {
        // big problem with a shared observation: x row in registers, JC particles per wave
        const int64_t JC = pick_jc(J, xrows);
        const int64_t items = xrows * ((J + JC - 1) / JC);
        const unsigned grid = grid_for_items(items);
        // p is read once: non-temporal loads leave L2 to the observation rows that ARE re-used.  Measured (probs form) from
        // 160 MB to 13.4 GB of p: 69 -> 74, 67 -> 74, 69 -> 73, 67 -> 72, 65 -> 74, 68 -> 82 % of the roofline; the logits form
        // gains 0-6 points.  (The backward, which also writes a stream, only gains beyond 4 GB: see launch_bwd.)
        static const int ntl_env = env_knob("ZS_K3_NTLOAD", -1);     // experiments only
        const bool ntl = ntl_env >= 0 ? ntl_env != 0 : true;
#define ZS_LAUNCH_FWD_X(W, UU, L)                                                                                          \
  ZS_LAUNCH(kid, (k_bern_logprob_xreuse<LOGITS, W, UU, L>), dim3(grid), dim3(256), st, (const float4*)p, (const float4*)x, \
            xrows, J, JC, lp, po, R, D4, sk, sr)
        if (rows >= 400000) {
          if (ntl) { if (probs_out) ZS_LAUNCH_FWD_X(true, 2, true); else ZS_LAUNCH_FWD_X(false, 2, true); }
          else     { if (probs_out) ZS_LAUNCH_FWD_X(true, 2, false); else ZS_LAUNCH_FWD_X(false, 2, false); }
        } else {
          if (ntl) { if (probs_out) ZS_LAUNCH_FWD_X(true, 1, true); else ZS_LAUNCH_FWD_X(false, 1, true); }
          else     { if (probs_out) ZS_LAUNCH_FWD_X(true, 1, false); else ZS_LAUNCH_FWD_X(false, 1, false); }
        }
#undef ZS_LAUNCH_FWD_X
      } else if (D4 <= 256 && K <= 65535 && (xrows == R || xrows == rows)) {
        // a wave per row, the row's (k, r) from the block indices: no index arithmetic at all
        const dim3 grid2((unsigned)((R + 3) / 4), (unsigned)K);
        const int x_full = xrows == rows && xrows != R;
        if (probs_out) ZS_LAUNCH(kid, (k_bern_logprob_longrow2d<LOGITS, true>), grid2, dim3(256), st, (const float4*)p, (const float4*)x, x_full, lp, po, R, D4, sk, sr);
        else ZS_LAUNCH(kid, (k_bern_logprob_longrow2d<LOGITS, false>), grid2, dim3(256), st, (const float4*)p, (const float4*)x, x_full, lp, po, R, D4, sk, sr);
      } else {
        const unsigned grid = grid_for(rows, 4);
        if (probs_out) ZS_LAUNCH(kid, (k_bern_logprob_longrow<LOGITS, true>), dim3(grid), dim3(256), st, (const float4*)p, (const float4*)x, xrows, lp, po, rows, R, D4, sk, sr);
        else ZS_LAUNCH(kid, (k_bern_logprob_longrow<LOGITS, false>), dim3(grid), dim3(256), st, (const float4*)p, (const float4*)x, xrows, lp, po, rows, R, D4, sk, sr);
      }
    } else {
      const int G = D4, rpw = 64 / G, p2 = next_pow2(G);
      const int64_t tiles = (rows + rpw - 1) / rpw;
      const unsigned grid = grid_for(tiles, 4);
      if (probs_out)
        ZS_LAUNCH(kid, (k_bern_logprob_rows<LOGITS, true>), dim3(grid), dim3(256), st, (const float4*)p,
                  (const float4*)x, xrows, lp, po, K, R, D4, G, rpw, p2, sk, sr);
      else
        ZS_LAUNCH(kid, (k_bern_logprob_rows<LOGITS, false>), dim3(grid), dim3(256), st, (const float4*)p,
                  (const float4*)x, xrows, lp, po, K, R, D4, G, rpw, p2, sk, sr);
    }
  } else {
    ZS_LAUNCH(LOGITS ? KID_BERN_LOGITS_LOGPROB : KID_BERN_LOGPROB, (k_bern_logprob_serial<LOGITS>), dim3(grid_for(K * R, 256)), dim3(256), st, p, x, Px,
                       lp, probs_out, K, R, D, sk, sr);
  }
  ZS_CHECK_LAUNCH();
  return 0;
}

// gscale (optional): the row gradient is glp[k, r] * gscale[r * gss] -- the objective's incoming gradient (a device scalar,
// gss = 0, or one value per datapoint) multiplied in here instead of by a separate pass over the coefficient matrix.
template <bool LOGITS>
int launch_bwd(const float* p, const float* x, int64_t Px, const float* glp, int64_t gsk, int64_t gsr, float* gp,
               int64_t K, int64_t R, int64_t D, hipStream_t st, const float* gscale = nullptr, int64_t gss = 0) {
  if (K < 1 || R < 0 || D < 1 || Px < 1) return ZS_EINVAL;
  const int64_t N = K * R * D;
  if (N == 0) return 0;
  if (!p || !x || !glp || !gp) return ZS_EINVAL;
  if (N % Px) return ZS_EINVAL;
  const bool vec = (D % 4 == 0) && Px >= D && (Px % D == 0) && aligned16(p) && aligned16(x) && aligned16(gp);
  if (vec) {
    const int D4 = (int)(D / 4);
    const int G = D4 >= 64 ? 64 : D4, rpw = 64 / G;
    const int64_t tiles = (K * R + rpw - 1) / rpw;
    const int kid = LOGITS ? KID_BERN_LOGITS_LOGPROB_BWD : KID_BERN_LOGPROB_BWD;
    const int64_t rows = K * R, xrows = Px / D;
    const int64_t J = rows / xrows;
    static const int nt_env = env_knob("ZS_K3_NT", -1);     // experiments only
    const bool nt = nt_env >= 0 ? nt_env != 0 : (double)N * 4.0 > 268435456.0;
    static const int xr_env = env_knob("ZS_K3_XREUSE", 1);     // experiments only
    static const int cap_env = env_knob("ZS_K3_GRIDCAP", 4096);
    if (xr_env && D4 >= 64 && D4 <= 256 && J >= 2 && rows > 32768) {
      const int64_t JC = pick_jc(J, xrows);
      const unsigned grid = grid_for_items(xrows * ((J + JC - 1) / JC));
      static const int u_env = env_knob("ZS_K3_BWD_U", 0);     // experiments only
      const bool two = u_env ? u_env == 2 : rows >= 400000;
      static const int ntl_env = env_knob("ZS_K3_NTLOAD", -1);     // experiments only
      // (non-temporal loads of p: 1.7 GB problem 72.6 -> 67.1 %, 6.6 GB 64.7 -> 66.5 %, 26 GB 63.8 -> 63.0 % in one run: from ~2.5 GB of p)
      const bool ntl = ntl_env >= 0 ? ntl_env != 0 : (double)N * 4.0 > 2.5e9;
#define ZS_LAUNCH_BWD_X(T, UU, L)                                                                                      \
  ZS_LAUNCH(kid, (k_bern_logprob_bwd_xreuse<LOGITS, T, UU, L>), dim3(grid), dim3(256), st, (const float4*)p, (const float4*)x, \
            xrows, J, JC, glp, gsk, gsr, gscale, gss, (float4*)gp, R, D4)
      if (ntl)     { if (two) ZS_LAUNCH_BWD_X(true, 2, true); else ZS_LAUNCH_BWD_X(true, 1, true); }
      else if (nt) { if (two) ZS_LAUNCH_BWD_X(true, 2, false); else ZS_LAUNCH_BWD_X(true, 1, false); }
      else         { if (two) ZS_LAUNCH_BWD_X(false, 2, false); else ZS_LAUNCH_BWD_X(false, 1, false); }
#undef ZS_LAUNCH_BWD_X
    } else if (D4 >= 64 && D4 <= 256 && K <= 65535 && rows <= 4ll * cap_env && (xrows == R || xrows == rows)) {
      // a wave per row, (k, r) from the block indices (k_bern_logprob_bwd_longrow2d)
      const dim3 grid2((unsigned)((R + 3) / 4), (unsigned)K);
      const int x_full = xrows == rows && xrows != R;
      if (nt)
        ZS_LAUNCH(kid, (k_bern_logprob_bwd_longrow2d<LOGITS, true>), grid2, dim3(256), st, (const float4*)p, (const float4*)x,
                  x_full, glp, gsk, gsr, gscale, gss, (float4*)gp, R, D4);
      else
        ZS_LAUNCH(kid, (k_bern_logprob_bwd_longrow2d<LOGITS, false>), grid2, dim3(256), st, (const float4*)p, (const float4*)x,
                  x_full, glp, gsk, gsr, gscale, gss, (float4*)gp, R, D4);
    } else if (nt) {
      ZS_LAUNCH(kid, (k_bern_logprob_bwd_rows<LOGITS, true>), dim3(grid_for(tiles, 4, (unsigned)cap_env)), dim3(256), st,
                (const float4*)p, (const float4*)x, xrows, glp, gsk, gsr, gscale, gss, (float4*)gp, K, R, D4, G, rpw);
    } else {
      ZS_LAUNCH(kid, (k_bern_logprob_bwd_rows<LOGITS, false>), dim3(grid_for(tiles, 4, (unsigned)cap_env)), dim3(256), st,
                (const float4*)p, (const float4*)x, xrows, glp, gsk, gsr, gscale, gss, (float4*)gp, K, R, D4, G, rpw);
    }
  } else {
    ZS_LAUNCH(LOGITS ? KID_BERN_LOGITS_LOGPROB_BWD : KID_BERN_LOGPROB_BWD, (k_bern_logprob_bwd_serial<LOGITS>), dim3(grid_for(N, 256)), dim3(256), st, p, x, Px,
                       glp, gsk, gsr, gscale, gss, gp, N, R, D);
  }
  ZS_CHECK_LAUNCH();
  return 0;
}

}  // namespace

extern "C" int zs_bernoulli_logprob_f32(const float* p, const float* x, int64_t Px, float* lp, int64_t K,
                                        int64_t R, int64_t D, int64_t sk, int64_t sr, void* stream) {
  return launch_fwd<false>(p, x, Px, lp, nullptr, K, R, D, sk, sr, (hipStream_t)stream);
}

extern "C" int zs_bernoulli_logprob_bwd_f32(const float* p, const float* x, int64_t Px, const float* glp,
                                            int64_t gsk, int64_t gsr, float* gp, int64_t K, int64_t R,
                                            int64_t D, void* stream) {
  return launch_bwd<false>(p, x, Px, glp, gsk, gsr, gp, K, R, D, (hipStream_t)stream);
}

// Gradient w.r.t. the observation (include/zs_hip.h): thread j owns gx[j] and walks the elements j, j + Px, j + 2 Px, ... of the
// [K, R, D] problem in ascending order -- consecutive threads read consecutive elements of p in every round (coalesced), the row
// gradient is a broadcast load, the row index advances by Px / D per round without a division (rows_step; the general case, a
// period that is not a whole number of rows, divides).  Four rounds in flight.  A rare path (an observed Bernoulli value that
// comes out of a differentiable net); the form for rows of whole 16-byte pieces follows (k_bern_obs_grad_v4): this one serves the rest
// and float64.
template <typename T, bool LOGITS, int U>
__global__ __launch_bounds__(256) void k_bern_obs_grad(const T* __restrict__ p, int64_t Px, const T* __restrict__ glp, int64_t sk,
                                                        int64_t sr, const T* __restrict__ gscale, int64_t gss, T* __restrict__ gx,
                                                        int64_t n, int64_t R, int64_t D, int64_t rows_step) {
  const int64_t reps = n / Px;
  for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < Px; j += (int64_t)gridDim.x * 256) {
    T acc = (T)0;
    int64_t row = j / D, k = row / R, r = row - k * R;
    for (int64_t m0 = 0; m0 < reps; m0 += U) {
      T pv[U], g[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {             // U rounds of loads in flight before the first logarithm
        const int64_t m = m0 + u;
        const bool live = m < reps;
        const int64_t i = j + (live ? m : m0) * Px;
        if (rows_step < 0 && live) {            // a period that cuts rows: the row of every element by division
          row = i / D; k = row / R; r = row - k * R;
        }
        pv[u] = live ? p[i] : (T)0.5;
        g[u] = live ? glp[k * sk + r * sr] * (gscale ? gscale[r * gss] : (T)1) : (T)0;
        if (rows_step >= 0 && live) {
          r += rows_step;
          while (r >= R) { r -= R; ++k; }
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {             // (added in ascending element order: deterministic, and the oracle's order)
        T q = pv[u];
        if (LOGITS) q = sigmoid_any(q);
        acc += g[u] * log_ratio_any(q);
      }
    }
    gx[j] = acc;
  }
}
// The same for rows of whole 16-byte pieces (D % 4 == 0, Px % 4 == 0, aligned): a thread owns FOUR consecutive observations -- one
// row, so one row gradient and one step of the row bookkeeping per 16-byte load instead of per element (the scalar form is bound
// by exactly that bookkeeping: ~45 instructions per element, 21 % of the roofline at the config size).  Same order of additions
// per element as the scalar form: the same bits.
template <bool LOGITS, int U, int KS, bool SPLIT>
__global__ __launch_bounds__(64 * KS) void k_bern_obs_grad_v4(const float4* __restrict__ p, int64_t Px4, const float* __restrict__ glp,
                                                              int64_t sk, int64_t sr, const float* __restrict__ gscale, int64_t gss,
                                                              float4* __restrict__ gx, int64_t n4, int64_t R, int64_t D4, int64_t rows_step) {
  // SPLIT (few observations, many repetitions: the config sizes, where one thread walking all K repetitions of its piece is a
  // chain of K / U dependent rounds): wave s of the workgroup takes the s-th share of the repetitions of ONE tile of 64 pieces, the
  // partial sums meet in LDS and wave 0 adds them in slice order (deterministic).  Otherwise every wave owns a tile of its own.
  __shared__ float4 part[SPLIT ? KS - 1 : 1][64];
  const int64_t reps = n4 / Px4;
  const int lane = threadIdx.x & 63, s = threadIdx.x >> 6;
  const int64_t per = SPLIT ? (reps + KS - 1) / KS : reps, m_lo = SPLIT ? s * per : 0, m_hi = (m_lo + per < reps) ? m_lo + per : reps;
  const int64_t tiles = SPLIT ? 1 : KS;
  for (int64_t j0 = ((int64_t)blockIdx.x * tiles + (SPLIT ? 0 : s)) * 64; j0 < Px4; j0 += (int64_t)gridDim.x * tiles * 64) {   // (SPLIT: workgroup-uniform, barriers inside)
    const int64_t j = j0 + lane;
    const bool on = j < Px4;
    const int64_t jc = on ? j : Px4 - 1;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    int64_t row = (jc + m_lo * Px4) / D4, k = row / R, r = row - k * R;
    for (int64_t m0 = m_lo; m0 < m_hi; m0 += U) {
      float4 pv[U];
      float g[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int64_t m = m0 + u;
        const bool live = m < m_hi;
        const int64_t i = jc + (live ? m : m0) * Px4;
        if (rows_step < 0 && live) {
          row = i / D4; k = row / R; r = row - k * R;
        }
        pv[u] = live ? p[i] : make_float4(0.5f, 0.5f, 0.5f, 0.5f);
        g[u] = live ? glp[k * sk + r * sr] * (gscale ? gscale[r * gss] : 1.0f) : 0.f;
        if (rows_step >= 0 && live) {
          r += rows_step;
          while (r >= R) { r -= R; ++k; }
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        float4 q = pv[u];
        if (LOGITS) { q.x = sigmoid_any(q.x); q.y = sigmoid_any(q.y); q.z = sigmoid_any(q.z); q.w = sigmoid_any(q.w); }
        acc.x += g[u] * log_ratio_any(q.x);
        acc.y += g[u] * log_ratio_any(q.y);
        acc.z += g[u] * log_ratio_any(q.z);
        acc.w += g[u] * log_ratio_any(q.w);
      }
    }
    if (SPLIT) {
      if (s > 0) part[s - 1][lane] = acc;
      __syncthreads();
      if (s == 0) {
#pragma unroll
        for (int t = 0; t < KS - 1; ++t) {
          const float4 o = part[t][lane];
          acc.x += o.x; acc.y += o.y; acc.z += o.z; acc.w += o.w;
        }
      }
      __syncthreads();
    }
    if ((!SPLIT || s == 0) && on) gx[j] = acc;
  }
}
__host__ bool launch_bern_obs_grad_v4(const float* p, int from_logits, int64_t Px, const float* glp, int64_t sk, int64_t sr, const float* gscale,
                                      int64_t gss, float* gx, int64_t n, int64_t R, int64_t D, hipStream_t st) {
  if ((D % 4) || (Px % 4) || !aligned16(p) || !aligned16(gx)) return false;
  const int64_t Px4 = Px / 4, D4 = D / 4;
  const int64_t rows_step = (Px4 % D4 == 0) ? Px4 / D4 : -1;
  const int64_t reps = n / Px;
  // few observations, many repetitions (x [B, X] against p [K, B, X] at the config sizes): the repetitions are shared out over the
  // four waves of a workgroup (11.0 against 24.2 us at B = 256, K = 50); otherwise a wave per 64 pieces walks them all, two waves
  // per workgroup (70 - 72 % of 8 TB/s from 0.4 GB up)
  const bool split = reps >= 8 && Px4 < (int64_t)64 * 4096;
  const dim3 grid(grid_for(Px4, split ? 64 : 128));
#define ZS_LAUNCH_OBS(L, KS, SP) ZS_LAUNCH(KID_BERN_LOGPROB_BWD_X, (k_bern_obs_grad_v4<L, 4, KS, SP>), grid, dim3(64 * KS), st, (const float4*)p, Px4, glp, \
                                           sk, sr, gscale, gss, (float4*)gx, n / 4, R, D4, rows_step)
  if (from_logits) { if (split) ZS_LAUNCH_OBS(true, 4, true); else ZS_LAUNCH_OBS(true, 2, false); }
  else             { if (split) ZS_LAUNCH_OBS(false, 4, true); else ZS_LAUNCH_OBS(false, 2, false); }
#undef ZS_LAUNCH_OBS
  return true;
}
__host__ bool launch_bern_obs_grad_v4(const double*, int, int64_t, const double*, int64_t, int64_t, const double*, int64_t, double*, int64_t, int64_t, int64_t,
                                      hipStream_t) {
  return false;          // (float64: the scalar form)
}

template <typename T>
int launch_bern_obs_grad(const T* p, int from_logits, int64_t Px, const T* glp, int64_t sk, int64_t sr, const T* gscale, int64_t gss,
                         T* gx, int64_t K, int64_t R, int64_t D, hipStream_t st) {
  if (K < 1 || R < 0 || D < 1 || Px < 1 || gss < 0) return ZS_EINVAL;
  const int64_t n = K * R * D;
  if (n == 0) return 0;
  if (!p || !glp || !gx) return ZS_EINVAL;
  if (n % Px) return ZS_EINVAL;
  if (launch_bern_obs_grad_v4(p, from_logits, Px, glp, sk, sr, gscale, gss, gx, n, R, D, st)) {
    ZS_CHECK_LAUNCH();
    return 0;
  }
  const int64_t rows_step = (Px % D == 0) ? Px / D : -1;
  const dim3 grid(grid_for(Px, 256));
  if (from_logits) ZS_LAUNCH(KID_BERN_LOGPROB_BWD_X, (k_bern_obs_grad<T, true, 4>), grid, dim3(256), st, p, Px, glp, sk, sr, gscale, gss, gx, n, R, D, rows_step);
  else ZS_LAUNCH(KID_BERN_LOGPROB_BWD_X, (k_bern_obs_grad<T, false, 4>), grid, dim3(256), st, p, Px, glp, sk, sr, gscale, gss, gx, n, R, D, rows_step);
  ZS_CHECK_LAUNCH();
  return 0;
}
extern "C" int zs_bernoulli_logprob_bwd_x_f32(const float* p, int from_logits, int64_t Px, const float* glp, int64_t glp_stride_k,
                                              int64_t glp_stride_r, const float* gscale, int64_t gscale_stride, float* gx,
                                              int64_t K, int64_t R, int64_t D, void* stream) {
  return launch_bern_obs_grad<float>(p, from_logits, Px, glp, glp_stride_k, glp_stride_r, gscale, gscale_stride, gx, K, R, D,
                                     (hipStream_t)stream);
}
extern "C" int zs_bernoulli_logprob_bwd_x_f64(const double* p, int from_logits, int64_t Px, const double* glp, int64_t glp_stride_k,
                                              int64_t glp_stride_r, const double* gscale, int64_t gscale_stride, double* gx,
                                              int64_t K, int64_t R, int64_t D, void* stream) {
  return launch_bern_obs_grad<double>(p, from_logits, Px, glp, glp_stride_k, glp_stride_r, gscale, gscale_stride, gx, K, R, D,
                                      (hipStream_t)stream);
}

extern "C" int zs_bernoulli_logits_logprob_f32(const float* logits, const float* x, int64_t Px, float* lp,
                                               float* probs_out, int64_t K, int64_t R, int64_t D, int64_t sk,
                                               int64_t sr, void* stream) {
  return launch_fwd<true>(logits, x, Px, lp, probs_out, K, R, D, sk, sr, (hipStream_t)stream);
}

extern "C" int zs_bernoulli_logits_logprob_bwd_f32(const float* logits, const float* x, int64_t Px,
                                                   const float* glp, int64_t gsk, int64_t gsr, float* glogits,
                                                   int64_t K, int64_t R, int64_t D, void* stream) {
  return launch_bwd<true>(logits, x, Px, glp, gsk, gsr, glogits, K, R, D, (hipStream_t)stream);
}

extern "C" int zs_bernoulli_sample_f32(const float* p, int64_t Pp, float* out, int64_t N, uint64_t seed,
                                       uint64_t offset, const uint64_t* rng_state, void* stream) {
  if (N < 0 || Pp < 1) return ZS_EINVAL;
  if (N == 0) return 0;
  if (!p || !out) return ZS_EINVAL;
  ZS_LAUNCH(KID_BERN_SAMPLE, k_bern_sample, dim3(grid_for((N + 3) / 4, 256)), dim3(256), (hipStream_t)stream, p, Pp,
                     out, N, seed, offset, rng_state);
  ZS_CHECK_LAUNCH();
  return 0;
}

// ======================================================================== IW1: generator side of the IW objective, one launch
// CUs of the current device (cached per device; no stream operation: safe under stream capture)
static int compute_units() {
  static int cached[64] = {0};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
  if (cached[dev] == 0) {
    int n = 0;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n < 1) n = 256;
    cached[dev] = n;
  }
  return cached[dev];
}

extern "C" int zs_bernoulli_iw_objective_f32(const float* p, int from_logits, const float* x, int64_t Px, int64_t K, int64_t R,
                                             int64_t D, const float* z, const float* pmu, int64_t Pm, const float* psigma,
                                             int64_t Ps, int64_t Dz, int psigma_is_logstd, const float* rows_a, int64_t ld_a,
                                             const float* logq, int64_t ld_q, int estimator, int want_mean, float* lp_x,
                                             float* lp_z, float* cost_b, float* bound_b, float* coef, float* mean_cost,
                                             uint64_t* acc, void* stream) {
  if (K < 1 || R < 0 || D < 1 || Px < 1 || ld_q < K || (rows_a && ld_a < K)) return ZS_EINVAL;
  if (estimator != ZS_IW_SGVB && estimator != ZS_IW_VIMCO) return ZS_EINVAL;
  if (estimator == ZS_IW_VIMCO && K < 2) return ZS_EINVAL;
  if (want_mean && (!mean_cost || !acc)) return ZS_EINVAL;
  if (R == 0) return 0;
  if (!p || !x || !logq || !lp_x || !cost_b) return ZS_EINVAL;
  if (z && (!pmu || !psigma || Dz < 1 || (Pm != 1 && Pm != R * Dz) || (Ps != 1 && Ps != R * Dz))) return ZS_EINVAL;
  const int64_t rows = K * R;
  if (Px != R * D && Px != rows * D) return ZS_ENOTSUP;            // observation shared by the particles, or full-size
  // the fused kernel's domain: lane = particle (K <= 64), rows of 256 .. 1024 elements read 16 B per lane, a latent row of at
  // most 64 16-byte pieces
  if (K > 64 || (D % 4) != 0 || D < 256 || D > 1024 || !aligned16(p) || !aligned16(x) || R > (1 << 20)) return ZS_ENOTSUP;
  const bool pm_s = z && Pm == 1 && R * Dz != 1, ps_s = z && Ps == 1 && R * Dz != 1;
  if (z && ((Dz % 4) != 0 || Dz > 256 || !aligned16(z) || (!pm_s && !aligned16(pmu)) || (!ps_s && !aligned16(psigma)))) return ZS_ENOTSUP;
  Iw1Args a = {};
  a.p = (const float4*)p;
  a.x = (const float4*)x;
  a.x_full = (Px == rows * D && Px != R * D) ? 1 : 0;
  a.R = R;
  a.D4 = (int)(D / 4);
  a.K = (int)K;
  a.has_z = z ? 1 : 0;
  a.z = z ? (const float4*)z : (const float4*)p;                   // (no term: readable stand-ins, results dropped)
  a.pmu = z ? pmu : p;
  a.psg = z ? psigma : p;
  a.pmu_scalar = z ? pm_s : 1;
  a.psg_scalar = z ? ps_s : 1;
  a.psg_is_logstd = psigma_is_logstd;
  a.Dz4 = z ? (int)(Dz / 4) : 1;
  a.rows_a = rows_a;
  a.ld_a = ld_a;
  a.logq = logq;
  a.ld_q = ld_q;
  a.estimator = estimator;
  a.lp_x = lp_x;
  a.lp_z = lp_z;
  a.cost_b = cost_b;
  a.bound_b = bound_b;
  a.coef_p = coef;
  a.coef_q = coef ? coef + R * K : nullptr;
  a.inv_B = 1.0f / (float)R;
  a.scale = want_mean ? a.inv_B : 1.0f;
  a.mean_cost = want_mean ? mean_cost : nullptr;
  a.acc = (unsigned long long*)acc;
  a.cb = iw1_cb(R);
  // The persistent form: ONE workgroup per CU (1024 threads, 100+ VGPRs: one is resident), workgroup g takes datapoints g, g + G, ...
  // 16 waves (fewer for K < 16): the rows spread evenly over the CU's four SIMDs.
  static const int nw_env = env_knob("ZS_IW1_NW", 0), grid_env = env_knob("ZS_IW1_GRID", 0);     // experiments only (zs_common.h)
  a.variant = 0;
  int nw = K < 16 ? (int)K : 16;
  if (nw_env > 0) nw = nw_env < K ? nw_env : (int)K;
  hipStream_t st = (hipStream_t)stream;
  int64_t G = compute_units();
  if (grid_env > 0) G = grid_env;
  if (G > R) G = R;
  if (G >= (1 << ZS_IW1_CNT_BITS)) G = (1 << ZS_IW1_CNT_BITS) - 1;
  a.sharded = 2;            // (reserved; the batch mean is finished by a watching wave: zs_iwpersist.h)
#define ZS_LAUNCH_IW1P(L, XF) ZS_LAUNCH(KID_BERN_IW_OBJECTIVE, (k_iw1_persist<L, XF>), dim3((unsigned)G), dim3(64 * nw), st, a)
  if (from_logits) { if (a.x_full) ZS_LAUNCH_IW1P(true, true); else ZS_LAUNCH_IW1P(true, false); }
  else             { if (a.x_full) ZS_LAUNCH_IW1P(false, true); else ZS_LAUNCH_IW1P(false, false); }
#undef ZS_LAUNCH_IW1P
  ZS_CHECK_LAUNCH();
  return 0;
}

// Backward of IW1: the Bernoulli term's gradient with the row gradients coef[0][r, k] * gout[r * gout_stride] formed in the
// kernel (no pass over the coefficient matrix), and -- when the variational node's operands are handed in -- the gradient of
// log q w.r.t. the parameters of a non-reparameterised Normal node, summed over the particles (normal.py:102,112-116), with
// row gradients coef[1][r, k] * gout[...].
extern "C" int zs_bernoulli_iw_objective_bwd_f32(const float* p, int from_logits, const float* x, int64_t Px, int64_t K,
                                                 int64_t R, int64_t D, const float* coef, const float* gout,
                                                 int64_t gout_stride, float* gp, const float* zq, const float* qmu,
                                                 const float* qsigma, int64_t Dq, int qsigma_is_logstd, float* gqmu,
                                                 float* gqsigma, void* stream) {
  if (K < 1 || R < 0 || D < 1 || Px < 1 || gout_stride < 0) return ZS_EINVAL;
  if (R == 0) return 0;
  if (!coef || !gout) return ZS_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  // both gradients wanted and both roles on their 16-byte paths: ONE launch
  static const int64_t bwd_rows = env_knob("ZS_IW1_BWD_ROWS", 32768);      // experiments only
  if (gp && zq && qmu && qsigma && gqmu && gqsigma && Dq >= 1 && p && x && (D % 4) == 0 && D >= 256 && D <= 1024 && K <= 65534 &&
      K * R <= bwd_rows && (Px == R * D || Px == K * R * D) && aligned16(p) && aligned16(x) && aligned16(gp) && (Dq % 4) == 0 &&
      aligned16(zq) && aligned16(qmu) && aligned16(qsigma) && aligned16(gqmu) && aligned16(gqsigma)) {
    const int64_t Mq4 = R * Dq / 4;
    const int64_t bx_rows = (R + 3) / 4, bx_q = (Mq4 + 63) / 64;
    const dim3 grid((unsigned)(bx_rows > bx_q ? bx_rows : bx_q), (unsigned)(K + 1));
    const int x_full = (Px == K * R * D && Px != R * D) ? 1 : 0;
    const bool nt = (double)K * (double)R * (double)D * 4.0 > 268435456.0;
#define ZS_LAUNCH_IW1B(L, T)                                                                                                 \
  ZS_LAUNCH(KID_BERN_IW_OBJECTIVE_BWD, (k_iw1_bwd<L, T>), grid, dim3(256), st, (const float4*)p, (const float4*)x, x_full, coef, \
            gout, gout_stride, (float4*)gp, K, R, (int)(D / 4), (const float4*)zq, (const float4*)qmu, (const float4*)qsigma,    \
            (float4*)gqmu, (float4*)gqsigma, Mq4, (int)(Dq / 4), qsigma_is_logstd != 0)
    if (from_logits) { if (nt) ZS_LAUNCH_IW1B(true, true); else ZS_LAUNCH_IW1B(true, false); }
    else             { if (nt) ZS_LAUNCH_IW1B(false, true); else ZS_LAUNCH_IW1B(false, false); }
#undef ZS_LAUNCH_IW1B
    ZS_CHECK_LAUNCH();
    return 0;
  }
  if (gp) {
    const int rc = from_logits ? launch_bwd<true>(p, x, Px, coef, 1, K, gp, K, R, D, st, gout, gout_stride)
                               : launch_bwd<false>(p, x, Px, coef, 1, K, gp, K, R, D, st, gout, gout_stride);
    if (rc != 0) return rc;
  }
  if (zq) {
    if (!qmu || !qsigma || Dq < 1 || !gqmu || !gqsigma) return ZS_EINVAL;
    launch_logprob_bwd_ksum<D_NORMAL>(KID_BERN_IW_OBJECTIVE_BWD, zq, qmu, qsigma, coef + R * K, 1, K, nullptr, gqmu, gqsigma, K, R, Dq,
                                      qsigma_is_logstd != 0, st, gout, gout_stride);
    ZS_CHECK_LAUNCH();
  }
  return 0;
}
