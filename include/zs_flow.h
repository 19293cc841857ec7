/*
 * zs_flow.h -- C ABI of the normalising-flow kernels (libzs_flow.so, gfx950).
 *
 * A third library next to libzs_hip.so (include/zs_hip.h) and libzs_mcmc.so (include/zs_mcmc.h), with the same conventions:
 * every pointer is a DEVICE pointer owned by the caller, nothing is allocated, freed or synchronised inside a call, `stream`
 * is a hipStream_t passed as void* (NULL = the null stream) and is the last argument of every entry, the return value is 0 on
 * success, a positive hipError_t if the launch failed, ZS_EINVAL / ZS_ENOTSUP (the codes of zs_hip.h) for rejected
 * arguments.  A call enqueues exactly one kernel: it can be captured in a hipGraph.
 *
 * The entries replace the strings of element-wise launches the reference's flow layers issue around their inner networks
 * (thuwzy/ZhuSuan-PyTorch, paths relative to its root): zhusuan/invertible/coupling.py:65-75 (MaskCoupling), :102-147
 * (Coupling), scaling.py:26-34 (Scaling), made.py:106-122 (MADE's affine) and distributions/flow_distribution.py:48-51.
 *
 * Every entry has an _f32 and an _f64 form; T is the element type.  All tensors are row-major [B, D] unless stated.  Any
 * pointer alignment of a T is accepted: 4-element accesses are used only when D is a multiple of 4 and every operand is
 * aligned to 4 T (16 bytes for _f32, 32 for _f64); any other layout takes the element path, with the same results bit for
 * bit.  Reductions run in a fixed order inside one workgroup (no floating-point atomics): two runs give the same bits.
 * B == 0 or D == 0 returns 0 without a launch.  ZS_EINVAL: a NULL required pointer, B < 0 or D < 0, an unknown mode / base /
 * kind, an odd D in ZS_FLOW_INTERLEAVE mode, sel outside {0, 1}, a column outside [0, D).
 * The arithmetic (csrc/zs_flow_math.h) is in T, one rounding per written operation, the accumulations of the reductions
 * included: nothing written here is contracted into an fma (exp, log, log1p, tanh and the division are the device library's).
 *
 * Coupling (mode ZS_FLOW_MASK: mask is [D]; mode ZS_FLOW_INTERLEAVE: mask is ignored, sel is the position, 0 or 1, inside
 * each pair of columns that is handed to the inner network and passes through unchanged; the other one, 1 - sel, is shifted)
 *
 *   split      MASK        out[b,d] = mask[d] * x[b,d]                                   out [B, D]
 *              INTERLEAVE  out[b,j] = x[b, 2j + sel]                                     out [B, D/2]
 *   split_bwd  MASK        gx[b,d] = mask[d] * g_out[b,d]
 *              INTERLEAVE  gx[b, 2j + sel] = g_out[b,j] ;  gx[b, 2j + 1 - sel] = 0
 *   merge      MASK        y = mask*x + ((1 - mask)*x + (sign*shift)*(1 - mask))          shift [B, D], evaluated in that order
 *              INTERLEAVE  y[b, 2j + 1 - sel] = x[b, 2j + 1 - sel] + sign*shift[b,j] ;  y[b, 2j + sel] = x[b, 2j + sel]
 *   merge_bwd  MASK        gx = mask*gy + (1 - mask)*gy ;  gshift = sign * (gy * (1 - mask))
 *              INTERLEAVE  gx = gy ;  gshift[b,j] = sign * gy[b, 2j + 1 - sel]
 *
 * Scaling (log_scale is [D])
 *
 *   scale_fwd  y[b,d] = x[b,d] * exp(sign * log_scale[d])   (y may alias x) ;   logdet[0] = sum_d log_scale[d]
 *   scale_bwd  gx[b,d] = gy[b,d] * exp(sign * log_scale[d])  (gx may alias gy)
 *              g_log_scale[d] = sign * sum_b gy[b,d]*y[b,d] + (g_logdet ? g_logdet[0] : 0)        y: the saved OUTPUT
 *
 * MADE's affine (net is the inner network's [B, 2D] output, read in place: m = net[b, d], loga = net[b, D + d])
 *
 *   made_fwd      u = (x - m) * exp(-loga) ;  logdet = -loga                              u, logdet [B, D]
 *   made_bwd      e = exp(-loga) ;  gx = gu*e ;  gnet[b, d] = -(gu*e) ;  gnet[b, D + d] = -(gu*u) - gld      gnet [B, 2D]
 *                 (u recomputed as in made_fwd; gu or gld may be NULL = zero, not both)
 *   made_inv_col  x[b,col] = u[b,col] * exp(loga[b,col]) + m[b,col]                       one column, the others untouched
 *
 * FlowDistribution tail (base ZS_FLOW_NORMAL: loc = mean, scale = std; ZS_FLOW_LOGISTIC: loc, scale; both [D] when
 * param_rows == 0 and [B, D] when param_rows == 1;  logdet_kind ZS_FLOW_LOGDET_NONE / _SCALAR ([1]) / _ROWS ([B]))
 *
 *   tail      out[b] = sum_d logpdf(z[b,d]; loc, scale) + logdet
 *             Normal:    (-0.5 log(2 pi) - log(scale)) - 0.5 * (1 / scale^2) * (z - loc)^2
 *             Logistic:  -(|t| + 2 log1p(exp(-|t|))) - log(scale),   t = (z - loc) / scale
 *   tail_bwd  gz[b,d] = g[b] * d logpdf / d z ;  g_logdet[b] = g[b] when g_logdet is non-NULL (the per-row log-det)
 *             Normal:  -(1 / scale^2) * (z - loc) ;  Logistic:  -tanh(t / 2) / scale
 */
#ifndef ZS_FLOW_H
#define ZS_FLOW_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ZS_FLOW_ABI_VERSION 1

#ifndef ZS_EINVAL
#define ZS_EINVAL (-1)
#define ZS_ENOTSUP (-2)
#endif

/* mode */
#define ZS_FLOW_MASK 0
#define ZS_FLOW_INTERLEAVE 1
/* base */
#define ZS_FLOW_NORMAL 0
#define ZS_FLOW_LOGISTIC 1
/* logdet_kind */
#define ZS_FLOW_LOGDET_NONE 0
#define ZS_FLOW_LOGDET_SCALAR 1
#define ZS_FLOW_LOGDET_ROWS 2

int zs_flow_abi_version(void);

#define ZS_FLOW_DECLARE(SFX)                                                                                                   \
  int zs_flow_split_##SFX(int mode, const void* x, const void* mask, void* out, int64_t B, int64_t D, int sel, void* stream); \
  int zs_flow_split_bwd_##SFX(int mode, const void* g_out, const void* mask, void* gx, int64_t B, int64_t D, int sel,         \
                              void* stream);                                                                                   \
  int zs_flow_merge_##SFX(int mode, const void* x, const void* mask, const void* shift, double sign, void* y, int64_t B,      \
                          int64_t D, int sel, void* stream);                                                                   \
  int zs_flow_merge_bwd_##SFX(int mode, const void* gy, const void* mask, double sign, void* gx, void* gshift, int64_t B,     \
                              int64_t D, int sel, void* stream);                                                               \
  int zs_flow_scale_fwd_##SFX(const void* x, const void* log_scale, double sign, void* y, void* logdet, int64_t B, int64_t D, \
                              void* stream);                                                                                   \
  int zs_flow_scale_bwd_##SFX(const void* gy, const void* y, const void* log_scale, const void* g_logdet, double sign,        \
                              void* gx, void* g_log_scale, int64_t B, int64_t D, void* stream);                                \
  int zs_flow_made_fwd_##SFX(const void* x, const void* net, void* u, void* logdet, int64_t B, int64_t D, void* stream);      \
  int zs_flow_made_bwd_##SFX(const void* gu, const void* gld, const void* x, const void* net, void* gx, void* gnet,           \
                             int64_t B, int64_t D, void* stream);                                                              \
  int zs_flow_made_inv_col_##SFX(const void* u, const void* net, void* x, int64_t B, int64_t D, int64_t col, void* stream);   \
  int zs_flow_tail_##SFX(int base, const void* z, const void* loc, const void* scale, int param_rows, const void* logdet,     \
                         int logdet_kind, void* out, int64_t B, int64_t D, void* stream);                                      \
  int zs_flow_tail_bwd_##SFX(int base, const void* g, const void* z, const void* loc, const void* scale, int param_rows,      \
                             void* gz, void* g_logdet, int64_t B, int64_t D, void* stream);

ZS_FLOW_DECLARE(f32)
ZS_FLOW_DECLARE(f64)

#ifdef __cplusplus
}
#endif
#endif /* ZS_FLOW_H */
