/*
 * zs_nf.h -- C ABI of the planar and Householder flow stacks (libzs_nf.so, gfx950): a whole stack of L layers applied to R rows
 * in one launch, with its backward.
 *
 * An eighth library next to libzs_hip.so, libzs_mcmc.so, libzs_flow.so, libzs_hmc.so, libzs_cat.so, libzs_mvn.so and
 * libzs_klpq.so, with the conventions of zs_mvn.h: every pointer is a DEVICE pointer owned by the caller, nothing is allocated,
 * freed or synchronised inside a call, `stream` is a hipStream_t passed as void* (NULL = the null stream), the return value is 0
 * on success, a positive hipError_t if the launch failed, ZS_EINVAL / ZS_ENOTSUP (the codes of zs_hip.h) for rejected arguments,
 * which write nothing.  A call only enqueues one kernel.  T is the element type of the suffix (_f32: float, _f64: double).
 *
 * Shapes.  R rows, D dimensions, L layers; every operand is contiguous:
 *   planar       u, w T[L, D];  b T[L];  x, y, gy, gx T[R, D];  logdet, gld T[R]
 *   Householder  v, gv T[L, R, D] (one reflection vector per layer and row);  x, y, gy, gx T[R, D]
 * ZS_EINVAL: a NULL required pointer, D < 1, R < 0, L < 0, a call with nothing to write, an n_wg outside
 * [1, zs_nf_max_workgroups()].  ZS_ENOTSUP: D > zs_nf_max_dim() or L > zs_nf_max_layers().  R == 0 or L == 0 returns 0 and
 * launches nothing.
 *
 * Kernel shape.  A group of G = next_pow2(D) consecutive lanes of one wave owns a row, lane i its component i, so a wave (= a
 * workgroup) holds 64 / G rows; the grid is capped at zs_nf_max_workgroups() and a workgroup past the cap walks row tiles.  A
 * planar workgroup first forms the per-layer parameter quantities (below) in LDS -- every workgroup does so redundantly, 3 L dots
 * of length D -- then walks its rows with z in registers through all L layers; dots are butterflies inside the group.  The
 * backwards recompute the forward from x with the same device functions (the same bits) and hold the layer inputs z_l of their
 * rows in LDS, at most L D elements per row: the reason for the layer cap.  NO WORKGROUP EVER WAITS FOR ANOTHER: the sums over
 * rows of the planar parameter gradients leave the backward as per-workgroup partials and are finished by a second, small launch.
 * No forward intermediate is ever stored in global memory.  No floating-point atomics, no scratch.  Every access is one element
 * wide: the results do not depend on the alignment of the operands, and the same call gives the same bits.
 *
 * Arithmetic is in T with one rounding per written operation, nothing is contracted into an fma; tanh, log, exp, log1p and
 * division are the device library's (zs_flow.h states the same for its kernels).
 *
 * Planar (Rezende & Mohamed 2015).  Per layer, from the parameters alone:
 *   s = w.u ;  n = w.w ;  k = softplus(s) - 1 - s ;  uh = u + k w / n ;  c = w.uh       softplus(s) = max(s, 0) + log1p(exp(-|s|))
 * so that w.uh = softplus(s) - 1 > -1 and the layer is invertible.  A row with NaN parameters gives NaN, with no check and no trap.
 */
#ifndef ZS_NF_H
#define ZS_NF_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ZS_NF_ABI_VERSION 1

/* ABI version of the loaded library (== ZS_NF_ABI_VERSION). */
int zs_nf_abi_version(void);
/* the widest row the kernels take (64) */
int zs_nf_max_dim(void);
/* the deepest stack one call takes (32) */
int zs_nf_max_layers(void);
/* lanes per row for D dimensions (host arithmetic; 0 outside [1, zs_nf_max_dim()]) */
int zs_nf_group_lanes(int64_t D);
/* the grid cap: past it a workgroup loops over row tiles */
int zs_nf_max_workgroups(void);
/* workgroups of zs_nf_planar_bwd for R rows of D dimensions = the leading extent of its `partials` (0 for R < 1 or a D outside
 * [1, zs_nf_max_dim()]) */
int zs_nf_planar_workgroups(int64_t R, int64_t D);

/* P1  the planar stack.  For l = 0 .. L-1:
 *   a = w_l.z + b_l ;  t = tanh(a) ;  z <- z + uh_l t ;  ld <- ld + log|1 + (1 - t^2) c_l|
 * y T[R, D] and logdet T[R] may be NULL, not both; y may alias x. */
int zs_nf_planar_fwd_f32(const void* u, const void* w, const void* b, const void* x, void* y, void* logdet, int64_t R, int64_t D,
                         int64_t L, void* stream);
int zs_nf_planar_fwd_f64(const void* u, const void* w, const void* b, const void* x, void* y, void* logdet, int64_t R, int64_t D,
                         int64_t L, void* stream);

/* P1b  backward of P1 from gy T[R, D] and gld T[R] (either may be NULL, meaning zero; not both).  With g = gy, for l = L-1 .. 0:
 *   h = 1 - t^2 ;  m = 1 + h c ;  gt = g.uh + gld (c / m) (-2 t) ;  ga = gt h
 *   Guh_l[d] += g[d] t ;  Gw_l[d] += ga z_l[d] ;  Gb_l += ga ;  Gc_l += gld h / m ;  then  g <- g + ga w_l
 * gx T[R, D] = g after layer 0 (may be NULL).  The four sums run over the workgroup's rows in ascending row order and go to
 * partials T[n_wg, L, 2 D + 2] (per layer: Guh[D], Gw[D], Gb, Gc), n_wg = zs_nf_planar_workgroups(R, D); a workgroup that walks
 * more than one row tile adds each later tile to its own slot.  partials may be NULL when only gx is wanted; not both. */
int zs_nf_planar_bwd_f32(const void* u, const void* w, const void* b, const void* x, const void* gy, const void* gld, void* gx,
                         void* partials, int64_t R, int64_t D, int64_t L, void* stream);
int zs_nf_planar_bwd_f64(const void* u, const void* w, const void* b, const void* x, const void* gy, const void* gld, void* gx,
                         void* partials, int64_t R, int64_t D, int64_t L, void* stream);

/* P1f  one workgroup adds the partials in ascending workgroup order and applies the parameter chain:
 *   Guh += Gc w ;  Gw += Gc uh ;  p = Guh.w ;  s' = sigmoid(s) - 1
 *   gu = Guh + (p / n) s' w ;  gw = Gw + Guh k / n + (p / n) s' u - 2 k p / n^2 w ;  gb = Gb
 * gu, gw T[L, D] and gb T[L] may be NULL, not all. */
int zs_nf_planar_finish_f32(const void* u, const void* w, const void* partials, int64_t n_wg, void* gu, void* gw, void* gb,
                            int64_t D, int64_t L, void* stream);
int zs_nf_planar_finish_f64(const void* u, const void* w, const void* partials, int64_t n_wg, void* gu, void* gw, void* gb,
                            int64_t D, int64_t L, void* stream);

/* H1  the Householder stack (Tomczak & Welling 2016).  For l = 0 .. L-1:  z <- z - 2 v_l ((v_l.z) / (v_l.v_l)).  The log-det is
 * zero and no operand carries it.  A row with v_l = 0 gives NaN in that row only (0 / 0), with no check and no trap.  y may
 * alias x. */
int zs_nf_householder_fwd_f32(const void* v, const void* x, void* y, int64_t R, int64_t D, int64_t L, void* stream);
int zs_nf_householder_fwd_f64(const void* v, const void* x, void* y, int64_t R, int64_t D, int64_t L, void* stream);

/* H1b  backward of H1 from gy T[R, D].  With g = gy, for l = L-1 .. 0, n = v.v, p = v.z_l, q = v.g:
 *   gv_l = -2 (p g + q z_l) / n + 4 p q v / n^2 ;  g <- g - 2 v q / n
 * gx T[R, D] = g after layer 0; gv T[L, R, D].  Every row is independent.  gx or gv may be NULL, not both. */
int zs_nf_householder_bwd_f32(const void* v, const void* x, const void* gy, void* gx, void* gv, int64_t R, int64_t D, int64_t L,
                              void* stream);
int zs_nf_householder_bwd_f64(const void* v, const void* x, const void* gy, void* gx, void* gv, int64_t R, int64_t D, int64_t L,
                              void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ZS_NF_H */
