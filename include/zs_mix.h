/*
 * zs_mix.h -- C ABI of the mixture-of-Gaussians density (libzs_mix.so, gfx950): the log-density of rows x under
 * p(x) = sum_c softmax(logits)_c N(x; mean_c, diag exp(2 logstd_c)) and its gradients with respect to x, logits, mean and logstd.
 * The [R, C] scores are formed tile by tile in matrix-core accumulators (v_mfma_f32_16x16x4_f32 / v_mfma_f64_16x16x4_f64),
 * reduced there, and never reach memory; nothing of size [R, C] or [R, C, D] is allocated or kept for the backward.
 *
 * A thirteenth library next to libzs_hip.so and the other satellites, with the conventions of zs_topic.h: every pointer is a
 * DEVICE pointer owned by the caller, nothing is allocated, freed or synchronised inside a call, `stream` is a hipStream_t passed
 * as void* (NULL = the null stream), the return value is 0 on success, a positive hipError_t if a launch failed, ZS_EINVAL /
 * ZS_ENOTSUP (the codes of zs_hip.h) for rejected arguments, which write nothing.  T is the element type of the suffix
 * (_f32: float, _f64: double).  Every access is one element wide and there are no floating-point atomics: the results do not
 * depend on the alignment of the operands, and the same call gives the same bits.
 *
 * Operands, all contiguous and row-major:
 *   logits T[C]   mean T[C, D]   logstd T[C, D]   x T[R, D]   g T[R] the cotangent of lp   lp T[R] the result of zs_mix_logprob
 *
 * The arithmetic.  With w = exp(-2 logstd), a per-dimension centre m_d = mean_c mean[c, d], y = x - m and nu = mean - m,
 *   b_c   = log_softmax(logits)_c - sum_d logstd[c, d] - (D / 2) log 2 pi - 1/2 sum_d w nu^2
 *   s_rc  = b_c + sum_d ( y_rd (w nu)_cd + y_rd^2 (-w / 2)_cd )           an [R, 2D] x [2D, C] product
 *   lp_r  = logsumexp_c s_rc
 *   G_rc  = g_r exp(s_rc - lp_r)          n_c = sum_r G_rc
 *   dx        = G (w nu) - y o (G w)
 *   dlogits_c = n_c - softmax(logits)_c sum_r g_r
 *   dmean     = w o (G^T Y - nu n)
 *   dlogstd   = w o (G^T Y^2 - 2 nu o G^T Y + nu^2 n) - n
 * The centre cancels algebraically (it carries no gradient); it is there because the expanded square cancels badly when all
 * means share an offset.  Scores are shifted by the running maximum before they are exponentiated: a row whose every score is
 * -1e4 and a component whose weight underflows to 0 both come out finite.
 *
 * Calling order.  zs_mix_prepare writes the `prep` workspace from (logits, mean, logstd): m, log_softmax(logits), b and the packed
 * component operand W[k, c], k = 2 d: (w nu)_cd, k = 2 d + 1: (-w / 2)_cd, zero-padded to 16 rows and to whole panels of
 * components (padded components get b = -inf).  The one operand serves the score product and, read the other way, the second
 * product of both backwards ([w nu | w] up to the exact factor -2).  One prepare serves the forward and both backwards.
 * zs_mix_grad_x and zs_mix_grad_params recompute the scores and read lp; zs_mix_grad_params needs a `part` workspace and a
 * number of row shares (zs_mix_row_shares).  Workspace sizes, in elements of T, come from zs_mix_workspace_elems.
 *
 * ZS_EINVAL: a NULL operand, output or workspace, R < 0, C < 1, D < 1, shares outside [1, ceil(R / 16)] (for R > 0).
 * ZS_ENOTSUP: D > zs_mix_max_dim(), C > zs_mix_max_components(), R >= 2^31.  R == 0 returns 0 and launches nothing.
 *
 * Kernel shape.  A component panel is 64 components (_f32) or 32 (_f64), staged in LDS as [K16, panel] (K16 = 2 D rounded up to
 * 16, at most 128 rows: 41 KB / 50 KB with the padding of 17 elements per row against bank conflicts).
 *   logprob      a wave owns 16 rows, a workgroup four such strips; the row operand [y | y^2] (interleaved) is built once from x
 *                and held in registers as A operands; ALL panels stream through LDS, so C is not limited by it.  A 16 x 16 score
 *                tile is ceil(2 D / 4) matrix instructions; the epilogue adds b_c and folds the tile into a per-lane running
 *                maximum and scaled sum; the four lanes that share a row combine once, at the end, and lp is written once per row.
 *   grad_x       the same walk; the tile is formed with the components in the accumulator's row index, so that G = g exp(s - lp)
 *                IS the B operand of the second product with the panel, whose contraction runs over the tile's 16 components:
 *                no transposition through LDS.  dx is written once per row.
 *   grad_params  grid = panels x row shares, a wave per 16 components of the panel; the tile has the rows in the accumulator's
 *                row index, G is the B operand of G^T [Y | Y^2] with the A operand read from x.  A workgroup writes one partial
 *                [K16 + 1, panel] (the last row is n) for its share; the finish launch adds the shares in order and applies the
 *                closed forms above.
 */
#ifndef ZS_MIX_H
#define ZS_MIX_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ZS_MIX_ABI_VERSION 1

/* which workspace zs_mix_workspace_elems sizes */
#define ZS_MIX_WS_PREP 0         /* prep: D + 1 + 2 Cpad + K16 Cpad, Cpad = C rounded up to whole panels */
#define ZS_MIX_WS_GRAD_PARAMS 1  /* part of zs_mix_grad_params: shares ((K16 + 1) Cpad + 1) */

/* ABI version of the loaded library (== ZS_MIX_ABI_VERSION). */
int zs_mix_abi_version(void);
/* the widest event the fused kernels take (64) */
int zs_mix_max_dim(void);
/* the most components the fused kernels take (65536) */
int zs_mix_max_components(void);
/* component panels of C components for elements of elem_bytes (4: 64 per panel, 8: 32); 0 for another size or C < 1 */
int64_t zs_mix_panels(int elem_bytes, int64_t C);
/* the row shares zs_mix_grad_params should be called with: enough for panels x shares workgroups to cover the device at small C,
 * at most the number of 16-row strips (host arithmetic; 0 for rejected arguments) */
int64_t zs_mix_row_shares(int elem_bytes, int64_t R, int64_t C);
/* elements of T in workspace `which` (shares is read for ZS_MIX_WS_GRAD_PARAMS only); -1 for rejected arguments */
int64_t zs_mix_workspace_elems(int which, int elem_bytes, int64_t C, int64_t D, int64_t shares);

/* The prologue: the centre and the log-sum-exp of the logits, then a thread per component for b and the packed operand. */
int zs_mix_prepare_f32(const void* logits, const void* mean, const void* logstd, void* prep, int64_t C, int64_t D, void* stream);
int zs_mix_prepare_f64(const void* logits, const void* mean, const void* logstd, void* prep, int64_t C, int64_t D, void* stream);

/* lp T[R] */
int zs_mix_logprob_f32(const void* x, const void* prep, void* lp, int64_t R, int64_t C, int64_t D, void* stream);
int zs_mix_logprob_f64(const void* x, const void* prep, void* lp, int64_t R, int64_t C, int64_t D, void* stream);

/* dx T[R, D] */
int zs_mix_grad_x_f32(const void* x, const void* g, const void* lp, const void* prep, void* dx, int64_t R, int64_t C, int64_t D,
                      void* stream);
int zs_mix_grad_x_f64(const void* x, const void* g, const void* lp, const void* prep, void* dx, int64_t R, int64_t C, int64_t D,
                      void* stream);

/* dlogits T[C], dmean T[C, D], dlogstd T[C, D] */
int zs_mix_grad_params_f32(const void* x, const void* g, const void* lp, const void* mean, const void* logstd, const void* prep,
                           void* part, void* dlogits, void* dmean, void* dlogstd, int64_t R, int64_t C, int64_t D, int64_t shares,
                           void* stream);
int zs_mix_grad_params_f64(const void* x, const void* g, const void* lp, const void* mean, const void* logstd, const void* prep,
                           void* part, void* dlogits, void* dmean, void* dlogstd, int64_t R, int64_t C, int64_t D, int64_t shares,
                           void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ZS_MIX_H */
