/*
 * zs_topic.h -- C ABI of the admixture (topic-model) likelihood (libzs_topic.so, gfx950): the log-likelihood of bag-of-words
 * counts under theta @ phi, theta = softmax(H) per row and phi = softmax(B) per topic, and its gradients with respect to the
 * document logits H and the topic logits B.  The [R, V] product is formed tile by tile in matrix-core accumulators
 * (v_mfma_f32_16x16x4_f32 / v_mfma_f64_16x16x4_f64) and never reaches memory.
 *
 * A tenth library next to libzs_hip.so and the other satellites, with the conventions of zs_mvn.h: every pointer is a DEVICE
 * pointer owned by the caller, nothing is allocated, freed or synchronised inside a call, `stream` is a hipStream_t passed as
 * void* (NULL = the null stream), the return value is 0 on success, a positive hipError_t if a launch failed, ZS_EINVAL /
 * ZS_ENOTSUP (the codes of zs_hip.h) for rejected arguments, which write nothing.  T is the element type of the suffix
 * (_f32: float, _f64: double).  Every access is one element wide and there are no floating-point atomics: the results do not
 * depend on the alignment of the operands, and the same call gives the same bits.
 *
 * Operands, all contiguous and row-major:
 *   H T[R, K]   document logits; the R rows are chains x documents
 *   B T[K, V]   topic logits
 *   X T[Dx, V]  non-negative counts, R % Dx == 0: row r reads X[r % Dx], so one count matrix serves every chain
 *   g T[R]      the cotangent of lp
 *
 *   lp[r]   = sum_v X[r % Dx, v] log( sum_k softmax(H[r])_k softmax(B[k])_v )        a term with X == 0 is exactly 0
 *   W[r,v]  = g[r] X / pred[r,v] ;  dtheta[r,k] = sum_v W[r,v] phi[k,v] ;  N_r = sum_v X[r % Dx, v] ;  s_k = sum_r theta dtheta
 *   dH[r,k] = theta[r,k] (dtheta[r,k] - g[r] N_r)            dB[k,v] = phi[k,v] (sum_r theta[r,k] W[r,v] - s_k)
 * There is no multinomial coefficient (upstream's UnnormalizedMultinomial at normalize_logits=False) and no gradient for X.
 *
 * Shifts.  The matrix operands are plain numbers in (0, 1]: E[r,k] = exp(H[r,k] - max_k H[r,.]) with Z_r = sum_k E[r,k], and
 * exp(B[k,v] - lse_k - c_v) with lse_k the log-sum-exp of row k of B and c_v = max_k (B[k,v] - lse_k); then
 * log pred = c_v + log(acc) - log Z_r.  A common offset on a row of H or of B cancels; a word that is rare under every topic
 * stays finite.  SUPPORTED DOMAIN: for every (r, v) with X > 0,
 *   max_k [ (H[r,k] - max H_r) + (log phi[k,v] - c_v) ] >= -60,
 * which holds whenever a row of H spreads less than 60 nats.  Outside it the accumulator may underflow: lp gets -inf and the
 * gradients inf / NaN, with no check and no trap.  Negative counts are not checked either (they are treated as zero).
 *
 * Calling order.  zs_topic_prepare writes the `prep` workspace (lse_k, the row sums N of X, Z_r, log Z_r and the operand E);
 * the three compute entry points read it, so one prepare serves a forward and both backwards of the same (H, B, X).  Each
 * compute entry point enqueues a main launch and a finish launch on `stream` and needs a `part` workspace of its own.  The
 * workspace sizes, in elements of T, come from zs_topic_workspace_elems (host arithmetic).
 *
 * ZS_EINVAL: a NULL operand, output or workspace, R < 0, K < 1, V < 1, Dx < 1, R % Dx != 0, splits outside
 * [1, zs_topic_panels] (for R > 0).  ZS_ENOTSUP: K > zs_topic_max_topics(), R or V >= 2^31.  R == 0 returns 0 and launches nothing.
 *
 * Kernel shape.  A column panel is 64 columns (_f32) or 32 (_f64).  A workgroup stages its shifted panel of B and c_v in LDS
 * once (K rounded up to 16 rows, zero filled).  A wave forms a 16 x 16 tile of the product by ceil(K / 4) matrix instructions,
 * the operand E in registers; the epilogue works on the accumulator registers.
 *   logprob      a workgroup per panel walks all row tiles, 16 rows per wave; per-panel partial row sums go to part[panels, R],
 *                the finish adds them in panel order and subtracts N_r log Z_r.
 *   grad_doc     grid = blocks of 64 rows x `splits` column splits.  The tile is formed transposed (columns in the accumulator's
 *                row index), so that g X / acc IS the B operand of the second product with the panel, whose contraction runs
 *                over the tile's 16 columns: no transposition through LDS.  Partials go to part[splits, R, K16]; the finish
 *                applies the softmax Jacobian.
 *   grad_topic   a workgroup per panel, a wave per 16 columns, walks ALL rows: the sum over r needs no partials.  It writes
 *                T = phi dphi into dB and per-panel partials of sum_v T (= s_k); the finish is one pass dB = T - phi s_k.
 */
#ifndef ZS_TOPIC_H
#define ZS_TOPIC_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ZS_TOPIC_ABI_VERSION 1

/* which workspace zs_topic_workspace_elems sizes */
#define ZS_TOPIC_WS_PREP 0        /* prep:  K + Dx + 2 R + R K16, K16 = K rounded up to a multiple of 16 */
#define ZS_TOPIC_WS_LOGPROB 1     /* part of zs_topic_logprob:     panels R */
#define ZS_TOPIC_WS_GRAD_DOC 2    /* part of zs_topic_grad_doc:    splits R K16 */
#define ZS_TOPIC_WS_GRAD_TOPIC 3  /* part of zs_topic_grad_topic:  panels K16 */

/* ABI version of the loaded library (== ZS_TOPIC_ABI_VERSION). */
int zs_topic_abi_version(void);
/* the most topics the fused kernels take (128) */
int zs_topic_max_topics(void);
/* column panels of V columns for elements of elem_bytes (4: 64 columns per panel, 8: 32); 0 for another size or V < 1 */
int64_t zs_topic_panels(int elem_bytes, int64_t V);
/* the column splits zs_topic_grad_doc should be called with: enough for rows / 64 x splits workgroups to cover the device at
 * small R, at most the number of panels (host arithmetic; 0 for rejected arguments) */
int64_t zs_topic_doc_splits(int elem_bytes, int64_t R, int64_t V);
/* elements of T in workspace `which` (splits is read for ZS_TOPIC_WS_GRAD_DOC only); -1 for rejected arguments */
int64_t zs_topic_workspace_elems(int which, int elem_bytes, int64_t R, int64_t K, int64_t V, int64_t Dx, int64_t splits);

/* The prologue, one launch: a workgroup per topic row for lse_k, a wave per row of H for E, Z and log Z, a wave per row of X for N. */
int zs_topic_prepare_f32(const void* H, const void* B, const void* X, void* prep, int64_t R, int64_t K, int64_t V, int64_t Dx,
                         void* stream);
int zs_topic_prepare_f64(const void* H, const void* B, const void* X, void* prep, int64_t R, int64_t K, int64_t V, int64_t Dx,
                         void* stream);

/* lp T[R] */
int zs_topic_logprob_f32(const void* B, const void* X, const void* prep, void* part, void* lp, int64_t R, int64_t K, int64_t V,
                         int64_t Dx, void* stream);
int zs_topic_logprob_f64(const void* B, const void* X, const void* prep, void* part, void* lp, int64_t R, int64_t K, int64_t V,
                         int64_t Dx, void* stream);

/* dH T[R, K] */
int zs_topic_grad_doc_f32(const void* B, const void* X, const void* g, const void* prep, void* part, void* dH, int64_t R,
                          int64_t K, int64_t V, int64_t Dx, int64_t splits, void* stream);
int zs_topic_grad_doc_f64(const void* B, const void* X, const void* g, const void* prep, void* part, void* dH, int64_t R,
                          int64_t K, int64_t V, int64_t Dx, int64_t splits, void* stream);

/* dB T[K, V] */
int zs_topic_grad_topic_f32(const void* B, const void* X, const void* g, const void* prep, void* part, void* dB, int64_t R,
                            int64_t K, int64_t V, int64_t Dx, void* stream);
int zs_topic_grad_topic_f64(const void* B, const void* X, const void* g, const void* prep, void* part, void* dB, int64_t R,
                            int64_t K, int64_t V, int64_t Dx, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ZS_TOPIC_H */
