/*
 * zs_lowrank.h -- C ABI of MultivariateNormalLowRank (libzs_lowrank.so, gfx950): a normal with mean `mean` and covariance
 * diag(d) + W W^T, W = `factor` [D, r] -- the log-density of given values, its backward, the draw and its backward.  Nothing of
 * size D x D exists anywhere: every heavy step is a thin product against the factor on v_mfma_f32_16x16x4_f32 /
 * v_mfma_f64_16x16x4_f64, with the D axis streamed through LDS in panels, so D is capped only by the grid (65 536).
 *
 * A fourteenth library next to libzs_hip.so and the other satellites, with the conventions of zs_mvn.h: every pointer is a DEVICE
 * pointer owned by the caller, nothing is allocated, freed or synchronised inside a call, `stream` is a hipStream_t passed as
 * void* (NULL = the null stream), the return value is 0 on success, a positive hipError_t if a launch failed, ZS_EINVAL /
 * ZS_ENOTSUP (the codes of zs_hip.h) for rejected arguments, which write nothing.  T is the element type of the suffix (_f32:
 * float, _f64: double).  Every access is one element wide and there are no atomics: the results do not depend on the alignment
 * of the operands, and the same call gives the same bits.
 *
 * Shapes.  R rows (the product of the batch shape), D dimensions, rank r, K particles; every operand is contiguous:
 *   mean T[R, D];  factor T[R, D, r];  diag T[R, D] (> 0, not checked);  per-particle tensors T[K, R, D];  lp T[K, R].
 * A value x is T[K, R, D] or T[R, D] (Px = K R D or R D elements; without the particle axis it is shared by the particles).
 *
 * The arithmetic.  Wd = W / d[:, None], C = I_r + W^T Wd (the capacitance), y = x - mean:
 *   u  = y Wd                                                          [K, r]
 *   lp = -1/2 (sum y^2 / d - |L^-1 u|^2) - 1/2 (sum log d + log|C|) - D/2 log 2 pi,   C = L L^T
 *   v  = u C^-1 ,  a = Sigma^-1 y = (y - v W^T) / d                    (A W = V: Sigma^-1 W = Wd C^-1)
 *   gx = -g a ;  gmean = sum_k g a ;  gfactor = A^T diag(g) V - (sum g) Wd C^-1 ;
 *   gdiag = 1/2 (sum_k g a^2 - (sum g) (1/d - rowsum((Wd C^-1) o Wd)))
 *   draw:  z = mean + sqrt(d) o eps_D + eps_r W^T ;  gmean = sum_k gz ;  gfactor = Gz^T E_r ;  gdiag = sum_k gz eps_D / (2 sqrt d)
 *
 * Calling order.  zs_lowrank_prepare writes the `prep` workspace of (factor, diag) -- per row (L^-1)^T, C^-1, log|C| and
 * sum log d -- which zs_lowrank_logprob and zs_lowrank_logprob_bwd read; it needs a `part` workspace and a number of D-splits.
 * zs_lowrank_logprob_bwd needs a `part` workspace and a number of particle shares.  zs_lowrank_splits gives the counts that fill
 * the device, zs_lowrank_workspace_elems the sizes in elements of T.  The draw and its backward need neither.
 *
 * ZS_EINVAL: a NULL operand, output or workspace (gx alone may be NULL), K < 0, R < 0, D < 1, r < 1, a period Px that is neither
 * K R D nor R D, splits outside [1, panels of D], shares outside [1, ceil(K / 16)].  ZS_ENOTSUP: D > zs_lowrank_max_dim(),
 * r > zs_lowrank_max_rank(), more than 2^31 - 1 workgroups.  R == 0 (and K == 0 where there are particles) returns 0 and
 * launches nothing.
 *
 * Noise contract, as in zs_mvn.h, over ONE stream of [K, R, D + r] normals: with `eps` NULL, element j of row (k R + row) --
 * j < D: eps_D[j], else eps_r[j - D] -- takes flat element (k R + row) (D + r) + j of what zs_philox_normal_f32(out,
 * K R (D + r), seed, call, rng_state) of zs_hip.h writes, bit-identical, widened for _f64; with rng_state (DEVICE pointer to two
 * uint64 {seed, base}) non-NULL the kernel itself reads seed = rng_state[0] and uses call + rng_state[1].  A non-NULL `eps`
 * T[K, R, D + r] replaces the stream and changes nothing else.
 *
 * Kernel shape.  A panel is 64 rows of the D axis of one row's factor, staged in LDS as [64][81] with the rank columns past r
 * and the rows past D zeroed (zs_lowrank_math.h has the bank arithmetic of the 81 and of the [16][68] particle operands); a
 * workgroup is four waves.
 *   prepare      grid = rows x D-splits.  A split streams its panels; the (r/16)^2 tiles of W^T Wd are dealt to the waves and
 *                accumulate in accumulator registers over the whole split; one partial [rp, rp] (rp = r rounded up to 16) and one
 *                partial sum log d per split.  The finish, a workgroup per row, adds the partials in split order, adds I,
 *                factors C in LDS (right-looking Cholesky), inverts L into the unused upper triangle, and writes prep.
 *   logprob      grid = rows x 16-particle tiles.  Per panel the workgroup stages the factor, 1 / d and y of its 16 particles;
 *                the four waves take every fourth k-step of the panel, each for all rank tiles: u tiles in accumulators.  The
 *                waves' partial u and sum y^2 / d combine through LDS in wave order; wave t forms rank tile t of u (L^-1)^T as a
 *                second product, squares and sums it; lp is written once per particle.
 *   logprob_bwd  grid = rows x particle shares; a share walks its 16-particle tiles.  Per tile: u as above, v = u C^-1 by the
 *                same second product, then a second pass over the panels in which wave t owns 16 of the 64 d-rows: the tile
 *                v W^T ([16, r] x [r, 16], the panel read transposed) gives a where the accumulator has it; gx is written, g a and
 *                g a^2 are summed over the tile, and a -- left in the accumulator -- is the A operand of A^T diag(g) V, whose
 *                contraction runs over the tile's 16 particles.  A share adds its tiles into ITS partial (the same thread, in tile
 *                order); the finish, a wave per d-row, adds the shares in order and applies the closed forms ((Wd C^-1) row by row
 *                from C^-1 in LDS).
 *   sample       grid = (rows x particle tiles, panels): eps_r of the tile in LDS, the tile eps_r W^T as above, z written once.
 *   sample_bwd   grid = rows x panels; wave t owns 16 d-rows and walks ALL particles in tiles of 16: gz and eps_r are read from
 *                memory (or regenerated) straight into the A and B operands of Gz^T E_r; one final result per element, no
 *                partials.  Its time grows linearly in K when R D is small: a K-split is not implemented.
 */
#ifndef ZS_LOWRANK_H
#define ZS_LOWRANK_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ZS_LOWRANK_ABI_VERSION 1

/* which workspace zs_lowrank_workspace_elems sizes, and which count zs_lowrank_splits gives */
#define ZS_LOWRANK_WS_PREP 0         /* prep: R (2 rp^2 + 2) */
#define ZS_LOWRANK_WS_PREPARE 1      /* part of zs_lowrank_prepare: R n (rp^2 + 1), n D-splits */
#define ZS_LOWRANK_WS_LOGPROB_BWD 2  /* part of zs_lowrank_logprob_bwd: R n D (r + 2), n particle shares */

/* ABI version of the loaded library (== ZS_LOWRANK_ABI_VERSION). */
int zs_lowrank_abi_version(void);
/* the widest row (65536) and the largest rank (64) the kernels take */
int zs_lowrank_max_dim(void);
int zs_lowrank_max_rank(void);
/* the D-splits zs_lowrank_prepare (which = ZS_LOWRANK_WS_PREPARE) or the particle shares zs_lowrank_logprob_bwd (which =
 * ZS_LOWRANK_WS_LOGPROB_BWD) should be called with (host arithmetic; 0 for rejected arguments; K is read for the shares only) */
int64_t zs_lowrank_splits(int which, int64_t K, int64_t R, int64_t D);
/* elements of T in workspace `which` (n: the splits or shares, read for the two part workspaces only); -1 for rejected arguments */
int64_t zs_lowrank_workspace_elems(int which, int64_t R, int64_t D, int64_t r, int64_t n);

/* prep from (factor, diag): two launches */
int zs_lowrank_prepare_f32(const void* factor, const void* diag, void* part, void* prep, int64_t R, int64_t D, int64_t r,
                           int64_t splits, void* stream);
int zs_lowrank_prepare_f64(const void* factor, const void* diag, void* part, void* prep, int64_t R, int64_t D, int64_t r,
                           int64_t splits, void* stream);

/* lp T[K, R]: one launch */
int zs_lowrank_logprob_f32(const void* mean, const void* factor, const void* diag, const void* prep, const void* x, int64_t Px,
                           void* lp, int64_t K, int64_t R, int64_t D, int64_t r, void* stream);
int zs_lowrank_logprob_f64(const void* mean, const void* factor, const void* diag, const void* prep, const void* x, int64_t Px,
                           void* lp, int64_t K, int64_t R, int64_t D, int64_t r, void* stream);

/* gx T[K, R, D] (whatever Px is; may be NULL), gmean T[R, D], gfactor T[R, D, r], gdiag T[R, D] from glp T[K, R]: two launches */
int zs_lowrank_logprob_bwd_f32(const void* mean, const void* factor, const void* diag, const void* prep, const void* x, int64_t Px,
                               const void* glp, void* part, void* gx, void* gmean, void* gfactor, void* gdiag, int64_t K, int64_t R,
                               int64_t D, int64_t r, int64_t shares, void* stream);
int zs_lowrank_logprob_bwd_f64(const void* mean, const void* factor, const void* diag, const void* prep, const void* x, int64_t Px,
                               const void* glp, void* part, void* gx, void* gmean, void* gfactor, void* gdiag, int64_t K, int64_t R,
                               int64_t D, int64_t r, int64_t shares, void* stream);

/* z T[K, R, D]: one launch */
int zs_lowrank_sample_f32(const void* mean, const void* factor, const void* diag, const void* eps, void* z, int64_t K, int64_t R,
                          int64_t D, int64_t r, uint64_t seed, uint64_t call, const uint64_t* rng_state, void* stream);
int zs_lowrank_sample_f64(const void* mean, const void* factor, const void* diag, const void* eps, void* z, int64_t K, int64_t R,
                          int64_t D, int64_t r, uint64_t seed, uint64_t call, const uint64_t* rng_state, void* stream);

/* gmean T[R, D], gfactor T[R, D, r], gdiag T[R, D] from gz T[K, R, D], eps injected or regenerated: one launch */
int zs_lowrank_sample_bwd_f32(const void* diag, const void* eps, const void* gz, void* gmean, void* gfactor, void* gdiag, int64_t K,
                              int64_t R, int64_t D, int64_t r, uint64_t seed, uint64_t call, const uint64_t* rng_state, void* stream);
int zs_lowrank_sample_bwd_f64(const void* diag, const void* eps, const void* gz, void* gmean, void* gfactor, void* gdiag, int64_t K,
                              int64_t R, int64_t D, int64_t r, uint64_t seed, uint64_t call, const uint64_t* rng_state, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ZS_LOWRANK_H */
