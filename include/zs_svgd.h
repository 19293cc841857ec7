/*
 * zs_svgd.h -- C ABI of Stein variational gradient descent (Liu & Wang 2016) over a set of K interacting particles
 * (libzs_svgd.so, gfx950), on the matrix cores (v_mfma_f32_16x16x4_f32 / v_mfma_f64_16x16x4_f64).
 *
 * A twelfth library next to libzs_hip.so and the other satellites, with the conventions of zs_mvn.h: every pointer inside a
 * table entry, and every other pointer, is a DEVICE pointer owned by the caller, nothing is allocated, freed or synchronised
 * inside a call, `stream` is a hipStream_t passed as void* (NULL = the null stream), the return value is 0 on success, a positive
 * hipError_t if the launch failed, ZS_EINVAL / ZS_ENOTSUP (the codes of zs_hip.h) for rejected arguments, which write nothing.
 * A call enqueues one kernel.  T is the element type of the suffix (_f32: float, _f64: double).  Every access is one element
 * wide and there are no atomics: the results do not depend on the alignment of the operands and the same call gives the same bits.
 *
 * Shapes.  K particles; the latents of a call are a HOST table of n_tensors (1 .. ZS_SVGD_MAX_TENSORS) tensors forming one flat
 * column space of D = sum_t row[t] columns: tensor t is contiguous T[K, row[t]] and owns the columns [col[t], col[t] + row[t]),
 * col[0] = 0, col[t + 1] = col[t] + row[t].  `start` of an entry is its first flat ELEMENT, K col[t] (the running element count
 * of zhusuan/_binding.flat_table), and n = K D is the total element count.  theta_i in R^D is row i of all tensors laid end to
 * end, g_i = grad of log p at theta_i likewise.
 *
 *   d_ij   = | theta_i - theta_j |^2                       (>= 0, the diagonal exactly 0, d_ij = d_ji bit for bit)
 *   h      = bandwidth, or med / log(K + 1), med the median of all K^2 entries of d (the mean of the two middle values for an
 *            even count), h = 1 when med == 0
 *   k_ij   = exp(-d_ij / h) ;  s_i = sum_j k_ij
 *   phi_i  = (1/K) sum_j [ k_ji g_j + (2/h) k_ji (theta_i - theta_j) ]
 *   plain    theta_i <- theta_i + step_size phi_i
 *   adagrad  H <- phi^2 (first != 0)  or  alpha H + (1 - alpha) phi^2 ;  theta_i <- theta_i + step_size phi_i / (fudge + sqrt(H))
 *
 * One step over one table is three launches:
 *
 * S1 zs_svgd_gram.  A workgroup (eight waves) owns slabs of ZS_SVGD_SLAB consecutive columns and holds all K particles of a slab
 *   in LDS (rows up to the next multiple of 16 are zero), subtracts every column's mean over the particles (any constant per
 *   column leaves d unchanged; the centred Gram matrix G = C C^T gives d_ij = G_ii + G_jj - 2 G_ij without the cancellation of a
 *   cloud far from the origin) and accumulates the 16 x 16 tile pairs (bi >= bj) of G on the matrix cores, four columns per
 *   instruction, the pairs dealt over the waves (pair p to wave p % 8) with the accumulators in registers.  Workgroups are
 *   persistent: zs_svgd_gram_slots(D) = min(ceil(D / ZS_SVGD_SLAB), ZS_SVGD_GRID_CAP) of them walk the slabs, workgroup w the
 *   slabs w, w + slots, ..., and each writes ONE partial, double[K, K] (both triangles), at partials + w K K.  Partials are double
 *   whatever T is: the tables of a step -- of both element types -- write consecutive slot ranges of one buffer.
 * S2 zs_svgd_finish (no suffix: it only sees doubles).  One workgroup adds the n_slots partials in ascending slot order, forms
 *   d (clamped at 0), finds the median by EXACT selection -- non-negative doubles order as their bit patterns, so the value of
 *   rank r is built bit by bit from the top with one workgroup-wide count per bit; not a sort, not an approximation --, forms h
 *   and writes the state block:
 *     state[0] = h   state[1] = 2 / h   state[2] = med (-1 with a given bandwidth)   state[3] = K
 *     state[4 .. 4 + K) = s   state[4 + K .. 4 + K + K K) = k, row-major           zs_svgd_state_doubles(K) doubles in all
 * S3 zs_svgd_update.  Per slab: U = G_slab - (2/h) C_slab (G the gradients, C the centred particles) is staged in LDS; wave b owns
 *   the 16-row strip b of the particles and keeps its strip of k as A operands in registers (K16 / 4 of them), forms k U on the
 *   matrix cores and finishes phi = (k U + (2/h) s_i c_i) / K, the step, and the stores of q_out (and h).  phi depends on
 *   differences only, so the centred rows give the same phi.  q_out may be q_in: a workgroup reads its slab before it writes it and
 *   no other workgroup touches those columns.
 *
 * Caps.  K <= zs_svgd_max_particles_of(sizeof(T)): 256 for _f32, 128 for _f64 (the strip of k in registers: K16 / 4 doubles are
 * K16 / 2 registers, and the sixteen waves of K = 256 leave a wave 128 registers), finish: K <= 256.
 *
 * ZS_EINVAL: a NULL table / partials / state, n_tensors < 1, K < 1, n < 0, n_slots < 1, a NULL q_in (gram), q_in / grad / q_out
 * (update) or h (update with adagrad), row < 1, a start that is not K col[t], n != K D, a bandwidth <= 0 (or NaN) without
 * `median`, step_size / alpha / fudge NaN.  ZS_ENOTSUP: K above the cap, n_tensors > ZS_SVGD_MAX_TENSORS.
 */
#ifndef ZS_SVGD_H
#define ZS_SVGD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ZS_SVGD_ABI_VERSION 1
#define ZS_SVGD_MAX_TENSORS 32
#define ZS_SVGD_MAX_PARTICLES 256
#define ZS_SVGD_MAX_PARTICLES_F64 128
#define ZS_SVGD_SLAB 32          /* columns of a slab */
#define ZS_SVGD_GRID_CAP 128     /* most workgroups, and partials, of one gram launch */
#define ZS_SVGD_STATE_HEADER 4   /* doubles before s in the state block */

/* One tensor of a gram or update launch (HOST table; the pointers in it are device pointers to T[K, row]).
 *   q_in    the particles (read by gram and update)
 *   grad    the gradient of the log density at q_in (update)
 *   q_out   update: the moved particles; may equal q_in
 *   h       update with adagrad: the second-moment state, read (unless first) and written
 *   start   flat index of the tensor's first element, K col[t]
 *   row     columns of the tensor (>= 1) */
struct zs_svgd_tensor {
  const void* q_in;
  const void* grad;
  void* q_out;
  void* h;
  int64_t start;
  int64_t row;
};

int zs_svgd_abi_version(void);
int zs_svgd_max_particles(void);                    /* 256 */
int zs_svgd_max_particles_of(int elem_bytes);       /* 4: 256, 8: 128, else 0 */
int zs_svgd_slab(void);                             /* ZS_SVGD_SLAB */
int zs_svgd_grid_cap(void);                         /* ZS_SVGD_GRID_CAP */
int64_t zs_svgd_gram_slots(int64_t D);              /* partials a gram launch over D columns writes; -1 for D < 1 */
int64_t zs_svgd_partial_doubles(int64_t K);         /* K K; -1 for K outside 1 .. 256 */
int64_t zs_svgd_state_doubles(int64_t K);           /* 4 + K + K K; -1 likewise */

/* S1: writes zs_svgd_gram_slots(n / K) partials at `partials`. */
int zs_svgd_gram_f32(const struct zs_svgd_tensor* tensors, int n_tensors, int64_t n, int64_t K, double* partials, void* stream);
int zs_svgd_gram_f64(const struct zs_svgd_tensor* tensors, int n_tensors, int64_t n, int64_t K, double* partials, void* stream);

/* S2: `median` != 0 takes the median rule and ignores `bandwidth`; else h = bandwidth > 0. */
int zs_svgd_finish(const double* partials, int64_t n_slots, int64_t K, int median, double bandwidth, double* state, void* stream);

/* S3: reads the state block that S2 wrote. */
int zs_svgd_update_f32(const struct zs_svgd_tensor* tensors, int n_tensors, int64_t n, int64_t K, const double* state,
                       double step_size, int adagrad, int first, double alpha, double fudge, void* stream);
int zs_svgd_update_f64(const struct zs_svgd_tensor* tensors, int n_tensors, int64_t n, int64_t K, const double* state,
                       double step_size, int adagrad, int first, double alpha, double fudge, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ZS_SVGD_H */
