/*
 * zs_mcmc.h -- C ABI of the stochastic-gradient MCMC update (libzs_mcmc.so, gfx950).
 *
 * A second library next to libzs_hip.so (include/zs_hip.h), with the same conventions: every pointer inside a table
 * entry is a DEVICE pointer owned by the caller, nothing is allocated, freed or synchronised inside a call, `stream` is a
 * hipStream_t passed as void* (NULL = the null stream), the return value is 0 on success, a positive hipError_t if the
 * launch failed, ZS_EINVAL / ZS_ENOTSUP (the codes of zs_hip.h) for rejected arguments.  A call only enqueues one kernel:
 * it can be captured in a hipGraph.
 *
 * One entry point replaces the per-latent update loops of the reference's samplers (thuwzy/ZhuSuan-PyTorch, paths relative
 * to its root): zhusuan/mcmc/SGLD.py:42-54 (SGLD), SGLD.py:67-82 (PSGLD) and zhusuan/mcmc/SGHMC.py:25-56 (SGHMC).  There, per
 * latent and step, one torch.normal on the host, three to six element-wise kernels and a detach; here ONE launch over all
 * latents of a step: the tensors form one flat index space [start[s], start[s+1]), a thread owns four consecutive elements
 * and finds their tensor by bisection (as zs_adam_step of zs_hip.h), the noise is drawn in registers, every operand is read
 * once and written once.
 *
 * With T the element type, g the gradient of the log joint, z a standard normal, a / v the state:
 *
 *   ZS_MCMC_SGLD        q' = q + (lr/2) g + sqrt(lr) z                                             SGLD.py:50-52
 *   ZS_MCMC_PSGLD       a' = decay a + (1 - decay) g^2 ;  G = 1 / (epsilon + sqrt(a'))              SGLD.py:77-78
 *                       q' = q + (lr/2) G g + sqrt(lr G) z                                         SGLD.py:79-80
 *   ZS_MCMC_SGHMC_PRE   (before the gradient)  v' = RESAMPLE_V ? sqrt(lr) z : v                    SGHMC.py:26-27,32-33
 *                       q' = SECOND_ORDER ? q + v'/2 : q                                           SGHMC.py:35-36
 *   ZS_MCMC_SGHMC_POST  first order:   v' = (1 - alpha) v + lr g + sqrt(2 (alpha - beta) lr) z     SGHMC.py:47
 *                                      q' = q + v'                                                 SGHMC.py:48
 *                       SECOND_ORDER:  d = exp(-alpha/2) ;  v' = d (d v + lr g + sqrt(2 (alpha - beta) lr) z)   SGHMC.py:52-53
 *                                      q' = q + v'/2                                               SGHMC.py:54
 *
 * Scalars derived from the hyper-parameters (lr/2, sqrt(lr), 1 - decay, exp(-alpha/2), ...) are formed once in double on
 * the host and rounded to T; the element arithmetic (csrc/zs_mcmc_math.h) is in T.
 *
 * Noise contract.  The standard normal of flat element i of a launch is bit-identical to element i of what
 * zs_philox_normal_f32(out, n, seed, call, rng_state) of zs_hip.h writes: component i % 4 of the Philox4x32-10 Box-Muller
 * group i / 4 of (seed, call); with rng_state (DEVICE pointer to two uint64 {seed, base}) non-NULL the kernel itself reads
 * seed = rng_state[0] and uses call + rng_state[1].  Where a tensor's `z` is non-NULL the kernel reads z[i - start] instead
 * and nothing else in the arithmetic changes.  For _f64 the drawn value is the same fp32 number widened; everything after it
 * is in double.
 */
#ifndef ZS_MCMC_H
#define ZS_MCMC_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ZS_MCMC_ABI_VERSION 1
#define ZS_MCMC_MAX_TENSORS 32

/* kind */
#define ZS_MCMC_SGLD 0
#define ZS_MCMC_PSGLD 1
#define ZS_MCMC_SGHMC_PRE 2
#define ZS_MCMC_SGHMC_POST 3

/* flags (SGHMC kinds) */
#define ZS_MCMC_SECOND_ORDER 1
#define ZS_MCMC_RESAMPLE_V 2

/* One tensor of the launch (HOST table; the pointers in it are device pointers to T).
 *   q_in, q_out   current and updated value; q_out may equal q_in
 *   grad          gradient of the log joint w.r.t. q_in (SGLD, PSGLD, SGHMC_POST; ignored by SGHMC_PRE)
 *   state         PSGLD's running second moment / SGHMC's velocity, updated in place (ignored by SGLD)
 *   z             injected standard normals, or NULL: drawn from the Philox stream
 *   start         flat index of the tensor's first element: start of entry 0 is 0, strictly ascending, the last tensor ends at n */
struct zs_mcmc_tensor {
  const void* q_in;
  void* q_out;
  const void* grad;
  void* state;
  const void* z;
  int64_t start;
};

/* ABI version of the loaded library (== ZS_MCMC_ABI_VERSION). */
int zs_mcmc_abi_version(void);

/* The update of `n_tensors` (<= ZS_MCMC_MAX_TENSORS, else ZS_ENOTSUP) tensors with `n` elements in all, in one launch.
 * ZS_EINVAL: unknown kind or flag, n < 0, lr < 0 (or NaN), PSGLD with decay outside [0, 1) or epsilon < 0, SGHMC_POST
 * with alpha < beta, a NULL q_in / q_out, a NULL grad or state where the kind reads it, starts that are not 0-based and
 * strictly ascending below n.  n == 0 returns 0 and launches nothing.  Hyper-parameters a kind does not use are ignored.
 * 16-byte loads and stores are used when every start and n are multiples of 4 and every pointer is 16-byte aligned
 * (32-byte for _f64); any other layout takes the element path, with the same results bit for bit. */
int zs_mcmc_update_f32(int kind, const struct zs_mcmc_tensor* tensors, int n_tensors, int64_t n, double lr, double decay,
                       double epsilon, double alpha, double beta, int flags, uint64_t seed, uint64_t call,
                       const uint64_t* rng_state, void* stream);
int zs_mcmc_update_f64(int kind, const struct zs_mcmc_tensor* tensors, int n_tensors, int64_t n, double lr, double decay,
                       double epsilon, double alpha, double beta, int flags, uint64_t seed, uint64_t call,
                       const uint64_t* rng_state, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ZS_MCMC_H */
