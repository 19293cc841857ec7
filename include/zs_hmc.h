/*
 * zs_hmc.h -- C ABI of Hamiltonian Monte Carlo with a Metropolis correction (libzs_hmc.so, gfx950).
 *
 * A fourth library next to libzs_hip.so, libzs_mcmc.so and libzs_flow.so, with the conventions of zs_mcmc.h: every pointer
 * inside a table entry is a DEVICE pointer owned by the caller, nothing is allocated, freed or synchronised inside a call,
 * `stream` is a hipStream_t passed as void* (NULL = the null stream), the return value is 0 on success, a positive
 * hipError_t if the launch failed, ZS_EINVAL / ZS_ENOTSUP (the codes of zs_hip.h) for rejected arguments, which write
 * nothing.  A call only enqueues one kernel.
 *
 * The latents of a launch form one flat index space [start[s], start[s+1]); a thread owns four consecutive elements and
 * finds their tensor by bisection.  There are C chains; tensor s holds `row[s]` elements per chain, chain-major, so that
 * flat element i of tensor s belongs to chain (i - start[s]) / row[s], and start[s+1] - start[s] = C row[s].
 *
 * Arithmetic (unit mass).  T is the element type, eps the step size -- a double in the device-resident state block, read
 * by the kernels themselves and rounded to T for the element arithmetic, as is eps/2 -- g the gradient of the log joint,
 * z standard normals.  Every multiply-add below is one fma in T.
 *
 *   ZS_HMC_BEGIN   p0 = z ;  K0[c] = 1/2 sum_{i in chain c} p0_i^2 ;  p = p0 + (eps/2) g(q0) ;  q = q0 + eps p
 *   ZS_HMC_STEP    p = p + eps g(q) ;  q = q + eps p                                           (L - 1 times)
 *   ZS_HMC_END     pL = p + (eps/2) g(q) ;  K1[c] = 1/2 sum pL_i^2                              (pL is not stored)
 *   decide         dH[c] = (logp1[c] - logp0[c]) - (K1[c] - K0[c])                              in double
 *                  a[c]  = finite(dH) ? exp(min(0, dH)) : 0 ;  accept[c] = finite(dH) && log(u[c]) < dH[c]
 *                  abar  = mean_c a[c]                                                          fixed order, double
 *                  adapting:  m += 1 ;  Hbar = (1 - 1/(m + t0)) Hbar + (delta - abar)/(m + t0)
 *                             log eps = mu - (sqrt(m)/gamma) Hbar ,  mu = log(10 eps_initial)
 *                             log epsbar = m^-kappa log eps + (1 - m^-kappa) log epsbar ;  next eps = exp(log eps)
 *                  not adapting, after having adapted (m > 0): next eps = exp(log epsbar) ;  never adapted: eps unchanged
 *   select         q_out = accept[chain(i)] ? q : q0
 *
 * So a NaN or +-inf anywhere in logp1 or K1 of a chain rejects that chain and only that chain.
 *
 * Kinetic sums.  p^2 is formed in T and summed in T in a fixed order without floating-point atomics: the flat index space
 * is cut into tiles of ZS_HMC_TILE elements, one workgroup sums the squares of a tile per (tensor, chain) by a segmented
 * tree in LDS whose shape depends on the flat indices only -- the same call repeated, and the vector and the element form,
 * give the same bits -- and writes one partial per (tensor, chain, tile) into the caller's workspace `ksum`:
 *
 *   pieces(row) = (row + ZS_HMC_TILE - 2) / ZS_HMC_TILE + 1       tiles that `row` consecutive flat elements can touch
 *   slots       = sum_s pieces(row[s])                            zs_hmc_ksum_slots()
 *   ksum        : C * slots elements of T, chain-major: the partial of (tensor s, chain c, k-th tile touched by that chain's
 *                 row) is ksum[c * slots + sum_{s' < s} pieces(row[s']) + k]; a row that touches one tile fewer than
 *                 pieces(row) gets a zero in its last slot.  Every element of ksum is written by a BEGIN or END launch.
 *
 * This covers one chain across many workgroups (C = 1, many tiles: many slots) and many chains per wave (row = 1: one slot
 * per chain, 1024 chains per tile).  `decide` adds the partials of a chain in double in slot order, chunk after chunk, and
 * halves the sum; everything of `decide` is in double.
 *
 * Noise contract, as in zs_mcmc.h.  The momentum of flat element i of a BEGIN launch is bit-identical to element i of what
 * zs_philox_normal_f32(out, n, seed, call, rng_state) of zs_hip.h writes; u[c] of decide is element c of
 * zs_philox_uniform_f32(out, C, seed, call, rng_state).  With rng_state (DEVICE pointer to two uint64 {seed, base})
 * non-NULL the kernel itself reads seed = rng_state[0] and uses call + rng_state[1].  A non-NULL `z` of a tensor, or `u` of
 * decide, replaces the draw and changes nothing else.  For _f64 the drawn fp32 number is widened.
 *
 * State block (DEVICE, 8 doubles, owned by the caller, initialised as {eps_initial, eps_initial, 0, 0, 0, 0, 0, 0}):
 *   [0] eps (read by the move kernels, replaced by decide)   [1] eps_initial   [2] m   [3] Hbar   [4] log eps
 *   [5] log epsbar   [6] abar of the last decide   [7] number of chains accepted by the last decide
 */
#ifndef ZS_HMC_H
#define ZS_HMC_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ZS_HMC_ABI_VERSION 1
#define ZS_HMC_MAX_TENSORS 32
#define ZS_HMC_MAX_CHUNKS 16
#define ZS_HMC_TILE 1024
#define ZS_HMC_STATE_DOUBLES 8

/* kind of a move */
#define ZS_HMC_BEGIN 0
#define ZS_HMC_STEP 1
#define ZS_HMC_END 2

/* One tensor of a move or select launch (HOST table; the pointers in it are device pointers to T).
 *   q0      position at the start of the trajectory (read by BEGIN and select)
 *   q       trajectory position: written by BEGIN, updated in place by STEP, read by select; may not alias q0
 *   p       momentum: written by BEGIN, updated in place by STEP, read by END
 *   grad    gradient of the log joint at q0 (BEGIN) or at q (STEP, END)
 *   z       BEGIN: injected standard normals, or NULL: drawn from the Philox stream
 *   p0      BEGIN: where the initial momentum is written, or NULL
 *   q_out   select: the result; may equal q0 or q
 *   start   flat index of the tensor's first element: start of entry 0 is 0, ascending, the last tensor ends at n
 *   row     elements per chain (>= 1): the tensor has exactly C * row elements */
struct zs_hmc_tensor {
  const void* q0;
  void* q;
  void* p;
  const void* grad;
  const void* z;
  void* p0;
  void* q_out;
  int64_t start;
  int64_t row;
};

/* The kinetic partials of one chunk (one move table) for decide: k0 written by its BEGIN, k1 by its END, `slots` as above. */
struct zs_hmc_chunk {
  const void* k0;
  const void* k1;
  int64_t slots;
  int32_t is_f64; /* element type of k0 / k1: 0 float, 1 double */
  int32_t pad;
};

/* ABI version of the loaded library (== ZS_HMC_ABI_VERSION). */
int zs_hmc_abi_version(void);

/* slots per chain of the ksum workspace for tensors with these rows (host arithmetic; -1 for a NULL table or a row < 1) */
int64_t zs_hmc_ksum_slots(const int64_t* rows, int n_tensors);

/* One move of kind BEGIN / STEP / END over `n_tensors` (<= ZS_HMC_MAX_TENSORS, else ZS_ENOTSUP) tensors with `n` elements
 * in all and C chains, in one launch.  `state`: the state block (eps is read from it on the device).  `ksum`: the workspace
 * of C * slots elements of T (BEGIN, END; ignored by STEP).  seed / call / rng_state: BEGIN's momentum draw.
 * ZS_EINVAL: unknown kind, n < 0, C < 0, a NULL state, a NULL pointer where the kind reads or writes (q0, q, p, grad for
 * BEGIN; q, p, grad for STEP; p, grad for END; ksum for BEGIN and END), starts that are not 0-based and ascending, a row < 1
 * or a tensor whose length is not C * row.  n == 0 or C == 0 returns 0 and launches nothing.
 * 16-byte loads and stores (32-byte for _f64) are used when every start and row is a multiple of 4 and every pointer is
 * aligned; any other layout takes the element path, with the same results bit for bit. */
int zs_hmc_move_f32(int kind, const struct zs_hmc_tensor* tensors, int n_tensors, int64_t n, int64_t C, const double* state,
                    void* ksum, uint64_t seed, uint64_t call, const uint64_t* rng_state, void* stream);
int zs_hmc_move_f64(int kind, const struct zs_hmc_tensor* tensors, int n_tensors, int64_t n, int64_t C, const double* state,
                    void* ksum, uint64_t seed, uint64_t call, const uint64_t* rng_state, void* stream);

/* The accept decision of C chains from the kinetic partials of `n_chunks` (1 .. ZS_HMC_MAX_CHUNKS, else ZS_ENOTSUP) chunks
 * and the log joints at both ends (T[C]; T is the suffix's type, also of an injected `u`, T[C] or NULL: drawn), and the
 * step-size update, in one launch of one workgroup.  Writes accept (int32[C], 0 / 1), out (double[5 C]: a, the Hamiltonian
 * -logp0 + K0 at the start, -logp1 + K1 at the end, dH, and the log joint of the selected state, C each) and the state block.
 * `adapting` != 0 runs the dual-averaging update with target acceptance `delta` and gamma, t0, kappa.
 * ZS_EINVAL: C < 0, n_chunks < 1, a NULL chunks / k0 / k1 / logp0 / logp1 / state / out / accept, slots < 1, and, when
 * adapting, delta outside (0, 1), gamma <= 0, t0 < 0 or kappa outside (0.5, 1].  C == 0 returns 0 and launches nothing. */
int zs_hmc_decide_f32(const struct zs_hmc_chunk* chunks, int n_chunks, int64_t C, const void* logp0, const void* logp1,
                      const void* u, double* state, double* out, int32_t* accept, int adapting, double delta, double gamma,
                      double t0, double kappa, uint64_t seed, uint64_t call, const uint64_t* rng_state, void* stream);
int zs_hmc_decide_f64(const struct zs_hmc_chunk* chunks, int n_chunks, int64_t C, const void* logp0, const void* logp1,
                      const void* u, double* state, double* out, int32_t* accept, int adapting, double delta, double gamma,
                      double t0, double kappa, uint64_t seed, uint64_t call, const uint64_t* rng_state, void* stream);

/* q_out = accept[chain] ? q : q0 over the tensors of a move table, in one launch.  ZS_EINVAL / ZS_ENOTSUP as for a move
 * (NULL q0, q, q_out or accept). */
int zs_hmc_select_f32(const struct zs_hmc_tensor* tensors, int n_tensors, int64_t n, int64_t C, const int32_t* accept,
                      void* stream);
int zs_hmc_select_f64(const struct zs_hmc_tensor* tensors, int n_tensors, int64_t n, int64_t C, const int32_t* accept,
                      void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ZS_HMC_H */
