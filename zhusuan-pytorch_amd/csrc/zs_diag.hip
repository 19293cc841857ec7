// The chain diagnostics: split R-hat, effective sample size and autocorrelation of a stack of Markov chains
// (include/zs_diag.h; its own library, ../lib/libzs_diag.so, `make diag`).
//
// A torch composition of the estimator takes about a dozen passes over the [T, C, E] array (chain means, variances, padded
// FFTs of every series, inverse FFTs, a cumulative test over all T lags) and complex temporaries of twice its size; here it is
// one launch.  A lane owns an element: its loads are one coalesced row per draw across the wave, its sums are doubles in its own
// registers (zs_diag_math.h), and it leaves the lag loop at the pair where Geyer's rule stops, so the work follows the chain's
// autocorrelation time, not T.  No LDS, no atomics, nothing crosses a lane.
#include "zs_common.h"
#include "zs_diag_math.h"
#include "../../include/zs_hip.h"
#include "../../include/zs_diag.h"

#pragma clang fp contract(off)

using namespace zs;

namespace {

template <typename T>
__global__ __launch_bounds__(ZS_DIAG_THREADS) void k_diag_summary(const T* __restrict__ x, int64_t st, int64_t sc, int64_t T_, int64_t C,
                                                                  int64_t E, int split, int64_t max_lag, T* __restrict__ mean,
                                                                  T* __restrict__ var_plus, T* __restrict__ rhat, T* __restrict__ ess,
                                                                  int32_t* __restrict__ lags, int32_t* __restrict__ capped) {
  const int64_t e = (int64_t)blockIdx.x * ZS_DIAG_THREADS + threadIdx.x;
  if (e < E) diag_summary_element<T>(x, st, sc, T_, C, split, max_lag, e, mean, var_plus, rhat, ess, lags, capped);
}

template <typename T>
__global__ __launch_bounds__(ZS_DIAG_THREADS) void k_diag_autocorr(const T* __restrict__ x, int64_t st, int64_t sc, int64_t T_, int64_t C,
                                                                   int64_t E, int64_t L, T* __restrict__ acf) {
  const int64_t e = (int64_t)blockIdx.x * ZS_DIAG_THREADS + threadIdx.x;
  if (e < E) diag_autocorr_element<T>(x, st, sc, T_, C, E, L, e, acf);
}

// what both entry points check first: 0 = go on, 1 = nothing to do, else the code to return
int check_operand(const void* x, int64_t st, int64_t sc, int64_t T_, int64_t C, int64_t E, bool anything_to_write) {
  if (!x || T_ < 0 || C < 0 || E < 0 || !anything_to_write) return ZS_EINVAL;
  if (E >= ((int64_t)1 << 31)) return ZS_ENOTSUP;
  if (T_ == 0 || C == 0 || E == 0) return 1;
  if (!diag_strides_ok(st, sc, T_, C, E)) return ZS_EINVAL;
  return 0;
}

unsigned blocks_for(int64_t E) { return (unsigned)((E + ZS_DIAG_THREADS - 1) / ZS_DIAG_THREADS); }          // E < 2^31

template <typename T>
int diag_summary(const void* x, int64_t st, int64_t sc, int64_t T_, int64_t C, int64_t E, int split, int64_t max_lag, void* mean,
                 void* var_plus, void* rhat, void* ess, int32_t* lags, int32_t* capped, void* stream) {
  const int rc = check_operand(x, st, sc, T_, C, E, mean || var_plus || rhat || ess || lags || capped);
  if (rc) return rc == 1 ? 0 : rc;
  if ((split ? T_ / 2 : T_) < 2) return ZS_EINVAL;
  hipLaunchKernelGGL((k_diag_summary<T>), dim3(blocks_for(E)), dim3(ZS_DIAG_THREADS), 0, (hipStream_t)stream, (const T*)x, st, sc, T_, C, E,
                     split, max_lag, (T*)mean, (T*)var_plus, (T*)rhat, (T*)ess, lags, capped);
  ZS_CHECK_LAUNCH();
  return 0;
}

template <typename T>
int diag_autocorr(const void* x, int64_t st, int64_t sc, int64_t T_, int64_t C, int64_t E, int64_t L, void* acf, void* stream) {
  const int rc = check_operand(x, st, sc, T_, C, E, acf != nullptr);
  if (rc == ZS_EINVAL || rc == ZS_ENOTSUP) return rc;
  if (L < 0 || (rc == 0 && L > T_ - 1)) return ZS_EINVAL;
  if (rc == 1) return 0;
  hipLaunchKernelGGL((k_diag_autocorr<T>), dim3(blocks_for(E)), dim3(ZS_DIAG_THREADS), 0, (hipStream_t)stream, (const T*)x, st, sc, T_, C, E,
                     L, (T*)acf);
  ZS_CHECK_LAUNCH();
  return 0;
}

}  // namespace

extern "C" int zs_diag_abi_version(void) { return ZS_DIAG_ABI_VERSION; }

#define ZS_DIAG_ENTRY(SFX, T)                                                                                                        \
  extern "C" int zs_diag_summary##SFX(const void* x, int64_t st, int64_t sc, int64_t T_, int64_t C, int64_t E, int split,            \
                                      int64_t max_lag, void* mean, void* var_plus, void* rhat, void* ess, int32_t* lags,             \
                                      int32_t* capped, void* stream) {                                                               \
    return diag_summary<T>(x, st, sc, T_, C, E, split, max_lag, mean, var_plus, rhat, ess, lags, capped, stream);                    \
  }                                                                                                                                  \
  extern "C" int zs_diag_autocorr##SFX(const void* x, int64_t st, int64_t sc, int64_t T_, int64_t C, int64_t E, int64_t L, void* acf, \
                                       void* stream) {                                                                               \
    return diag_autocorr<T>(x, st, sc, T_, C, E, L, acf, stream);                                                                    \
  }

ZS_DIAG_ENTRY(_f32, float)
ZS_DIAG_ENTRY(_f64, double)
