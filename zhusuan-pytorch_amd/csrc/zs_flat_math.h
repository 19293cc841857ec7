// What all seven satellite libraries share (zs_mcmc.hip and zs_hmc.hip directly; zs_flow.hip, zs_cat.hip, zs_mvn.hip, zs_klpq.hip
// and zs_nf.hip through zs_group_math.h): the explicit fma, the index maps of a flat index space over a table of tensors, and
// the 16-byte group of four.  __host__ __device__, so that the host-side sanitizer tests (tests/host_math/) run the same code.
#pragma once
#include <stdint.h>
#include <hip/hip_runtime.h>

#ifndef ZS_HD
#define ZS_HD __host__ __device__ __forceinline__
#endif

namespace zs {

// one wide access per operand: four consecutive elements of T
template <typename T>
struct alignas(16) Vec4 { T v[4]; };

ZS_HD float flat_fma(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
ZS_HD double flat_fma(double a, double b, double c) { return __builtin_fma(a, b, c); }

// tensor of flat element i: the last s with start[s] <= i (start[0] = 0, ascending)
ZS_HD int flat_tensor_of(const int64_t* start, int n_tensors, int64_t i) {
  int lo = 0, hi = n_tensors - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (start[mid] <= i) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// The element form's walk over one group of four: element j of group gi is flat index 4 gi + j when that is below n,
// else (clamped: the loads stay unconditional, the store is dropped) the group's first element.
ZS_HD int64_t flat_clamped_index(int64_t gi, int j, int64_t n) {
  const int64_t i0 = gi << 2;
  const int cnt = n - i0 < 4 ? (int)(n - i0) : 4;
  return i0 + (j < cnt ? j : 0);
}
ZS_HD bool flat_element_live(int64_t gi, int j, int64_t n) { return (gi << 2) + j < n; }

}  // namespace zs
