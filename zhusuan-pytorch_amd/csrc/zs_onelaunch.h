// Shared pieces of the one-launch kernels (zs_logjoint.hip: LJ1, MS1; zs_layers.hip: PL1, CS1, AB1, PR1): the 4-element vector
// operand and the cross-workgroup hand-off they all end with.  (Their element math is zs_elem_math.h, their reductions
// zs_common.h's.)
#pragma once
#include "zs_elem_math.h"
#include "../../include/zs_hip.h"

using namespace zs;

namespace {

template <typename T>
struct alignas(4 * sizeof(T)) V4 { T v[4]; };

// ---------------------------------------------------------------- cross-workgroup hand-off without a release fence
// "Every workgroup writes partial results, the LAST one to arrive combines them" needs the partials to be visible across
// CUs and XCDs (per-XCD L2s are not coherent with each other, a CU's L1 is never refreshed by other CUs' stores).  An
// agent-scope RELEASE on the ticket does that by writing back the XCD's whole dirty L2 (buffer_wbl2: 1.7 us clean, 6.5 us
// with 16 KB freshly dirtied, per workgroup) -- it was most of these kernels' time.  The cheaper valid form
// (MI355X_MICROARCH.md, inter-workgroup visibility: "ONE lane of each storing workgroup adds to one counter; the workgroup
// whose add came last consumes"):
//   producer  every byte of the hand-off is stored WRITE-THROUGH (relaxed agent-scope atomic store = global_store ... sc1);
//             every storing wave waits for its stores (s_waitcnt vmcnt(0)); workgroup barrier; ONE lane adds to the ticket
//             with a RELAXED agent-scope atomic;
//   consumer  the workgroup whose add returned count - 1: either it reads the hand-off with sc1 loads only (relaxed agent
//             atomic loads; at most a couple per thread: they are issued one after the other), after a workgroup barrier
//             behind the adding lane -- or that lane runs ONE agent-scope acquire (buffer_inv sc1: invalidates this CU's
//             L1), waits for it, and after a barrier the workgroup reads with plain loads (many per thread, batched).
__device__ __forceinline__ void drain_stores() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
template <typename T>
__device__ __forceinline__ void store_wt(T* p, T v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
template <typename T>
__device__ __forceinline__ T load_wt(const T* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ unsigned ticket_take(unsigned* t) {
  return __hip_atomic_fetch_add(t, 1u, ZS_TICKET_ORDER, __HIP_MEMORY_SCOPE_AGENT);      // (relaxed; acq_rel in the strict build, zs_common.h)
}
__device__ __forceinline__ void ticket_return(unsigned* t) { __hip_atomic_store(t, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

}  // namespace
