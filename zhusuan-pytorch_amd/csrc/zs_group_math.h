// The lane-group map of the satellite kernels that give a row to a group of lanes (zs_cat.hip, zs_mvn.hip, zs_klpq.hip,
// zs_nf.hip): the width of a group, the place of a thread in its group and workgroup, the rows of a workgroup, and the exchanges
// inside a group.  The map is __host__ __device__ and the butterfly has a host restatement, so that the programs under
// tests/host_math/ walk the same code on the host under the sanitizers.
#pragma once
#include <math.h>
#include "zs_flat_math.h"

#ifndef ZS_WAVE
#define ZS_WAVE 64
#endif

namespace zs {

// ---------------------------------------------------------------- the map
// A group of G = 2^k <= 64 consecutive lanes of one wave owns a row; what a lane of the group owns inside the row (a component,
// every G-th particle, every G-th chunk) is the library's own.  G: the smallest power of two >= n, at least 1, at most a wave.
ZS_HD int group_lanes(int64_t n) {
  int g = 1;
  while (g < ZS_WAVE && g < n) g <<= 1;
  return g;
}
struct GroupPlace {
  int lane;         // lane within the group
  int first;        // the group's first lane within its wave of 64
  int grp;          // the group within the workgroup
  int groups;       // groups per workgroup = rows per step
};
// thread `thread` of a workgroup of `threads` (a multiple of G): G divides 64, so a group never crosses its wave
ZS_HD GroupPlace group_place(int thread, int threads, int G) {
  GroupPlace p;
  p.groups = threads / G;
  p.lane = thread & (G - 1);
  p.first = (thread & (ZS_WAVE - 1)) & ~(G - 1);
  p.grp = thread / G;
  return p;
}
// The rows of a workgroup, as the kernels walk them -- the trip count is the same for every lane of the workgroup, so the
// exchanges below are never diverged; a group past the last row idles through them and stores nothing:
//   for (int64_t rb = group_row_first(block, pl); rb < R; rb += group_row_step(blocks, pl)) { r = rb + pl.grp; valid = r < R; ... }
ZS_HD int64_t group_row_first(int block, const GroupPlace& p) { return (int64_t)block * p.groups; }
ZS_HD int64_t group_row_step(int blocks, const GroupPlace& p) { return (int64_t)blocks * p.groups; }
// workgroups of `threads` for rows >= 1 rows in groups of G lanes; past `cap` a workgroup walks several steps
ZS_HD int group_workgroups(int64_t rows, int G, int threads, int cap) {
  const int64_t per = threads / G, b = (rows + per - 1) / per;
  return b > cap ? cap : (int)(b < 1 ? 1 : b);
}

// ---------------------------------------------------------------- the exchanges
// The xor butterfly over the G lanes of a group: log2(G) exchanges, after which every lane holds op over the group's G values,
// combined in an order that depends on G alone.
template <typename T, typename Op>
__device__ __forceinline__ T group_butterfly(T v, int G, Op op) {
  for (int o = G >> 1; o > 0; o >>= 1) v = op(v, __shfl_xor(v, o, ZS_WAVE));
  return v;
}
ZS_HD float group_fmax(float a, float b) { return fmaxf(a, b); }
ZS_HD double group_fmax(double a, double b) { return fmax(a, b); }
template <typename T>
__device__ __forceinline__ T group_sum(T v, int G) {
  return group_butterfly(v, G, [](T a, T b) { return a + b; });
}
template <typename T>
__device__ __forceinline__ T group_max(T v, int G) {
  return group_butterfly(v, G, [](T a, T b) { return group_fmax(a, b); });
}
// The same butterfly as one thread sees it (v[0 .. G) is overwritten; every entry ends as the group's value): what the kernels'
// shuffles compute, for the host programs.
template <typename T, typename Op>
inline void group_butterfly_host(T* v, int G, Op op) {
  T t[ZS_WAVE];
  for (int o = G >> 1; o > 0; o >>= 1) {
    for (int l = 0; l < G; ++l) t[l] = op(v[l], v[l ^ o]);
    for (int l = 0; l < G; ++l) v[l] = t[l];
  }
}

}  // namespace zs
