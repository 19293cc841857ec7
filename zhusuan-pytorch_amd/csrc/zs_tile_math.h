// The matrix-core tile of the satellite kernels that multiply on v_mfma_{f32,f64}_16x16x4 (zs_topic.hip, zs_matvar.hip,
// zs_svgd.hip, zs_mix.hip): the place of a lane in the instruction, the row map of its accumulator, the staged panel of the
// topic and mix kernels, and the wrapper of the instruction itself.  The map is __host__ __device__, so that
// tests/host_math/zs_tile_host_math.hip walks it, and the bank figures quoted below, on the host under the sanitizers.
#pragma once
#include "zs_common.h"

namespace zs {

// ---------------------------------------------------------------- the map
// v_mfma_*_16x16x4: lane l = 16 q + m of a wave holds A[i = m][k = q], B[k = q][j = m] and four values D[acc_row(q, v)][j = m],
// v = 0..3.  The two element types differ ONLY in acc_row: the f32 instruction gives a lane four consecutive rows, the f64 one
// every fourth row.  So the output rows 2 t and 2 t + 1 are neighbours: in one lane (f32: registers v and v | 1) or in the
// lanes q and q ^ 1 (f64: the same register).
template <typename T> struct MfmaTile;
template <> struct MfmaTile<float> {
  static ZS_HD int acc_row(int q, int v) { return 4 * q + v; }
};
template <> struct MfmaTile<double> {
  static ZS_HD int acc_row(int q, int v) { return 4 * v + q; }
};

// the place of thread `thread` of a workgroup: lane 16 q + m of wave `wave`
ZS_HD int mfma_m(int thread) { return thread & 15; }
ZS_HD int mfma_q(int thread) { return (thread & 63) >> 4; }
ZS_HD int mfma_wave(int thread) { return thread >> 6; }

// 16-wide blocks (tiles, rows of tiles) that cover d
template <typename I>
ZS_HD I blocks16(I d) { return (d + 15) / 16; }

// ---------------------------------------------------------------- the staged panel
// The topic and mix kernels stage one operand in LDS a panel of PANEL columns at a time, k-major: as many columns as keep the
// panel within 32 - 50 KB at 128 k-rows.  A row of the panel is padded by 17 elements, so that the four k-rows
// (4 s + q) LD + m, q = 0..3, which the 64 lanes of one matrix step read, START in four different 4-byte banks of the 64: 17
// banks apart for float, where the step's 64 words fall into 61 banks (the last row wraps onto the first three banks of the
// first: three banks serve two lanes); at word 0, 34, 4, 38 (mod 64, plus the step's common offset) for double, where the
// step's 128 words reach all 64 banks, none more than three times (two is the least possible).
template <typename T>
struct MfmaPanel {
  static constexpr int PANEL = sizeof(T) == 4 ? 64 : 32, LD = PANEL + 17;
};
ZS_HD int panel_cols(int elem_bytes) { return elem_bytes == 4 ? MfmaPanel<float>::PANEL : (elem_bytes == 8 ? MfmaPanel<double>::PANEL : 0); }
// panels that cover n columns; 0 for an unknown element size or n < 1
ZS_HD int64_t panels(int elem_bytes, int64_t n) {
  const int p = panel_cols(elem_bytes);
  return (p == 0 || n < 1) ? 0 : (n + p - 1) / p;
}

// ---------------------------------------------------------------- the instruction
typedef float mfma_f4 __attribute__((ext_vector_type(4)));
typedef double mfma_d4 __attribute__((ext_vector_type(4)));

// acc + A B for the lane's share of a 16 x 4 by 4 x 16 product (the host pass only parses it)
template <typename T> struct Mfma;
template <> struct Mfma<float> {
  typedef mfma_f4 Acc;
  static __device__ __forceinline__ Acc run(float a, float b, Acc acc) {
#if ZS_ON_DEVICE
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc, 0, 0, 0);
#else
    return acc;
#endif
  }
};
template <> struct Mfma<double> {
  typedef mfma_d4 Acc;
  static __device__ __forceinline__ Acc run(double a, double b, Acc acc) {
#if ZS_ON_DEVICE
    return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
#else
    return acc;
#endif
  }
};

template <typename T>
__device__ __forceinline__ T neg_inf() { return -(T)INFINITY; }

// the dynamic LDS of a launch, as elements of T
template <typename T>
__device__ __forceinline__ T* tile_lds() {
  extern __shared__ __align__(16) unsigned char tile_lds_bytes[];
  return reinterpret_cast<T*>(tile_lds_bytes);
}

// One 16 x 16 tile of (rows) @ (panel) over the 16 columns at Bc = (the staged panel) + (first column of the tile); a[s] is the
// lane's element [row m][4 s + q] of the row operand.  The same two values serve the tile and its transpose, by the order of
// the instruction's operands: ROWS_FIRST leaves acc[v] = out[row acc_row(q, v)][column m], else out[column acc_row(q, v)][row m].
template <typename T, bool ROWS_FIRST, int MAX_STEPS>
__device__ __forceinline__ typename Mfma<T>::Acc panel_tile(const T (&a)[MAX_STEPS], const T* Bc, int q, int m, int steps) {
  constexpr int LD = MfmaPanel<T>::LD;
  typename Mfma<T>::Acc acc = {0, 0, 0, 0};
#pragma unroll
  for (int s = 0; s < MAX_STEPS; ++s) {
    if (s < steps) {          // (uniform; a break would keep the loop, and a[], from unrolling into registers)
      const T b = Bc[(4 * s + q) * LD + m];
      acc = ROWS_FIRST ? Mfma<T>::run(a[s], b, acc) : Mfma<T>::run(b, a[s], acc);
    }
  }
  return acc;
}

}  // namespace zs
