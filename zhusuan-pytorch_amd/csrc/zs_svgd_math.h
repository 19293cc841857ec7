// The arithmetic of Stein variational gradient descent (include/zs_svgd.h) that is not scheduling: the leading dimensions of the
// LDS tiles (the lanes' places in them: zs_tile_math.h), the deal of the Gram matrix's tile pairs over the waves, the padded-row mask, the bit-pattern selection of the
// median, the bandwidth and the per-element step.  __host__ __device__ like the other *_math.h headers
// (tests/host_math/zs_svgd_host_math.hip runs it on the host); zs_svgd.hip only stages, multiplies and reduces.
#pragma once
#include "zs_common.h"
#include "zs_flat_math.h"
#include "zs_tile_math.h"
#include "../../include/zs_svgd.h"

#define ZS_SVGD_GRAM_WAVES 8
#define ZS_SVGD_GRAM_THREADS (64 * ZS_SVGD_GRAM_WAVES)
#define ZS_SVGD_FINISH_THREADS 1024
// Leading dimensions of the LDS tiles.  Gram: both operands are read along a row, lane 16 q + m at m LD + 4 s + q; LD = 36 is four
// times an odd number, so the 64 lanes fall into 64 different 4-byte banks.  Update: the B operand is read down a column, lane
// 16 q + m at (4 s + q) LD + 16 cb + m; with LD = 48 the four k-rows start 48 banks apart: 0, 48, 32, 16.  (float32; the words
// of a float64 step fall into every bank twice, the least possible, with either.)
#define ZS_SVGD_LD_GRAM (ZS_SVGD_SLAB + 4)
#define ZS_SVGD_LD_UPDATE (ZS_SVGD_SLAB + 16)
// LDS (bytes; the tile, THREADS / 32 x 32 column-sum partials, 32 means, update: the row sums):
//   gram   f32 K = 256: 256 * 36 * 4 = 36 864 + 2 048 + 128;        f64 K = 128: 128 * 36 * 8 = 36 864 + 4 096 + 256
//   update f32 K = 256: 256 * 48 * 4 = 49 152 + 4 096 + 128 + 1 024; f64 K = 128: 128 * 48 * 8 = 49 152 + 4 096 + 256 + 1 024

namespace zs {

template <typename T>
struct SvgdCap {
  static constexpr int MAX_K = sizeof(T) == 4 ? ZS_SVGD_MAX_PARTICLES : ZS_SVGD_MAX_PARTICLES_F64;
};

ZS_HD int svgd_max_particles_of(int elem_bytes) {
  return elem_bytes == 4 ? ZS_SVGD_MAX_PARTICLES : (elem_bytes == 8 ? ZS_SVGD_MAX_PARTICLES_F64 : 0);
}
ZS_HD int svgd_blocks(int K) { return blocks16(K); }          // blocks of 16 particles
ZS_HD bool svgd_row_live(int row, int K) { return row < K; }          // rows K .. 16 blocks(K) of a tile are zero
ZS_HD int64_t svgd_slabs(int64_t D) { return (D + ZS_SVGD_SLAB - 1) / ZS_SVGD_SLAB; }
ZS_HD int64_t svgd_gram_slots(int64_t D) {
  const int64_t s = svgd_slabs(D);
  return s < ZS_SVGD_GRID_CAP ? s : ZS_SVGD_GRID_CAP;
}

// The tile pairs (bi >= bj) of the lower triangle of nb x nb blocks, numbered row by row: pair p = bi (bi + 1) / 2 + bj.  Pair p
// is accumulator p / WAVES of wave p % WAVES; a wave of a launch compiled for PPW accumulators covers nb up to svgd_max_blocks(PPW).
ZS_HD int svgd_pairs(int nb) { return nb * (nb + 1) / 2; }
ZS_HD void svgd_pair_of(int p, int& bi, int& bj) {
  bi = 0;
  while ((bi + 1) * (bi + 2) / 2 <= p) ++bi;
  bj = p - bi * (bi + 1) / 2;
}
ZS_HD int svgd_pair_index(int wave, int slot) { return slot * ZS_SVGD_GRAM_WAVES + wave; }
ZS_HD int svgd_pairs_per_wave(int nb) { return (svgd_pairs(nb) + ZS_SVGD_GRAM_WAVES - 1) / ZS_SVGD_GRAM_WAVES; }

// d_ij from the centred Gram matrix: clamped at 0, the diagonal exactly 0
ZS_HD double svgd_dist(double gii, double gjj, double gij, bool diagonal) {
  const double d = (gii + gjj) - 2.0 * gij;
  return (diagonal || !(d > 0.0)) ? 0.0 : d;
}

// Exact selection.  Non-negative doubles order as their bit patterns.  The value of rank r (0-based, ascending) of a set is the
// LARGEST pattern a with #{x < a} <= r; it is built from bit 62 down: a candidate a | bit is kept when at most r values lie below
// it.  One count over the set per bit; svgd_select_step is the decision, the count is the caller's.
ZS_HD uint64_t svgd_bits(double x) {
  uint64_t b;
  memcpy(&b, &x, 8);
  return b;
}
ZS_HD double svgd_from_bits(uint64_t b) {
  double x;
  memcpy(&x, &b, 8);
  return x;
}
ZS_HD uint64_t svgd_candidate(uint64_t a, int bit) { return a | ((uint64_t)1 << bit); }
ZS_HD uint64_t svgd_select_step(uint64_t a, int bit, int64_t below, int64_t rank) { return below <= rank ? svgd_candidate(a, bit) : a; }
// the two ranks whose mean is the median of `count` values (equal for an odd count), as numpy.median takes them
ZS_HD int64_t svgd_rank_lo(int64_t count) { return (count - 1) / 2; }
ZS_HD int64_t svgd_rank_hi(int64_t count) { return count / 2; }
ZS_HD double svgd_median_of(double lo, double hi) { return 0.5 * (lo + hi); }
ZS_HD double svgd_bandwidth(double med, int K) { return med > 0.0 ? med / log((double)K + 1.0) : 1.0; }

ZS_HD float svgd_sqrt(float x) { return sqrtf(x); }
ZS_HD double svgd_sqrt(double x) { return sqrt(x); }

// what a launch knows about the step
template <typename T>
struct SvgdStep {
  T step, alpha, one_minus_alpha, fudge, two_over_h, inv_k;
  int adagrad, first;
};
// phi of one element from (k U)[i][c], s_i and the centred theta_i[c]
template <typename T>
ZS_HD T svgd_phi(T ku, T s, T centred, const SvgdStep<T>& st) {
  return (ku + st.two_over_h * s * centred) * st.inv_k;
}
// the step of one element; `h` is the element of the second-moment state (adagrad only: read unless first, written)
template <typename T>
ZS_HD T svgd_move(T theta, T phi, T* h, const SvgdStep<T>& st) {
  if (!st.adagrad) return theta + st.step * phi;
  const T sq = phi * phi;
  const T H = st.first ? sq : st.alpha * *h + st.one_minus_alpha * sq;
  *h = H;
  return theta + st.step * (phi / (st.fudge + svgd_sqrt(H)));
}

}  // namespace zs
