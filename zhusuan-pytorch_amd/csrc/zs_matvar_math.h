// The arithmetic of MatrixVariateNormalCholesky (include/zs_matvar.h) that is not scheduling: the padding of an event's tile,
// the LDS budget and the caps that follow from it, the split of the particles into shares, the layout of the
// partials workspace, and the per-element expressions.  __host__ __device__ like the other *_math.h headers; zs_matvar.hip only
// stages, multiplies, substitutes and reduces.
#pragma once
#include "zs_common.h"
#include "zs_flat_math.h"
#include "zs_group_math.h"
#include "zs_tile_math.h"

#define ZS_MATVAR_THREADS 256          // four waves
#define ZS_MATVAR_WAVES 4
#define ZS_MATVAR_MAX_DIM_F32 128
#define ZS_MATVAR_MAX_DIM_F64 64
#define ZS_MATVAR_PAD 12               // LD = p16 + 12, see below
#define ZS_MATVAR_GRID_TARGET 256      // backward: workgroups wanted when the rows alone are fewer (one per CU)
#define ZS_MATVAR_MAX_SHARES 16        // backward: at most this many partials per row, whatever K is
#define ZS_MATVAR_LDS_BYTES (160 * 1024)

namespace zs {

// An event is held in LDS as a tile of n16 x LD elements (the lanes' places in it: zs_tile_math.h), n16 / p16 = n / p rounded up
// to 16, LD = p16 + 12.  LD = 4 (4 j + 3) is four times an odd number: the 64 addresses m LD + 4 s + q of an operand read along a
// row (m = 0..15, q = 0..3) fall into 64 different float32 banks (float64: every bank twice, the least possible), and the four
// k-rows (4 s + q) LD + m of an operand read down a column start in four different banks, LD mod 64 = 12, 28, 44 or 60 apart.
//
// LDS budget (bytes; two tiles, the staged inverses of the 16 x 16 diagonal blocks of both factors, four reduction slots):
//   float32, n = p = 128:  2 * 128 * 140 * 4 = 143 360;  inverses (8 + 8) * 256 * 4 = 16 384;  slots 16;  total 159 760 <= 163 840
//   float64, n = p =  64:  2 *  64 *  76 * 8 =  77 824;  inverses (4 + 4) * 256 * 8 = 16 384;  slots 32;  total  94 240
//   float64, n = p = 128:  2 * 128 * 140 * 8 = 286 720: does not fit (nor does 96: 190 464); the float64 cap is half the float32
//   one, 64, the element sizes' ratio.
template <typename T>
struct MatvarCap {
  static constexpr int MAX_DIM = sizeof(T) == 4 ? ZS_MATVAR_MAX_DIM_F32 : ZS_MATVAR_MAX_DIM_F64;
};

ZS_HD int matvar_max_dim(int elem_bytes) { return elem_bytes == 4 ? ZS_MATVAR_MAX_DIM_F32 : (elem_bytes == 8 ? ZS_MATVAR_MAX_DIM_F64 : 0); }
ZS_HD int matvar_ld(int p) { return 16 * blocks16(p) + ZS_MATVAR_PAD; }
// elements of LDS: two tiles, the inverses of the diagonal blocks of U and of V, four reduction slots
ZS_HD int64_t matvar_lds_elems(int n, int p) {
  return 2 * (int64_t)(16 * blocks16(n)) * matvar_ld(p) + 256 * (int64_t)(blocks16(n) + blocks16(p)) + 4;
}

// The backwards cut a row's K particles into `shares` contiguous runs of `per` particles; a workgroup walks one run in ascending
// k.  Enough shares for ZS_MATVAR_GRID_TARGET workgroups when the rows are few, never more than ZS_MATVAR_MAX_SHARES: one row
// with five particles (a BNN layer) runs on five workgroups.
ZS_HD int64_t matvar_shares(int64_t K, int64_t R) {
  if (K < 1 || R < 1) return 0;
  int64_t s = (ZS_MATVAR_GRID_TARGET + R - 1) / R;
  if (s > ZS_MATVAR_MAX_SHARES) s = ZS_MATVAR_MAX_SHARES;
  if (s > K) s = K;
  const int64_t per = (K + s - 1) / s;
  return (K + per - 1) / per;          // no empty share
}
ZS_HD int64_t matvar_share_len(int64_t K, int64_t shares) { return (K + shares - 1) / shares; }

// the partials of one (share, row): gmean [n, p], gU [n, n], gV [p, p] (the blocks above the diagonal are never touched)
ZS_HD int64_t matvar_part_stride(int64_t n, int64_t p) { return n * p + n * n + p * p; }
ZS_HD int64_t matvar_part_elems(int64_t K, int64_t R, int64_t n, int64_t p) { return matvar_shares(K, R) * R * matvar_part_stride(n, p); }

ZS_HD float matvar_log(float x) { return logf(x); }
ZS_HD double matvar_log(double x) { return log(x); }

// c(U, V) - 1/2 ss, c = -(n p / 2) log 2 pi - p slog_u - n slog_v
template <typename T>
ZS_HD T matvar_lp(int n, int p, T slog_u, T slog_v, T ss) {
  const T c0 = (T)(-0.5 * 1.8378770664093454835606594728112 * (double)n * (double)p);
  return ((c0 - (T)p * slog_u) - (T)n * slog_v) - (T)0.5 * ss;
}

}  // namespace zs
