// The arithmetic of the admixture likelihood (include/zs_topic.h) that is not scheduling: the sizes and the layout of the
// workspaces, the split of the grad_doc grid, and the per-element expressions of the epilogues; the tile of the two matrix
// instructions, its row map and the staged panel of B are zs_tile_math.h's (MfmaTile, MfmaPanel, panel_tile).  __host__
// __device__ like the other *_math.h headers; zs_topic.hip only stages, multiplies and reduces.
#pragma once
#include "zs_common.h"
#include "zs_flat_math.h"
#include "zs_group_math.h"
#include "zs_tile_math.h"

#define ZS_TOPIC_MAX_TOPICS 128
#define ZS_TOPIC_MAX_STEPS (ZS_TOPIC_MAX_TOPICS / 4)          // matrix instructions per 16 x 16 tile: the k axis in fours
#define ZS_TOPIC_MAX_KTILES (ZS_TOPIC_MAX_TOPICS / 16)
#define ZS_TOPIC_ROWS_PER_BLOCK 64                            // grad_doc: four waves of 16 rows
#define ZS_TOPIC_GRID_TARGET 512                              // grad_doc: workgroups wanted at small R (two per CU)

namespace zs {

ZS_HD int64_t topic_k16(int64_t K) { return blocks16(K) * 16; }          // rows of the staged panel, row stride of E
ZS_HD int topic_steps(int64_t K) { return (int)((K + 3) / 4); }
ZS_HD int64_t topic_doc_splits(int elem_bytes, int64_t R, int64_t V) {
  const int64_t panels = zs::panels(elem_bytes, V);
  if (panels == 0 || R < 1) return 0;
  const int64_t blocks = (R + ZS_TOPIC_ROWS_PER_BLOCK - 1) / ZS_TOPIC_ROWS_PER_BLOCK;
  const int64_t s = (ZS_TOPIC_GRID_TARGET + blocks - 1) / blocks;
  return s > panels ? panels : s;
}

// the prep workspace: lse[K], N[Dx], Z[R], logZ[R], E[R, K16]
template <typename T>
struct TopicPrep {
  T *lse, *n, *z, *logz, *e;
};
template <typename T>
ZS_HD TopicPrep<T> topic_prep(T* p, int64_t R, int64_t K, int64_t Dx) {
  TopicPrep<T> w;
  w.lse = p;
  w.n = w.lse + K;
  w.z = w.n + Dx;
  w.logz = w.z + R;
  w.e = w.logz + R;
  return w;
}
ZS_HD int64_t topic_prep_elems(int64_t R, int64_t K, int64_t Dx) { return K + Dx + 2 * R + R * topic_k16(K); }

// float: the 1-ulp instructions where an expression runs per element of the [R, V] product (the logarithm of the epilogue),
// libm-grade everywhere else (the prologue and the staging run once per element of H and B)
ZS_HD float topic_exp(float x) { return expf(x); }
ZS_HD double topic_exp(double x) { return exp(x); }
ZS_HD float topic_log(float x) { return logf(x); }
ZS_HD double topic_log(double x) { return log(x); }
ZS_HD float topic_log_acc(float x) { return ln_fast(x); }
ZS_HD double topic_log_acc(double x) { return log(x); }

// x (c_v + log acc): one term of lp before - N_r log Z_r; a zero count contributes exactly 0 whatever acc is
template <typename T>
ZS_HD T topic_term(T x, T c, T acc) { return x > (T)0 ? x * (c + topic_log_acc(acc)) : (T)0; }
// g x / acc: W without its column scale exp(-c_v) and row scale Z_r, which cancel against those of the second operand
template <typename T>
ZS_HD T topic_weight(T g, T x, T acc) { return x > (T)0 ? g * x / acc : (T)0; }

}  // namespace zs
