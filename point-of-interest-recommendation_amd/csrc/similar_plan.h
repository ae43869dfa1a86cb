// The launch decisions of the similar-rows walk (similar.hip: poi_similar_topk, poi_similar_rows).  Plain host arithmetic, no HIP: a
// test compiles it on its own.
#pragma once
#include "split_plan.h"

#define SIMILAR_SPLIT_LIMIT 64              // slices the row range may be cut into (what one merge wave folds in a few rounds)
#define SIMILAR_SPLIT_MAX_DEFAULT 16384     // option "similar_split_max": 512 query blocks - beyond them two workgroups per CU leave one slice anyway
#define SIMILAR_TILES_PER_SLICE 16          // 32-row tiles a slice keeps when the CUs set the slice count: four per wave
#define SIMILAR_ROWS_MAX_DEFAULT 1024       // option "similar_rows_max" (DESIGN.md section 29 has the table it is read from)
#define SIMILAR_ROWS_MAX_LIMIT 4096         // ... and its upper end: the rows one selection sequence takes

// path: 0 one workgroup per 32-query block, 1 slices (+ merge), 2 score rows + selection
struct SimilarPlan { int path, n_split; };

// The slices of a call of n_q queries against n rows - the walk of either route.  At most split_max queries: the row range is cut into
// slices, one workgroup per (32-query block, slice) - grid_opt slices when set, otherwise two workgroups per CU over the call's query
// blocks while a slice keeps SIMILAR_TILES_PER_SLICE tiles.  Larger calls: one workgroup per query block.
inline SplitPlan similar_split(int n_q, int n, int split_max, int grid_opt, int num_cu) {
  const int n_qblock = (n_q + 31) / 32, ntile = (n + 31) / 32;
  return plan_split(n_q, n_qblock > 0 ? n_qblock : 1, split_max, grid_opt, 2, num_cu, ntile / SIMILAR_TILES_PER_SLICE, 1, SIMILAR_SPLIT_LIMIT);
}

// poi_similar_topk.  Calls of at most rows_max queries write their score rows and select from them (for few queries that route is the
// faster one) - while the selection can take the call at all: k <= n (it lists no more than it has columns) and the score rows fit
// rows_fit queries of workspace.  Both routes give the same bits.
inline SimilarPlan similar_plan(int n_q, int n, int k, int rows_max, long long rows_fit, int split_max, int grid_opt, int num_cu) {
  const SplitPlan sp = similar_split(n_q, n, split_max, grid_opt, num_cu);
  if (n_q <= rows_max && n_q <= rows_fit && k <= n) return SimilarPlan{2, sp.n_split};
  return SimilarPlan{sp.split, sp.n_split};
}
