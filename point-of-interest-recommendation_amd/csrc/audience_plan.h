// The launch decision of the audience walk (audience.hip: poi_score_audience, poi_audience_rows).  Plain host arithmetic, no HIP: a test
// compiles it on its own.
#pragma once
#include "split_plan.h"

#define AUDIENCE_SPLIT_LIMIT 64             // slices the user range may be cut into (what one merge wave folds in a few rounds)
#define AUDIENCE_TILES_PER_SLICE 16         // 32-row user tiles a slice keeps when the CUs set the slice count: four per wave

// A call of n_q query POIs against n candidate rows.  At most split_max queries (live traffic: few POIs, the whole user table): the user
// range is cut into slices, one workgroup per (32-query block, slice) - grid_opt slices when set, otherwise two workgroups per CU over
// the call's query blocks while a slice keeps AUDIENCE_TILES_PER_SLICE tiles.  Larger calls: one workgroup per query block.
inline SplitPlan audience_plan(int n_q, int n, int split_max, int grid_opt, int num_cu) {
  const int n_qblock = (n_q + 31) / 32, ntile = (n + 31) / 32;
  return plan_split(n_q, n_qblock > 0 ? n_qblock : 1, split_max, grid_opt, 2, num_cu, ntile / AUDIENCE_TILES_PER_SLICE, 1, AUDIENCE_SPLIT_LIMIT);
}
