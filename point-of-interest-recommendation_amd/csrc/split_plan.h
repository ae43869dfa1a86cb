// The split decision of the serving paths that cut a row's (tile's, group's) item range over several workgroups (near.hip, group.hip,
// route.hip, diverse.hip).  Plain host arithmetic, no HIP: a test compiles it on its own.
#pragma once

struct SplitPlan { int split, n_split; };   // split: the call takes the split path; n_split: workgroups per unit (1 on the other path)

// `rows` <= split_max takes the split path.  Its workgroups per unit: the grid option when set, as given; otherwise per_cu * num_cu over
// the `units` the call has (rows, 32-row tiles, group tiles), at most `cap` (what the item range can feed), at least `floor`.  Either
// way at most `limit`, the lists the merge folds.
inline SplitPlan plan_split(int rows, int units, int split_max, int grid_opt, int per_cu, int num_cu, int cap, int floor, int limit) {
  if (rows > split_max) return SplitPlan{0, 1};
  int s = grid_opt;
  if (grid_opt <= 0) {
    s = per_cu * num_cu / units;
    if (s > cap) s = cap;
    if (s < floor) s = floor;
  }
  return SplitPlan{1, s > limit ? limit : s};
}

// The item ranges of the walks that give every WAVE a range of its own (rank.hip, select.hip's score_rows): 8 waves per CU over the call's
// `n_utile` 32-row tiles, at least 8 of the `ntile` item tiles per range, at least one range.  `cap` > 0 (poi_score_rank's "rank_grid")
// caps the count; `tiles_max` > 0 (rank.hip's 16-bit per-lane counters) is the most tiles a range may hold, and wins over the cap.
inline int plan_wave_ranges(int n_utile, int ntile, int num_cu, int cap, int tiles_max) {
  int want = (num_cu * 8 + n_utile - 1) / n_utile;
  if (want > ntile / 8) want = ntile / 8;
  if (cap > 0 && want > cap) want = cap;
  if (want < 1) want = 1;
  if (tiles_max > 0 && want < (ntile + tiles_max - 1) / tiles_max) want = (ntile + tiles_max - 1) / tiles_max;
  return want;
}
