// The path decision of the filtered top-K (poi_score_topk_filtered, filter.hip).  Plain host arithmetic, no HIP: a test compiles it on
// its own.  Both paths give the same bits, so the rule is free to decide by cost alone.
#pragma once

enum { FILTER_PATH_AUTO = 0, FILTER_PATH_WALK = 1, FILTER_PATH_GATHER = 2 };      // = POI_FILTER_* (include/poi_hip.h)

// "filter_gather_cost": what one gathered candidate costs in units of one (row tile, POI) cell of the walk.  MEASURED
// (tools/bench_filtered.py on an MI355X, 100 k POIs, dim 128; the table is in DESIGN.md section 27): where the two paths cross, the
// cost is 0.19 - 0.22 at 4096 rows, below 0.1 at 64 rows (the gather wins at every pass fraction measured) and 2.2 at one row - it
// rounds to 0 or 2; 1 is the smallest value the rule admits (0 would send every hinted call to the gather, which loses 3 x at 4096
// rows and a 50 % predicate).  With 1 the rule never gathers where the walk is faster by more than 1.1 x; at 64+ rows it still walks
// above a pass fraction of 3 %, where the gather is up to 2.9 x faster (64 rows, 10 %) until the walk takes over (4096 rows, 15 %).
#define FILTER_GATHER_COST_DEFAULT 1

// The walk costs a 32-row tile one pass over the item table whatever the predicate (ceil(n / 32) * n_item cells; fewer only where whole
// tiles pass nothing), the gather one item row per (row, passing POI): n * cand_hint candidates, `gather_cost` cells each.  cand_hint:
// the caller's upper bound of the pass count of the predicates in use, 0 = unknown.  A finite radius is the gather path's alone.
inline int plan_filter_path(int requested, bool radius, long long n, long long n_item, long long cand_hint, long long gather_cost) {
  if (requested == FILTER_PATH_WALK || requested == FILTER_PATH_GATHER) return requested;
  if (radius) return FILTER_PATH_GATHER;
  if (cand_hint > 0 && n * cand_hint * gather_cost < ((n + 31) / 32) * n_item) return FILTER_PATH_GATHER;
  return FILTER_PATH_WALK;
}
