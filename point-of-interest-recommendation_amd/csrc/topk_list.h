// 64-entry top-K lists sorted by better() (poi_common.h: higher score, then lower id), held one entry per lane of a wave or in LDS:
// the pad entry, the two merges, and the emit of the kernels that cut a row into slices (near.hip, geoie_score.hip).
#pragma once
#include "poi_common.h"

namespace poi {

constexpr int PAD_ID = 0x7fffffff;      // an empty list entry: sorts behind every POI of the same score

// (cs, ci) sorted best-first over the lanes, (ns, ni) in any order -> the best 64 of the 128, sorted
__device__ __forceinline__ void top64_merge(float& cs, int& ci, float ns, int ni) {
  wave_sort_desc(ns, ni);
  const float rs = __shfl(ns, 63 - lane_id(), 64);
  const int ri = __shfl(ni, 63 - lane_id(), 64);
  if (better(rs, ri, cs, ci)) { cs = rs; ci = ri; }
  wave_sort_desc(cs, ci);
}

// merge a wave's 64 (unsorted) new candidates of one row into the row's LDS list (sorted, best first; entries 0 .. K-1 exact): the
// wave sorts only when one candidate beats the list's K-th entry, then the half-cleaner merge of two sorted lists
__device__ __forceinline__ void lds_list_merge(float* ls, int* li, float s, int i, int K) {
  const int lane = lane_id();
  const bool cand = better(s, i, ls[K - 1], li[K - 1]);
  if (!__ballot(cand)) return;
  if (!cand) { s = -INFINITY; i = PAD_ID; }
  wave_sort_desc(s, i);
  float rs = __shfl(s, 63 - lane, 64);
  int ri = __shfl(i, 63 - lane, 64);
  const float cs = ls[lane];
  const int ci = li[lane];
  if (better(cs, ci, rs, ri)) { rs = cs; ri = ci; }      // best 64 of the union: a bitonic sequence
#pragma unroll
  for (int j = 32; j > 0; j >>= 1) {
    const float ps = __shfl_xor(rs, j, 64);
    const int pi = __shfl_xor(ri, j, 64);
    const bool mine = better(rs, ri, ps, pi);
    if (((lane & j) == 0) != mine) { rs = ps; ri = pi; }
  }
  __builtin_amdgcn_wave_barrier();
  ls[lane] = rs; li[lane] = ri;
  __builtin_amdgcn_wave_barrier();
}

// wave 0 of a workgroup: lane l holds entry l of a sorted list.  `split`: the list of slice s goes to the row's partial lists (KMAX
// entries each, the caller's merge kernel combines them), otherwise it is the row's answer.
template <int KMAX, class Args>
__device__ __forceinline__ void list_emit(const Args& A, bool split, int r, int s, float sc, int id, int cnt) {
  const int lane = lane_id();
  if (split) {
    const size_t at = (size_t)r * A.n_split + s;
    if (lane < KMAX) { A.part_s[at * KMAX + lane] = sc; A.part_i[at * KMAX + lane] = id; }
    if (lane == 0) A.part_cnt[at] = cnt;
    return;
  }
  if (lane < A.k) {
    A.idx_out[(size_t)r * A.k + lane] = id == PAD_ID ? -1 : id;
    if (A.score_out) A.score_out[(size_t)r * A.k + lane] = id == PAD_ID ? neg_inf() : sc;
  }
  if (lane == 0 && A.count_out) A.count_out[r] = cnt;
}

}  // namespace poi
