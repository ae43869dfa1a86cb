// 64-entry top-K lists sorted by better() (poi_common.h: higher score, then lower id), held one entry per lane of a wave or in LDS:
// the pad entry, the bit rank of the queue compactions, the merges and the insertion, the fold of a workgroup's four lists, and the emit and the fold of the kernels that cut
// a row into slices (near.hip, geoie_score.hip, group.hip, diverse.hip, route.hip, filter.hip; the merge kernel itself is topk_merge.hip).
#pragma once
#include "poi_common.h"

namespace poi {

constexpr int PAD_ID = 0x7fffffff;      // an empty list entry: sorts behind every POI of the same score

// position of the t-th (0-based) set bit of m; m has more than t bits set
__device__ __forceinline__ int nth_bit(unsigned long long m, int t) {
  int pos = 0;
#pragma unroll
  for (int w = 32; w > 0; w >>= 1) {
    const int c = __popcll((m >> pos) & ((1ull << w) - 1ull));
    if (t >= c) { t -= c; pos += w; }
  }
  return pos;
}

// (cs, ci) sorted best-first over the lanes, (ns, ni) in any order -> the best 64 of the 128, sorted
__device__ __forceinline__ void top64_merge(float& cs, int& ci, float ns, int ni) {
  wave_sort_desc(ns, ni);
  const float rs = __shfl(ns, 63 - lane_id(), 64);
  const int ri = __shfl(ni, 63 - lane_id(), 64);
  if (better(rs, ri, cs, ci)) { cs = rs; ci = ri; }
  wave_sort_desc(cs, ci);
}

// merge a wave's 64 (unsorted) new candidates of one row into the row's LDS list (sorted, best first; entries 0 .. K-1 exact): the
// wave sorts only when one candidate beats the list's K-th entry, then the half-cleaner merge of two sorted lists.  LEN: the entries the
// LDS list holds (64, or 32: audience.hip keeps 32 lists per wave) - the lanes behind it hold pads and write nothing back
template <int LEN = 64>
__device__ __forceinline__ void lds_list_merge(float* ls, int* li, float s, int i, int K) {
  const int lane = lane_id();
  const bool cand = better(s, i, ls[K - 1], li[K - 1]);
  if (!__ballot(cand)) return;
  if (!cand) { s = -INFINITY; i = PAD_ID; }
  wave_sort_desc(s, i);
  float rs = __shfl(s, 63 - lane, 64);
  int ri = __shfl(i, 63 - lane, 64);
  const float cs = (LEN == 64 || lane < LEN) ? ls[lane] : neg_inf();
  const int ci = (LEN == 64 || lane < LEN) ? li[lane] : PAD_ID;
  if (better(cs, ci, rs, ri)) { rs = cs; ri = ci; }      // best 64 of the union: a bitonic sequence
#pragma unroll
  for (int j = 32; j > 0; j >>= 1) {
    const float ps = __shfl_xor(rs, j, 64);
    const int pi = __shfl_xor(ri, j, 64);
    const bool mine = better(rs, ri, ps, pi);
    if (((lane & j) == 0) != mine) { rs = ps; ri = pi; }
  }
  __builtin_amdgcn_wave_barrier();
  if (LEN == 64 || lane < LEN) { ls[lane] = rs; li[lane] = ri; }
  __builtin_amdgcn_wave_barrier();
}

// the lanes of `bal` hold candidates (v, j) for the sorted 64-entry list (ls, lx), entry l on lane l.  A few (the common tile, once the
// list has warmed up): one at a time - the entries in front of the newcomer are a prefix of the sorted list, the others move down one
// lane.  Many (the first tiles): lds_list_merge's sort.  The list is the best 64 of everything offered either way: the same bits.
template <int LEN = 64>
__device__ __forceinline__ void list_take(float* ls, int* lx, unsigned long long bal, bool cand, float v, int j, int K) {
  if (__popcll(bal) > 8) { lds_list_merge<LEN>(ls, lx, cand ? v : neg_inf(), cand ? j : PAD_ID, K); return; }
  const int lane = lane_id();
  __builtin_amdgcn_wave_barrier();
  float cs = (LEN == 64 || lane < LEN) ? ls[lane] : neg_inf();
  int ci = (LEN == 64 || lane < LEN) ? lx[lane] : PAD_ID;
  while (bal) {
    const int src = __ffsll((long long)bal) - 1;
    bal &= bal - 1;
    const float nv = readlane_f(v, src);
    const int nj = __builtin_amdgcn_readlane(j, src);
    const int pos = __popcll(__ballot(better(cs, ci, nv, nj)));
    const float us = __shfl_up(cs, 1, 64);
    const int ui = __shfl_up(ci, 1, 64);
    if (lane == pos) { cs = nv; ci = nj; }
    else if (lane > pos) { cs = us; ci = ui; }
  }
  __builtin_amdgcn_wave_barrier();
  if (LEN == 64 || lane < LEN) { ls[lane] = cs; lx[lane] = ci; }
  __builtin_amdgcn_wave_barrier();                  // (a wave's LDS accesses complete in order: the next read needs no wait, only this place in the code)
}

// one wave, after a barrier: the four waves' KMAX-entry lists in LDS (wave w's at m_s / m_i + w * stride) -> their best 64, sorted over the lanes
template <int KMAX>
__device__ __forceinline__ void block_lists_fold(const float* m_s, const int* m_i, int stride, float& as, int& ai) {
  static_assert(KMAX == 32 && POI_NWAVE == 4, "lane half h folds the lists of waves h and 2 + h");
  const int at = (lane_id() >> 5) * stride + (lane_id() & (KMAX - 1));
  float s = m_s[at], bs = m_s[at + 2 * stride];
  int i = m_i[at], bi = m_i[at + 2 * stride];
  wave_sort_desc(s, i);
  top64_merge(s, i, bs, bi);
  as = s; ai = i;
}

// one wave: the best 64 of n_lists partial lists of KMAX sorted entries each (list l at (base + l) * KMAX), 64 / KMAX lists per merge,
// in list order.  The order better() is total, so the result does not depend on how the lists were cut.
template <int KMAX>
__device__ __forceinline__ void fold_slice_lists(const float* part_s, const int* part_i, size_t base, int n_lists, float& cs, int& ci) {
  const int lane = lane_id();
  float s = neg_inf();                              // (locals, not the references: through them the compiler turns the sorts' selects into branches)
  int i = PAD_ID;
  for (int l0 = 0; l0 < n_lists; l0 += 64 / KMAX) {
    const int l = l0 + lane / KMAX;
    const size_t at = (base + l) * KMAX + (lane & (KMAX - 1));
    const float ns = l < n_lists ? part_s[at] : neg_inf();
    const int ni = l < n_lists ? part_i[at] : PAD_ID;
    top64_merge(s, i, ns, ni);
  }
  cs = s; ci = i;
}

// wave 0 of a workgroup: lane l holds entry l of a sorted list.  `split`: the list of slice s goes to the row's partial lists (KMAX
// entries each, topk_slices_merge_kernel combines them), otherwise it is the row's answer.
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
