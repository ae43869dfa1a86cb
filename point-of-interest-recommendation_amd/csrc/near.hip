// Restricted recommendation (poi_score_topk_near): top-K over the POIs within a radius of an anchor POI, minus a per-row exclusion list -
// the ranking of public/Valuate.py:132-146 over the candidate sets of public/Load_Data_fpmc_lr.py:114-143 instead of over every POI.
//
// Candidates of row r:  C(r) = { j : (anchor[r] < 0 or c(anchor[r], j) < c_r or j == anchor[r]) and j not in ex[ex_off[r] .. ex_off[r + 1]) }.
// `c` is haversine_c (poi_common.h: float64, cal_dis's operation order - the term poi_fpmc_neighbor_* and poi_dist_prob evaluate) and c_r
// the exact host threshold data.ud_threshold(r km), so c < c_r <=> dist <= r km.  A row with a radius walks only the latitude band
// |lat_j - lat_anchor| <= band_deg of the stable latitude order (lat_bound, as the FPMC-LR neighbour passes): a conservative superset,
// the exact test alone decides.  A row without one walks the ids 0 .. n_item - 1.
//
// One workgroup = one row and one contiguous slice of its band; a wave takes 64 positions per round, one per lane: the exact test, the
// distance bin (bin_of_c, same c) and a binary search of the exclusion list.  The survivors are compacted (ballot + rank) into a 64-entry
// queue held one entry per lane; a full queue is scored: 16 lanes per candidate (a float4 of the item row per lane and 64 columns), two
// candidates per lane group in flight, the user row in registers.
//   score = users[r] . items[j]: per lane an fma chain over its columns in ascending order, then a 16-lane butterfly - one fixed order per
//   pair, whatever the slice, the wave or the grid - plus wd * sts[r][bin] for bin < n_dist when the row has an anchor.
// Each wave keeps its best 64 sorted over its lanes (top64_merge, topk_list.h: sort the batch, keep the better of cur[l] / new[63 - l], sort); a batch
// without an entry above the K-th best so far is dropped after one ballot.  The four waves' lists meet in LDS.  Row path: that list is
// the answer.  Split path: it goes to a (row, slice) partial list and a one-wave merge kernel per row (topk_merge.hip) combines the slices.  The order
// (descending score, ascending id) is total over distinct ids, so the result does not depend on how a band was cut: every grid gives the
// same bits.  No atomics touch a result; a rejected row is counted with one integer atomic.
//
// Bytes per candidate: the item row (4 dim, or 2 dim from a half table); per band position 4 (order) + 24 (lat, lon, cos lat) when the
// row has an anchor, plus ~log2(list) exclusion ids for the positions inside the radius.
#include "poi_common.h"
#include "poi_kernels.h"
#include "topk_list.h"

namespace poi {

namespace {

// scores the queue (lane l: candidate q_id, PAD_ID = none; m = entries in use) and folds it into the wave's list
template <int NJ>
__device__ __forceinline__ void near_score(const NearArgs& A, int r, const float4 (&u)[NJ], float wd, int q_id, int q_bin, int m, float& cs, int& ci) {
  const int lane = lane_id(), grp = lane >> 4, gl = lane & 15, D = A.dim;
  float mine = neg_inf();
  const int iters = (__builtin_amdgcn_readfirstlane(m) + 7) >> 3;
  for (int i = 0; i < iters; ++i) {
    const int ia = __shfl(q_id, 8 * i + grp, 64), ib = __shfl(q_id, 8 * i + 4 + grp, 64);
    float4 va[NJ], vb[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int col = gl * 4 + 64 * j;
      va[j] = (col < D && ia != PAD_ID) ? ld4t(A.items, (size_t)ia * D + col, A.items_f16) : make_float4(0.f, 0.f, 0.f, 0.f);
      vb[j] = (col < D && ib != PAD_ID) ? ld4t(A.items, (size_t)ib * D + col, A.items_f16) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    float sa = 0.f, sb = 0.f;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      sa = fmaf(u[j].x, va[j].x, sa); sa = fmaf(u[j].y, va[j].y, sa); sa = fmaf(u[j].z, va[j].z, sa); sa = fmaf(u[j].w, va[j].w, sa);
      sb = fmaf(u[j].x, vb[j].x, sb); sb = fmaf(u[j].y, vb[j].y, sb); sb = fmaf(u[j].z, vb[j].z, sb); sb = fmaf(u[j].w, vb[j].w, sb);
    }
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) { sa += __shfl_xor(sa, o, 64); sb += __shfl_xor(sb, o, 64); }
    // candidate 8 i + 4 b + g was summed by lane group g: lane l = 8 i + 4 b + g takes it
    const float ta = __shfl(sa, (lane & 3) << 4, 64), tb = __shfl(sb, (lane & 3) << 4, 64);
    if ((lane >> 3) == i) mine = (lane & 4) ? tb : ta;
  }
  if (q_id == PAD_ID) mine = neg_inf();
  else if (q_bin < A.n_dist) mine += wd * A.sts[(size_t)r * (A.n_dist + 1) + q_bin];
  const float ts = __shfl(cs, A.k - 1, 64);
  const int ti = __shfl(ci, A.k - 1, 64);
  if (__ballot(q_id != PAD_ID && better(mine, q_id, ts, ti))) top64_merge(cs, ci, mine, q_id);
}

}  // namespace

template <int NJ>
__global__ __launch_bounds__(256) void near_kernel(NearArgs A) {
  __shared__ int s_band[2];
  __shared__ float m_s[POI_NWAVE][NEAR_K_MAX];
  __shared__ int m_i[POI_NWAVE][NEAR_K_MAX];
  __shared__ int m_cnt[POI_NWAVE];
  const int tid = threadIdx.x, lane = lane_id(), w = wave_id(), gl = lane & 15;
  const int S = A.n_split, r = blockIdx.x / S, s = blockIdx.x - r * S;
  const int D = A.dim, N = A.n_item;
  const int anchor = A.anchor ? A.anchor[r] : -1;
  const int e0 = A.ex ? A.ex_off[r] : 0, e1 = A.ex ? A.ex_off[r + 1] : 0;
  int bad = anchor < -1 || anchor >= N || e1 < e0 || e0 < 0;
  if (!bad)
    for (int i = e0 + tid; i < e1; i += 256) bad |= (unsigned)A.ex[i] >= (unsigned)N;
  if (__syncthreads_or(bad)) {      // a rejected row: an empty list, counted once
    if (s == 0 && tid == 0) atomicAdd(A.bad, 1);
    if (w == 0) list_emit<NEAR_K_MAX>(A, A.part_s != nullptr, r, s, neg_inf(), PAD_ID, 0);
    return;
  }
  const bool radius = anchor >= 0 && A.c_r < __builtin_huge_val();
  const bool geo = anchor >= 0 && A.wd != nullptr;
  double lat1 = 0.0, lon1 = 0.0, c1 = 0.0;
  if (radius || geo) { lat1 = A.coords[2 * (size_t)anchor]; lon1 = A.coords[2 * (size_t)anchor + 1]; c1 = A.cphi[anchor]; }
  if (tid == 0) {
    s_band[0] = radius ? lat_bound<false>(A.coords, A.order, N, lat1 - A.band_deg) : 0;
    s_band[1] = radius ? lat_bound<true>(A.coords, A.order, N, lat1 + A.band_deg) : N;
  }
  __syncthreads();
  const int b0 = s_band[0];
  const long long L = s_band[1] - b0;
  const int lo = b0 + (int)(L * s / S), hi = b0 + (int)(L * (s + 1) / S);
  const float wd = A.wd ? A.wd[0] : 0.f;
  float4 u[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int col = gl * 4 + 64 * j;
    u[j] = col < D ? ld4(A.users + (size_t)r * D + col) : make_float4(0.f, 0.f, 0.f, 0.f);
  }
  float cs = neg_inf();
  int ci = PAD_ID;                  // the wave's best 64 so far, sorted over its lanes
  int q_id = PAD_ID, q_bin = A.n_dist, qn = 0, count = 0;
  for (int p0 = lo + w * 64; p0 < hi; p0 += 256) {
    const int p = p0 + lane;
    int id = -1, bin = A.n_dist;
    bool hit = p < hi;
    if (hit) { id = radius ? A.order[p] : p; hit = (unsigned)id < (unsigned)N; }
    if (hit && (radius || geo)) {
      const double c = haversine_c(lat1, lon1, c1, A.coords[2 * (size_t)id], A.coords[2 * (size_t)id + 1], A.cphi[id]);
      if (radius) hit = c < A.c_r || id == anchor;
      if (hit && geo) bin = bin_of_c(c, A.thr, A.n_dist, A.bin_scale);
    }
    if (hit && e1 > e0) {           // ascending ids: first entry >= id
      int a = e0, b = e1;
      while (a < b) { const int md = (a + b) >> 1; if (A.ex[md] < id) a = md + 1; else b = md; }
      hit = !(a < e1 && A.ex[a] == id);
    }
    const unsigned long long bal = __ballot(hit);
    const int h = __popcll(bal);
    count += h;
    // queue lane qn + t takes the hit of rank t
    int t = lane - qn;
    bool take = t >= 0 && t < h;
    int src = take ? nth_bit(bal, t) : 0;
    int gi = __shfl(id, src, 64), gb = __shfl(bin, src, 64);
    if (take) { q_id = gi; q_bin = gb; }
    if (qn + h >= 64) {
      near_score<NJ>(A, r, u, wd, q_id, q_bin, 64, cs, ci);
      t = lane + 64 - qn;           // the hits the full queue had no room for open the next one
      take = t < h;
      src = take ? nth_bit(bal, t) : 0;
      gi = __shfl(id, src, 64); gb = __shfl(bin, src, 64);
      q_id = take ? gi : PAD_ID; q_bin = take ? gb : A.n_dist;
      qn += h - 64;
    } else {
      qn += h;
    }
  }
  if (qn > 0) near_score<NJ>(A, r, u, wd, q_id, q_bin, qn, cs, ci);
  if (lane < NEAR_K_MAX) { m_s[w][lane] = cs; m_i[w][lane] = ci; }
  if (lane == 0) m_cnt[w] = count;
  __syncthreads();
  if (w == 0) {
    float as;
    int ai;
    block_lists_fold<NEAR_K_MAX>(&m_s[0][0], &m_i[0][0], NEAR_K_MAX, as, ai);
    list_emit<NEAR_K_MAX>(A, A.part_s != nullptr, r, s, as, ai, (m_cnt[0] + m_cnt[1]) + (m_cnt[2] + m_cnt[3]));
  }
}

hipError_t launch_near(NearArgs& A, hipStream_t st, Timing* tm) {
  const dim3 grid((unsigned)A.n * (unsigned)A.n_split);
  tm->begin("score_topk_near", st);
  switch ((A.dim + 63) / 64) {
    case 1: hipLaunchKernelGGL(near_kernel<1>, grid, dim3(256), 0, st, A); break;
    case 2: hipLaunchKernelGGL(near_kernel<2>, grid, dim3(256), 0, st, A); break;
    case 3: hipLaunchKernelGGL(near_kernel<3>, grid, dim3(256), 0, st, A); break;
    case 4: hipLaunchKernelGGL(near_kernel<4>, grid, dim3(256), 0, st, A); break;
    default: return hipErrorInvalidValue;
  }
  if (A.part_s) launch_topk_slices_merge(slice_lists(A), NEAR_K_MAX, A.n, st);
  tm->end(st);
  return hipGetLastError();
}

}  // namespace poi
