// Group recommendation (poi_group_topk, poi_group_topk_scores): the top-K of an AGGREGATE of the members' scores - the mean, or the
// minimum ("least misery") - for a party of users, without the (members, n_item) score matrix.
//
//   s(m, j)  = poi_score_rank's s(r, j): users[m] . items[j] from tile_product (tile_product.h), plus wd * sts[m][bin(last_poi[m], j)]
//   a(g, j)  = min over the group's list, or the float32 sum over the list IN LIST ORDER (a left-to-right chain from the first member)
//              divided by float(M)
//   C(g)     = [0, n_item) minus the group's exclusion list;  the list is C(g) by descending a, ties by ascending id.
//
// group_kernel: a workgroup owns GROUP_GPT consecutive groups and one slice of the item range; its four waves take a quarter of the slice
// each.  The groups are packed, whole, into PASSES of at most 32 member rows (greedy, in call order); a pass gathers its member rows once
// (A fragments in registers) and streams the slice's 32-item tiles past them on the f32 matrix pipe, as rank.hip does.  The epilogue is a
// segmented reduction over the member rows of the accumulator tile: the tile (distance term added in the registers) goes through LDS,
// lane (item, half) walks the rows of one group of a pair - the two halves take the two groups - in list order, so the order of the
// additions is a function of the member's position alone, whatever row of the tile the group was packed into.  A group of more than 32
// members is a pass of its own: per item tile its rows are walked in chunks of 32 and the chain carries on from chunk to chunk.
// Every pair's aggregate is first compared with the K-th entry of its group's list (LDS reads only; one ballot for the common tile);
// the survivors are looked up in the exclusion list and inserted into the wave's sorted LDS list, one at a time (list_take; many at
// once, as in the first tiles, through lds_list_merge's sort).  The waves' lists meet in LDS; on the split path they go to per-slice
// partial lists that topk_slices_merge_kernel (topk_merge.hip) folds.  The order (descending a, ascending id) is total, the aggregate of a pair
// does not depend on the slice, the wave or the pass: every grid gives the same bits, and a group gives the same bits alone as in a
// call of thousands.  No float atomics; a rejected group is counted with one integer atomic.
//
// Bytes: per pass the slice of the item table once (4 dim n_item per workgroup row of the grid, 2 dim from a half table), + 24 n_item of
// coordinates with the distance term; 8 groups of 4 members are ONE pass.  Flops 2 (32 rows) n_item dim per pass on the f32 matrix pipe.
//
// group_scores_kernel applies the same definition to explicit score rows (one workgroup per group, coalesced reads of the members' rows).
#include "poi_common.h"
#include "poi_kernels.h"
#include "launch_common.h"
#include "tile_walk.h"
#include "topk_list.h"

namespace poi {

namespace {

constexpr int GROUP_LD = 40;                // row stride of the LDS score tile (the two lane halves write rows 4 apart: other banks)

// one step of the aggregate over a group's list, in list order; `first`: the list's first member
__device__ __forceinline__ float agg_step(int agg, bool first, float v, float x) {
  if (first) return x;
  if (agg) return (x < v || x != x) ? x : v;       // the minimum; a NaN stays
  return v + x;
}
// mean: one IEEE division; least misery: -0 becomes +0, so that the bits do not depend on which of two zeros came first
__device__ __forceinline__ float agg_final(int agg, float v, int M) { return agg ? v + 0.f : v / (float)M; }

// group g's lists: members inside [0, n), offsets in order, exclusion ids ascending inside [0, n_item).  Contains a barrier.
__device__ __forceinline__ int group_check(const GroupArgs& A, int g, int& a, int& b, int& e0, int& e1) {
  const int tid = threadIdx.x;
  a = A.g_off[g]; b = A.g_off[g + 1]; e0 = 0; e1 = 0;
  int bad = a < 0 || b < a;
  if (!bad)
    for (int p = a + tid; p < b; p += POI_BLOCK) bad |= (unsigned)A.g_mem[p] >= (unsigned)A.n;
  if (A.ex) {
    e0 = A.ex_off[g]; e1 = A.ex_off[g + 1];
    if (e0 < 0 || e1 < e0) bad = 1;
    else
      for (int p = e0 + tid; p < e1; p += POI_BLOCK) { const int v = A.ex[p]; bad |= (unsigned)v >= (unsigned)A.n_item || (p > e0 && A.ex[p - 1] >= v); }
  }
  return __syncthreads_or(bad);
}

// lanes with `mine` offer (v, j) to the sorted list (ls, lx) of a group whose exclusion list is ex[e0 .. e1)
__device__ __forceinline__ void offer(float* ls, int* lx, const int* ex, int e0, int e1, bool mine, float v, int j, int K) {
  bool cand = mine && better(v, j, ls[K - 1], lx[K - 1]);
  if (cand && e1 > e0) cand = !listed(ex, e0, e1, j);
  const unsigned long long bal = __ballot(cand);
  if (bal) list_take(ls, lx, bal, cand, v, j, K);
}

}  // namespace

// BIG = false: GROUP_GPT groups per workgroup, those of at most 32 members.  BIG = true: one group per workgroup, those of more than 32
// members (a workgroup whose group is smaller leaves at once): the same walk with the member rows reloaded chunk by chunk per item tile.
// Every group is emitted by exactly one of the two.
template <int D8, bool DB, bool GEO, bool BIG>
__global__ __launch_bounds__(POI_BLOCK) void group_kernel(GroupArgs A) {
  constexpr int GPT = BIG ? 1 : GROUP_GPT;
  __shared__ float s_sc[POI_NWAVE][32 * GROUP_LD];
  __shared__ float l_s[POI_NWAVE][GPT][64];
  __shared__ int l_i[POI_NWAVE][GPT][64];
  __shared__ int s_g0[GPT], s_gm[GPT], s_e0[GPT], s_e1[GPT];                        // member list start, size (-1: rejected), exclusion list
  __shared__ int s_mem[POI_NWAVE][32], s_has[POI_NWAVE][32], s_r0[POI_NWAVE][GPT];  // per wave: a tile row's member, has a last POI; a group's first row
  __shared__ double s_ulat[POI_NWAVE][32], s_ulon[POI_NWAVE][32], s_ucp[POI_NWAVE][32];
  extern __shared__ __align__(16) double s_thr[];    // GEO: thr[n_dist]
  const int tid = threadIdx.x, lane = lane_id(), w = wave_id(), li = lane & 31, h = lane >> 5;
  const int S = A.n_split, gt = blockIdx.x / S, sl = blockIdx.x - gt * S;
  const int D = A.dim, N = A.n_item, K = A.k, agg = A.agg;

  if constexpr (BIG) {
    const int a = A.g_off[gt], b = A.g_off[gt + 1];
    if (a < 0 || b - a <= 32) return;               // (block-uniform: before any barrier)
  }
  for (int q = 0; q < GPT; ++q) {
    const int g = gt * GPT + q;
    int a = 0, b = 0, e0 = 0, e1 = 0, bad = 0;
    if (g < A.n_grp) bad = group_check(A, g, a, b, e0, e1);       // (block-uniform)
    if (BIG && bad) return;                          // (the other kernel reports it)
    if (tid == 0) {
      s_g0[q] = a; s_gm[q] = bad ? -1 : b - a; s_e0[q] = bad ? 0 : e0; s_e1[q] = bad ? 0 : e1;
      if (bad && sl == 0) atomicAdd(A.bad, 1);
    }
  }
  if (GEO)
    for (int i = tid; i < A.n_dist; i += POI_BLOCK) s_thr[i] = A.thr[i];
  for (int q = 0; q < GPT; ++q) { l_s[w][q][lane] = neg_inf(); l_i[w][q][lane] = PAD_ID; }
  __syncthreads();

  int ntile, tb, te;
  wave_tile_range(N, sl, S, w, ntile, tb, te);
  const float wd = GEO ? A.wd[0] : 0.f;

  int q = 0;
  while (tb < te && q < GPT) {
    if (s_gm[q] <= 0 || (!BIG && s_gm[q] > 32)) { ++q; continue; }
    // the next pass: groups q0 .. q1 - 1, whole, while they fit 32 rows - or (BIG) the one group in nch chunks
    const int q0 = q, M0 = s_gm[q0];
    const int nch = BIG ? (M0 + 31) / 32 : 1;
    if (BIG) ++q;
    else {
      int rows = 0;
      while (q < GPT && rows + max(s_gm[q], 0) <= 32) { rows += max(s_gm[q], 0); ++q; }
    }
    const int q1 = q;
    if (lane == 0) {
      int rs = 0;
      for (int p = q0; p < q1; ++p) { s_r0[w][p - q0] = rs; rs += max(s_gm[p], 0); }
    }

    // rows of chunk c: the members of the pass's groups in list order (one chunk), or members 32 c .. of the one group
    auto setup_rows = [&](int c) {
      if (lane < 32) {
        int member = -1;
        if (BIG) {
          const int pos = 32 * c + lane;
          if (pos < M0) member = A.g_mem[s_g0[q0] + pos];
        } else {
          int off = lane;
          for (int p = q0; p < q1; ++p) {
            const int M = max(s_gm[p], 0);
            if (off >= 0 && off < M) member = A.g_mem[s_g0[p] + off];
            off -= M;
          }
        }
        s_mem[w][lane] = member;
        if (GEO) {                                    // (load_row_geo's text, and block_lists_fold's below: through the helpers this kernel compiles to other code)
          const int lp = member >= 0 ? A.last_poi[member] : -1;
          const int lc = min(max(lp, 0), N - 1);                 // (an id outside the table reads no memory outside it)
          s_has[w][lane] = lp >= 0;
          s_ulat[w][lane] = A.coords[2 * (size_t)lc]; s_ulon[w][lane] = A.coords[2 * (size_t)lc + 1]; s_ucp[w][lane] = A.cphi[lc];
        }
      }
      wave_fence();
    };

    float4 af[D8];
    setup_rows(0);
    if (!BIG) load_frag<D8>(af, A.users, 0, (size_t)max(s_mem[w][li], 0), D, h);

    float4 b0[D8], b1[DB ? D8 : 1];
    load_item_tile<D8>(b0, A, tb, li, h);
    for (int tile = tb; tile < te; ++tile) {
      if constexpr (DB) { if (tile + 1 < te) load_item_tile<D8>(b1, A, tile + 1, li, h); }
      const int j = tile * 32 + li;
      const bool jvalid = j < N;
      double jlat, jlon, jcp;
      item_tile_coords<GEO>(A, j, jlat, jlon, jcp);
      float carry = 0.f;                            // BIG: the group's chain, from chunk to chunk
      for (int c = 0; c < nch; ++c) {
        if (BIG) {
          if (c > 0 || tile > tb) setup_rows(c);
          load_frag<D8>(af, A.users, 0, (size_t)max(s_mem[w][li], 0), D, h);
        }
        const f32x16 acc = tile_product<D8>(af, b0);      // (tile_walk.h: the walk's contract)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int ul = acc_tile_row(r, 4 * h);
          float s = acc[r];
          if (GEO) {
            if (s_has[w][ul]) s = __fmaf_rn(wd, geo_prob(A, s_thr, s_mem[w][ul], s_ulat[w][ul], s_ulon[w][ul], s_ucp[w][ul], jlat, jlon, jcp), s);
          }
          s_sc[w][ul * GROUP_LD + li] = s;
          if (GEO) __builtin_amdgcn_sched_barrier(0);      // one row's distance term in flight at a time (the scheduler would issue all 16 rows' first)
        }
        wave_fence();
        if (BIG) {
          const int rows = min(32, M0 - 32 * c);
          for (int m = 0; m < rows; ++m) carry = agg_step(agg, c == 0 && m == 0, carry, s_sc[w][m * GROUP_LD + li]);
          wave_fence();                             // the tile is read before the next chunk overwrites it
        }
      }
      if constexpr (BIG) {
        offer(l_s[w][q0], l_i[w][q0], A.ex, s_e0[q0], s_e1[q0], h == 0 && jvalid, agg_final(agg, carry, M0), j, K);
      } else {
        // pairs of groups: lane half h reduces group q0 + 2 i + h.  First every pair's aggregate and its compare with the K-th entry of
        // the group's list (LDS reads only: they overlap), then the rare insertions
        float vq[GPT / 2];
        unsigned cm = 0u;
#pragma unroll
        for (int i = 0; i < GPT / 2; ++i) {
          const int mq = q0 + 2 * i + h;
          const int M = mq < q1 ? s_gm[mq] : 0;
          float v = 0.f;
          if (M > 0) {
            const int r0 = s_r0[w][mq - q0];
            for (int m = 0; m < M; ++m) v = agg_step(agg, m == 0, v, s_sc[w][(r0 + m) * GROUP_LD + li]);
            v = agg_final(agg, v, M);
            if (jvalid && better(v, j, l_s[w][mq][K - 1], l_i[w][mq][K - 1])) cm |= 1u << i;
          }
          vq[i] = v;
        }
        if (__ballot(cm != 0u)) {
#pragma unroll
          for (int i = 0; i < GPT / 2; ++i) {
#pragma unroll
            for (int hh = 0; hh < 2; ++hh) {
              const int qq = q0 + 2 * i + hh;
              bool cand = h == hh && ((cm >> i) & 1u);
              if (!__ballot(cand)) continue;          // (wave-uniform; a lane of half hh with the bit set has qq < q1)
              if (cand && s_e1[qq] > s_e0[qq]) cand = !listed(A.ex, s_e0[qq], s_e1[qq], j);
              const unsigned long long bal = __ballot(cand);
              if (bal) list_take(l_s[w][qq], l_i[w][qq], bal, cand, vq[i], j, K);
            }
          }
        }
        wave_fence();                               // the tile is read before the next one overwrites it
      }
      if constexpr (DB) {
#pragma unroll
        for (int m = 0; m < D8; ++m) b0[m] = b1[m];
      } else {
        if (tile + 1 < te) load_item_tile<D8>(b0, A, tile + 1, li, h);
      }
    }
  }

  __syncthreads();
  if (w == 0) {
    for (int p = 0; p < GPT; ++p) {
      const int g = gt * GPT + p;
      if (g >= A.n_grp) break;
      if (!BIG && s_gm[p] > 32) continue;           // (the other kernel's)
      const int l = lane & (GROUP_K_MAX - 1), hw = lane >> 5;
      float as = l_s[hw][p][l], bs = l_s[2 + hw][p][l];
      int ai = l_i[hw][p][l], bi = l_i[2 + hw][p][l];
      wave_sort_desc(as, ai);
      top64_merge(as, ai, bs, bi);
      const int cnt = (s_gm[p] > 0 && sl == 0) ? N - (s_e1[p] - s_e0[p]) : 0;
      list_emit<GROUP_K_MAX>(A, A.part_s != nullptr, g, sl, as, ai, cnt);
    }
  }
}

// The definition on explicit score rows: one workgroup per group, a wave takes 64 POIs per round and reads the members' rows in list order.
__global__ __launch_bounds__(POI_BLOCK) void group_scores_kernel(const float* __restrict__ scores, GroupArgs A) {
  __shared__ float l_s[POI_NWAVE][64];
  __shared__ int l_i[POI_NWAVE][64];
  const int g = blockIdx.x, lane = lane_id(), w = wave_id(), N = A.n_item, K = A.k, agg = A.agg;
  int a, b, e0, e1;
  const int bad = group_check(A, g, a, b, e0, e1);
  const int M = bad ? 0 : b - a;
  if (bad && threadIdx.x == 0) atomicAdd(A.bad, 1);
  l_s[w][lane] = neg_inf(); l_i[w][lane] = PAD_ID;
  wave_fence();
  if (M > 0) {
    for (int j0 = w * 64; j0 < N; j0 += POI_BLOCK) {
      const int j = j0 + lane;
      const bool jvalid = j < N;
      float v = 0.f;
      for (int m = 0; m < M; ++m) {
        const int mem = A.g_mem[a + m];
        v = agg_step(agg, m == 0, v, jvalid ? scores[(size_t)mem * N + j] : 0.f);
      }
      offer(l_s[w], l_i[w], A.ex, e0, e1, jvalid, agg_final(agg, v, M), j, K);
    }
  }
  __syncthreads();
  if (w == 0) {
    float as;
    int ai;
    block_lists_fold<GROUP_K_MAX>(&l_s[0][0], &l_i[0][0], 64, as, ai);
    list_emit<GROUP_K_MAX>(A, false, g, 0, as, ai, M > 0 ? N - (e1 - e0) : 0);
  }
}

template <bool GEO>
static hipError_t launch_group_g(const GroupArgs& A, hipStream_t st) {
  return by_dim<64>(A.dim, [&](auto d8, auto db) -> hipError_t {
    constexpr int D8 = decltype(d8)::value;
    constexpr bool DB = decltype(db)::value;
    const unsigned n_gtile = (unsigned)((A.n_grp + GROUP_GPT - 1) / GROUP_GPT), S = (unsigned)A.n_split;
    const size_t lds = GEO ? sizeof(double) * A.n_dist : 0;
    hipLaunchKernelGGL((group_kernel<D8, DB, GEO, false>), dim3(n_gtile * S), dim3(POI_BLOCK), lds, st, A);
    hipLaunchKernelGGL((group_kernel<D8, DB, GEO, true>), dim3((unsigned)A.n_grp * S), dim3(POI_BLOCK), lds, st, A);
    return hipSuccess;
  });
}

hipError_t launch_group(GroupArgs& A, hipStream_t st, Timing* tm) {
  Timing::Scope rec(tm, "group_topk", st);
  const hipError_t e = A.wd ? launch_group_g<true>(A, st) : launch_group_g<false>(A, st);
  if (e != hipSuccess) return e;
  if (A.part_s) launch_topk_slices_merge(slice_lists(A), GROUP_K_MAX, A.n_grp, st);
  return rec.close();
}

hipError_t launch_group_scores(const float* scores, GroupArgs& A, hipStream_t st, Timing* tm) {
  tm->begin("group_topk_scores", st);
  hipLaunchKernelGGL(group_scores_kernel, dim3((unsigned)A.n_grp), dim3(POI_BLOCK), 0, st, scores, A);
  tm->end(st);
  return hipGetLastError();
}

}  // namespace poi
