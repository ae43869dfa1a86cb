// Filtered recommendation (poi_filter_build, poi_score_topk_filtered, poi_topk_filtered_scores): the top-K among the POIs that pass an
// attribute predicate - "the best restaurants for this user" - without the (n, n_item) score matrix and without an exclusion list that
// names the complement.
//
//   pass(q, j) = (list of q empty or cat[j] in it) and (flags[j] & need) == need and (any == 0 or flags[j] & any) and !(flags[j] & forbid)
//   bits       (n_pred, ldw) words: POI j is bit j & 31 of word j >> 5 of its predicate's row; bits at j >= n_item are never trusted
//   C(r)       = { j : bit j of bits[pred[r]] and (no radius or c(anchor[r], j) < c_r or j == anchor[r]) and j not on the row's list }
//   s(r, j)    poi_score_rank's s(r, j) on EVERY path: users[r] . items[j] from tile_product (tile_product.h), plus
//              wd * sts[r][bin(anchor[r], j)] for bin < n_dist through geo_prob; a row without an anchor has no distance term
//   result     the best min(k, |selectable C(r)|) entries by better() (descending score, ascending id), k <= 32.  NaN and -inf are not
//              selectable, +inf is; -0.0 and +0.0 are one score, written as +0.0.  count = |C(r)|.
//
// filter_build_kernel: one predicate per blockIdx.y, its category list as an n_cat-bit set in LDS, one POI per lane, a ballot forms two
// words.  Integer work only.
//
// filter_walk_kernel: the item-stationary tile walk in tile_walk.h's steps - a workgroup owns a 32-row tile and a slice of the item range,
// its waves a quarter of the slice each (wave_tile_range), the rows' A fragments in registers (load_row_tile), the item tiles streamed
// past them (load_item_tile), one sorted list per (wave, row) in LDS (topk_list.h).  A 32-item
// tile is exactly one bitmap word per row: lane li fetches row li's word two tiles ahead, so that one ballot decides BEFORE the item
// rows of a tile are requested whether any row wants it - a tile whose 32 words are zero costs neither a load nor a product.  Bit li of
// the row's word (a broadcast read from LDS) gates the distance term and the compare against the row's K-th entry; the exclusion lookup
// and the insertions stay in the rare part.  count = popcount of the row's words - the listed ids whose bit is set: integers, summed
// over the slices by the merge.
//
// filter_gather_kernel: near.hip's structure - one workgroup per row and slice, candidates compacted into a 64-entry queue.  Without a
// radius a wave reads 64 bitmap words per round and every lane offers its lowest remaining bit until a ballot finds none; with one it
// walks the latitude band and tests the bit after the exact Haversine test.  A full queue is scored as two tile_product tiles with the
// row's fragment in every A row and the gathered item rows as B (rank_targets_kernel's trick): every accumulator of a lane holds the
// score of ITS candidate, in the walk's bits.  31/32 of the matrix work is wasted; the path pays where the item-row gathers bound it.
//
// Both paths keep exact lists under one total order over one score definition: the same bits, on every grid, a row alone or among
// thousands.  No float atomics; rejected rows (predicate index, anchor or exclusion list out of range) are counted with one integer
// atomic.
//
// filter_scores_kernel applies the definition to explicit float32 score rows, one workgroup per row.
#include "poi_common.h"
#include "poi_kernels.h"
#include "launch_common.h"
#include "tile_walk.h"
#include "topk_list.h"

namespace poi {

namespace {

constexpr int WALK_LIST = 64;                                                // list stride: list_take works on one entry per lane
constexpr int WALK_LISTS_BYTES = POI_NWAVE * 32 * WALK_LIST * 8;             // the waves' per-row lists: scores, then ids

}  // namespace

__global__ __launch_bounds__(POI_BLOCK) void filter_build_kernel(FilterBuildArgs A) {
  __shared__ unsigned s_set[FILTER_NCAT_MAX / 32];
  const int q = blockIdx.y, tid = threadIdx.x, lane = lane_id(), w = wave_id();
  const int c0 = A.pc_off[q], c1 = A.pc_off[q + 1];
  const bool any_cat = c1 <= c0;
  for (int i = tid; i < FILTER_NCAT_MAX / 32; i += POI_BLOCK) s_set[i] = 0u;
  __syncthreads();
  for (int i = c0 + tid; i < c1; i += POI_BLOCK) {
    const int c = A.pc[i];
    if ((unsigned)c < (unsigned)A.n_cat) atomicOr(&s_set[c >> 5], 1u << (c & 31));
  }
  __syncthreads();
  const unsigned need = A.need[q], any = A.any[q], forbid = A.forbid[q];
  const bool flagged = A.flags && (need | any | forbid) != 0u;      // (a predicate without flag words reads no flags: every word passes it)
  const long long span = A.ldw * 32;                // bit positions of a row, the pad words included
  unsigned* const out = A.bits + (size_t)q * A.ldw;
  int cnt = 0, nbad = 0;
  for (long long j0 = ((long long)blockIdx.x * POI_NWAVE + w) * 64; j0 < span; j0 += (long long)gridDim.x * POI_BLOCK) {
    const long long j = j0 + lane;
    bool pass = false, stray = false;
    if (j < A.n_item) {
      const unsigned f = flagged ? A.flags[j] : 0u;
      pass = (f & need) == need && (any == 0u || (f & any) != 0u) && (f & forbid) == 0u;
      if (A.cat) {
        const int c = A.cat[j];
        stray = (unsigned)c >= (unsigned)A.n_cat;
        if (!any_cat) pass = pass && !stray && ((s_set[c >> 5] >> (c & 31)) & 1u);
      }
    }
    const unsigned long long bal = __ballot(pass);
    cnt += __popcll(bal);
    nbad += __popcll(__ballot(stray));
    const long long wi = j0 >> 5;
    if (lane == 0) out[wi] = (unsigned)bal;
    if (lane == 32 && wi + 1 < A.ldw) out[wi + 1] = (unsigned)(bal >> 32);
  }
  if (lane == 0) {
    if (A.count && cnt) atomicAdd(A.count + q, cnt);
    if (q == 0 && nbad) atomicAdd(A.bad, nbad);      // a POI is counted once, whatever the number of predicates
  }
}

__global__ __launch_bounds__(256) void filter_scores_kernel(FilterScoresArgs A) {
  __shared__ float m_s[POI_NWAVE][FILTER_K_MAX];
  __shared__ int m_i[POI_NWAVE][FILTER_K_MAX];
  __shared__ int m_cnt[POI_NWAVE];
  const int tid = threadIdx.x, lane = lane_id(), w = wave_id();
  const int r = blockIdx.x, N = A.n_item;
  const int q = A.pred ? A.pred[r] : 0;
  const int e0 = A.ex ? A.ex_off[r] : 0, e1 = A.ex ? A.ex_off[r + 1] : 0;
  int bad = (unsigned)q >= (unsigned)A.n_pred || e1 < e0 || e0 < 0;
  if (!bad) bad = ex_slice_bad(A.ex, e0, e1, N, tid, 256);
  if (__syncthreads_or(bad)) {      // a rejected row: an empty list, counted once
    if (tid == 0) atomicAdd(A.bad, 1);
    if (w == 0) list_emit<FILTER_K_MAX>(A, false, r, 0, neg_inf(), PAD_ID, 0);
    return;
  }
  const unsigned* const bw = A.bits + (size_t)q * A.ldw;
  const float* const sr = A.scores + (size_t)r * A.ld;
  float cs = neg_inf();
  int ci = PAD_ID, count = 0;       // the wave's best 64 so far, sorted over its lanes
  for (int p0 = w * 64; p0 < N; p0 += 256) {
    const int p = p0 + lane;
    bool hit = p < N && ((bw[p >> 5] >> (p & 31)) & 1u);
    if (hit && e1 > e0) hit = !listed(A.ex, e0, e1, p);
    count += __popcll(__ballot(hit));
    float s = hit ? one_zero(sr[p]) : neg_inf();
    const bool sel = hit && selectable(s);
    s = sel ? s : neg_inf();
    const int id = sel ? p : PAD_ID;
    const float ts = __shfl(cs, A.k - 1, 64);
    const int ti = __shfl(ci, A.k - 1, 64);
    if (__ballot(sel && better(s, id, ts, ti))) top64_merge(cs, ci, s, id);
  }
  if (lane < FILTER_K_MAX) { m_s[w][lane] = cs; m_i[w][lane] = ci; }
  if (lane == 0) m_cnt[w] = count;
  __syncthreads();
  if (w == 0) {
    float as;
    int ai;
    block_lists_fold<FILTER_K_MAX>(&m_s[0][0], &m_i[0][0], FILTER_K_MAX, as, ai);
    list_emit<FILTER_K_MAX>(A, false, r, 0, as, ai, (m_cnt[0] + m_cnt[1]) + (m_cnt[2] + m_cnt[3]));
  }
}

template <int D8, bool DB, bool GEO>
__global__ __launch_bounds__(POI_BLOCK) void filter_walk_kernel(FilterArgs A) {
  __shared__ int s_e0[32], s_e1[32], s_ok[32], s_has[32];      // per tile row: exclusion list, ranked at all, has an anchor
  __shared__ long long s_pb[32];                                // ... and where its predicate's words start
  __shared__ double s_ulat[32], s_ulon[32], s_ucp[32];
  __shared__ unsigned s_word[POI_NWAVE][32];                    // the rows' words of the tile a wave is at
  __shared__ int s_cnt[POI_NWAVE][32];
  extern __shared__ __align__(16) unsigned char s_dyn[];       // lists (WALK_LISTS_BYTES) | GEO: thr[n_dist]
  float* const l_s = reinterpret_cast<float*>(s_dyn);
  int* const l_i = reinterpret_cast<int*>(s_dyn + WALK_LISTS_BYTES / 2);
  double* const s_thr = reinterpret_cast<double*>(s_dyn + WALK_LISTS_BYTES);
  const int tid = threadIdx.x, lane = lane_id(), w = wave_id(), li = lane & 31, h = lane >> 5;
  const int S = A.n_split, ut = blockIdx.x / S, sl = blockIdx.x - ut * S;
  const int N = A.n_item, K = A.k;

  // the tile's rows: predicate index and anchor in range, exclusion lists with offsets in order and ids ascending inside [0, N)
  for (int i = w; i < 32; i += POI_NWAVE) {
    const int r = ut * 32 + i;
    int bad = 0, e0 = 0, e1 = 0, q = 0;
    if (r < A.n) {
      q = A.pred ? A.pred[r] : 0;
      const int an = A.last_poi ? A.last_poi[r] : -1;
      bad = (unsigned)q >= (unsigned)A.n_pred || an < -1 || an >= N;
      if (A.ex) bad |= check_ex_row(A.ex_off, A.ex, r, N, lane, e0, e1);
    }
    bad = __any(bad) ? 1 : 0;
    if (lane == 0) {
      const int ok = r < A.n && !bad;
      s_ok[i] = ok; s_e0[i] = ok ? e0 : 0; s_e1[i] = ok ? e1 : 0; s_pb[i] = ok ? (long long)q * A.ldw : 0;
      if (bad && sl == 0) atomicAdd(A.bad, 1);
      if (GEO) load_row_geo(A, ok ? r : -1, N, s_has[i], s_ulat[i], s_ulon[i], s_ucp[i]);
    }
  }
  if (GEO)
    for (int i = tid; i < A.n_dist; i += POI_BLOCK) s_thr[i] = A.thr[i];
  for (int e = tid; e < POI_NWAVE * 32 * WALK_LIST; e += POI_BLOCK) { l_s[e] = neg_inf(); l_i[e] = PAD_ID; }
  __syncthreads();

  int ntile, tb, te;
  wave_tile_range(N, sl, S, w, ntile, tb, te);
  const float wd = GEO ? A.wd[0] : 0.f;
  float* const ls = l_s + w * 32 * WALK_LIST;
  int* const lx = l_i + w * 32 * WALK_LIST;

  // row li's word of tile t (both lane halves hold it); a row that is not ranked has none, the table's last word loses its tail
  const bool rowlive = s_ok[li] != 0;
  const unsigned* const wp = A.bits + s_pb[li];
  const unsigned tmask = tail_mask(N);
  auto word = [&](int t) -> unsigned {
    if (t >= te || !rowlive) return 0u;
    const unsigned v = wp[t];
    return t == ntile - 1 ? v & tmask : v;
  };

  float4 af[D8];
  load_row_tile<D8>(af, A, ut, li, h);
  float4 b0[D8], b1[DB ? D8 : 1];
  unsigned w0 = word(tb), w1 = word(tb + 1);
  bool live = __ballot(w0 != 0u) != 0ull;           // (wave-uniform) some row of the tile wants this item tile
  if (live) load_item_tile<D8>(b0, A, tb, li, h);
  int pc = 0;                                       // passing POIs of row li in this wave's tiles
  for (int tile = tb; tile < te; ++tile) {
    const unsigned w2 = word(tile + 2);
    const bool live1 = __ballot(w1 != 0u) != 0ull;
    if constexpr (DB) { if (live1) load_item_tile<D8>(b1, A, tile + 1, li, h); }
    pc += __popc(w0);
    if (live) {
      __builtin_amdgcn_wave_barrier();
      s_word[w][li] = w0;
      __builtin_amdgcn_wave_barrier();              // (a wave's LDS accesses complete in order: the reads below see it)
      f32x16 acc = tile_product<D8>(af, b0);       // (tile_walk.h: the walk's contract)
      const int j = tile * 32 + li;
      double jlat, jlon, jcp;
      item_tile_coords<GEO>(A, j, jlat, jlon, jcp);
      const int hb = opaque_half_base(h);
      unsigned cm = 0u;                             // bit r: acc[r] passes and beats the K-th entry of its row's list
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int ul = acc_tile_row(r, hb);
        const bool bit = (s_word[w][ul] >> li) & 1u;
        float s = acc[r];
        if (GEO) {
          if (bit && s_has[ul]) s = geo_add(A, wd, s_thr, ut, ul, s_ulat, s_ulon, s_ucp, jlat, jlon, jcp, s);
        }
        s = one_zero(s);
        acc[r] = s;
        if (bit && selectable(s) && better(s, j, ls[ul * WALK_LIST + K - 1], lx[ul * WALK_LIST + K - 1])) cm |= 1u << r;
        if (GEO) __builtin_amdgcn_sched_barrier(0); // one row's distance term in flight at a time (the scheduler would issue all 16 rows' first)
      }
      if (__ballot(cm != 0u)) {
        // the rare part: row by row, the exclusion lookup and the insertions
        for (int row = 0; row < 32; ++row) {
          int rr;
          bool cand = rare_row(row, h, cm, rr);
          if (!__ballot(cand)) continue;            // (wave-uniform)
          const float v = acc_row(acc, rr);
          const int e0 = s_e0[row], e1 = s_e1[row];
          if (cand && e1 > e0) cand = !listed(A.ex, e0, e1, j);
          const unsigned long long bal = __ballot(cand);
          if (bal) list_take(ls + row * WALK_LIST, lx + row * WALK_LIST, bal, cand, v, j, K);
        }
      }
    }
    if constexpr (DB) {
      if (live1) {
#pragma unroll
        for (int m = 0; m < D8; ++m) b0[m] = b1[m];
      }
    } else {
      if (live1) load_item_tile<D8>(b0, A, tile + 1, li, h);
    }
    w0 = w1; w1 = w2; live = live1;
  }
  if (h == 0) s_cnt[w][li] = pc;

  __syncthreads();
  // the four waves' lists of a row meet: wave w folds rows w, w + 4, ...
  for (int i = w; i < 32; i += POI_NWAVE) {
    const int row = ut * 32 + i;
    if (row >= A.n) break;
    float cs = l_s[i * WALK_LIST + lane];
    int ci = l_i[i * WALK_LIST + lane];
    for (int ww = 1; ww < POI_NWAVE; ++ww)
      top64_merge(cs, ci, l_s[(ww * 32 + i) * WALK_LIST + lane], l_i[(ww * 32 + i) * WALK_LIST + lane]);
    int cnt = 0;
    if (s_ok[i]) {
      cnt = (s_cnt[0][i] + s_cnt[1][i]) + (s_cnt[2][i] + s_cnt[3][i]);
      if (sl == 0) {                                // the listed ids that pass leave the count (the list is ascending: each id once)
        const unsigned* const rw = A.bits + s_pb[i];
        int x = 0;
        for (int p = s_e0[i] + lane; p < s_e1[i]; p += 64) { const int id = A.ex[p]; x += (rw[id >> 5] >> (id & 31)) & 1u; }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
        cnt -= x;
      }
    }
    list_emit<FILTER_K_MAX>(A, A.part_s != nullptr, row, sl, cs, ci, cnt);
  }
}

namespace {

// scores the queue (lane l: candidate q_id, PAD_ID = none; m = entries in use, wave-uniform) and folds it into the wave's list: two
// tiles of 32 candidates, the row's fragment in every A row - each accumulator of lane l is the score of the candidate of lane l & 31
template <int D8, bool GEO>
__device__ __forceinline__ void gather_score(const FilterArgs& A, int r, const float4 (&af)[D8], float wd, bool has, double ulat, double ulon,
                                             double ucp, int q_id, int m, float& cs, int& ci) {
  const int lane = lane_id(), li = lane & 31, h = lane >> 5, D = A.dim;
  float4 bf[D8];
  const int ia = __shfl(q_id, li, 64);
  load_frag<D8>(bf, A.items, A.items_f16, (size_t)(ia == PAD_ID ? 0 : ia), D, h);
  f32x16 acc = tile_product<D8>(af, bf);
  float mine = acc[0];
  if (m > 32) {
    const int ib = __shfl(q_id, 32 + li, 64);
    load_frag<D8>(bf, A.items, A.items_f16, (size_t)(ib == PAD_ID ? 0 : ib), D, h);
    acc = tile_product<D8>(af, bf);
    if (h) mine = acc[0];
  }
  const bool there = q_id != PAD_ID;
  if (GEO) {
    if (there && has) mine = __fmaf_rn(wd, geo_prob(A, A.thr, r, ulat, ulon, ucp, A.coords[2 * (size_t)q_id], A.coords[2 * (size_t)q_id + 1], A.cphi[q_id]), mine);
  }
  mine = one_zero(mine);
  const bool sel = there && selectable(mine);
  mine = sel ? mine : neg_inf();
  const int id = sel ? q_id : PAD_ID;
  const float ts = __shfl(cs, A.k - 1, 64);
  const int ti = __shfl(ci, A.k - 1, 64);
  if (__ballot(sel && better(mine, id, ts, ti))) top64_merge(cs, ci, mine, id);
}

}  // namespace

template <int D8, bool GEO>
__global__ __launch_bounds__(256) void filter_gather_kernel(FilterArgs A) {
  __shared__ int s_band[2];
  __shared__ float m_s[POI_NWAVE][FILTER_K_MAX];
  __shared__ int m_i[POI_NWAVE][FILTER_K_MAX];
  __shared__ int m_cnt[POI_NWAVE];
  const int tid = threadIdx.x, lane = lane_id(), w = wave_id();
  const int S = A.n_split, r = blockIdx.x / S, s = blockIdx.x - r * S;
  const int D = A.dim, N = A.n_item;
  const int q = A.pred ? A.pred[r] : 0;
  const int anchor = A.last_poi ? A.last_poi[r] : -1;
  const int e0 = A.ex ? A.ex_off[r] : 0, e1 = A.ex ? A.ex_off[r + 1] : 0;
  int bad = (unsigned)q >= (unsigned)A.n_pred || anchor < -1 || anchor >= N || e1 < e0 || e0 < 0;
  if (!bad) bad = ex_slice_bad(A.ex, e0, e1, N, tid, 256);
  if (__syncthreads_or(bad)) {      // a rejected row: an empty list, counted once
    if (s == 0 && tid == 0) atomicAdd(A.bad, 1);
    if (w == 0) list_emit<FILTER_K_MAX>(A, A.part_s != nullptr, r, s, neg_inf(), PAD_ID, 0);
    return;
  }
  const bool radius = anchor >= 0 && A.c_r < __builtin_huge_val();
  const bool has = GEO && anchor >= 0;
  double lat1 = 0.0, lon1 = 0.0, c1 = 0.0;
  if (radius || has) { lat1 = A.coords[2 * (size_t)anchor]; lon1 = A.coords[2 * (size_t)anchor + 1]; c1 = A.cphi[anchor]; }
  if (tid == 0) {
    s_band[0] = radius ? lat_bound<false>(A.coords, A.order, N, lat1 - A.band_deg) : 0;
    s_band[1] = radius ? lat_bound<true>(A.coords, A.order, N, lat1 + A.band_deg) : N;
  }
  __syncthreads();
  const unsigned* const bw = A.bits + (size_t)q * A.ldw;
  const float wd = GEO ? A.wd[0] : 0.f;
  float4 af[D8];
  load_frag<D8>(af, A.users, 0, (size_t)r, D, lane >> 5);
  float cs = neg_inf();
  int ci = PAD_ID;                  // the wave's best 64 so far, sorted over its lanes
  int q_id = PAD_ID, qn = 0, count = 0;

  // the lanes with `hit` offer candidate `id`: the exclusion list, then queue lane qn + t takes the hit of rank t; a full queue is scored
  auto offer = [&](bool hit, int id) {
    if (hit && e1 > e0) hit = !listed(A.ex, e0, e1, id);
    const unsigned long long bal = __ballot(hit);
    const int n_hit = __popcll(bal);
    count += n_hit;
    int t = lane - qn;
    bool take = t >= 0 && t < n_hit;
    int gi = __shfl(id, take ? nth_bit(bal, t) : 0, 64);
    if (take) q_id = gi;
    if (qn + n_hit >= 64) {
      gather_score<D8, GEO>(A, r, af, wd, has, lat1, lon1, c1, q_id, 64, cs, ci);
      t = lane + 64 - qn;           // the hits the full queue had no room for open the next one
      take = t < n_hit;
      gi = __shfl(id, take ? nth_bit(bal, t) : 0, 64);
      q_id = take ? gi : PAD_ID;
      qn += n_hit - 64;
    } else {
      qn += n_hit;
    }
  };

  if (radius) {
    const int b0 = s_band[0];
    const long long L = s_band[1] - b0;
    const int lo = b0 + (int)(L * s / S), hi = b0 + (int)(L * (s + 1) / S);
    for (int p0 = lo + w * 64; p0 < hi; p0 += 256) {
      const int p = p0 + lane;
      int id = -1;
      bool hit = p < hi;
      if (hit) { id = A.order[p]; hit = (unsigned)id < (unsigned)N; }
      if (hit) {
        const double c = haversine_c(lat1, lon1, c1, A.coords[2 * (size_t)id], A.coords[2 * (size_t)id + 1], A.cphi[id]);
        hit = (c < A.c_r || id == anchor) && ((bw[id >> 5] >> (id & 31)) & 1u);
      }
      offer(hit, id);
    }
  } else {
    const int W = (N + 31) >> 5;
    const int lo = (int)((long long)W * s / S), hi = (int)((long long)W * (s + 1) / S);
    const unsigned tmask = tail_mask(N);
    for (int v0 = lo + w * 64; v0 < hi; v0 += 256) {
      const int wi = v0 + lane;
      unsigned m = wi < hi ? bw[wi] : 0u;
      if (wi == W - 1) m &= tmask;
      while (__ballot(m != 0u)) {   // every lane offers its lowest remaining bit
        const bool hit = m != 0u;
        const int id = hit ? wi * 32 + __ffs((int)m) - 1 : -1;
        m &= m - 1u;
        offer(hit, id);
      }
    }
  }
  if (qn > 0) gather_score<D8, GEO>(A, r, af, wd, has, lat1, lon1, c1, q_id, __builtin_amdgcn_readfirstlane(qn), cs, ci);
  if (lane < FILTER_K_MAX) { m_s[w][lane] = cs; m_i[w][lane] = ci; }
  if (lane == 0) m_cnt[w] = count;
  __syncthreads();
  if (w == 0) {
    float as;
    int ai;
    block_lists_fold<FILTER_K_MAX>(&m_s[0][0], &m_i[0][0], FILTER_K_MAX, as, ai);
    list_emit<FILTER_K_MAX>(A, A.part_s != nullptr, r, s, as, ai, (m_cnt[0] + m_cnt[1]) + (m_cnt[2] + m_cnt[3]));
  }
}

hipError_t launch_filter_build(const FilterBuildArgs& A, hipStream_t st, Timing* tm) {
  Timing::Scope rec(tm, "filter_build", st);
  if (A.count) {
    const hipError_t e = hipMemsetAsync(A.count, 0, sizeof(int) * (size_t)A.n_pred, st);
    if (e != hipSuccess) return e;
  }
  const long long rounds = (A.ldw * 32 + POI_BLOCK - 1) / POI_BLOCK;
  hipLaunchKernelGGL(filter_build_kernel, dim3((unsigned)(rounds < 4096 ? rounds : 4096), (unsigned)A.n_pred), dim3(POI_BLOCK), 0, st, A);
  return rec.close();
}

hipError_t launch_filter_scores(const FilterScoresArgs& A, hipStream_t st, Timing* tm) {
  tm->begin("topk_filtered_scores", st);
  hipLaunchKernelGGL(filter_scores_kernel, dim3((unsigned)A.n), dim3(256), 0, st, A);
  tm->end(st);
  return hipGetLastError();
}

template <bool GEO>
static hipError_t launch_walk_g(const FilterArgs& A, hipStream_t st) {
  return by_dim<64>(A.dim, [&](auto d8, auto db) -> hipError_t {
    constexpr auto kernel = &filter_walk_kernel<decltype(d8)::value, decltype(db)::value, GEO>;
    const hipError_t oe = lds_opt_in<kernel>(WALK_LISTS_BYTES + (int)sizeof(double) * FILTER_NDIST_MAX);
    if (oe != hipSuccess) return oe;
    const unsigned n_utile = (unsigned)((A.n + 31) / 32);
    const size_t lds = WALK_LISTS_BYTES + (GEO ? sizeof(double) * A.n_dist : 0);
    hipLaunchKernelGGL(kernel, dim3(n_utile * (unsigned)A.n_split), dim3(POI_BLOCK), lds, st, A);
    return hipGetLastError();
  });
}

hipError_t launch_filter_walk(FilterArgs& A, hipStream_t st, Timing* tm) {
  if (A.wd && A.n_dist > FILTER_NDIST_MAX) return hipErrorInvalidValue;
  Timing::Scope rec(tm, "score_topk_filtered", st);
  const hipError_t e = A.wd ? launch_walk_g<true>(A, st) : launch_walk_g<false>(A, st);
  if (e != hipSuccess) return e;
  if (A.part_s) launch_topk_slices_merge(slice_lists(A), FILTER_K_MAX, A.n, st);
  return rec.close();
}

template <bool GEO>
static hipError_t launch_gather_g(const FilterArgs& A, hipStream_t st) {
  return by_dim<64>(A.dim, [&](auto d8, auto) -> hipError_t {
    hipLaunchKernelGGL((filter_gather_kernel<decltype(d8)::value, GEO>), dim3((unsigned)A.n * (unsigned)A.n_split), dim3(256), 0, st, A);
    return hipGetLastError();
  });
}

hipError_t launch_filter_gather(FilterArgs& A, hipStream_t st, Timing* tm) {
  Timing::Scope rec(tm, "score_topk_filtered", st);
  const hipError_t e = A.wd ? launch_gather_g<true>(A, st) : launch_gather_g<false>(A, st);
  if (e != hipSuccess) return e;
  if (A.part_s) launch_topk_slices_merge(slice_lists(A), FILTER_K_MAX, A.n, st);
  return rec.close();
}

}  // namespace poi
