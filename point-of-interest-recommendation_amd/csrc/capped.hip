// Capped recommendation (poi_labels_build, poi_score_topk_capped, poi_topk_capped_scores): the top-K with at most `per` POIs of one
// label - "the best 20 places, but no more than 2 of a category" - without the (n, n_item) score matrix and without a candidate pool
// of a fixed depth.
//
//   labels     (n_item) int32: labels[j] >= 0 names POI j's group, < 0 = unlabelled: a group of its own, never capped
//   C(r)       filter.hip's candidate set without a radius: bit j of bits[pred[r]] (bits null: every POI) minus the row's exclusion list
//   s(r, j)    poi_score_rank's s(r, j): tile_product (tile_product.h) plus the distance term through geo_prob, one zero
//   result     walk the selectable members of C(r) by better(); take j unless `per` entries taken carry its label; stop at k.
//              Equivalently: j is kept iff fewer than `per` selectable candidates of its label precede it - the form the merges use.
//
// Every list here is CAP-VALID (no label more than `per` times), sorted, and made of real candidates only.  Two facts carry the kernels
// (DESIGN.md section 30 has the argument and the counter-example of the shortcut that does not work):
//   streaming  capped_take: a candidate with `per` better same-label entries is rejected; otherwise it is inserted at its rank and the
//              worst entry of its label leaves if the label now holds per + 1, else the list's last entry.
//   merging    capped_merge: two lists are sorted as one, an entry stays iff fewer than `per` same-label entries precede it, the kept
//              are compacted and cut to 32.  The cap is re-applied after EVERY pairwise merge: a plain best-64 of several lists
//              followed by one cap lets a strong label crowd the others out.
// The gate: a candidate is offered only if it beats entry g - 1 of its row's list, g = min(k, fill[pred[r]][per]) - under a cap the
// list may never reach k entries, and entry k - 1 would stay a pad that everything beats.  The entries behind g are never emitted.
// With the gate a list is EXACT ONLY IN ITS FIRST g ENTRIES: behind them it may be stale - a better candidate that failed the gate
// was never inserted, and an entry there may have same-label candidates in front of it that the list never saw.  Every position of
// a list only improves, so what fails the gate once could never have reached the first g.  Merging the full 32-entry lists and
// emitting g entries is still right: the answer has at most g entries; each of them is among the first g of the capped list of
// its own subset, hence present, and kept, because a count inside a union of real candidates never exceeds the true count; and a
// stale or foreign entry of the union that stands in front of the answer's last entry has `per` better candidates of its label,
// which belong to the answer, are present and push it out.  What survives behind the answer is never emitted.
//
// labels_hist_kernel / labels_fill_kernel: per predicate the histogram of the passing POIs' labels (integer atomics) and from it
// fill[q][m] = #(unlabelled passing POIs) + sum over labels of min(m, #passing POIs of the label), m = 0 .. 32.
//
// capped_walk_kernel: the item-stationary tile walk in tile_walk.h's steps (wave_tile_range: a workgroup owns a 32-row tile and an item
// slice, its waves a quarter of the slice each; load_row_tile / load_item_tile; the distance term through geo_add; the rare part row
// by row through rare_row / acc_row) with filter.hip's bitmap pipeline (one word per row and tile fetched two tiles ahead, zero-word
// tiles skipped) and lists of 32 entries that carry the label beside score and id.  capped_slices_merge_kernel folds the slices' lists of the split regime in
// slice order.  capped_scores_kernel applies the definition to explicit float32 score rows, one workgroup per row.
//
// No float atomics; the same bits on every grid, in both regimes, a row alone or among thousands.
#include "poi_common.h"
#include "poi_kernels.h"
#include "launch_common.h"
#include "tile_walk.h"
#include "topk_list.h"

namespace poi {

namespace {

constexpr int CAP_LIST = CAPPED_K_MAX;                                        // list stride: entries 0 .. 31 on the lanes 0 .. 31
constexpr int CAP_LISTS_BYTES = POI_NWAVE * 32 * CAP_LIST * 12;               // the waves' per-row lists: scores, ids, labels

// entries a row's list is exact to: min(k, fill[q][per]); q out of range (a bad row) or fill null: k
__device__ __forceinline__ int row_gate(const int* fill, int q, int n_rows, int per, int k) {
  if (!fill || (unsigned)q >= (unsigned)n_rows) return k;
  const int f = fill[(size_t)q * CAPPED_FILL_LD + per];
  return f < 0 ? 0 : (f < k ? f : k);
}

// The wave's list: entry l on lane l < 32 (the lanes behind hold pads and never change), sorted, cap-valid.  The lanes of `bal` offer
// (v, j, lab), one at a time in lane order.  gi: the gate entry - a candidate that does not beat it is skipped.
__device__ __forceinline__ void capped_take(float& cs, int& ci, int& cl, unsigned long long bal, float v, int j, int lab, int per, int gi) {
  const int lane = lane_id();
  while (bal) {
    const int src = __ffsll((long long)bal) - 1;
    bal &= bal - 1;
    const float nv = readlane_f(v, src);
    const int nj = __builtin_amdgcn_readlane(j, src);
    const int nl = __builtin_amdgcn_readlane(lab, src);
    const unsigned long long mb = __ballot(better(cs, ci, nv, nj));          // the entries in front of the newcomer: a prefix
    const int pos = __popcll(mb);
    if (pos > gi) continue;                                                   // (the gate entry has moved up since the offer)
    const unsigned long long ms = nl >= 0 ? __ballot(ci != PAD_ID && cl == nl) : 0ull;
    if (__popcll(ms & mb) >= per) continue;                                   // `per` better entries of its label
    // who leaves: the label's worst entry if the label is full (it is behind the newcomer), else the last entry
    const int out = __popcll(ms) >= per ? 63 - __clzll((long long)ms) : CAP_LIST - 1;
    const float us = __shfl_up(cs, 1, 64);
    const int ui = __shfl_up(ci, 1, 64);
    const int ul = __shfl_up(cl, 1, 64);
    if (lane == pos) { cs = nv; ci = nj; cl = nl; }
    else if (lane > pos && lane <= out) { cs = us; ci = ui; cl = ul; }
  }
}

// Lanes 0 .. 31 and lanes 32 .. 63 hold one cap-valid list each (any order) -> their capped merge on the lanes 0 .. 31, pads behind;
// cl returns the labels.  The labels come from the table: the sort moves scores and ids only.
__device__ __forceinline__ void capped_merge(float& cs, int& ci, int& cl, const int* labels, int per) {
  const int lane = lane_id();
  float s = cs;
  int i = ci;
  wave_sort_desc(s, i);
  const int lab = i == PAD_ID ? -1 : labels[i];
  int before = 0;                                                             // same-label entries in front of this one
#pragma unroll
  for (int t = 0; t < 63; ++t) before += (t < lane && __builtin_amdgcn_readlane(lab, t) == lab) ? 1 : 0;
  const bool keep = i != PAD_ID && (lab < 0 || before < per);
  const unsigned long long m = __ballot(keep);
  const int nk = __popcll(m);
  const bool live = lane < nk && lane < CAP_LIST;
  const int src = live ? nth_bit(m, lane) : 0;
  const float ns = __shfl(s, src, 64);
  const int ni = __shfl(i, src, 64);
  const int nl = __shfl(lab, src, 64);
  cs = live ? ns : neg_inf(); ci = live ? ni : PAD_ID; cl = live ? nl : -1;
}

// wave 0 (or the only wave): lane l < 32 holds entry l of the row's list; g: the entries it is exact to
template <class Args>
__device__ __forceinline__ void capped_emit(const Args& A, int r, float sc, int id, int lab, int g, int cnt) {
  const int lane = lane_id();
  if (lane < A.k) {
    const bool there = lane < g && id != PAD_ID;
    A.idx_out[(size_t)r * A.k + lane] = there ? id : -1;
    if (A.score_out) A.score_out[(size_t)r * A.k + lane] = there ? sc : neg_inf();
    if (A.label_out) A.label_out[(size_t)r * A.k + lane] = there ? lab : -1;
  }
  if (lane == 0 && A.count_out) A.count_out[r] = cnt;
}

}  // namespace

// ---- poi_labels_build -----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(POI_BLOCK) void labels_hist_kernel(LabelsBuildArgs A) {
  const int q = blockIdx.y, lane = lane_id();
  const unsigned* const bw = A.bits ? A.bits + (size_t)q * A.ldw : nullptr;
  int* const hist = A.hist + (size_t)q * A.n_label;
  int unl = 0, nbad = 0;
  for (long long j0 = (long long)blockIdx.x * POI_BLOCK + (threadIdx.x - lane); j0 < A.n_item; j0 += (long long)gridDim.x * POI_BLOCK) {
    const long long j = j0 + lane;
    bool pass = false, stray = false;
    int lab = -1;
    if (j < A.n_item) {
      lab = A.labels[j];
      stray = lab >= A.n_label;
      pass = !bw || ((bw[j >> 5] >> (j & 31)) & 1u);
      if (q == 0 && A.count && lab >= 0 && !stray) atomicAdd(A.count + lab, 1);
    }
    if (pass && lab >= 0 && !stray) atomicAdd(hist + lab, 1);
    unl += __popcll(__ballot(pass && (lab < 0 || stray)));                    // a stray label counts as unlabelled: fill stays an upper bound
    nbad += __popcll(__ballot(stray));
  }
  if (lane == 0) {
    if (unl) atomicAdd(A.unl + q, unl);
    if (q == 0 && nbad && A.bad) atomicAdd(A.bad, nbad);                      // a POI is counted once, whatever the number of predicates (and of chunks: the first has the counter)
  }
}

// one workgroup per predicate: ge[i] = #labels with at least i passing POIs (i capped at 32), fill[m] = unl + ge[1] + .. + ge[m]
__global__ __launch_bounds__(POI_BLOCK) void labels_fill_kernel(LabelsBuildArgs A) {
  __shared__ int s_at[CAPPED_PER_MAX + 1];
  const int q = blockIdx.x, tid = threadIdx.x;
  const int* const hist = A.hist + (size_t)q * A.n_label;
  if (tid <= CAPPED_PER_MAX) s_at[tid] = 0;
  __syncthreads();
  for (int l = tid; l < A.n_label; l += POI_BLOCK) {
    const int hcnt = hist[l];
    if (hcnt > 0) atomicAdd(&s_at[hcnt < CAPPED_PER_MAX ? hcnt : CAPPED_PER_MAX], 1);
  }
  __syncthreads();
  if (tid == 0) {
    int* const out = A.fill + (size_t)q * CAPPED_FILL_LD;
    int ge[CAPPED_PER_MAX + 2];
    ge[CAPPED_PER_MAX + 1] = 0;
    for (int i = CAPPED_PER_MAX; i >= 1; --i) ge[i] = ge[i + 1] + s_at[i];
    int f = A.unl[q];
    out[0] = f;
    for (int m = 1; m <= CAPPED_PER_MAX; ++m) { f += ge[m]; out[m] = f; }
  }
}

// ---- poi_topk_capped_scores -----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void capped_scores_kernel(CappedScoresArgs A) {
  __shared__ float m_s[POI_NWAVE][CAP_LIST];
  __shared__ int m_i[POI_NWAVE][CAP_LIST];
  __shared__ int m_cnt[POI_NWAVE];
  const int tid = threadIdx.x, lane = lane_id(), w = wave_id();
  const int r = blockIdx.x, N = A.n_item, per = A.per;
  const int q = (A.bits && A.pred) ? A.pred[r] : 0;
  const int e0 = A.ex ? A.ex_off[r] : 0, e1 = A.ex ? A.ex_off[r + 1] : 0;
  int bad = (unsigned)q >= (unsigned)A.n_pred || e1 < e0 || e0 < 0;
  if (!bad) bad = ex_slice_bad(A.ex, e0, e1, N, tid, 256);
  if (__syncthreads_or(bad)) {      // a rejected row: an empty list, counted once
    if (tid == 0) atomicAdd(A.bad, 1);
    if (w == 0) capped_emit(A, r, neg_inf(), PAD_ID, -1, 0, 0);
    return;
  }
  const int g = row_gate(A.fill, q, A.n_pred, per, A.k), gi = (g > 0 ? g : 1) - 1;
  const unsigned* const bw = A.bits ? A.bits + (size_t)q * A.ldw : nullptr;
  const float* const sr = A.scores + (size_t)r * A.ld;
  float cs = neg_inf();
  int ci = PAD_ID, cl = -1, count = 0;      // the wave's capped list so far
  for (int p0 = w * 64; p0 < N; p0 += 256) {
    const int p = p0 + lane;
    bool hit = p < N && (!bw || ((bw[p >> 5] >> (p & 31)) & 1u));
    if (hit && e1 > e0) hit = !listed(A.ex, e0, e1, p);
    count += __popcll(__ballot(hit));
    const float s = hit ? one_zero(sr[p]) : neg_inf();
    const bool sel = hit && selectable(s);
    const float ts = __shfl(cs, gi, 64);
    const int ti = __shfl(ci, gi, 64);
    const bool cand = sel && better(s, p, ts, ti);
    const unsigned long long bal = __ballot(cand);
    if (bal) capped_take(cs, ci, cl, bal, s, p, cand ? A.labels[p] : -1, per, gi);
  }
  if (lane < CAP_LIST) { m_s[w][lane] = cs; m_i[w][lane] = ci; }
  if (lane == 0) m_cnt[w] = count;
  __syncthreads();
  if (w == 0) {
    for (int ww = 1; ww < POI_NWAVE; ++ww) {
      if (lane >= 32) { cs = m_s[ww][lane - 32]; ci = m_i[ww][lane - 32]; }
      capped_merge(cs, ci, cl, A.labels, per);
    }
    capped_emit(A, r, cs, ci, cl, g, (m_cnt[0] + m_cnt[1]) + (m_cnt[2] + m_cnt[3]));
  }
}

// ---- poi_score_topk_capped ------------------------------------------------------------------------------------------------------------
template <int D8, bool DB, bool GEO>
__global__ __launch_bounds__(POI_BLOCK) void capped_walk_kernel(CappedArgs A) {
  __shared__ int s_e0[32], s_e1[32], s_ok[32], s_has[32], s_g[32];      // per tile row: exclusion list, ranked at all, has an anchor, gate
  __shared__ long long s_pb[32];                                         // ... and where its predicate's words start
  __shared__ double s_ulat[32], s_ulon[32], s_ucp[32];
  __shared__ unsigned s_word[POI_NWAVE][32];                             // the rows' words of the tile a wave is at
  __shared__ int s_cnt[POI_NWAVE][32];
  extern __shared__ __align__(16) unsigned char s_dyn[];                // lists (CAP_LISTS_BYTES) | GEO: thr[n_dist]
  float* const l_s = reinterpret_cast<float*>(s_dyn);
  int* const l_i = reinterpret_cast<int*>(s_dyn + CAP_LISTS_BYTES / 3);
  int* const l_l = reinterpret_cast<int*>(s_dyn + 2 * (CAP_LISTS_BYTES / 3));
  double* const s_thr = reinterpret_cast<double*>(s_dyn + CAP_LISTS_BYTES);
  const int tid = threadIdx.x, lane = lane_id(), w = wave_id(), li = lane & 31, h = lane >> 5;
  const int S = A.n_split, ut = blockIdx.x / S, sl = blockIdx.x - ut * S;
  const int N = A.n_item, per = A.per;

  // the tile's rows: predicate index and anchor in range, exclusion lists with offsets in order and ids ascending inside [0, N)
  for (int i = w; i < 32; i += POI_NWAVE) {
    const int r = ut * 32 + i;
    int bad = 0, e0 = 0, e1 = 0, q = 0;
    if (r < A.n) {
      q = (A.bits && A.pred) ? A.pred[r] : 0;
      const int an = A.last_poi ? A.last_poi[r] : -1;
      bad = (unsigned)q >= (unsigned)A.n_pred || an < -1 || an >= N;
      if (A.ex) bad |= check_ex_row(A.ex_off, A.ex, r, N, lane, e0, e1);
    }
    bad = __any(bad) ? 1 : 0;
    if (lane == 0) {
      const int ok = r < A.n && !bad;
      s_ok[i] = ok; s_e0[i] = ok ? e0 : 0; s_e1[i] = ok ? e1 : 0; s_pb[i] = ok ? (long long)q * A.ldw : 0;
      s_g[i] = ok ? row_gate(A.fill, q, A.n_pred, per, A.k) : 0;
      if (bad && sl == 0) atomicAdd(A.bad, 1);
      if (GEO) load_row_geo(A, ok ? r : -1, N, s_has[i], s_ulat[i], s_ulon[i], s_ucp[i]);
    }
  }
  if (GEO)
    for (int i = tid; i < A.n_dist; i += POI_BLOCK) s_thr[i] = A.thr[i];
  for (int e = tid; e < POI_NWAVE * 32 * CAP_LIST; e += POI_BLOCK) { l_s[e] = neg_inf(); l_i[e] = PAD_ID; l_l[e] = -1; }
  __syncthreads();

  int ntile, tb, te;
  wave_tile_range(N, sl, S, w, ntile, tb, te);
  const float wd = GEO ? A.wd[0] : 0.f;
  float* const ls = l_s + w * 32 * CAP_LIST;
  int* const lx = l_i + w * 32 * CAP_LIST;
  int* const ll = l_l + w * 32 * CAP_LIST;

  // row li's word of tile t (both lane halves hold it); a row that is not ranked has none, the table's last word loses its tail;
  // without a bitmap every word is all ones and nothing is loaded
  const bool rowlive = s_ok[li] != 0;
  const unsigned* const wp = A.bits ? A.bits + s_pb[li] : nullptr;
  const unsigned tmask = tail_mask(N);
  auto word = [&](int t) -> unsigned {
    if (t >= te || !rowlive) return 0u;
    const unsigned v = wp ? wp[t] : ~0u;
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
      const int j = tile * 32 + li;
      const int lab = A.labels[min(j, N - 1)];      // lane li: the label of its item column, fetched with the tile
      __builtin_amdgcn_wave_barrier();
      s_word[w][li] = w0;
      __builtin_amdgcn_wave_barrier();              // (a wave's LDS accesses complete in order: the reads below see it)
      f32x16 acc = tile_product<D8>(af, b0);       // (tile_walk.h: the walk's contract)
      double jlat, jlon, jcp;
      item_tile_coords<GEO>(A, j, jlat, jlon, jcp);
      const int hb = opaque_half_base(h);
      unsigned cm = 0u;                             // bit r: acc[r] passes and beats the gate entry of its row's list
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
        const int gv = s_g[ul], ge = ul * CAP_LIST + (gv > 0 ? gv : 1) - 1;
        if (bit && selectable(s) && better(s, j, ls[ge], lx[ge])) cm |= 1u << r;
        if (GEO) __builtin_amdgcn_sched_barrier(0); // one row's distance term in flight at a time
      }
      if (__ballot(cm != 0u)) {
        // the rare part: row by row, the exclusion lookup and the cap-aware insertions
        for (int row = 0; row < 32; ++row) {
          int rr;
          bool cand = rare_row(row, h, cm, rr);
          if (!__ballot(cand)) continue;            // (wave-uniform)
          const float v = acc_row(acc, rr);
          const int e0 = s_e0[row], e1 = s_e1[row];
          if (cand && e1 > e0) cand = !listed(A.ex, e0, e1, j);
          const unsigned long long bal = __ballot(cand);
          if (bal) {
            const int gv = s_g[row];
            __builtin_amdgcn_wave_barrier();
            float cs = lane < CAP_LIST ? ls[row * CAP_LIST + lane] : neg_inf();
            int ci = lane < CAP_LIST ? lx[row * CAP_LIST + lane] : PAD_ID;
            int cl = lane < CAP_LIST ? ll[row * CAP_LIST + lane] : -1;
            capped_take(cs, ci, cl, bal, v, j, lab, per, (gv > 0 ? gv : 1) - 1);
            __builtin_amdgcn_wave_barrier();
            if (lane < CAP_LIST) { ls[row * CAP_LIST + lane] = cs; lx[row * CAP_LIST + lane] = ci; ll[row * CAP_LIST + lane] = cl; }
            __builtin_amdgcn_wave_barrier();
          }
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
  // the four waves' lists of a row meet, pairwise, the cap re-applied after each merge: wave w folds rows w, w + 4, ...
  for (int i = w; i < 32; i += POI_NWAVE) {
    const int row = ut * 32 + i;
    if (row >= A.n) break;
    float cs = l_s[(h * 32 + i) * CAP_LIST + li];
    int ci = l_i[(h * 32 + i) * CAP_LIST + li], cl = -1;
    capped_merge(cs, ci, cl, A.labels, per);
    for (int ww = 2; ww < POI_NWAVE; ++ww) {
      if (h) { cs = l_s[(ww * 32 + i) * CAP_LIST + li]; ci = l_i[(ww * 32 + i) * CAP_LIST + li]; }
      capped_merge(cs, ci, cl, A.labels, per);
    }
    int cnt = 0;
    if (s_ok[i]) {
      cnt = (s_cnt[0][i] + s_cnt[1][i]) + (s_cnt[2][i] + s_cnt[3][i]);
      if (sl == 0) {                                // the listed ids that pass leave the count (the list is ascending: each id once)
        const unsigned* const rw = A.bits ? A.bits + s_pb[i] : nullptr;
        int x = 0;
        for (int p = s_e0[i] + lane; p < s_e1[i]; p += 64) { const int id = A.ex[p]; x += rw ? (rw[id >> 5] >> (id & 31)) & 1u : 1u; }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
        cnt -= x;
      }
    }
    if (A.part_s) {
      const size_t at = (size_t)row * S + sl;
      if (lane < CAP_LIST) { A.part_s[at * CAP_LIST + lane] = cs; A.part_i[at * CAP_LIST + lane] = ci; }
      if (lane == 0) A.part_cnt[at] = cnt;
    } else {
      capped_emit(A, row, cs, ci, cl, s_g[i], cnt);
    }
  }
}

// the split regime's second kernel: one wave per row folds the slices' lists in slice order, pairwise, and sums the counts
__global__ __launch_bounds__(64) void capped_slices_merge_kernel(CappedArgs A) {
  const int r = blockIdx.x, lane = lane_id(), S = A.n_split, li = lane & 31, h = lane >> 5;
  const size_t base = (size_t)r * S;
  float cs = neg_inf();
  int ci = PAD_ID, cl = -1, cnt = 0;
  if (h == 0) { cs = A.part_s[base * CAP_LIST + li]; ci = A.part_i[base * CAP_LIST + li]; }
  else if (S > 1) { cs = A.part_s[(base + 1) * CAP_LIST + li]; ci = A.part_i[(base + 1) * CAP_LIST + li]; }
  capped_merge(cs, ci, cl, A.labels, A.per);
  for (int s = 2; s < S; ++s) {
    if (h) { cs = A.part_s[(base + s) * CAP_LIST + li]; ci = A.part_i[(base + s) * CAP_LIST + li]; }
    capped_merge(cs, ci, cl, A.labels, A.per);
  }
  for (int s = lane; s < S; s += 64) cnt += A.part_cnt[base + s];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
  const int q = (A.bits && A.pred) ? A.pred[r] : 0;
  capped_emit(A, r, cs, ci, cl, row_gate(A.fill, q, A.n_pred, A.per, A.k), cnt);
}

hipError_t launch_labels_build(const LabelsBuildArgs& A, hipStream_t st, Timing* tm) {
  Timing::Scope rec(tm, "labels_build", st);
  const int rows = A.n_pred > 0 ? A.n_pred : 1;
  hipError_t e = hipMemsetAsync(A.hist, 0, sizeof(int) * ((size_t)rows * A.n_label + rows), st);      // (unl lies right behind hist)
  if (e != hipSuccess) return e;
  if (A.count && (e = hipMemsetAsync(A.count, 0, sizeof(int) * (size_t)A.n_label, st)) != hipSuccess) return e;
  const long long rounds = ((long long)A.n_item + POI_BLOCK - 1) / POI_BLOCK;
  hipLaunchKernelGGL(labels_hist_kernel, dim3((unsigned)(rounds < 1024 ? rounds : 1024), (unsigned)rows), dim3(POI_BLOCK), 0, st, A);
  hipLaunchKernelGGL(labels_fill_kernel, dim3((unsigned)rows), dim3(POI_BLOCK), 0, st, A);
  return rec.close();
}

hipError_t launch_capped_scores(const CappedScoresArgs& A, hipStream_t st, Timing* tm) {
  tm->begin("topk_capped_scores", st);
  hipLaunchKernelGGL(capped_scores_kernel, dim3((unsigned)A.n), dim3(256), 0, st, A);
  tm->end(st);
  return hipGetLastError();
}

template <bool GEO>
static hipError_t launch_walk_g(const CappedArgs& A, hipStream_t st) {
  return by_dim<64>(A.dim, [&](auto d8, auto db) -> hipError_t {
    constexpr auto kernel = &capped_walk_kernel<decltype(d8)::value, decltype(db)::value, GEO>;
    const hipError_t oe = lds_opt_in<kernel>(CAP_LISTS_BYTES + (int)sizeof(double) * CAPPED_NDIST_MAX);
    if (oe != hipSuccess) return oe;
    const unsigned n_utile = (unsigned)((A.n + 31) / 32);
    const size_t lds = CAP_LISTS_BYTES + (GEO ? sizeof(double) * A.n_dist : 0);
    hipLaunchKernelGGL(kernel, dim3(n_utile * (unsigned)A.n_split), dim3(POI_BLOCK), lds, st, A);
    return hipGetLastError();
  });
}

hipError_t launch_capped_walk(const CappedArgs& A, hipStream_t st, Timing* tm) {
  if (A.wd && A.n_dist > CAPPED_NDIST_MAX) return hipErrorInvalidValue;
  const long span = tm->span_begin("score_topk_capped", st);      // the call; inside it the walk and (split regime) the merge on their own
  tm->begin("capped_walk", st);
  const hipError_t e = A.wd ? launch_walk_g<true>(A, st) : launch_walk_g<false>(A, st);
  tm->end(st);
  if (e != hipSuccess) { tm->span_end(span, st); return e; }
  if (A.part_s) {
    tm->begin("capped_merge", st);
    hipLaunchKernelGGL(capped_slices_merge_kernel, dim3((unsigned)A.n), dim3(64), 0, st, A);
    tm->end(st);
  }
  tm->span_end(span, st);
  return hipGetLastError();
}

}  // namespace poi
