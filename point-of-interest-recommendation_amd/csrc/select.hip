// Candidate generation (poi_score_rows, poi_topk_select, poi_score_candidates): the exact top-K of every row for K up to 4096 - the
// hand-over of a retrieval stage to a downstream ranker.  The sorted per-lane lists of the other ranking kernels (topk_list.h) end at
// 64 entries; this is selection, not sorted insertion.
//
//   C(r)        = [0, n_item) minus the exclusion list of row r (the conventions of poi_score_rank)
//   selectable  = an entry of C(r) whose score is neither NaN nor -inf (+inf is selectable, as in poi_score_topk)
//   result      = the best K' = min(k, |selectable|) entries under better() (descending score, ascending id), sorted best first,
//                 -1 ids and -inf scores behind; -0.0 and +0.0 are the SAME score (the id decides) and come out as +0.0
//
// score_rows_kernel: the item-stationary tile walk in tile_walk.h's steps (wave_tile_chunk, load_row_tile / load_item_tile, geo_add) with
// a store epilogue - a wave owns a 32-row tile and a range of 32-item tiles, the
// accumulator register of a row holds 32 consecutive items and goes to scores_out[r * ld + j] as it is.  The same tile_product and the
// same distance-term expression as rank.hip: a pair's score has the bits of poi_score_rank's score_out.
//
// The selection reads explicit float32 score rows.  key = the order-preserving uint32 image of the score with -0.0 folded onto +0.0;
// 0 (below every valid key) stands for NaN / -inf and is never counted.  Exclusions are looked up only for entries that would count.
// The histogram and collect kernels read a row through walk_keys: float4 loads behind an alignment peel, every id exactly once.
//   select_prep_kernel     one wave per row: the exclusion list is checked (rank.hip's rule), the row's state is reset, count_out written
//   select_hist_kernel<P>  three digit passes of 11 / 11 / 10 bits.  A workgroup owns (row, slice of the id range) and counts the keys
//                          whose higher digits equal the prefix found so far into 2048 LDS bins (8 KB), then adds its nonzero bins to
//                          the row's bins in global memory: INTEGER atomic adds only, so the sums do not depend on the grid
//   select_scan_kernel<P>  one wave per row walks the bins from the top, fixes the digit that holds the K'-th entry and the count above
//                          it, and clears the bins for the next pass.  After the last pass: the exact K'-th key T, G = |{key > T}|, and
//                          whether every entry with key == T is taken
//   select_collect_kernel  every entry with key > T (key >= T when all ties are taken) gets a slot from an integer counter - their order
//                          is irrelevant, a total-order sort follows
//   select_ties_kernel     only where the cut falls INSIDE a tie group: one workgroup per row walks the ids in ascending order with an
//                          ordered compaction (ballot + prefix) and takes exactly the K' - G lowest ids with key == T; it stops as soon
//                          as it has them (a plateau row ends after ceil(K' / 256) steps)
//   select_sort_kernel     one workgroup per row (a thread per pair of a step, up to 1024): bitonic network in LDS over
//                          (key << 32 | ~id), descending - better()'s order, total because ids are unique - then ids, scores and the
//                          -1 / -inf fill
// The selected SET is fixed by integer counts, the order by a total order: identical bits on every grid, for every slice count and
// chunking, for a row alone or in a call of thousands.  No float atomics, vector stores only.
#include "poi_common.h"
#include "poi_kernels.h"
#include "launch_common.h"
#include "tile_walk.h"

namespace poi {

namespace {

constexpr int SELECT_UNROLL = 2;              // float4 loads per lane in flight in the histogram / collect walks
constexpr int SELECT_SORT_BLOCK = 1024;      // threads of the sort's workgroup at k > 1024
constexpr int ST_BAD = 0, ST_PREFIX = 1, ST_KLEFT = 2, ST_KP = 3, ST_SLOT = 4, ST_TIEALL = 5, ST_E0 = 6, ST_E1 = 7;

// 0 for a score that is never selected (NaN, -inf); otherwise f2ord of the score with -0.0 folded onto +0.0 (>= 0x00800000)
__device__ __forceinline__ unsigned sel_key(float s) {
  unsigned u = __float_as_uint(s);
  if ((u & 0x7fffffffu) > 0x7f800000u || u == 0xff800000u) return 0u;
  if ((u << 1) == 0u) u = 0u;
  return f2ord(__uint_as_float(u));
}

// [e0, e1) narrowed to the ids of [lo, hi)
__device__ __forceinline__ void narrow_list(const int* ex, int& e0, int& e1, int lo, int hi) {
  int a = e0, b = e1;
  while (a < b) { const int md = (a + b) >> 1; if (ex[md] < lo) a = md + 1; else b = md; }
  const int first = a;
  b = e1;
  while (a < b) { const int md = (a + b) >> 1; if (ex[md] < hi) a = md + 1; else b = md; }
  e0 = first; e1 = a;
}

// One workgroup visits every id j of [lo, hi) of the score row sr once: f(j, key of sr[j]).  Every thread calls f the same number of
// times (f holds wave-wide votes); a call that stands for no id gets the key 0, which nothing counts.  Up to three ids in front until
// the address is 16-byte aligned, then float4 loads (two per lane in flight: dword loads reach a third of the HBM rate), then the rest.
template <class F>
__device__ __forceinline__ void walk_keys(const float* __restrict__ sr, int lo, int hi, int tid, F&& f) {
  const int mis = (int)((reinterpret_cast<size_t>(sr + lo) >> 2) & 3);
  const int head = min(hi, lo + ((4 - mis) & 3));
  { const int j = lo + tid; f(j, j < head ? sel_key(sr[j]) : 0u); }
  const int nv = (hi - head) >> 2;                  // whole float4 groups
  const float* body = sr + head;
  for (int g0 = 0; g0 < nv; g0 += SELECT_UNROLL * POI_BLOCK) {
    float4 v[SELECT_UNROLL];
#pragma unroll
    for (int u = 0; u < SELECT_UNROLL; ++u) {
      const int g = g0 + u * POI_BLOCK + tid;
      v[u] = g < nv ? ld4(body + 4 * (size_t)g) : make_float4(neg_inf(), neg_inf(), neg_inf(), neg_inf());      // (-inf: key 0)
    }
#pragma unroll
    for (int u = 0; u < SELECT_UNROLL; ++u) {
      const int j = head + 4 * (g0 + u * POI_BLOCK + tid);
      f(j, sel_key(v[u].x)); f(j + 1, sel_key(v[u].y)); f(j + 2, sel_key(v[u].z)); f(j + 3, sel_key(v[u].w));
    }
  }
  { const int j = head + 4 * nv + tid; f(j, j < hi ? sel_key(sr[j]) : 0u); }
}

}  // namespace

template <int D8, bool DB, bool GEO>
__global__ __launch_bounds__(POI_BLOCK) void score_rows_kernel(ScoreRowsArgs A) {
  __shared__ int s_has[32];
  __shared__ double s_ulat[32], s_ulon[32], s_ucp[32];
  extern __shared__ __align__(16) double s_thr[];   // GEO: thr[n_dist]
  const int lane = lane_id(), w = wave_id(), li = lane & 31, h = lane >> 5;
  const int N = A.n_item, ut = blockIdx.x;
  const int split = blockIdx.y * POI_NWAVE + w;
  int t_begin, t_end;
  wave_tile_chunk(N, A.n_split, split, t_begin, t_end);
  if (GEO) {
    for (int i = threadIdx.x; i < A.n_dist; i += POI_BLOCK) s_thr[i] = A.thr[i];
    if (threadIdx.x < 32) {
      const int r = ut * 32 + (int)threadIdx.x;
      load_row_geo(A, r < A.n ? r : -1, N, s_has[threadIdx.x], s_ulat[threadIdx.x], s_ulon[threadIdx.x], s_ucp[threadIdx.x]);
    }
  }
  __syncthreads();
  if (t_begin >= t_end) return;
  const float wd = GEO ? A.wd[0] : 0.f;

  float4 af[D8];
  load_row_tile<D8>(af, A, ut, li, h);
  float4 b0[D8], b1[DB ? D8 : 1];
  load_item_tile<D8>(b0, A, t_begin, li, h);
  for (int tile = t_begin; tile < t_end; ++tile) {
    if constexpr (DB) { if (tile + 1 < t_end) load_item_tile<D8>(b1, A, tile + 1, li, h); }
    const f32x16 acc = tile_product<D8>(af, b0);   // (tile_walk.h: the walk's contract)
    const int j = tile * 32 + li;
    double jlat, jlon, jcp;
    item_tile_coords<GEO>(A, j, jlat, jlon, jcp);
    const int hb = opaque_half_base(h);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int ul = acc_tile_row(r, hb), row = ut * 32 + ul;
      float s = acc[r];
      if (GEO) {
        if (s_has[ul]) s = geo_add(A, wd, s_thr, ut, ul, s_ulat, s_ulon, s_ucp, jlat, jlon, jcp, s);
      }
      if (row < A.n && j < N) A.out[(size_t)row * (size_t)A.ld + j] = s;      // 32 consecutive floats per row: one 128-byte segment
      if (GEO) __builtin_amdgcn_sched_barrier(0);   // one row's distance term in flight at a time
    }
    if constexpr (DB) {
#pragma unroll
      for (int m = 0; m < D8; ++m) b0[m] = b1[m];
    } else {
      if (tile + 1 < t_end) load_item_tile<D8>(b0, A, tile + 1, li, h);
    }
  }
}

__global__ __launch_bounds__(64) void select_prep_kernel(SelectArgs A) {
  const int row = blockIdx.x, lane = lane_id();
  int e0 = 0, e1 = 0, bad = 0;
  if (A.ex) bad = check_ex_row(A.ex_off, A.ex, row, A.n_item, lane, e0, e1);
  bad = __any(bad) ? 1 : 0;
  if (bad) { e0 = 0; e1 = 0; }
  int* stt = A.state + (size_t)row * SELECT_STATE_INTS;
  if (lane < SELECT_STATE_INTS) stt[lane] = lane == ST_BAD ? bad : lane == ST_E0 ? e0 : lane == ST_E1 ? e1 : 0;
  if (lane == 0) {
    if (bad) atomicAdd(A.bad, 1);
    if (A.count_out) A.count_out[row] = bad ? 0 : A.n_item - (e1 - e0);
  }
}

template <int PASS>
__global__ __launch_bounds__(POI_BLOCK) void select_hist_kernel(SelectArgs A) {
  constexpr int SHIFT = PASS == 0 ? 21 : PASS == 1 ? 10 : 0;
  constexpr int NB = PASS == 2 ? 1024 : 2048;
  constexpr unsigned HIMASK = PASS == 0 ? 0u : PASS == 1 ? 0xFFE00000u : 0xFFFFFC00u;
  __shared__ int s_h[NB];
  const int tid = threadIdx.x, lane = lane_id();
  const int S = A.n_split, row = blockIdx.x / S, sl = blockIdx.x - row * S, N = A.n_item;
  const int* stt = A.state + (size_t)row * SELECT_STATE_INTS;
  if (stt[ST_BAD] || (PASS > 0 && stt[ST_KP] == 0)) return;      // (workgroup-uniform)
  const unsigned prefix = (unsigned)stt[ST_PREFIX];
  int e0 = stt[ST_E0], e1 = stt[ST_E1];
  const int lo = (int)((long long)N * sl / S), hi = (int)((long long)N * (sl + 1) / S);
  if (lo >= hi) return;
  for (int b = tid; b < NB; b += POI_BLOCK) s_h[b] = 0;
  if (e1 > e0) narrow_list(A.ex, e0, e1, lo, hi);
  __syncthreads();
  const float* sr = A.scores + (size_t)row * (size_t)A.ld;
  walk_keys(sr, lo, hi, tid, [&](int j, unsigned key) {
    bool act = key != 0u && (key & HIMASK) == prefix;
    if (act && e1 > e0) act = !listed(A.ex, e0, e1, j);
    const int digit = (int)((key >> SHIFT) & (unsigned)(NB - 1));
    const unsigned long long bal = __ballot(act);
    if (bal) {                                      // (wave-uniform)  a wave whose counted keys share one digit - a plateau, the later passes - adds once
      const int first = __ffsll((long long)bal) - 1;
      const int d0 = __shfl(digit, first, 64);
      if (__all(!act || digit == d0)) { if (lane == first) atomicAdd(&s_h[d0], __popcll(bal)); }
      else if (act) atomicAdd(&s_h[digit], 1);
    }
  });
  __syncthreads();
  int* hb = A.hist + (size_t)row * SELECT_BINS;
  for (int b = tid; b < NB; b += POI_BLOCK) { const int v = s_h[b]; if (v) atomicAdd(&hb[b], v); }
}

template <int PASS>
__global__ __launch_bounds__(64) void select_scan_kernel(SelectArgs A) {
  constexpr int SHIFT = PASS == 0 ? 21 : PASS == 1 ? 10 : 0;
  constexpr int NB = PASS == 2 ? 1024 : 2048;
  constexpr int PER = NB / 64;                      // lane l owns the bins l PER .. l PER + PER - 1: lane 63 the top ones
  const int row = blockIdx.x, lane = lane_id();
  int* stt = A.state + (size_t)row * SELECT_STATE_INTS;
  if (stt[ST_BAD] || (PASS > 0 && stt[ST_KP] == 0)) return;
  const unsigned prefix = (unsigned)stt[ST_PREFIX];
  int* hb = A.hist + (size_t)row * SELECT_BINS + lane * PER;
  int v[PER], sum = 0;
#pragma unroll
  for (int i = 0; i < PER; ++i) { v[i] = hb[i]; hb[i] = 0; sum += v[i]; }
  int incl = sum;                                   // inclusive suffix sum over the lanes
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) { const int t = __shfl_down(incl, o, 64); if (lane + o < 64) incl += t; }
  const int above = incl - sum, total = __shfl(incl, 0, 64);
  const int kleft = PASS == 0 ? min(A.k, total) : stt[ST_KLEFT];
  if (PASS == 0 && lane == 0) stt[ST_KP] = kleft;
  if (kleft <= 0) return;
  if (above < kleft && kleft <= above + sum) {      // the one lane whose bins hold the K'-th entry
    int acc = above, d = -1, left = 0, at = 0;
#pragma unroll
    for (int i = PER - 1; i >= 0; --i) {
      if (d < 0 && acc + v[i] >= kleft) { d = lane * PER + i; left = kleft - acc; at = v[i]; }
      acc += v[i];
    }
    stt[ST_PREFIX] = (int)(prefix | ((unsigned)d << SHIFT));
    stt[ST_KLEFT] = left;                           // after the last pass: the entries with key == T that are taken
    if (PASS == 2) stt[ST_TIEALL] = left == at ? 1 : 0;
  }
}

__global__ __launch_bounds__(POI_BLOCK) void select_collect_kernel(SelectArgs A) {
  const int tid = threadIdx.x, lane = lane_id();
  const int S = A.n_split, row = blockIdx.x / S, sl = blockIdx.x - row * S, N = A.n_item;
  int* stt = A.state + (size_t)row * SELECT_STATE_INTS;
  if (stt[ST_BAD] || stt[ST_KP] == 0) return;
  const unsigned T = (unsigned)stt[ST_PREFIX];
  const unsigned floor_key = stt[ST_TIEALL] ? T : T + 1u;       // (T + 1 == 0 only for a NaN pattern, which has no key)
  int e0 = stt[ST_E0], e1 = stt[ST_E1];
  const int lo = (int)((long long)N * sl / S), hi = (int)((long long)N * (sl + 1) / S);
  if (lo >= hi || floor_key == 0u) return;
  if (e1 > e0) narrow_list(A.ex, e0, e1, lo, hi);
  const float* sr = A.scores + (size_t)row * (size_t)A.ld;
  unsigned long long* cand = A.cand + (size_t)row * A.k;
  walk_keys(sr, lo, hi, tid, [&](int j, unsigned key) {
    bool take = key >= floor_key;                   // (floor_key >= 1: the key 0 of NaN / -inf / no id is never taken)
    if (take && e1 > e0) take = !listed(A.ex, e0, e1, j);
    const unsigned long long bal = __ballot(take);
    if (bal) {
      const int first = __ffsll((long long)bal) - 1;
      int slot0 = 0;
      if (lane == first) slot0 = atomicAdd(&stt[ST_SLOT], __popcll(bal));
      slot0 = __shfl(slot0, first, 64);
      const int slot = slot0 + __popcll(bal & ((1ull << lane) - 1ull));
      if (take && slot < A.k) cand[slot] = ((unsigned long long)key << 32) | (unsigned)~j;
    }
  });
}

__global__ __launch_bounds__(POI_BLOCK) void select_ties_kernel(SelectArgs A) {
  __shared__ int s_cnt[POI_NWAVE];
  const int tid = threadIdx.x, lane = lane_id(), w = wave_id();
  const int row = blockIdx.x, N = A.n_item;
  const int* stt = A.state + (size_t)row * SELECT_STATE_INTS;
  if (stt[ST_BAD] || stt[ST_KP] == 0 || stt[ST_TIEALL]) return;
  const unsigned T = (unsigned)stt[ST_PREFIX];
  const int want = stt[ST_KLEFT], G = stt[ST_KP] - want;
  const int e0 = stt[ST_E0], e1 = stt[ST_E1];
  const float* sr = A.scores + (size_t)row * (size_t)A.ld;
  unsigned long long* cand = A.cand + (size_t)row * A.k;
  int taken = 0;
  for (int base = 0; base < N && taken < want; base += POI_BLOCK) {      // ids in ascending order, 256 at a time
    const int j = base + tid;
    bool is = false;
    if (j < N) {
      is = sel_key(sr[j]) == T;
      if (is && e1 > e0) is = !listed(A.ex, e0, e1, j);
    }
    const unsigned long long bal = __ballot(is);
    if (lane == 0) s_cnt[w] = __popcll(bal);
    __syncthreads();
    int before = 0, all = 0;
#pragma unroll
    for (int i = 0; i < POI_NWAVE; ++i) { const int c = s_cnt[i]; before += i < w ? c : 0; all += c; }
    const int pos = taken + before + __popcll(bal & ((1ull << lane) - 1ull));
    if (is && pos < want) cand[G + pos] = ((unsigned long long)T << 32) | (unsigned)~j;
    taken += all;
    __syncthreads();
  }
}

__global__ __launch_bounds__(SELECT_SORT_BLOCK) void select_sort_kernel(SelectArgs A) {
  extern __shared__ __align__(16) unsigned long long s_k[];      // the next power of two >= k entries
  const int tid = threadIdx.x, row = blockIdx.x, K = A.k;
  const int* stt = A.state + (size_t)row * SELECT_STATE_INTS;
  const int Kp = stt[ST_BAD] ? 0 : min(stt[ST_KP], K);
  int P = 1;
  while (P < Kp) P <<= 1;
  const unsigned long long* cand = A.cand + (size_t)row * K;
  for (int i = tid; i < P; i += (int)blockDim.x) s_k[i] = i < Kp ? cand[i] : 0ull;
  __syncthreads();
  for (int k2 = 2; k2 <= P; k2 <<= 1)
    for (int jj = k2 >> 1; jj > 0; jj >>= 1) {
      for (int t = tid; t < (P >> 1); t += (int)blockDim.x) {
        const int i = ((t & ~(jj - 1)) << 1) | (t & (jj - 1)), x = i | jj;      // the t-th pair of this step
        const unsigned long long a = s_k[i], b = s_k[x];
        const bool desc = (i & k2) == 0;
        if (desc ? a < b : a > b) { s_k[i] = b; s_k[x] = a; }
      }
      __syncthreads();
    }
  for (int i = tid; i < K; i += (int)blockDim.x) {
    const unsigned long long e = i < Kp ? s_k[i] : 0ull;
    A.idx_out[(size_t)row * K + i] = i < Kp ? (int)~(unsigned)e : -1;
    if (A.score_out) A.score_out[(size_t)row * K + i] = i < Kp ? ord2f((unsigned)(e >> 32)) : neg_inf();
  }
}

template <bool GEO>
static hipError_t launch_score_rows_g(const ScoreRowsArgs& A, hipStream_t st) {
  return by_dim<128>(A.dim, [&](auto d8, auto db) -> hipError_t {
    const dim3 grid((A.n + 31) / 32, (A.n_split + POI_NWAVE - 1) / POI_NWAVE);
    hipLaunchKernelGGL((score_rows_kernel<decltype(d8)::value, decltype(db)::value, GEO>), grid, dim3(POI_BLOCK), GEO ? sizeof(double) * A.n_dist : 0, st, A);
    return hipGetLastError();
  });
}

hipError_t launch_score_rows(const ScoreRowsArgs& A, hipStream_t st, Timing* tm) {
  tm->begin("score_rows", st);
  const hipError_t e = A.wd ? launch_score_rows_g<true>(A, st) : launch_score_rows_g<false>(A, st);
  tm->end(st);
  return e;
}

hipError_t launch_select(const SelectArgs& A, hipStream_t st, Timing* tm) {
  const unsigned rows = (unsigned)A.n, cut = (unsigned)A.n * (unsigned)A.n_split;
  hipError_t e = hipMemsetAsync(A.hist, 0, sizeof(int) * (size_t)A.n * SELECT_BINS, st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(select_prep_kernel, dim3(rows), dim3(64), 0, st, A);
  tm->begin("select_pass0", st);
  hipLaunchKernelGGL(select_hist_kernel<0>, dim3(cut), dim3(POI_BLOCK), 0, st, A);
  hipLaunchKernelGGL(select_scan_kernel<0>, dim3(rows), dim3(64), 0, st, A);
  tm->end(st);
  tm->begin("select_pass1", st);
  hipLaunchKernelGGL(select_hist_kernel<1>, dim3(cut), dim3(POI_BLOCK), 0, st, A);
  hipLaunchKernelGGL(select_scan_kernel<1>, dim3(rows), dim3(64), 0, st, A);
  tm->end(st);
  tm->begin("select_pass2", st);
  hipLaunchKernelGGL(select_hist_kernel<2>, dim3(cut), dim3(POI_BLOCK), 0, st, A);
  hipLaunchKernelGGL(select_scan_kernel<2>, dim3(rows), dim3(64), 0, st, A);
  tm->end(st);
  tm->begin("select_collect", st);
  hipLaunchKernelGGL(select_collect_kernel, dim3(cut), dim3(POI_BLOCK), 0, st, A);
  hipLaunchKernelGGL(select_ties_kernel, dim3(rows), dim3(POI_BLOCK), 0, st, A);
  tm->end(st);
  int P = 1;
  while (P < A.k) P <<= 1;
  tm->begin("select_sort", st);
  const int threads = P / 2 < 64 ? 64 : P / 2 > SELECT_SORT_BLOCK ? SELECT_SORT_BLOCK : P / 2;      // a thread per pair of a step, up to 1024
  hipLaunchKernelGGL(select_sort_kernel, dim3(rows), dim3(threads), sizeof(unsigned long long) * (size_t)P, st, A);
  tm->end(st);
  return hipGetLastError();
}

}  // namespace poi
