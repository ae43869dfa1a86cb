// Label recommendation (poi_score_labels, poi_score_topk_labels, poi_labels_scores): which category / district comes next, and how
// likely - per row and label the softmax MASS of the label's POIs, the label's best POI and the number of its candidates, without the
// (n, n_item) score matrix.
//
//   labels     (n_item) int32: labels[j] in [0, n_label) names POI j's label; anything else is unlabelled and goes to bucket n_label
//   C(r)       every POI minus the row's exclusion list (CSR, ascending); a NaN or -inf score is no candidate
//   s(r, j)    poi_score_rank's s(r, j): tile_product (tile_product.h) plus the distance term through geo_prob at the row's anchor
//              (none while the anchor is < 0), one zero
//   M(r)       max of s(r, j) over ALL j with a non-NaN score - the exclusion list does not move it
//   q(r, j)    round_to_nearest_uint64(exp(double(s) - double(M)) 2^36), <= 2^36
//   mass_q     sum of q over the label's candidates (uint64: n_item < 2^27 keeps it below 2^63)
//   best       the label's candidate that wins under better(); count: the label's candidates
// Three accumulators per (row, bucket), all of them order-free: a 64-bit integer add, a 64-bit max on the packed key
// (f2ord(score) << 32) | (0xFFFFFFFF - id), a 32-bit add.  Whatever the grid, the regime, the accumulator's home or the chunking of
// the rows, the bits are the same.  No float atomics.
//
// labels_walk_kernel<.., MODE>: the item-stationary tile walk in tile_walk.h's steps (wave_tile_range: a workgroup owns a 32-row tile
// and an item slice, its waves a quarter of the slice each; load_row_tile / load_item_tile, labels[j] fetched with the tile; the
// distance term through geo_add), no bitmap, and exclusion cursors in the kernel's own text (lane r walks row r's list, a tile with
// listed ids gets one mask per row through LDS - BEFORE the product: tile_walk.h's contract came from this kernel).
//   MODE 0   the max pass: M(r) alone - per-lane running maxima, one butterfly and one integer atomicMax per row and wave
//   MODE 1   accumulators of the workgroup's 32 rows in LDS (few labels: 32 (n_label + 1) 20 bytes), flushed once with global atomics
//   MODE 2   atomics straight on the context's global accumulator (many labels)
// labels_scores_kernel: the same definition on explicit float32 score rows, one workgroup per row (M, then the accumulators).
// labels_finish_kernel: one workgroup per row turns the accumulators into the dense outputs, log p and the top k labels (k rounds of
// a block-wide arg-max under "higher key, then lower label id": by mass the key is mass_q, by max the packed best key).
#include "poi_common.h"
#include "poi_kernels.h"
#include "launch_common.h"
#include "tile_walk.h"
#include <limits.h>

namespace poi {

namespace {

typedef unsigned long long u64;

__device__ __forceinline__ bool finite_f(float x) { return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u; }
__device__ __forceinline__ u64 mass_term(float s, double M) { return __double2ull_rn(exp((double)s - M) * (double)(1ull << LABELS_Q_BITS)); }
__device__ __forceinline__ u64 best_key(float s, int j) { return ((u64)f2ord(s) << 32) | (u64)(0xFFFFFFFFu - (unsigned)j); }
__device__ __forceinline__ int bucket_of(int lab, int L) { return (unsigned)lab < (unsigned)L ? lab : L; }
__device__ __forceinline__ float key_max(unsigned mk) { return mk ? ord2f(mk) : neg_inf(); }

// one candidate into the accumulators at `at` (LDS or global: the same three integer atomics)
__device__ __forceinline__ void acc_add(u64* mass, u64* best, unsigned* cnt, size_t at, u64 q, u64 key) {
  if (q) atomicAdd(mass + at, q);
  atomicMax(best + at, key);
  atomicAdd(cnt + at, 1u);
}

// LDS accumulators [0, cells) -> the global ones at `base`: cells that saw a candidate only
__device__ __forceinline__ void acc_flush(const LabelsAcc& G, const u64* l_mass, const u64* l_best, const unsigned* l_cnt, int cells, size_t base,
                                          int tid, int nthr) {
  for (int e = tid; e < cells; e += nthr) {
    const unsigned c = l_cnt[e];
    if (c) {
      if (l_mass[e]) atomicAdd(G.mass + base + e, l_mass[e]);
      atomicMax(G.best + base + e, l_best[e]);
      atomicAdd(G.cnt + base + e, c);
    }
  }
}

}  // namespace

size_t labels_lds_bytes(int rows, int n_label) { return (size_t)rows * ((size_t)n_label + 1) * LABELS_ROW_BYTES; }

// ---- the walk: MODE 0 max pass, 1 accumulate in LDS, 2 accumulate in global memory ------------------------------------------------------
template <int D8, bool DB, bool GEO, int MODE>
__global__ __launch_bounds__(POI_BLOCK) void labels_walk_kernel(LabelsArgs A) {
  __shared__ int s_e0[32], s_e1[32], s_ok[32], s_has[32];               // per tile row: exclusion list, accumulated at all, has an anchor
  __shared__ double s_ulat[32], s_ulon[32], s_ucp[32], s_M[32];
  __shared__ unsigned s_exm[POI_NWAVE][32];                              // the rows' masks of listed ids in the tile a wave is at
  extern __shared__ __align__(16) unsigned char s_dyn[];                // MODE 1: mass | best | cnt (32 (n_label + 1) cells); GEO: thr[n_dist]
  const int L1 = A.n_label + 1, cells = 32 * L1;
  u64* const l_mass = reinterpret_cast<u64*>(s_dyn);
  u64* const l_best = l_mass + cells;
  unsigned* const l_cnt = reinterpret_cast<unsigned*>(l_best + cells);
  double* const s_thr = reinterpret_cast<double*>(s_dyn + (MODE == 1 ? (size_t)cells * LABELS_ROW_BYTES : 0));
  const int tid = threadIdx.x, lane = lane_id(), w = wave_id(), li = lane & 31, h = lane >> 5;
  const int S = A.n_split, ut = blockIdx.x / S, sl = blockIdx.x - ut * S;
  const int N = A.n_item;

  // the tile's rows: anchor in range, exclusion lists with offsets in order and ids ascending inside [0, N); M(r) finite
  for (int i = w; i < 32; i += POI_NWAVE) {
    const int r = ut * 32 + i;
    int bad = 0, e0 = 0, e1 = 0;
    if (MODE != 0 && r < A.n) {
      const int an = A.last_poi ? A.last_poi[r] : -1;
      bad = an < -1 || an >= N;
      if (A.ex) bad |= check_ex_row(A.ex_off, A.ex, r, N, lane, e0, e1);
    }
    bad = __any(bad) ? 1 : 0;
    if (lane == 0) {
      float M = 0.f;
      if (MODE != 0 && r < A.n) M = key_max(A.acc.mkey[r]);
      const int ok = r < A.n && !bad && finite_f(M);
      s_ok[i] = ok; s_e0[i] = ok ? e0 : 0; s_e1[i] = ok ? e1 : 0; s_M[i] = (double)M;
      if (bad && sl == 0) { atomicAdd(A.bad, 1); A.acc.status[r] = 1; }
      if (GEO) load_row_geo(A, r < A.n ? r : -1, N, s_has[i], s_ulat[i], s_ulon[i], s_ucp[i]);
    }
  }
  if (GEO)
    for (int i = tid; i < A.n_dist; i += POI_BLOCK) s_thr[i] = A.thr[i];
  if (MODE == 1)
    for (int e = tid; e < cells; e += POI_BLOCK) { l_mass[e] = 0ull; l_best[e] = 0ull; l_cnt[e] = 0u; }
  __syncthreads();

  int ntile, tb, te;
  wave_tile_range(N, sl, S, w, ntile, tb, te);
  const float wd = GEO ? A.wd[0] : 0.f;

  if (tb < te) {                                    // (wave-uniform)
    // lane r < 32: cursor into row r's exclusion list, at the first id of this wave's item range
    int xpos = 0, xend = 0, xnext = INT_MAX;
    if (MODE != 0 && A.ex && lane < 32 && s_ok[lane] && s_e1[lane] > s_e0[lane]) {
      int a = s_e0[lane], b = s_e1[lane];
      const int first = tb * 32;
      while (a < b) { const int md = (a + b) >> 1; if (A.ex[md] < first) a = md + 1; else b = md; }
      xpos = a; xend = s_e1[lane];
      if (xpos < xend) xnext = A.ex[xpos];
    }
    bool exdirty = false;
    if (lane < 32) s_exm[w][lane] = 0u;
    wave_fence();

    float mx[MODE == 0 ? 16 : 1];
#pragma unroll
    for (int r = 0; r < (MODE == 0 ? 16 : 1); ++r) mx[r] = neg_inf();

    float4 af[D8];
    load_row_tile<D8>(af, A, ut, li, h);
    float4 b0[D8], b1[DB ? D8 : 1];
    load_item_tile<D8>(b0, A, tb, li, h);
    for (int tile = tb; tile < te; ++tile) {
      if constexpr (DB) { if (tile + 1 < te) load_item_tile<D8>(b1, A, tile + 1, li, h); }
      const int j = tile * 32 + li;
      const bool jvalid = j < N;
      const int lab = MODE != 0 ? A.labels[min(j, N - 1)] : 0;      // lane li: the label of its item column, fetched with the tile
      if (MODE != 0) {
        // listed ids of this tile -> one 32-bit mask per row
        const bool anyex = __any(xnext < tile * 32 + 32);
        if (anyex || exdirty) {                     // (wave-uniform; a tile without listed ids after one with some clears the masks)
          unsigned mask = 0u;
          while (xnext < tile * 32 + 32) {
            const unsigned o = (unsigned)(xnext - tile * 32);
            if (o < 32u) mask |= 1u << o;
            ++xpos;
            xnext = xpos < xend ? A.ex[xpos] : INT_MAX;
          }
          if (lane < 32) s_exm[w][lane] = mask;
          wave_fence();
          exdirty = anyex;
        }
      }
      double jlat, jlon, jcp;
      item_tile_coords<GEO>(A, j, jlat, jlon, jcp);
      const int bk = bucket_of(lab, A.n_label);
      f32x16 acc = tile_product<D8>(af, b0);       // (tile_walk.h: the walk's contract)
      const int hb = opaque_half_base(h);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int ul = acc_tile_row(r, hb);
        float s = acc[r];
        if (GEO) {
          if (s_has[ul]) s = geo_add(A, wd, s_thr, ut, ul, s_ulat, s_ulon, s_ucp, jlat, jlon, jcp, s);
        }
        s = one_zero(s);
        if constexpr (MODE == 0) {
          mx[r] = (jvalid && s > mx[r]) ? s : mx[r];                          // (a NaN compares false: it never becomes the maximum)
        } else {
          const bool live = jvalid && s_ok[ul] && !((s_exm[w][ul] >> li) & 1u) && selectable(s);
          if (live) {
            const u64 q = mass_term(s, s_M[ul]), key = best_key(s, j);
            if constexpr (MODE == 1) acc_add(l_mass, l_best, l_cnt, (size_t)(ul * L1 + bk), q, key);
            else acc_add(A.acc.mass, A.acc.best, A.acc.cnt, (size_t)(ut * 32 + ul) * L1 + bk, q, key);
          }
        }
        __builtin_amdgcn_sched_barrier(0);          // one row's distance term / exponential in flight at a time
      }
      if (MODE != 0) wave_fence();                  // the masks are read before the next tile overwrites them
      if constexpr (DB) {
        if (tile + 1 < te) {
#pragma unroll
          for (int m = 0; m < D8; ++m) b0[m] = b1[m];
        }
      } else {
        if (tile + 1 < te) load_item_tile<D8>(b0, A, tile + 1, li, h);
      }
    }

    if constexpr (MODE == 0) {
      // one butterfly per row over the 32 lanes of the half wave, one integer atomic each
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = ut * 32 + acc_tile_row(r, 4 * h);
        float v = mx[r];
#pragma unroll
        for (int o = 16; o > 0; o >>= 1) { const float u = __shfl_xor(v, o, 64); v = u > v ? u : v; }
        if (li == 0 && row < A.n) atomicMax(A.acc.mkey + row, f2ord(v));
      }
    }
  }

  if constexpr (MODE == 1) {
    __syncthreads();
    acc_flush(A.acc, l_mass, l_best, l_cnt, cells, (size_t)ut * 32 * L1, tid, POI_BLOCK);
  }
}

// ---- poi_labels_scores: one workgroup per explicit score row ------------------------------------------------------------------------------
template <bool LDSH>
__global__ __launch_bounds__(256) void labels_scores_kernel(LabelsScoresArgs A) {
  __shared__ float s_red[POI_NWAVE];
  extern __shared__ __align__(16) unsigned char s_dyn[];                // LDSH: mass | best | cnt (n_label + 1 cells)
  const int L1 = A.n_label + 1;
  u64* const l_mass = reinterpret_cast<u64*>(s_dyn);
  u64* const l_best = l_mass + L1;
  unsigned* const l_cnt = reinterpret_cast<unsigned*>(l_best + L1);
  const int tid = threadIdx.x, lane = lane_id(), w = wave_id();
  const int r = blockIdx.x, N = A.n_item;
  const int e0 = A.ex ? A.ex_off[r] : 0, e1 = A.ex ? A.ex_off[r + 1] : 0;
  int bad = e1 < e0 || e0 < 0;
  if (!bad) bad = ex_slice_bad(A.ex, e0, e1, N, tid, 256);
  if (__syncthreads_or(bad)) {      // a rejected row: nothing accumulated, counted once
    if (tid == 0) { atomicAdd(A.bad, 1); A.acc.status[r] = 1; }
    return;
  }
  const float* const sr = A.scores + (size_t)r * A.ld;
  float m = neg_inf();
  for (int p = tid; p < N; p += 256) { const float s = one_zero(sr[p]); m = s > m ? s : m; }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { const float u = __shfl_xor(m, o, 64); m = u > m ? u : m; }
  if (lane == 0) s_red[w] = m;
  if (LDSH)
    for (int e = tid; e < L1; e += 256) { l_mass[e] = 0ull; l_best[e] = 0ull; l_cnt[e] = 0u; }
  __syncthreads();
  m = s_red[0];
#pragma unroll
  for (int i = 1; i < POI_NWAVE; ++i) m = s_red[i] > m ? s_red[i] : m;
  if (tid == 0) A.acc.mkey[r] = f2ord(m);
  if (!finite_f(m)) return;                         // (uniform) an empty, all-NaN or +inf row
  const double M = (double)m;
  const size_t base = (size_t)r * L1;
  for (int p = tid; p < N; p += 256) {
    const float s = one_zero(sr[p]);
    if (!selectable(s) || (e1 > e0 && listed(A.ex, e0, e1, p))) continue;
    const int bk = bucket_of(A.labels[p], A.n_label);
    const u64 q = mass_term(s, M), key = best_key(s, p);
    if (LDSH) acc_add(l_mass, l_best, l_cnt, (size_t)bk, q, key);
    else acc_add(A.acc.mass, A.acc.best, A.acc.cnt, base + bk, q, key);
  }
  if (LDSH) {
    __syncthreads();
    acc_flush(A.acc, l_mass, l_best, l_cnt, L1, base, tid, 256);
  }
}

// ---- the finish: accumulators -> dense outputs, log p, the top k labels -------------------------------------------------------------------
__device__ __forceinline__ double log_share(u64 mass, u64 total) {
  return mass ? log((double)mass) - log((double)total) : (double)neg_inf();
}

__global__ __launch_bounds__(256) void labels_finish_kernel(LabelsFinishArgs A) {
  __shared__ u64 s_total;
  __shared__ u64 s_p[POI_NWAVE];
  __shared__ int s_l[POI_NWAVE];
  const int tid = threadIdx.x, lane = lane_id(), w = wave_id();
  const int r = blockIdx.x, L = A.n_label, L1 = L + 1, k = A.k;
  const size_t base = (size_t)r * L1;
  const u64* const mass = A.acc.mass + base;
  const u64* const best = A.acc.best + base;
  const unsigned* const cnt = A.acc.cnt + base;
  const bool rejected = A.acc.status[r] != 0;
  const float M = rejected ? neg_inf() : key_max(A.acc.mkey[r]);
  if (tid == 0) s_total = 0ull;
  __syncthreads();
  u64 mine = 0ull;
  for (int l = tid; l < L1; l += 256) {
    const u64 ms = mass[l], key = best[l];
    mine += ms;
    if (A.mass_out) A.mass_out[base + l] = ms;
    if (A.best_id_out) A.best_id_out[base + l] = key ? (int)(0xFFFFFFFFu - (unsigned)(key & 0xFFFFFFFFull)) : -1;
    if (A.best_score_out) A.best_score_out[base + l] = key ? ord2f((unsigned)(key >> 32)) : neg_inf();
    if (A.count_out) A.count_out[base + l] = (int)cnt[l];
  }
  if (mine) atomicAdd(&s_total, mine);              // (an integer sum: any order)
  __syncthreads();
  const u64 total = s_total;
  if (tid == 0) {
    if (A.m_out) A.m_out[r] = M;
    if (A.lognorm_out) A.lognorm_out[r] = total ? (double)M + log((double)total * (1.0 / (double)(1ull << LABELS_Q_BITS))) : (double)neg_inf();
    if (A.rest_logp_out) A.rest_logp_out[r] = log_share(mass[L], total);
  }
  if (k <= 0) return;
  // k rounds: the best label under (higher key, then lower id) that comes after the one listed last
  const bool by_max = A.by == LABELS_BY_MAX;
  u64 lastp = ~0ull;
  int lastl = -1, listed_n = 0;
  for (int t = 0; t < k; ++t) {
    u64 bp = 0ull;
    int bl = -1;
    if (lastl != INT_MAX) {
      for (int l = tid; l < L; l += 256) {
        if (!cnt[l]) continue;
        const u64 pv = by_max ? best[l] : mass[l];
        const bool after = pv < lastp || (pv == lastp && l > lastl);
        if (after && (bl < 0 || pv > bp || (pv == bp && l < bl))) { bp = pv; bl = l; }
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const unsigned lo = __shfl_xor((unsigned)bp, o, 64), hi = __shfl_xor((unsigned)(bp >> 32), o, 64);
        const u64 op = ((u64)hi << 32) | lo;
        const int ol = __shfl_xor(bl, o, 64);
        if (ol >= 0 && (bl < 0 || op > bp || (op == bp && ol < bl))) { bp = op; bl = ol; }
      }
    }
    __syncthreads();                                // (the round before has been read)
    if (lane == 0) { s_p[w] = bp; s_l[w] = bl; }
    __syncthreads();
    bp = s_p[0]; bl = s_l[0];
#pragma unroll
    for (int i = 1; i < POI_NWAVE; ++i)
      if (s_l[i] >= 0 && (bl < 0 || s_p[i] > bp || (s_p[i] == bp && s_l[i] < bl))) { bp = s_p[i]; bl = s_l[i]; }
    if (bl >= 0) { lastp = bp; lastl = bl; ++listed_n; } else lastl = INT_MAX;      // nothing left: the rest of the list is fill
    if (tid == 0) {
      const size_t at = (size_t)r * k + t;
      const u64 key = bl >= 0 ? best[bl] : 0ull;
      A.label_out[at] = bl;
      if (A.logp_out) A.logp_out[at] = bl >= 0 ? log_share(mass[bl], total) : (double)neg_inf();
      if (A.top_id_out) A.top_id_out[at] = key ? (int)(0xFFFFFFFFu - (unsigned)(key & 0xFFFFFFFFull)) : -1;
      if (A.top_score_out) A.top_score_out[at] = key ? ord2f((unsigned)(key >> 32)) : neg_inf();
    }
  }
  if (tid == 0 && A.n_listed_out) A.n_listed_out[r] = listed_n;
}

// ---- launches ----------------------------------------------------------------------------------------------------------------------------
template <bool GEO, int MODE>
static hipError_t launch_walk_g(const LabelsArgs& A, hipStream_t st) {
  return by_dim<64>(A.dim, [&](auto d8, auto db) -> hipError_t {
    constexpr auto kernel = &labels_walk_kernel<decltype(d8)::value, decltype(db)::value, GEO, MODE>;
    const hipError_t oe = lds_opt_in<kernel>((MODE == 1 ? LABELS_LDS_KB_MAX << 10 : 0) + (int)sizeof(double) * LABELS_NDIST_MAX);
    if (oe != hipSuccess) return oe;
    const unsigned n_utile = (unsigned)((A.n + 31) / 32);
    const size_t lds = (MODE == 1 ? labels_lds_bytes(32, A.n_label) : 0) + (GEO ? sizeof(double) * A.n_dist : 0);
    hipLaunchKernelGGL(kernel, dim3(n_utile * (unsigned)A.n_split), dim3(POI_BLOCK), lds, st, A);
    return hipGetLastError();
  });
}

hipError_t launch_labels_max(const LabelsArgs& A, hipStream_t st, Timing* tm) {
  if (A.wd && A.n_dist > LABELS_NDIST_MAX) return hipErrorInvalidValue;
  tm->begin("labels_max", st);
  const hipError_t e = A.wd ? launch_walk_g<true, 0>(A, st) : launch_walk_g<false, 0>(A, st);
  tm->end(st);
  return e;
}

hipError_t launch_labels_walk(const LabelsArgs& A, hipStream_t st, Timing* tm) {
  if (A.wd && A.n_dist > LABELS_NDIST_MAX) return hipErrorInvalidValue;
  if (A.lds_home && labels_lds_bytes(32, A.n_label) > ((size_t)LABELS_LDS_KB_MAX << 10)) return hipErrorInvalidValue;
  tm->begin("labels_walk", st);
  hipError_t e;
  if (A.lds_home) e = A.wd ? launch_walk_g<true, 1>(A, st) : launch_walk_g<false, 1>(A, st);
  else e = A.wd ? launch_walk_g<true, 2>(A, st) : launch_walk_g<false, 2>(A, st);
  tm->end(st);
  return e;
}

hipError_t launch_labels_scores(const LabelsScoresArgs& A, hipStream_t st, Timing* tm) {
  if (A.lds_home && labels_lds_bytes(1, A.n_label) > ((size_t)LABELS_LDS_KB_MAX << 10)) return hipErrorInvalidValue;
  Timing::Scope rec(tm, "labels_scores", st);
  if (A.lds_home) {
    const hipError_t oe = lds_opt_in<&labels_scores_kernel<true>>(LABELS_LDS_KB_MAX << 10);
    if (oe != hipSuccess) return oe;
    hipLaunchKernelGGL(labels_scores_kernel<true>, dim3((unsigned)A.n), dim3(256), labels_lds_bytes(1, A.n_label), st, A);
  } else {
    hipLaunchKernelGGL(labels_scores_kernel<false>, dim3((unsigned)A.n), dim3(256), 0, st, A);
  }
  return rec.close();
}

hipError_t launch_labels_finish(const LabelsFinishArgs& A, hipStream_t st, Timing* tm) {
  tm->begin("labels_finish", st);
  hipLaunchKernelGGL(labels_finish_kernel, dim3((unsigned)A.n), dim3(256), 0, st, A);
  tm->end(st);
  return hipGetLastError();
}

}  // namespace poi
