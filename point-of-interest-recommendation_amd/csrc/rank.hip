// Exact rank of given target POIs among all POIs (poi_score_rank, poi_rank_scores): the number every rank metric beyond a top-K list
// follows from - MRR, mean / median rank, recall at any cut-off, AUC over all negatives - without the (n, n_item) score matrix.
//
//   C(r)        = [0, n_item) minus the exclusion list of row r
//   rank[r][i]  = |{ j in C(r), j != t : s(r, j) > s(r, t) or (s(r, j) == s(r, t) and j < t) }|,  t = tgt[r][i]
// the tie rule of the top-K kernels (better(), poi_common.h): the 0-based position t would have in an endless top-K list.
//
// Pass 1 (rank_targets_kernel, one wave per 32-row tile): the scores of the row's targets.  The B operand of the tile product is the
// gathered item rows of the 32 rows' i-th targets, the row's own score is the diagonal of the 32x32 result: the SAME product routine
// (tile_product, tile_product.h: v_mfma_f32_32x32x2_f32 in one k order) and the same distance-term expression as pass 2, so a POI whose item row equals
// the target's ties bit for bit and the index rule decides.  The pass also validates: a masked position, a target outside [0, n_item)
// (counted), an excluded target and every target of a row with a malformed exclusion list (counted once) get rank -1 and take no part
// in pass 2; the other ranks start at 0.
// Pass 2 (rank_kernel): the tile walk of score_topk.hip - a wave owns a 32-row tile (A fragments in registers, operands straight from
// HBM / L2 to VGPRs, exact float32 products) and a contiguous range of 32-item tiles; the item range is split over the waves of
// gridDim.y workgroups so that a few rows still fill the machine.  The epilogue compares each score of the 32x32 tile with the row's
// targets (score + id in LDS, read as broadcasts) and adds 0 / 1 to per-lane counters, two 16-bit counters per register (a wave walks
// at most 65535 tiles: host-checked).  Exclusion: lane r < 32 walks row r's ascending list with one cursor, a tile that holds listed
// ids gets a 32-bit mask per row through LDS (one ballot decides; the common tile has none).  At the end of the range: a 32-lane
// butterfly per (row, target) and ONE integer atomicAdd into rank_out.  Integer adds only: every grid gives the same counts.
// A walk takes up to four targets per row (five to eight: a second walk over the items) - eight targets' counters beside the operands
// of dim 256 spilled to scratch.
//
// Bytes: per 32-row tile the item table once (4 dim n_item, or 2 dim from a half table), + 24 n_item of coordinates with the distance
// term; flops 2 n n_item dim on the f32 matrix pipe.  No (n, n_item) matrix, no LDS candidate lists, no float atomics.
//
// rank_scores_kernel applies the same definition to explicit score rows (poi_rank_scores: the counterpart of poi_topk).
#include "poi_common.h"
#include "poi_kernels.h"
#include "launch_common.h"
#include "tile_walk.h"
#include <limits.h>

namespace poi {

template <int D8, bool GEO>
__global__ __launch_bounds__(64) void rank_targets_kernel(RankArgs A) {
  __shared__ int s_badrow[32];
  const int lane = lane_id(), li = lane & 31, h = lane >> 5, ut = blockIdx.x;
  const int D = A.dim, N = A.n_item, LT = A.len_t;
  // the tile's exclusion lists: offsets in order, ids ascending and inside [0, N)
  for (int i = 0; i < 32; ++i) {
    const int r = ut * 32 + i;
    int bad = 0;
    if (r < A.n && A.ex) {
      const int e0 = A.ex_off[r], e1 = A.ex_off[r + 1];
      bad = e0 < 0 || e1 < e0;
      if (!bad)
        for (int p = e0 + lane; p < e1; p += 64) { const int v = A.ex[p]; bad |= (unsigned)v >= (unsigned)N || (p > e0 && A.ex[p - 1] >= v); }
    }
    bad = __any(bad) ? 1 : 0;
    if (lane == 0) s_badrow[i] = bad;
  }
  __syncthreads();
  const int row = ut * 32 + li, rowc = min(row, A.n - 1);
  const bool inrow = row < A.n;
  const bool own = h == ((li >> 2) & 1);           // this lane's accumulators hold the diagonal element of row li ...
  const int rsel = (li & 3) + 4 * (li >> 3);       // ... in register rsel
  const int badrow = s_badrow[li];
  int e0 = 0, e1 = 0;
  if (A.ex && !badrow) { e0 = A.ex_off[rowc]; e1 = A.ex_off[rowc + 1]; }
  float4 af[D8];
  load_frag<D8>(af, A.users, 0, (size_t)rowc, D, h);
  const float wd = GEO ? A.wd[0] : 0.f;
  double ulat = 0.0, ulon = 0.0, ucp = 0.0;
  if (GEO) { const int lp = min(max(A.last_poi[rowc], 0), N - 1); ulat = A.coords[2 * (size_t)lp]; ulon = A.coords[2 * (size_t)lp + 1]; ucp = A.cphi[lp]; }
  if (own && inrow) {
    if (badrow) atomicAdd(A.bad, 1);
    if (A.count_out) A.count_out[row] = badrow ? 0 : N - (e1 - e0);
  }
  for (int i = 0; i < RANK_LT_MAX; ++i) {
    RankTgt out; out.s = pos_inf(); out.id = -1;
    if (i < LT) {                                   // (wave-uniform: the matrix instructions run with every lane on)
      const int t = A.tgt[(size_t)rowc * LT + i];
      const bool live = inrow && A.tmask[(size_t)rowc * LT + i] != 0;
      const bool oor = (unsigned)t >= (unsigned)N;
      const int tc = oor ? 0 : t;
      float4 bf[D8];
      load_frag<D8>(bf, A.items, A.items_f16, (size_t)tc, D, h);
      const f32x16 acc = tile_product<D8>(af, bf);
      float sc = acc[0];
#pragma unroll
      for (int r = 1; r < 16; ++r) sc = rsel == r ? acc[r] : sc;
      if (GEO) sc = __fmaf_rn(wd, geo_prob(A, A.thr, rowc, ulat, ulon, ucp, A.coords[2 * (size_t)tc], A.coords[2 * (size_t)tc + 1], A.cphi[tc]), sc);
      const bool ok = live && !oor && !badrow && !listed(A.ex, e0, e1, t);
      if (ok) { out.s = sc; out.id = t; }
      if (own && inrow) {
        if (live && oor) atomicAdd(A.bad, 1);
        A.rank_out[(size_t)row * LT + i] = ok ? 0 : -1;
        if (A.score_out) A.score_out[(size_t)row * LT + i] = ok ? sc : -pos_inf();
      }
    }
    if (own) A.tl[(size_t)row * RANK_LT_MAX + i] = out;      // (every row of the padded tile: pass 2 reads whole tiles)
  }
}

template <int D8, bool DB, bool GEO, int LT>
__global__ __launch_bounds__(POI_BLOCK) void rank_kernel(RankArgs A) {
  constexpr int NP = (LT + 1) / 2;                  // counter registers per row: two 16-bit counters each
  __shared__ RankTgt s_t[32][LT];
  __shared__ unsigned s_exm[POI_NWAVE][32];
  extern __shared__ __align__(16) double s_geo[];   // GEO: thr[n_dist] | row lat[32] | lon[32] | cos(lat)[32]
  const int lane = lane_id(), w = wave_id(), li = lane & 31, h = lane >> 5;
  const int N = A.n_item, ut = blockIdx.x;
  const int split = blockIdx.y * POI_NWAVE + w;
  int t_begin, t_end;
  wave_tile_chunk(N, A.n_split, split, t_begin, t_end);
  for (int e = threadIdx.x; e < 32 * LT; e += POI_BLOCK) s_t[e / LT][e % LT] = A.tl[(size_t)(ut * 32 + e / LT) * RANK_LT_MAX + A.t_off + e % LT];
  double* s_ulat = s_geo + A.n_dist; double* s_ulon = s_ulat + 32; double* s_ucp = s_ulon + 32;
  if (GEO) {
    for (int i = threadIdx.x; i < A.n_dist; i += POI_BLOCK) s_geo[i] = A.thr[i];
    if (threadIdx.x < 32) {
      const int lp = min(max(A.last_poi[min(ut * 32 + (int)threadIdx.x, A.n - 1)], 0), N - 1);      // (an id outside the table reads no memory outside it)
      s_ulat[threadIdx.x] = A.coords[2 * (size_t)lp]; s_ulon[threadIdx.x] = A.coords[2 * (size_t)lp + 1]; s_ucp[threadIdx.x] = A.cphi[lp];
    }
  }
  __syncthreads();
  if (t_begin >= t_end) return;
  const float wd = GEO ? A.wd[0] : 0.f;

  float4 af[D8];
  load_row_tile<D8>(af, A, ut, li, h);

  // lane r < 32: cursor into row r's exclusion list, at the first id of this wave's item range
  int xpos = 0, xend = 0, xnext = INT_MAX;
  if (A.ex && lane < 32 && ut * 32 + lane < A.n) {
    const int e0 = A.ex_off[ut * 32 + lane], e1 = A.ex_off[ut * 32 + lane + 1];
    if (e0 >= 0 && e1 > e0) {
      int a = e0, b = e1;
      const int first = t_begin * 32;
      while (a < b) { const int md = (a + b) >> 1; if (A.ex[md] < first) a = md + 1; else b = md; }
      xpos = a; xend = e1;
      if (xpos < xend) xnext = A.ex[xpos];
    }
  }

  bool exdirty = false;
  if (lane < 32) s_exm[w][lane] = 0u;
  wave_fence();
  unsigned cnt[16][NP];
#pragma unroll
  for (int r = 0; r < 16; ++r)
#pragma unroll
    for (int p = 0; p < NP; ++p) cnt[r][p] = 0u;

  float4 b0[D8], b1[DB ? D8 : 1];
  load_item_tile<D8>(b0, A, t_begin, li, h);

  for (int tile = t_begin; tile < t_end; ++tile) {
    if constexpr (DB) { if (tile + 1 < t_end) load_item_tile<D8>(b1, A, tile + 1, li, h); }
    // (tile_walk.h: the walk's contract - not met here, the mask branch stands behind the product: DESIGN.md section 1)
    const f32x16 acc = tile_product<D8>(af, b0);
    const int j = tile * 32 + li;
    const bool jvalid = j < N;
    // listed ids of this tile -> one 32-bit mask per row
    const bool anyex = __any(xnext < tile * 32 + 32);
    if (anyex || exdirty) {                         // (wave-uniform; a tile without listed ids after one with some clears the masks)
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
    double jlat, jlon, jcp;
    item_tile_coords<GEO>(A, j, jlat, jlon, jcp);
    const int hb = opaque_half_base(h);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int ul = acc_tile_row(r, hb);
      float s = acc[r];
      if (GEO) s = geo_add(A, wd, s_geo, ut, ul, s_ulat, s_ulon, s_ucp, jlat, jlon, jcp, s);      // (unguarded: every ranked row has a last POI)
      const bool live = jvalid & !((s_exm[w][ul] >> li) & 1u);
      s = live ? s : __builtin_nanf("");            // compares false with everything: contributes nothing
#pragma unroll
      for (int p = 0; p < NP; ++p) {
        const RankTgt t0 = s_t[ul][2 * p];
        unsigned add = better(s, j, t0.s, t0.id) ? 1u : 0u;
        if constexpr (LT > 1) {
          const RankTgt t1 = s_t[ul][2 * p + 1];
          add |= better(s, j, t1.s, t1.id) ? 0x10000u : 0u;
        }
        cnt[r][p] += add;
      }
      __builtin_amdgcn_sched_barrier(0);            // one row's target reads in flight at a time (the scheduler would issue all 16 rows' first)
    }
    wave_fence();                                   // the masks are read before the next tile overwrites them
    if constexpr (DB) {
#pragma unroll
      for (int m = 0; m < D8; ++m) b0[m] = b1[m];
    } else {
      if (tile + 1 < t_end) load_item_tile<D8>(b0, A, tile + 1, li, h);
    }
  }

  // one reduction per (row, target) over the 32 lanes of the half wave, one integer atomic each
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int ul = acc_tile_row(r, 4 * h), row = ut * 32 + ul;
    int mine = 0;                                   // lane li = i of the half wave keeps target i's sum
#pragma unroll
    for (int i = 0; i < LT; ++i) {
      int v = (int)((cnt[r][i >> 1] >> (16 * (i & 1))) & 0xFFFFu);
#pragma unroll
      for (int o = 16; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
      mine = li == i ? v : mine;
    }
    if (li < LT && A.t_off + li < A.len_t && row < A.n && mine > 0) atomicAdd(&A.rank_out[(size_t)row * A.len_t + A.t_off + li], mine);
    __builtin_amdgcn_sched_barrier(0);              // (row by row: 128 butterflies in flight would set the kernel's register count)
  }
}

// The definition on explicit score rows: one workgroup per row.
__global__ __launch_bounds__(POI_BLOCK) void rank_scores_kernel(const float* __restrict__ scores, int n, int N, const int* __restrict__ tgt,
                                                                const int* __restrict__ tmask, int LT, const int* __restrict__ ex_off,
                                                                const int* __restrict__ ex, int* __restrict__ rank_out,
                                                                int* __restrict__ count_out, int* __restrict__ bad_out) {
  __shared__ int s_red[POI_NWAVE][RANK_LT_MAX];
  const int row = blockIdx.x, tid = threadIdx.x, lane = lane_id(), w = wave_id();
  const float* sr = scores + (size_t)row * N;
  int e0 = 0, e1 = 0, bad = 0;
  if (ex) {
    e0 = ex_off[row]; e1 = ex_off[row + 1];
    bad = e0 < 0 || e1 < e0;
    if (!bad)
      for (int p = e0 + tid; p < e1; p += POI_BLOCK) { const int v = ex[p]; bad |= (unsigned)v >= (unsigned)N || (p > e0 && ex[p - 1] >= v); }
  }
  const int badrow = __syncthreads_or(bad);
  if (badrow) { e0 = 0; e1 = 0; }
  float ts[RANK_LT_MAX]; int ti[RANK_LT_MAX]; int cnt[RANK_LT_MAX];
  int n_oor = 0;
#pragma unroll
  for (int i = 0; i < RANK_LT_MAX; ++i) {
    ts[i] = pos_inf(); ti[i] = -1; cnt[i] = 0;
    if (i < LT && tmask[(size_t)row * LT + i] != 0) {
      const int t = tgt[(size_t)row * LT + i];
      if ((unsigned)t >= (unsigned)N) ++n_oor;
      else if (!badrow && !listed(ex, e0, e1, t)) { ts[i] = sr[t]; ti[i] = t; }
    }
  }
  if (tid == 0 && (n_oor || badrow)) atomicAdd(bad_out, n_oor + (badrow ? 1 : 0));
  for (int j = tid; j < N; j += POI_BLOCK) {
    if (e1 > e0 && listed(ex, e0, e1, j)) continue;
    const float s = sr[j];
#pragma unroll
    for (int i = 0; i < RANK_LT_MAX; ++i) cnt[i] += better(s, j, ts[i], ti[i]) ? 1 : 0;
  }
#pragma unroll
  for (int i = 0; i < RANK_LT_MAX; ++i) {
    int v = cnt[i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if (lane == 0) s_red[w][i] = v;
  }
  __syncthreads();
  if (tid < LT) {
    int v = 0;
#pragma unroll
    for (int i = 0; i < RANK_LT_MAX; ++i)
      if (i == tid) v = ti[i] >= 0 ? (s_red[0][i] + s_red[1][i]) + (s_red[2][i] + s_red[3][i]) : -1;
    rank_out[(size_t)row * LT + tid] = v;
  }
  if (tid == 0 && count_out) count_out[row] = badrow ? 0 : N - (e1 - e0);
}

template <bool GEO>
static hipError_t launch_rank_g(const RankArgs& A, hipStream_t st) {
  return by_dim<128>(A.dim, [&](auto d8, auto db) -> hipError_t {
    constexpr int D8 = decltype(d8)::value;
    constexpr bool DB = decltype(db)::value;
    const int n_utile = (A.n + 31) / 32;
    const size_t lds = GEO ? sizeof(double) * (A.n_dist + 96) : 0;
    hipLaunchKernelGGL((rank_targets_kernel<D8, GEO>), dim3(n_utile), dim3(64), 0, st, A);
    const dim3 grid(n_utile, (A.n_split + POI_NWAVE - 1) / POI_NWAVE);
    if (A.len_t <= 1) hipLaunchKernelGGL((rank_kernel<D8, DB, GEO, 1>), grid, dim3(POI_BLOCK), lds, st, A);
    else {
      // four targets per walk (their counters and the product's operands fit the register file without scratch); more take a second walk
      RankArgs B = A;
      for (B.t_off = 0; B.t_off < A.len_t; B.t_off += 4) hipLaunchKernelGGL((rank_kernel<D8, DB, GEO, 4>), grid, dim3(POI_BLOCK), lds, st, B);
    }
    return hipGetLastError();
  });
}

hipError_t launch_rank(const RankArgs& A, hipStream_t st, Timing* tm) {
  tm->begin("score_rank", st);
  const hipError_t e = A.wd ? launch_rank_g<true>(A, st) : launch_rank_g<false>(A, st);
  tm->end(st);
  return e;
}

hipError_t launch_rank_scores(const float* scores, int n, int n_item, const int* tgt, const int* tmask, int len_t, const int* ex_off,
                              const int* ex, int* rank_out, int* count_out, int* bad, hipStream_t st) {
  hipLaunchKernelGGL(rank_scores_kernel, dim3((unsigned)n), dim3(POI_BLOCK), 0, st, scores, n, n_item, tgt, tmask, len_t, ex_off, ex, rank_out,
                     count_out, bad);
  return hipGetLastError();
}

}  // namespace poi
