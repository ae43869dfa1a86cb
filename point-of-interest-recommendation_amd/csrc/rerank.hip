// Re-ranking (poi_score_lists, poi_rerank_lists, poi_rerank): the second stage of a two-stage recommender - every row brings an
// EXPLICIT list of candidate POIs, the lists are scored under this model and come back in order.  The counterpart of select.hip, whose
// lists are what a retrieval stage hands over.
//
//   s(r, j)     = users[r] . items[j] (+ wd * P(bin of the distance last_poi[r] -> j) for rows with a last POI), the expression of
//                 score_rows_kernel (select.hip) and rank_targets_kernel (rank.hip): the SAME tile_product through load_frag and the same
//                 distance-term expression, so a pair's score has the bits of poi_score_rows / poi_score_rank
//   padding     = a negative id: its score is -inf
//   rejected    = a ragged row whose offsets are negative, descending or end beyond n_cand, or that holds an id >= n_item; a shared list
//                 that holds an id >= n_item rejects every row of the call.  All -inf, counted once, nothing outside cand[0 .. n_cand)
//                 or the tables is read
//
// lists_check_kernel          one workgroup per ragged row (one for a shared list): the rule above into flag[row], the count into bad
// score_lists_ragged_kernel   grid (row, chunks of the row's list taken with stride gridDim.y).  A wave scores 64 entries with two tile
//                             products: the row's fragment in EVERY A row, 32 gathered item rows as B (gather_score's trick, filter.hip) -
//                             every accumulator of lane l is the score of the entry of lane l & 31.  An output element depends on its
//                             own (row, id) only: every grid gives the same bits by construction.  The output is filled with -inf first;
//                             a rejected row writes nothing
// score_lists_shared_kernel   the tile walk of score_rows_kernel over ONE list: 32 rows as A, 32 gathered candidates as B, an item row is
//                             fetched once per 32-row tile instead of once per row; out[r * n_cand + c]
// rerank_sort_kernel          explicit scores (optionally blended with a prior in float64) -> the best k of every list.  One workgroup
//                             per row: keys (order image of the score << 32 | ~id, then ~position) into LDS, a bitonic network over the
//                             next power of two - descending score, ascending id, ascending position: total, so duplicates are kept and
//                             every grid gives the same bits - then ids, keys, positions and the -1 / -inf fill.  Integer and compare
//                             work only
// No float atomics, vector stores only.
#include "poi_common.h"
#include "poi_kernels.h"
#include "launch_common.h"
#include "tile_walk.h"

namespace poi {

namespace {

// 0 for a key that is never selected (NaN, -inf); otherwise f2ord of the key with -0.0 folded onto +0.0 (select.hip's rule)
__device__ __forceinline__ unsigned rerank_key(float s) {
  unsigned u = __float_as_uint(s);
  if ((u & 0x7fffffffu) > 0x7f800000u || u == 0xff800000u) return 0u;
  if ((u << 1) == 0u) u = 0u;
  return f2ord(__uint_as_float(u));
}

}  // namespace

__global__ __launch_bounds__(POI_BLOCK) void lists_check_kernel(const int* __restrict__ cand_off, const int* __restrict__ cand, int n_cand, int n_item,
                                                                 int* __restrict__ flag, int* __restrict__ bad_out) {
  const int row = blockIdx.x, tid = threadIdx.x;
  int o0 = 0, o1 = n_cand;
  if (cand_off) { o0 = cand_off[row]; o1 = cand_off[row + 1]; }
  int bad = o0 < 0 || o1 < o0 || o1 > n_cand;
  if (!bad)
    for (int p = o0 + tid; p < o1; p += POI_BLOCK) bad |= cand[p] >= n_item;
  bad = __syncthreads_or(bad);
  if (tid == 0) {
    flag[row] = bad ? 1 : 0;
    if (bad) atomicAdd(bad_out, 1);
  }
}

template <int D8, bool GEO>
__global__ __launch_bounds__(POI_BLOCK) void score_lists_ragged_kernel(ScoreListsArgs A) {
  const int lane = lane_id(), w = wave_id(), li = lane & 31, h = lane >> 5;
  const int D = A.dim, N = A.n_item, r = blockIdx.x;
  if (A.flag[r]) return;                            // rejected: the -inf fill stands
  const int o0 = A.cand_off[r], o1 = A.cand_off[r + 1];
  const int nchunk = (o1 - o0 + RERANK_CHUNK - 1) / RERANK_CHUNK;
  if ((int)blockIdx.y >= nchunk) return;
  float4 af[D8];
  load_frag<D8>(af, A.users, 0, (size_t)r, D, h);
  const float wd = GEO ? A.wd[0] : 0.f;
  int has = 0;
  double ulat = 0.0, ulon = 0.0, ucp = 0.0;
  if (GEO) load_row_geo(A, r, N, has, ulat, ulon, ucp);
  for (int c = blockIdx.y; c < nchunk; c += gridDim.y) {
    const int p0 = o0 + c * RERANK_CHUNK + w * 64;  // the wave's first entry
    if (p0 >= o1) continue;                         // (wave-uniform: the matrix instructions run with every lane on)
    const int p = p0 + lane;
    const int id = p < o1 ? A.cand[p] : -1;
    const int idc = min(max(id, 0), N - 1);         // (padding reads row 0; the check has seen every id below N)
    float4 bf[D8];
    load_frag<D8>(bf, A.items, A.items_f16, (size_t)__shfl(idc, li, 64), D, h);
    f32x16 acc = tile_product<D8>(af, bf);
    float mine = acc[0];
    if (p0 + 32 < o1) {
      load_frag<D8>(bf, A.items, A.items_f16, (size_t)__shfl(idc, 32 + li, 64), D, h);
      acc = tile_product<D8>(af, bf);
      if (h) mine = acc[0];
    }
    if (GEO) {
      if (has && id >= 0) mine = __fmaf_rn(wd, geo_prob(A, A.thr, r, ulat, ulon, ucp, A.coords[2 * (size_t)idc], A.coords[2 * (size_t)idc + 1], A.cphi[idc]), mine);
    }
    mine = one_zero(mine);
    if (p < o1) A.out[p] = id >= 0 ? mine : neg_inf();
  }
}

template <int D8, bool DB, bool GEO>
__global__ __launch_bounds__(POI_BLOCK) void score_lists_shared_kernel(ScoreListsArgs A) {
  __shared__ int s_has[32];
  __shared__ double s_ulat[32], s_ulon[32], s_ucp[32];
  extern __shared__ __align__(16) double s_thr[];   // GEO: thr[n_dist]
  const int lane = lane_id(), w = wave_id(), li = lane & 31, h = lane >> 5;
  const int D = A.dim, N = A.n_item, C = A.n_cand, ut = blockIdx.x;
  const int split = blockIdx.y * POI_NWAVE + w;
  int t_begin, t_end;
  wave_tile_chunk(C, A.n_split, split, t_begin, t_end);
  const bool rejected = A.flag[0] != 0;             // (workgroup-uniform)
  if (GEO && !rejected) {
    for (int i = threadIdx.x; i < A.n_dist; i += POI_BLOCK) s_thr[i] = A.thr[i];
    if (threadIdx.x < 32) {
      const int r = ut * 32 + (int)threadIdx.x;
      load_row_geo(A, r < A.n ? r : -1, N, s_has[threadIdx.x], s_ulat[threadIdx.x], s_ulon[threadIdx.x], s_ucp[threadIdx.x]);
    }
  }
  __syncthreads();
  if (t_begin >= t_end) return;
  if (rejected) {                                   // every row of the call: -inf
    for (int tile = t_begin; tile < t_end; ++tile)
      for (int ul = h; ul < 32; ul += 2) {
        const int row = ut * 32 + ul, c = tile * 32 + li;
        if (row < A.n && c < C) A.out[(size_t)row * (size_t)C + c] = neg_inf();
      }
    return;
  }
  const float wd = GEO ? A.wd[0] : 0.f;

  float4 af[D8];
  load_row_tile<D8>(af, A, ut, li, h);
  // the id of list position c, -1 behind the list; what is read of the tables: padding reads row 0
  auto id_at = [&](int c) { return c < C ? A.cand[c] : -1; };
  int id0 = id_at(t_begin * 32 + li), id1 = -1;
  float4 b0[D8], b1[DB ? D8 : 1];
  load_frag<D8>(b0, A.items, A.items_f16, (size_t)min(max(id0, 0), N - 1), D, h);
  for (int tile = t_begin; tile < t_end; ++tile) {
    if (tile + 1 < t_end) id1 = id_at((tile + 1) * 32 + li);
    if constexpr (DB) { if (tile + 1 < t_end) load_frag<D8>(b1, A.items, A.items_f16, (size_t)min(max(id1, 0), N - 1), D, h); }
    const f32x16 acc = tile_product<D8>(af, b0);   // (tile_walk.h: the walk's contract)
    const int c = tile * 32 + li, jc = min(max(id0, 0), N - 1);
    double jlat = 0.0, jlon = 0.0, jcp = 0.0;
    if (GEO) { jlat = A.coords[2 * (size_t)jc]; jlon = A.coords[2 * (size_t)jc + 1]; jcp = A.cphi[jc]; }
    const int hb = opaque_half_base(h);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int ul = acc_tile_row(r, hb), row = ut * 32 + ul;
      float s = acc[r];
      if (GEO) {
        if (s_has[ul]) s = geo_add(A, wd, s_thr, ut, ul, s_ulat, s_ulon, s_ucp, jlat, jlon, jcp, s);
      }
      s = one_zero(s);
      if (row < A.n && c < C) A.out[(size_t)row * (size_t)C + c] = id0 >= 0 ? s : neg_inf();      // 32 consecutive floats per row
      if (GEO) __builtin_amdgcn_sched_barrier(0);   // one row's distance term in flight at a time
    }
    if constexpr (DB) {
#pragma unroll
      for (int m = 0; m < D8; ++m) b0[m] = b1[m];
    } else {
      if (tile + 1 < t_end) load_frag<D8>(b0, A.items, A.items_f16, (size_t)min(max(id1, 0), N - 1), D, h);
    }
    id0 = id1;
  }
}

__global__ __launch_bounds__(RERANK_SORT_BLOCK) void rerank_sort_kernel(RerankListsArgs A) {
  extern __shared__ __align__(16) unsigned long long s_k[];      // p_max keys, then p_max position words
  __shared__ int s_cnt;
  unsigned* const s_p = reinterpret_cast<unsigned*>(s_k + A.p_max);
  const int tid = threadIdx.x, nt = (int)blockDim.x, row = blockIdx.x, K = A.k;
  int o0 = 0, o1 = A.n_cand, bad = 0;
  if (A.cand_off) {
    o0 = A.cand_off[row]; o1 = A.cand_off[row + 1];
    bad = o0 < 0 || o1 < o0 || o1 > A.n_cand || o1 - o0 > RERANK_LEN_MAX;
  }
  const int flagged = A.flag ? A.flag[A.cand_off ? row : 0] : 0;      // poi_rerank: the scoring stage has rejected AND counted this row
  if (tid == 0) {
    s_cnt = 0;
    if (bad && !flagged) atomicAdd(A.bad, 1);
  }
  const int L = bad ? 0 : o1 - o0;                  // (a flagged row with sound offsets sorts its -inf scores: what the two calls give)
  const size_t sb = A.cand_off ? (size_t)o0 : (size_t)row * (size_t)A.n_cand;      // the row's scores / priors
  int P = 1;
  while (P < L) P <<= 1;
  __syncthreads();
  int mine = 0;
  for (int i = tid; i < P; i += nt) {
    unsigned long long e = 0ull;
    unsigned q = 0u;
    if (i < L) {
      const int id = A.cand[o0 + i];
      float t = A.score[sb + i];
      if (A.prior) t = __double2float_rn(__dadd_rn(__dmul_rn(A.w_score, (double)t), __dmul_rn(A.w_prior, (double)A.prior[sb + i])));
      const unsigned key = id < 0 ? 0u : rerank_key(t);
      if (key) { e = ((unsigned long long)key << 32) | (unsigned)~id; q = ~(unsigned)i; ++mine; }
    }
    s_k[i] = e; s_p[i] = q;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mine += __shfl_xor(mine, o, 64);
  if (lane_id() == 0 && mine) atomicAdd(&s_cnt, mine);
  __syncthreads();
  for (int k2 = 2; k2 <= P; k2 <<= 1)
    for (int jj = k2 >> 1; jj > 0; jj >>= 1) {
      for (int t = tid; t < (P >> 1); t += nt) {
        const int i = ((t & ~(jj - 1)) << 1) | (t & (jj - 1)), x = i | jj;      // the t-th pair of this step
        const unsigned long long a = s_k[i], b = s_k[x];
        const unsigned qa = s_p[i], qb = s_p[x];
        const bool desc = (i & k2) == 0;
        const bool a_lt_b = a < b || (a == b && qa < qb);
        const bool a_gt_b = a > b || (a == b && qa > qb);
        if (desc ? a_lt_b : a_gt_b) { s_k[i] = b; s_k[x] = a; s_p[i] = qb; s_p[x] = qa; }
      }
      __syncthreads();
    }
  const int count = s_cnt, Kp = min(K, count);
  for (int i = tid; i < K; i += nt) {
    const bool in = i < Kp;
    const unsigned long long e = in ? s_k[i] : 0ull;
    A.idx_out[(size_t)row * K + i] = in ? (int)~(unsigned)e : -1;
    if (A.score_out) A.score_out[(size_t)row * K + i] = in ? ord2f((unsigned)(e >> 32)) : neg_inf();
    if (A.pos_out) A.pos_out[(size_t)row * K + i] = in ? (int)~s_p[i] : -1;
  }
  if (tid == 0 && A.count_out) A.count_out[row] = count;
}

template <bool GEO>
static hipError_t launch_score_lists_g(const ScoreListsArgs& A, hipStream_t st) {
  return by_dim<128>(A.dim, [&](auto d8, auto db) -> hipError_t {
    constexpr int D8 = decltype(d8)::value;
    if (A.cand_off) {
      hipLaunchKernelGGL((score_lists_ragged_kernel<D8, GEO>), dim3((unsigned)A.n, (unsigned)A.n_split), dim3(POI_BLOCK), 0, st, A);
    } else {
      const dim3 grid((A.n + 31) / 32, (A.n_split + POI_NWAVE - 1) / POI_NWAVE);
      hipLaunchKernelGGL((score_lists_shared_kernel<D8, decltype(db)::value, GEO>), grid, dim3(POI_BLOCK), GEO ? sizeof(double) * A.n_dist : 0, st, A);
    }
    return hipGetLastError();
  });
}

hipError_t launch_score_lists(const ScoreListsArgs& A, hipStream_t st, Timing* tm) {
  Timing::Scope rec(tm, "score_lists", st);
  hipLaunchKernelGGL(lists_check_kernel, dim3(A.cand_off ? (unsigned)A.n : 1u), dim3(POI_BLOCK), 0, st, A.cand_off, A.cand, A.n_cand, A.n_item, A.flag, A.bad);
  if (A.cand_off) {                                 // a rejected ragged row writes nothing: its -inf is this fill's
    const hipError_t e = hipMemsetD32Async((hipDeviceptr_t)A.out, (int)0xff800000u, (size_t)A.n_cand, st);
    if (e != hipSuccess) return e;
  }
  return A.wd ? launch_score_lists_g<true>(A, st) : launch_score_lists_g<false>(A, st);
}

hipError_t launch_rerank_lists(const RerankListsArgs& A, hipStream_t st, Timing* tm) {
  tm->begin("rerank_lists", st);
  const int half = A.p_max / 2;
  const int threads = half < 64 ? 64 : half > RERANK_SORT_BLOCK ? RERANK_SORT_BLOCK : half;      // a thread per pair of a step, up to 1024
  hipLaunchKernelGGL(rerank_sort_kernel, dim3((unsigned)A.n), dim3(threads), (sizeof(unsigned long long) + sizeof(unsigned)) * (size_t)A.p_max, st, A);
  tm->end(st);
  return hipGetLastError();
}

}  // namespace poi
