// Route recommendation (poi_route_expand, poi_route_merge): one step of a beam search over a session's next POIs - per hypothesis row the
// best b candidates by the model's score AND the normaliser of that score over all POIs, in one pass over the item table, without the
// (rows, n_item) score matrix.
//
//   s(r, j)  = poi_score_rank's s(r, j): users[r] . items[j] from tile_product (tile_product.h), plus wd * sts[r][bin(last_poi[r], j)]
//              for bin < n_dist; a row with last_poi[r] < 0 has no distance term
//   lse(r)   = log sum_{j in [0, n_item)} exp(double(s(r, j))), excluded POIs included, NaN scores left out
//   C(r)     = [0, n_item) minus the exclusion list of the row's slot (list row / rows_per_list) minus the row's own path
//   list     = the best min(b, |C(r)|) of C(r) by better() (higher score, then lower id)
//
// route_expand_kernel: the item-stationary tile walk in tile_walk.h's steps (load_row_tile / load_item_tile, item_tile_coords, geo_add;
// the item BLOCK ranges are its own).  A workgroup owns a 32-row tile and one slice of the item range; each
// of its four waves walks a contiguous range of ITEM BLOCKS (ROUTE_LSE_TILES tiles = 512 POIs) with the rows' A fragments in registers.
// Epilogue per 32 x 32 tile and accumulator register (one (row, item) pair per lane):
//   normaliser  a per-lane running (max, float64 sum) of the pairs this lane has seen in the current block - lane `li` of the half wave
//               sees the items j = li (mod 32) of the block in ascending order.  At the block's end the 32 lanes' partials are rescaled to
//               the block's maximum and summed by an xor butterfly (16, 8, 4, 2, 1), and (max, sum) of (row, block) goes to the workspace.
//               The block partials do not depend on which wave of which grid walked the block.
//   selection   the score is compared with the b-th entry of the row's sorted list in LDS (one broadcast read); the rare survivors are
//               looked up in the slot's exclusion list (binary search) and the row's path (linear scan, <= 16) and inserted one at a time.
// route_finish_row (one wave per row) folds the row's partial lists (top64_merge, a total order: every cut gives the same list) and
// the block partials: M = max over the blocks, S = sum of sum_b * exp(max_b - M) over the blocks IN ASCENDING BLOCK ORDER (a serial
// float64 chain), lse = M + log(S).  Split path: route_finish_kernel; tile path: the workgroup finishes its own 32 rows.
// No float atomics; a rejected row is counted with one integer atomic.
//
// Bytes: per 32-row tile the item table once (4 dim n_item, 2 dim from a half table), + 24 n_item of coordinates with the distance term,
// + 16 bytes per (row, block) of normaliser partials and 64 per (row, wave) of list partials.  Flops: 2 (32 rows) n_item dim on the f32
// matrix pipe and one float64 exp per (row, item) pair on the vector ALUs.
//
// route_merge_kernel: one wave per slot, one proposal per lane (parents x b <= 64): total = parent's total + (double(score) - lse), ranked
// by (higher total, lower parent, lower POI id) with a 64-step all-pairs count; the best b survive.
#include "poi_common.h"
#include "poi_kernels.h"
#include "launch_common.h"
#include "tile_walk.h"
#include "topk_list.h"
#include <limits.h>

namespace poi {

static_assert(ROUTE_NWAVE == POI_NWAVE, "the host sizes the partial lists by ROUTE_NWAVE");

namespace {

__device__ __forceinline__ double neg_inf_d() { return -__builtin_huge_val(); }

// the lanes of `bal` hold candidates (v, j) for the sorted ROUTE_B_MAX-entry list (ls, lx) in LDS: one at a time - the entries in front of
// the newcomer are a prefix of the sorted list, the others move down one lane (topk_list.h's list_take on a short list)
__device__ __forceinline__ void list8_take(float* ls, int* lx, unsigned long long bal, float v, int j) {
  const int lane = lane_id();
  float cs = lane < ROUTE_B_MAX ? ls[lane] : neg_inf();
  int ci = lane < ROUTE_B_MAX ? lx[lane] : PAD_ID;
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
  if (lane < ROUTE_B_MAX) { ls[lane] = cs; lx[lane] = ci; }
  wave_fence();
}

// one wave: the answer of row `row` from its W partial lists and its block partials
__device__ __forceinline__ void route_finish_row(const RouteArgs& A, int row, int W) {
  const int lane = lane_id(), b = A.b;
  const int st = A.row_st[row];
  if (st != 1) {                                    // dead (0) or rejected (2)
    if (lane < b) { A.idx_out[(size_t)row * b + lane] = -1; A.score_out[(size_t)row * b + lane] = neg_inf(); }
    if (lane == 0) { A.lse_out[row] = __builtin_nan(""); if (A.count_out) A.count_out[row] = 0; }
    return;
  }
  float cs;
  int ci;
  fold_slice_lists<ROUTE_B_MAX>(A.part_s, A.part_i, (size_t)row * W, W, cs, ci);
  if (lane < b) {
    A.idx_out[(size_t)row * b + lane] = ci == PAD_ID ? -1 : ci;
    A.score_out[(size_t)row * b + lane] = ci == PAD_ID ? neg_inf() : cs;
  }
  // the normaliser: the maximum first (exact in any order), then the rescaled block sums in ascending block order
  const int nblk = A.n_blk;
  const double* pl = A.part_lse + (size_t)row * nblk * 2;
  double M = neg_inf_d();
  for (int q = lane; q < nblk; q += 64) M = fmax(M, pl[2 * q]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) M = fmax(M, __shfl_xor(M, o, 64));
  double S = 0.0;
  for (int q0 = 0; q0 < nblk; q0 += 64) {
    const int q = q0 + lane;
    double term = 0.0;
    if (q < nblk) { const double mb = pl[2 * q]; if (mb > neg_inf_d()) term = pl[2 * q + 1] * exp(mb - M); }
    const int cnt = min(64, nblk - q0);
    for (int i = 0; i < cnt; ++i) S += __shfl(term, i, 64);
  }
  if (lane == 0) {
    A.lse_out[row] = M + log(S);
    if (A.count_out) A.count_out[row] = A.row_cnt[row];
  }
}

}  // namespace

template <int D8, bool DB, bool GEO>
__global__ __launch_bounds__(POI_BLOCK) void route_expand_kernel(RouteArgs A) {
  __shared__ float l_s[POI_NWAVE][32][ROUTE_B_MAX];
  __shared__ int l_i[POI_NWAVE][32][ROUTE_B_MAX];
  __shared__ int s_st[32], s_e0[32], s_e1[32], s_has[32];
  __shared__ int s_path[32][ROUTE_T_MAX];
  __shared__ double s_ulat[32], s_ulon[32], s_ucp[32];
  extern __shared__ __align__(16) double s_thr[];   // GEO: thr[n_dist]
  const int tid = threadIdx.x, lane = lane_id(), w = wave_id(), li = lane & 31, h = lane >> 5;
  const int S = A.n_split, ut = blockIdx.x / S, sl = blockIdx.x - ut * S;
  const int N = A.n_item, b = A.b, PL = A.path_len;

  // the tile's rows: live? exclusion list ascending inside [0, N), path ids inside [0, N); |C(r)|
  for (int i = w; i < 32; i += POI_NWAVE) {
    const int row = ut * 32 + i;
    int st = 0, e0 = 0, e1 = 0, cnt = 0, pv = -1;
    if (row < A.n && (!A.live || A.live[row] != 0)) {      // (wave-uniform)
      int bad = 0;
      if (A.ex) bad = check_ex_row(A.ex_off, A.ex, row / A.rows_per_list, N, lane, e0, e1);
      if (lane < PL) { pv = A.path[(size_t)row * A.path_stride + lane]; bad |= (unsigned)pv >= (unsigned)N; }
      bad = __any(bad) ? 1 : 0;
      st = bad ? 2 : 1;
      if (bad) { e0 = 0; e1 = 0; pv = -1; }
      else {
        int extra = 0;                              // path ids that the list does not hold already, each once
        if (lane < PL) {
          extra = !listed(A.ex, e0, e1, pv);
          for (int q = 0; q < lane; ++q) extra &= A.path[(size_t)row * A.path_stride + q] != pv;
        }
        cnt = N - (e1 - e0) - __popcll(__ballot(extra != 0));
      }
    }
    if (lane < ROUTE_T_MAX) s_path[i][lane] = lane < PL ? pv : -1;
    if (lane == 0) {
      s_st[i] = st; s_e0[i] = e0; s_e1[i] = e1;
      if (sl == 0) {
        A.row_st[row] = st; A.row_cnt[row] = cnt;
        if (st == 2) atomicAdd(A.bad, 1);
      }
      if (GEO) load_row_geo(A, row < A.n ? row : -1, N, s_has[i], s_ulat[i], s_ulon[i], s_ucp[i]);
    }
  }
  if (GEO)
    for (int i = tid; i < A.n_dist; i += POI_BLOCK) s_thr[i] = A.thr[i];
  for (int e = lane; e < 32 * ROUTE_B_MAX; e += 64) { (&l_s[w][0][0])[e] = neg_inf(); (&l_i[w][0][0])[e] = PAD_ID; }
  __syncthreads();
  const int any_live = __syncthreads_or(tid < 32 && s_st[tid & 31] == 1);

  const int W = S * POI_NWAVE, wv = sl * POI_NWAVE + w;
  const int ntile = (N + 31) / 32, nblk = A.n_blk;
  const int q_begin = (int)((long long)nblk * wv / W), q_end = (int)((long long)nblk * (wv + 1) / W);
  const int t_begin = q_begin * ROUTE_LSE_TILES, t_end = min(ntile, q_end * ROUTE_LSE_TILES);

  if (any_live && t_begin < t_end) {                // (wave-uniform)
    const float wd = GEO ? A.wd[0] : 0.f;
    float4 af[D8];
    load_row_tile<D8>(af, A, ut, li, h);
    float mx[16];
    double sm[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) { mx[r] = neg_inf(); sm[r] = 0.0; }

    float4 b0[D8], b1[DB ? D8 : 1];
    load_item_tile<D8>(b0, A, t_begin, li, h);
    for (int tile = t_begin; tile < t_end; ++tile) {
      if constexpr (DB) { if (tile + 1 < t_end) load_item_tile<D8>(b1, A, tile + 1, li, h); }
      f32x16 acc = tile_product<D8>(af, b0);       // (tile_walk.h: the walk's contract)
      const int j = tile * 32 + li;
      const bool jvalid = j < N;
      double jlat, jlon, jcp;
      item_tile_coords<GEO>(A, j, jlat, jlon, jcp);
      const int hb = opaque_half_base(h);
      unsigned cm = 0u;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int ul = acc_tile_row(r, hb);
        float s = acc[r];
        if (GEO) {
          if (s_has[ul]) s = geo_add(A, wd, s_thr, ut, ul, s_ulat, s_ulon, s_ucp, jlat, jlon, jcp, s);
          acc[r] = s;
        }
        if (jvalid && s == s) {                     // (a NaN adds nothing)
          if (s > mx[r]) { sm[r] = sm[r] * exp((double)mx[r] - (double)s) + 1.0; mx[r] = s; }
          else if (s > neg_inf()) sm[r] += exp((double)s - (double)mx[r]);
        }
        if (jvalid && s_st[ul] == 1 && better(s, j, l_s[w][ul][b - 1], l_i[w][ul][b - 1])) cm |= 1u << r;
        __builtin_amdgcn_sched_barrier(0);          // one row's exp in flight at a time (the scheduler would issue all 16 rows' first)
      }
      if (__ballot(cm != 0u)) {                     // (rare once the lists have warmed up)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
#pragma unroll
          for (int hh = 0; hh < 2; ++hh) {
            bool cand = h == hh && ((cm >> r) & 1u);
            if (!__ballot(cand)) continue;          // (wave-uniform)
            const int ul = acc_tile_row(r, 4 * hh);
            if (cand) {
              bool out = s_e1[ul] > s_e0[ul] && listed(A.ex, s_e0[ul], s_e1[ul], j);
              for (int q = 0; q < PL; ++q) out |= s_path[ul][q] == j;
              cand = !out;
            }
            const unsigned long long bal = __ballot(cand);
            if (bal) list8_take(l_s[w][ul], l_i[w][ul], bal, acc[r], j);
          }
        }
      }
      // the end of an item block: the 32 lanes' partials of every row -> (max, sum) of (row, block)
      if (((tile + 1) % ROUTE_LSE_TILES) == 0 || tile + 1 == t_end) {
        const int blk = tile / ROUTE_LSE_TILES;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int ul = acc_tile_row(r, 4 * h);
          float M = mx[r];
#pragma unroll
          for (int o = 16; o > 0; o >>= 1) M = fmaxf(M, __shfl_xor(M, o, 64));
          double t = mx[r] > neg_inf() ? sm[r] * exp((double)mx[r] - (double)M) : 0.0;
#pragma unroll
          for (int o = 16; o > 0; o >>= 1) t += __shfl_xor(t, o, 64);
          if (li == 0) {
            double* pl = A.part_lse + ((size_t)(ut * 32 + ul) * nblk + blk) * 2;
            pl[0] = (double)M; pl[1] = t;
          }
          mx[r] = neg_inf(); sm[r] = 0.0;
          __builtin_amdgcn_sched_barrier(0);
        }
      }
      if constexpr (DB) {
#pragma unroll
        for (int m = 0; m < D8; ++m) b0[m] = b1[m];
      } else {
        if (tile + 1 < t_end) load_item_tile<D8>(b0, A, tile + 1, li, h);
      }
    }
  }

  // the wave's lists -> the rows' partial lists
  if (any_live) {
    for (int e = lane; e < 32 * ROUTE_B_MAX; e += 64) {
      const int i = e / ROUTE_B_MAX;
      const size_t at = ((size_t)(ut * 32 + i) * W + wv) * ROUTE_B_MAX + (e & (ROUTE_B_MAX - 1));
      A.part_s[at] = l_s[w][i][e & (ROUTE_B_MAX - 1)]; A.part_i[at] = l_i[w][i][e & (ROUTE_B_MAX - 1)];
    }
  }
  if (A.finish) {                                   // tile path (S = 1): the workgroup's own 32 rows
    __threadfence_block();
    __syncthreads();
    for (int i = w; i < 32; i += POI_NWAVE)
      if (ut * 32 + i < A.n) route_finish_row(A, ut * 32 + i, W);
  }
}

// split path: one wave per row
__global__ __launch_bounds__(64) void route_finish_kernel(RouteArgs A) { route_finish_row(A, blockIdx.x, A.n_split * POI_NWAVE); }

// one wave per slot, one proposal per lane
__global__ __launch_bounds__(64) void route_merge_kernel(RouteMergeArgs A) {
  const int s = blockIdx.x, lane = lane_id(), P = A.n_par, B = A.b;
  const int p = lane / B, e = lane - p * B;
  const int n_live = A.n_live ? min(max(A.n_live[s], 0), P) : P;
  double tot = neg_inf_d(), lp = neg_inf_d();
  int poi = PAD_ID, par = INT_MAX;
  if (p < n_live) {
    const size_t row = (size_t)s * P + p;
    const int id = A.idx[row * B + e];
    if (id >= 0) {
      const double x = (double)A.score[row * B + e] - A.lse[row];
      const double t = A.total_in[row] + x;
      if (t == t && t > neg_inf_d()) { tot = t; lp = x; poi = id; par = p; }      // (-inf and NaN totals: dead)
    }
  }
  int rank = 0;
  for (int i = 0; i < 64; ++i) {
    const double ot = __shfl(tot, i, 64);
    const int op = __shfl(par, i, 64), oi = __shfl(poi, i, 64);
    rank += (ot > tot || (ot == tot && (op < par || (op == par && oi < poi)))) ? 1 : 0;
  }
  const int n_valid = __popcll(__ballot(par != INT_MAX));
  const size_t base = (size_t)s * B;
  if (par != INT_MAX && rank < B) {
    A.parent_out[base + rank] = par; A.poi_out[base + rank] = poi; A.total_out[base + rank] = tot;
    if (A.steplp_out) A.steplp_out[base + rank] = lp;
  }
  if (lane < B && lane >= n_valid) {                // dead beams keep their own place's prefix
    A.parent_out[base + lane] = min(lane, P - 1); A.poi_out[base + lane] = -1; A.total_out[base + lane] = neg_inf_d();
    if (A.steplp_out) A.steplp_out[base + lane] = neg_inf_d();
  }
  if (lane == 0 && A.nlive_out) A.nlive_out[s] = min(n_valid, B);
}

template <bool GEO>
static hipError_t launch_route_g(const RouteArgs& A, hipStream_t st) {
  return by_dim<64>(A.dim, [&](auto d8, auto db) -> hipError_t {
    const unsigned n_utile = (unsigned)((A.n + 31) / 32);
    const size_t lds = GEO ? sizeof(double) * A.n_dist : 0;
    hipLaunchKernelGGL((route_expand_kernel<decltype(d8)::value, decltype(db)::value, GEO>), dim3(n_utile * (unsigned)A.n_split), dim3(POI_BLOCK), lds, st, A);
    return hipSuccess;
  });
}

hipError_t launch_route_expand(const RouteArgs& A, hipStream_t st, Timing* tm) {
  Timing::Scope rec(tm, "route_expand", st);
  const hipError_t e = A.wd ? launch_route_g<true>(A, st) : launch_route_g<false>(A, st);
  if (e != hipSuccess) return e;
  if (!A.finish) hipLaunchKernelGGL(route_finish_kernel, dim3((unsigned)A.n), dim3(64), 0, st, A);
  return rec.close();
}

hipError_t launch_route_merge(const RouteMergeArgs& A, hipStream_t st, Timing* tm) {
  tm->begin("route_merge", st);
  hipLaunchKernelGGL(route_merge_kernel, dim3((unsigned)A.n_slot), dim3(64), 0, st, A);
  tm->end(st);
  return hipGetLastError();
}

}  // namespace poi
