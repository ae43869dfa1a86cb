// Diversified recommendation (poi_diverse_pool, poi_diverse_rerank, poi_diverse_topk): a pool of the best <= 64 candidates of every
// row without the (n, n_item) score matrix, and its re-ranking for relevance against redundancy (maximal marginal relevance, MMR).
//
// Stage 1, the pool.
//   C(r)     = [0, n_item) minus the exclusion list of row r (the conventions of poi_score_rank)
//   s(r, j)  = poi_score_rank's s(r, j): users[r] . items[j] from tile_product (tile_product.h), plus wd * sts[r][bin(last_poi[r], j)]
//              for bin < n_dist; a row with last_poi < 0 has no distance term
//   P(r)     = the best min(pool, |selectable C(r)|) candidates by better() (descending score, ascending id).  NaN, -inf and +inf scores
//              are never pooled (+inf is pooled by poi_score_topk: stage 2 normalises the scores, so it must stay out here).
// diverse_pool_kernel: a workgroup owns a 32-row tile and one slice of the item range, its four waves a quarter of the slice each - the
// item-stationary tile walk in tile_walk.h's steps: the rows' A fragments in registers, the slice's 32-item tiles streamed past them on
// the f32 matrix pipe,
// the distance term added in the accumulator registers.  Every wave keeps one sorted 64-entry list per row in LDS (topk_list.h).  Per tile
// each of the lane's 16 scores is compared with the K-th entry of its row's list (LDS broadcast reads, one ballot for the common
// tile); only the survivors are looked up in the exclusion list and inserted, a row at a time: a few by single insertion (the entries
// in front of the newcomer are a prefix of the sorted list, the others move down one lane), many - the first tiles - through
// lds_list_merge's sort.  Either way the list is the best 64 of everything offered, and everything that beats the list's K-th entry is
// offered: with K = pool <= 64 entries 0 .. K - 1 are exact, to the last one.  The four waves' lists meet in LDS (top64_merge); on the
// split path they go to per-slice partial lists of 64 entries that topk_slices_merge_kernel folds.  The order is total and a pair's score
// does not depend on the slice or the wave: every grid gives the same bits, a row gives the same bits alone as in a call of thousands.
//
// Stage 2, the re-rank (everything in float64).  Pool position i = the i-th best, m = the entries before the first -1.
//   rel_i    = (s_i - s_{m-1}) / (s_0 - s_{m-1}), 1 when s_0 == s_{m-1}
//   d(i, l)  = 12742 asin(min(1, sqrt(sin^2(dlat pi/360) + cos(lat_i) cos(lat_l) sin^2(dlon pi/360))))  km
//              - the sin^2 form, NOT haversine_c's (1 - cos) / 2: that form loses the relative accuracy of nearby pairs to cancellation
//              (the distance bins never saw it, both sides of their compare hold the same c), and the similarity below is most
//              sensitive exactly where POIs are metres apart
//   geo      = exp(-d / scale_km);   emb = x_i . x_l / (|x_i| |x_l|), 0 if either norm is 0;   sim = g geo + (1 - g) emb
//              (a part with zero weight is not evaluated: its inputs may be null)
//   greedy   the first pick is position 0; after each pick l, pen_i = max(pen_i, sim(i, l)) (= sim(i, l) after the first); step t >= 1
//            picks the unselected i with the largest obj_i = trade rel_i - (1 - trade) pen_i, ties to the lower position; min(k, m) picks.
// diverse_rerank_kernel: one wave per row, lane i owns pool position i - the pool is the wave.  Per step one (objective, position)
// arg-max butterfly, the winner broadcast, every lane updates its pen against the winner: one float64 distance and one exp, and / or
// one float64 dot product against the winner's row.  The pool's item rows are staged once in LDS as float32 (64 rows, row stride
// dim + 4 floats: the lanes' float4 reads fall into different banks); a dot product is four interleaved float64 fma chains over the
// columns c = 0, 4, 8 .. (chain q takes columns 4 i + q), closed as (a0 + a1) + (a2 + a3): one order per dim.  trade == 1 evaluates no
// similarity at all.  No atomics on a result; a rejected row is counted with one integer atomic.
#include "poi_common.h"
#include "poi_kernels.h"
#include "pair_sim.h"
#include "launch_common.h"
#include "tile_walk.h"
#include "topk_list.h"

namespace poi {

namespace {

constexpr int POOL_LISTS_BYTES = POI_NWAVE * 32 * DIVERSE_POOL_MAX * 8;      // the waves' per-row lists: scores, then ids
constexpr int RERANK_LDS_MAX = DIVERSE_POOL_MAX * (256 + 4) * 4;

__device__ __forceinline__ bool finite_f(float s) { return (__float_as_uint(s) & 0x7f800000u) != 0x7f800000u; }

}  // namespace

template <int D8, bool DB, bool GEO>
__global__ __launch_bounds__(POI_BLOCK) void diverse_pool_kernel(DiverseArgs A) {
  __shared__ int s_e0[32], s_e1[32], s_ok[32], s_has[32];      // per tile row: exclusion list, ranked at all, has a last POI
  __shared__ double s_ulat[32], s_ulon[32], s_ucp[32];
  extern __shared__ __align__(16) unsigned char s_dyn[];       // lists (POOL_LISTS_BYTES) | GEO: thr[n_dist]
  float* const l_s = reinterpret_cast<float*>(s_dyn);
  int* const l_i = reinterpret_cast<int*>(s_dyn + POOL_LISTS_BYTES / 2);
  double* const s_thr = reinterpret_cast<double*>(s_dyn + POOL_LISTS_BYTES);
  const int tid = threadIdx.x, lane = lane_id(), w = wave_id(), li = lane & 31, h = lane >> 5;
  const int S = A.n_split, ut = blockIdx.x / S, sl = blockIdx.x - ut * S;
  const int N = A.n_item, K = A.k;

  // the tile's rows: exclusion lists with offsets in order, ids ascending inside [0, N)
  for (int i = w; i < 32; i += POI_NWAVE) {
    const int r = ut * 32 + i;
    int bad = 0, e0 = 0, e1 = 0;
    if (r < A.n && A.ex) bad = check_ex_row(A.ex_off, A.ex, r, N, lane, e0, e1);
    bad = __any(bad) ? 1 : 0;
    if (lane == 0) {
      s_ok[i] = r < A.n && !bad; s_e0[i] = bad ? 0 : e0; s_e1[i] = bad ? 0 : e1;
      if (bad && sl == 0) atomicAdd(A.bad, 1);
      if (GEO) load_row_geo(A, r < A.n ? r : -1, N, s_has[i], s_ulat[i], s_ulon[i], s_ucp[i]);
    }
  }
  if (GEO)
    for (int i = tid; i < A.n_dist; i += POI_BLOCK) s_thr[i] = A.thr[i];
  for (int e = tid; e < POI_NWAVE * 32 * DIVERSE_POOL_MAX; e += POI_BLOCK) { l_s[e] = neg_inf(); l_i[e] = PAD_ID; }
  __syncthreads();

  int ntile, tb, te;
  wave_tile_range(N, sl, S, w, ntile, tb, te);
  const float wd = GEO ? A.wd[0] : 0.f;
  float* const ls = l_s + w * 32 * DIVERSE_POOL_MAX;
  int* const lx = l_i + w * 32 * DIVERSE_POOL_MAX;

  unsigned rok = 0u;                                // the lane's 16 accumulator rows that are ranked
#pragma unroll
  for (int r = 0; r < 16; ++r) rok |= s_ok[acc_tile_row(r, 4 * h)] ? 1u << r : 0u;

  float4 af[D8];
  load_row_tile<D8>(af, A, ut, li, h);
  float4 b0[D8], b1[DB ? D8 : 1];
  load_item_tile<D8>(b0, A, tb, li, h);
  for (int tile = tb; tile < te; ++tile) {
    if constexpr (DB) { if (tile + 1 < te) load_item_tile<D8>(b1, A, tile + 1, li, h); }
    f32x16 acc = tile_product<D8>(af, b0);         // (tile_walk.h: the walk's contract)
    const int j = tile * 32 + li;
    double jlat, jlon, jcp;
    item_tile_coords<GEO>(A, j, jlat, jlon, jcp);
    const int hb = opaque_half_base(h);
    unsigned cm = 0u;                               // bit r: acc[r] beats the K-th entry of its row's list
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int ul = acc_tile_row(r, hb);
      float s = acc[r];
      if (GEO) {
        if (s_has[ul]) s = geo_add(A, wd, s_thr, ut, ul, s_ulat, s_ulon, s_ucp, jlat, jlon, jcp, s);
        acc[r] = s;
      }
      if (finite_f(s) && better(s, j, ls[ul * DIVERSE_POOL_MAX + K - 1], lx[ul * DIVERSE_POOL_MAX + K - 1])) cm |= 1u << r;
      if (GEO) __builtin_amdgcn_sched_barrier(0);   // one row's distance term in flight at a time (the scheduler would issue all 16 rows' first)
    }
    cm = j < N ? cm & rok : 0u;
    if (__ballot(cm != 0u)) {
      // the rare part: row by row, the exclusion lookup and the insertions
      for (int row = 0; row < 32; ++row) {
        int rr;
        bool cand = rare_row(row, h, cm, rr);
        if (!__ballot(cand)) continue;              // (wave-uniform)
        const float v = acc_row(acc, rr);
        const int e0 = s_e0[row], e1 = s_e1[row];
        if (cand && e1 > e0) cand = !listed(A.ex, e0, e1, j);
        const unsigned long long bal = __ballot(cand);
        if (bal) list_take(ls + row * DIVERSE_POOL_MAX, lx + row * DIVERSE_POOL_MAX, bal, cand, v, j, K);
      }
    }
    if constexpr (DB) {
#pragma unroll
      for (int m = 0; m < D8; ++m) b0[m] = b1[m];
    } else {
      if (tile + 1 < te) load_item_tile<D8>(b0, A, tile + 1, li, h);
    }
  }

  __syncthreads();
  // the four waves' lists of a row meet: wave w folds rows w, w + 4, ...
  for (int i = w; i < 32; i += POI_NWAVE) {
    const int row = ut * 32 + i;
    if (row >= A.n) break;
    float cs = l_s[i * DIVERSE_POOL_MAX + lane];
    int ci = l_i[i * DIVERSE_POOL_MAX + lane];
    for (int ww = 1; ww < POI_NWAVE; ++ww)
      top64_merge(cs, ci, l_s[(ww * 32 + i) * DIVERSE_POOL_MAX + lane], l_i[(ww * 32 + i) * DIVERSE_POOL_MAX + lane]);
    const int cnt = (s_ok[i] && sl == 0) ? N - (s_e1[i] - s_e0[i]) : 0;
    list_emit<DIVERSE_POOL_MAX>(A, A.part_s != nullptr, row, sl, cs, ci, cnt);
  }
}

template <bool GEO, bool EMB>
__global__ __launch_bounds__(64) void diverse_rerank_kernel(RerankArgs A) {
#pragma clang fp contract(off)
  extern __shared__ __align__(16) float s_x[];      // EMB: the pool's item rows, 64 x (dim + 4)
  const int r = blockIdx.x, lane = lane_id();
  const int P = A.pool, K = A.k, N = A.n_item, D = A.dim, LD = D + 4;
  const int id = lane < P ? A.pool_idx[(size_t)r * P + lane] : -1;
  const float sc = lane < P ? A.pool_score[(size_t)r * P + lane] : neg_inf();
  const unsigned long long neg = __ballot(id < 0);
  int m = neg ? __ffsll((long long)neg) - 1 : 64;   // the entries before the first -1
  if (__ballot(lane < m && id >= N)) {              // an id outside the table: the row is rejected (all -1), counted once
    if (lane == 0) atomicAdd(A.bad, 1);
    m = 0;
  }
  const bool live = lane < m;
  const int idc = live ? id : 0;
  const int steps = min(K, m);
  const double trade = A.trade, omt = 1.0 - A.trade, g = A.geo_weight, omg = 1.0 - A.geo_weight;
  const bool need_sim = A.trade != 1.0 && steps > 1;          // (wave-uniform)

  double rel = 1.0;
  if (m > 0) {
    const double s0 = (double)__shfl(sc, 0, 64), sl = (double)__shfl(sc, m - 1, 64);
    const double den = s0 - sl;
    rel = den == 0.0 ? 1.0 : ((double)sc - sl) / den;
  }
  double lat = 0.0, lon = 0.0, cp = 0.0, nrm = 0.0;
  if (GEO && need_sim) { lat = A.coords[2 * (size_t)idc]; lon = A.coords[2 * (size_t)idc + 1]; cp = A.cphi[idc]; }
  // one order per dim: four interleaved chains over the float4 columns, closed pairwise (pair_sim.h)
  auto dot_rows = [&](int a, int b) { return dot_rows_f64(s_x + a * LD, s_x + b * LD, D); };
  if (EMB && need_sim) {
    // 16 lanes per row, four rows at a time
    const int grp = lane >> 4, gl = lane & 15;
    for (int t = 0; t < 16; ++t) {
      const int p = 4 * t + grp;
      const int pid = __shfl(idc, p, 64);
      for (int c = gl * 4; c < D; c += 64)
        *reinterpret_cast<float4*>(s_x + p * LD + c) = p < m ? ld4t(A.items, (size_t)pid * D + c, A.items_f16) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    wave_fence();
    nrm = sqrt(dot_rows(lane, lane));
  }

  double pen = 0.0;
  bool taken = false;
  int o_id = -1, o_pos = -1;
  float o_sc = neg_inf();
  double o_obj = -__builtin_huge_val();
  for (int t = 0; t < steps; ++t) {
    const double obj = trade * rel - omt * pen;     // (pen is 0 before the first pick: trade rel_0)
    int win = 0;
    if (t > 0) {
      // (objective, position) arg-max; a NaN objective ranks with -inf, a dead lane behind every live one
      const bool in = live && !taken;
      double bk = (in && obj == obj) ? obj : -__builtin_huge_val();
      int bp = in ? lane : 64 + lane;
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const double ok = __shfl_xor(bk, o, 64);
        const int op = __shfl_xor(bp, o, 64);
        if (ok > bk || (ok == bk && op < bp)) { bk = ok; bp = op; }
      }
      win = __builtin_amdgcn_readfirstlane(bp);
    }
    const double wobj = __shfl(obj, win, 64);
    const int wid = __shfl(id, win, 64);
    const float wsc = __shfl(sc, win, 64);
    if (lane == t) { o_id = wid; o_pos = win; o_sc = wsc; o_obj = wobj; }
    if (lane == win) taken = true;
    if (need_sim && t + 1 < steps) {
      double sim = 0.0, e = 0.0;
      if (GEO) {
        const double wlat = __shfl(lat, win, 64), wlon = __shfl(lon, win, 64), wcp = __shfl(cp, win, 64);
        sim = geo_part(g, sin2_dist_km(lat, lon, cp, wlat, wlon, wcp), A.scale_km);
      }
      if (EMB) {
        const double wn = __shfl(nrm, win, 64);
        const double dt = dot_rows(lane, win);
        e = (nrm == 0.0 || wn == 0.0) ? 0.0 : dt / (nrm * wn);
      }
      sim = sim_mix<GEO, EMB>(sim, omg, e);
      pen = t == 0 ? sim : fmax(pen, sim);
    }
  }
  if (lane < K) {
    const size_t at = (size_t)r * K + lane;
    A.idx_out[at] = o_id;
    if (A.score_out) A.score_out[at] = o_sc;
    if (A.pos_out) A.pos_out[at] = o_pos;
    if (A.obj_out) A.obj_out[at] = o_obj;
  }
}

template <bool GEO>
static hipError_t launch_pool_g(const DiverseArgs& A, hipStream_t st) {
  return by_dim<64>(A.dim, [&](auto d8, auto db) -> hipError_t {
    constexpr auto kernel = &diverse_pool_kernel<decltype(d8)::value, decltype(db)::value, GEO>;
    const hipError_t oe = lds_opt_in<kernel>(POOL_LISTS_BYTES + (int)sizeof(double) * DIVERSE_NDIST_MAX);
    if (oe != hipSuccess) return oe;
    const unsigned n_utile = (unsigned)((A.n + 31) / 32);
    const size_t lds = POOL_LISTS_BYTES + (GEO ? sizeof(double) * A.n_dist : 0);
    hipLaunchKernelGGL(kernel, dim3(n_utile * (unsigned)A.n_split), dim3(POI_BLOCK), lds, st, A);
    return hipGetLastError();
  });
}

hipError_t launch_diverse_pool(DiverseArgs& A, hipStream_t st, Timing* tm) {
  if (A.wd && A.n_dist > DIVERSE_NDIST_MAX) return hipErrorInvalidValue;
  Timing::Scope rec(tm, "diverse_pool", st);
  const hipError_t e = A.wd ? launch_pool_g<true>(A, st) : launch_pool_g<false>(A, st);
  if (e != hipSuccess) return e;
  if (A.part_s) launch_topk_slices_merge(slice_lists(A), DIVERSE_POOL_MAX, A.n, st);
  return rec.close();
}

template <bool GEO, bool EMB>
static hipError_t launch_rerank_t(const RerankArgs& A, hipStream_t st) {
  const hipError_t oe = lds_opt_in<&diverse_rerank_kernel<GEO, EMB>>(RERANK_LDS_MAX);
  if (oe != hipSuccess) return oe;
  const size_t lds = EMB ? sizeof(float) * DIVERSE_POOL_MAX * (size_t)(A.dim + 4) : 0;
  hipLaunchKernelGGL((diverse_rerank_kernel<GEO, EMB>), dim3((unsigned)A.n), dim3(64), lds, st, A);
  return hipGetLastError();
}

hipError_t launch_diverse_rerank(const RerankArgs& A, hipStream_t st, Timing* tm) {
  if (A.dim > 256 && A.geo_weight < 1.0) return hipErrorInvalidValue;
  const bool geo = A.geo_weight > 0.0, emb = A.geo_weight < 1.0;
  tm->begin("diverse_rerank", st);
  const hipError_t e = geo ? (emb ? launch_rerank_t<true, true>(A, st) : launch_rerank_t<true, false>(A, st)) : launch_rerank_t<false, true>(A, st);
  tm->end(st);
  return e;
}

}  // namespace poi
