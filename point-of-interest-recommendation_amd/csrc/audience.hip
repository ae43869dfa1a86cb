// Audience recommendation (poi_score_audience, poi_audience_rows): given a POI, which users?  The top-K candidate ROWS of each query POI
// by the score every other serving kernel computes, without the (n, n_item) score matrix read down a column.
//
//   s(u, j)  = poi_score_rows' s(u, j): users[u] . items[j] from tile_product (tile_product.h: user fragment a, item fragment b), plus
//              wd * sts[u][bin(last_poi[u], j)] for a row with a last POI
//   C(q)     = [0, n) minus the query's exclusion list (ascending row indices);  the list is C(q) by descending s, ties by ascending row.
//
// audience_kernel is the tile walk of tile_walk.h with the axes swapped (wave_tile_range over the USER tiles).  A workgroup owns a block
// of 32 query POIs and one slice of the user range;
// its four waves take a quarter of the slice each.  The queries' item rows are gathered once (b fragments in registers, a half table
// through items_f16), their coordinates and cos(lat) too; the 32-row user tiles stream past as the a fragments.  In tile_product's
// accumulator a lane then holds 16 user rows of ITS OWN query (item = lane & 31): a query's 32 candidates of a tile sit in the registers
// of lanes q and q + 32.  Every score is compared with the query's K-th entry, kept in a register; one ballot decides whether the tile
// offers anything (the common tile offers nothing).  A tile that does goes through LDS, transposed: per query with an offer, lane l
// holds user row l and list_take<32> (topk_list.h) inserts into the wave's sorted 32-entry LDS list of that query (32 queries x 32
// entries x 8 B = 8 KB per wave).  Exclusion: lane q < 32 walks query q's ascending list with one cursor, a tile that holds listed rows
// gets a 32-bit mask per query through LDS - rank_kernel's mechanism along the other axis.  The distance term's row side is the streamed
// side: last_poi[u], then that POI's coordinates - a dependent gather per user tile, requested a tile (the id: two tiles) ahead of the
// product that needs it and parked in LDS after the epilogue of the tile before.  The user tile itself: two register buffers up to
// dim 64; beyond, one buffer whose next tile is requested right behind the product, in front of the epilogue.
// The waves' lists meet in LDS (block_lists_fold); with slices they go to per-slice partial lists that topk_slices_merge_kernel folds.
// The order is total and a pair's score does not depend on the slice, the wave, the block or the query's place in it: every grid gives
// the same bits.  No float atomics; a rejected query is counted with one integer atomic.
//
// ROWS: the same walk with a store epilogue - the tile goes through LDS so that a query's 32 consecutive rows leave as one 128-byte
// segment of scores_out[q * ld + u].
//
// Bytes: per query block the slice of the user table once (4 dim n), + 28 n (last_poi, coordinates, cos(lat)) and the sts gathers with
// the distance term; flops 2 * 32 * n * dim per query block on the f32 matrix pipe.
#include "poi_common.h"
#include "poi_kernels.h"
#include "launch_common.h"
#include "tile_walk.h"
#include "topk_list.h"
#include <limits.h>

namespace poi {

namespace {
constexpr int AUD_LD = 33;                  // row stride of the LDS score tile: rows and columns both fall on 32 different banks
constexpr int Q_REJECTED = -1, Q_NONE = -2; // s_q: a query that was rejected; a position of the block behind the call's last query
}  // namespace

template <int D8, bool DB, bool GEO, bool ROWS>
__global__ __launch_bounds__(POI_BLOCK) void audience_kernel(AudienceArgs A) {
  __shared__ float l_s[POI_NWAVE][32][AUDIENCE_K_MAX];
  __shared__ int l_i[POI_NWAVE][32][AUDIENCE_K_MAX];
  __shared__ float s_sc[POI_NWAVE][32 * AUD_LD];
  __shared__ unsigned s_exm[POI_NWAVE][32];
  __shared__ int s_q[32], s_e0[32], s_e1[32];       // the query's POI (or Q_REJECTED / Q_NONE), its exclusion list
  __shared__ int s_has[POI_NWAVE][32];              // per wave: has the tile's row a last POI; its latitude, longitude, cos(latitude)
  __shared__ double s_ulat[POI_NWAVE][32], s_ulon[POI_NWAVE][32], s_ucp[POI_NWAVE][32];
  extern __shared__ __align__(16) double s_thr[];   // GEO: thr[n_dist]
  const int tid = threadIdx.x, lane = lane_id(), w = wave_id(), li = lane & 31, h = lane >> 5;
  const int S = A.n_split, qb = blockIdx.x / S, sl = blockIdx.x - qb * S;
  const int D = A.dim, n = A.n, K = A.k;

  // the block's queries: the POI inside [0, n_item), the list's offsets in order and its rows ascending inside [0, n)
  for (int i = w; i < 32; i += POI_NWAVE) {         // (wave-uniform)
    const int q = qb * 32 + i;
    int poi = Q_NONE, e0 = 0, e1 = 0;
    if (q < A.n_q) {
      poi = A.pois[q];
      int bad = (unsigned)poi >= (unsigned)A.n_item;
      if (!ROWS && A.ex) bad |= check_ex_row(A.ex_off, A.ex, q, n, lane, e0, e1);
      if (__any(bad)) { poi = Q_REJECTED; e0 = 0; e1 = 0; }
    }
    if (lane == 0) {
      s_q[i] = poi; s_e0[i] = e0; s_e1[i] = e1;
      if (poi == Q_REJECTED && sl == 0) atomicAdd(A.bad, 1);
    }
  }
  if (!ROWS) {                                      // (every wave clears its own 32 lists)
    for (int e = lane; e < 32 * AUDIENCE_K_MAX; e += 64) { (&l_s[w][0][0])[e] = neg_inf(); (&l_i[w][0][0])[e] = PAD_ID; }
  }
  if (GEO)
    for (int i = tid; i < A.n_dist; i += POI_BLOCK) s_thr[i] = A.thr[i];
  __syncthreads();

  int ntile, tb, te;
  wave_tile_range(n, sl, S, w, ntile, tb, te);
  const float wd = GEO ? A.wd[0] : 0.f;
  const int myq = s_q[li];
  const bool qlive = myq >= 0;

  if (tb < te) {                                    // (wave-uniform; a wave without tiles keeps its empty lists)
    float4 bf[D8];
    load_frag<D8>(bf, A.items, A.items_f16, (size_t)max(myq, 0), D, h);
    double jlat = 0.0, jlon = 0.0, jcp = 0.0;
    if (GEO) { const int jc = max(myq, 0); jlat = A.coords[2 * (size_t)jc]; jlon = A.coords[2 * (size_t)jc + 1]; jcp = A.cphi[jc]; }

    // lane q < 32: cursor into query q's exclusion list, at the first row of this wave's range
    int xpos = 0, xend = 0, xnext = INT_MAX;
    if (!ROWS && A.ex && lane < 32 && s_e1[lane] > s_e0[lane]) {
      int a = s_e0[lane], b = s_e1[lane];
      const int first = tb * 32;
      while (a < b) { const int md = (a + b) >> 1; if (A.ex[md] < first) a = md + 1; else b = md; }
      xpos = a; xend = s_e1[lane];
      if (xpos < xend) xnext = A.ex[xpos];
    }
    bool exdirty = false;
    if (lane < 32) s_exm[w][lane] = 0u;

    // the distance term's row side: row li of tile t has last POI row_lp(t); its coordinates are fetched one tile ahead, the id two
    auto row_lp = [&](int t) { const int u = t * 32 + li; return (t < te && u < n) ? A.last_poi[u] : -1; };
    int lp_n = -1;
    if (GEO) {
      const int lp = row_lp(tb);
      const int lc = min(max(lp, 0), A.n_item - 1);                      // (an id outside the table reads no memory outside it)
      if (lane < 32) { s_has[w][lane] = lp >= 0; s_ulat[w][lane] = A.coords[2 * (size_t)lc]; s_ulon[w][lane] = A.coords[2 * (size_t)lc + 1]; s_ucp[w][lane] = A.cphi[lc]; }
      lp_n = row_lp(tb + 1);
    }
    wave_fence();

    float ths = neg_inf();                          // the K-th entry of this lane's query in this wave's list
    int thi = PAD_ID;
    float4 a0[D8], a1[DB ? D8 : 1];
    load_frag<D8>(a0, A.users, 0, (size_t)min(tb * 32 + li, n - 1), D, h);

    for (int tile = tb; tile < te; ++tile) {
      if constexpr (DB) { if (tile + 1 < te) load_frag<D8>(a1, A.users, 0, (size_t)min((tile + 1) * 32 + li, n - 1), D, h); }
      int n_has = 0, lp_n2 = -1;
      double n_lat = 0.0, n_lon = 0.0, n_cp = 0.0;
      if (GEO) {                                    // (requested here, parked in LDS behind this tile's epilogue)
        const int lc = min(max(lp_n, 0), A.n_item - 1);
        n_has = lp_n >= 0;
        n_lat = A.coords[2 * (size_t)lc]; n_lon = A.coords[2 * (size_t)lc + 1]; n_cp = A.cphi[lc];
        lp_n2 = row_lp(tile + 2);
      }
      // (tile_walk.h: the walk's contract - not met here, the mask branch stands behind the product: DESIGN.md section 1)
      const f32x16 acc = tile_product<D8>(a0, bf);
      // one buffer: the next tile's rows are requested as soon as the product has read this tile's, behind them the whole epilogue
      if constexpr (!DB) { if (tile + 1 < te) load_frag<D8>(a0, A.users, 0, (size_t)min((tile + 1) * 32 + li, n - 1), D, h); }
      unsigned xm = 0u;
      if (!ROWS && A.ex) {
        // listed rows of this tile -> one 32-bit mask per query
        const bool anyex = __any(xnext < tile * 32 + 32);
        if (anyex || exdirty) {                     // (wave-uniform; a tile without listed rows after one with some clears the masks)
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
        xm = s_exm[w][li];
      }
      float sv[16];
      unsigned cm = 0u;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int ul = acc_tile_row(r, 4 * h), u = tile * 32 + ul;
        float s = acc[r];
        if (GEO) {
          if (s_has[w][ul]) s = __fmaf_rn(wd, geo_prob(A, s_thr, u, s_ulat[w][ul], s_ulon[w][ul], s_ucp[w][ul], jlat, jlon, jcp), s);
        }
        if (!ROWS) {
          const bool live = qlive && u < n && !((xm >> ul) & 1u);
          s = live ? s : quiet_nan();               // compares false with everything: never offered
          cm |= better(s, u, ths, thi) ? 1u << r : 0u;
        }
        sv[r] = s;
        if (GEO) __builtin_amdgcn_sched_barrier(0); // one row's distance term in flight at a time
      }
      if (ROWS) {
#pragma unroll
        for (int r = 0; r < 16; ++r) s_sc[w][acc_tile_row(r, 4 * h) * AUD_LD + li] = sv[r];
        wave_fence();
        const int u = tile * 32 + li;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const int q = 2 * i + h, poi = s_q[q];
          if (poi != Q_NONE && u < n) A.rows_out[(size_t)(qb * 32 + q) * (size_t)A.ld + u] = poi >= 0 ? s_sc[w][li * AUD_LD + q] : neg_inf();
        }
        wave_fence();                               // the tile is read before the next one overwrites it
      } else {
        const unsigned long long offers = __ballot(cm != 0u);
        if (offers) {                               // (wave-uniform; rare once the lists have warmed up)
#pragma unroll
          for (int r = 0; r < 16; ++r) s_sc[w][acc_tile_row(r, 4 * h) * AUD_LD + li] = sv[r];
          wave_fence();
          unsigned qs = (unsigned)(offers | (offers >> 32));
          const int u = tile * 32 + li;
          while (qs) {
            const int q = __ffs(qs) - 1;
            qs &= qs - 1u;
            float* ls = l_s[w][q];
            int* lx = l_i[w][q];
            const float v = s_sc[w][li * AUD_LD + q];
            const bool cand = h == 0 && better(v, u, ls[K - 1], lx[K - 1]);
            const unsigned long long bal = __ballot(cand);
            if (bal) list_take<AUDIENCE_K_MAX>(ls, lx, bal, cand, v, u, K);
          }
          wave_fence();
          ths = l_s[w][li][K - 1]; thi = l_i[w][li][K - 1];
          wave_fence();                             // the tile is read before the next one overwrites it
        }
      }
      if (GEO) {
        wave_fence();                               // this tile's rows are read before the next tile's replace them
        if (lane < 32) { s_has[w][lane] = n_has; s_ulat[w][lane] = n_lat; s_ulon[w][lane] = n_lon; s_ucp[w][lane] = n_cp; }
        wave_fence();
        lp_n = lp_n2;
      }
      if constexpr (DB) {
#pragma unroll
        for (int m = 0; m < D8; ++m) a0[m] = a1[m];
      }
    }
  }
  if (ROWS) return;

  __syncthreads();
  for (int i = w; i < 32; i += POI_NWAVE) {         // (wave-uniform) the four waves' lists of query i -> its best 32
    const int q = qb * 32 + i;
    if (q >= A.n_q) break;
    float as;
    int ai;
    block_lists_fold<AUDIENCE_K_MAX>(&l_s[0][i][0], &l_i[0][i][0], 32 * AUDIENCE_K_MAX, as, ai);
    const int cnt = (s_q[i] >= 0 && sl == 0) ? n - (s_e1[i] - s_e0[i]) : 0;
    list_emit<AUDIENCE_K_MAX>(A, A.part_s != nullptr, q, sl, as, ai, cnt);
  }
}

template <bool GEO, bool ROWS>
static hipError_t launch_audience_g(const AudienceArgs& A, hipStream_t st) {
  return by_dim<64>(A.dim, [&](auto d8, auto db) -> hipError_t {
    const unsigned n_qblock = (unsigned)((A.n_q + 31) / 32);
    const size_t lds = GEO ? sizeof(double) * A.n_dist : 0;
    hipLaunchKernelGGL((audience_kernel<decltype(d8)::value, decltype(db)::value, GEO, ROWS>), dim3(n_qblock * (unsigned)A.n_split), dim3(POI_BLOCK), lds, st, A);
    return hipSuccess;
  });
}

hipError_t launch_audience(const AudienceArgs& A, hipStream_t st, Timing* tm) {
  const long span = tm->span_begin("score_audience", st);      // the call; inside it the walk and (split regime) the merge on their own
  tm->begin("audience_walk", st);
  const hipError_t e = A.wd ? launch_audience_g<true, false>(A, st) : launch_audience_g<false, false>(A, st);
  tm->end(st);
  if (e != hipSuccess) { tm->span_end(span, st); return e; }
  if (A.part_s) {
    tm->begin("audience_merge", st);
    launch_topk_slices_merge(slice_lists(A), AUDIENCE_K_MAX, A.n_q, st);
    tm->end(st);
  }
  tm->span_end(span, st);
  return hipGetLastError();
}

hipError_t launch_audience_rows(const AudienceArgs& A, hipStream_t st, Timing* tm) {
  Timing::Scope rec(tm, "audience_rows", st);
  const hipError_t e = A.wd ? launch_audience_g<true, true>(A, st) : launch_audience_g<false, true>(A, st);
  if (e != hipSuccess) return e;
  return rec.close();
}

}  // namespace poi
