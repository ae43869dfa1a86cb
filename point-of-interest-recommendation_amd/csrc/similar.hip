// Similar rows (poi_row_inv_norms, poi_similar_topk, poi_similar_rows, poi_similar_nearest): "places like this one", "users like this
// one", and "because you visited X".  The top-K rows of ONE table x (n, dim) most similar to each query row, without an (n, n) matrix
// and without a normalised copy of the table.
//
//   inv[i]   = 1 / sqrt(x_i . x_i) in float64 (pair_sim.h's summation order), 0 for a zero row
//   emb(i,j) = (double)dot32(i, j) * (inv[i] * inv[j]);  dot32 = tile_product's float32 product (the bits of poi_score_rows)
//   geo(i,j) = exp(-d(i, j) / scale_km), d the sin^2 Haversine distance of poi_diverse_rerank (pair_sim.h)
//   sim(i,j) = (float)(g geo + (1 - g) emb), formed in float64 without contraction, rounded once; -0.0 is written as +0.0
//   C(q)     = [0, n) minus the query's own row minus its exclusion list;  the list is C(q) by descending sim, ties by ascending row.
//
// similar_kernel is the tile walk of tile_walk.h along the streamed rows (wave_tile_range, acc_tile_row), as in audience.hip, with the
// table on both sides.  A workgroup owns a block of 32 query rows and one slice of the
// row range; its four waves take a quarter of the slice each.  The queries' fragments, inv, coordinates and cos(lat) stay in registers;
// the 32-row tiles of the same table stream past as the a fragments.  In tile_product's accumulator a lane holds 16 streamed rows of
// ITS OWN query (lane & 31).  The streamed rows' inv and coordinates are direct loads by tile (no dependent gather), requested a tile
// ahead of the product that needs them and parked in LDS behind the epilogue of the tile before.  The float64 epilogue runs per
// accumulator entry, one row's transcendental chain in flight at a time.  With the geographic part a pair whose bound g + (1 - g) emb
// (geo <= 1, every step rounds monotonically) does not beat the K-th entry of its query's list cannot enter it: its distance is not
// evaluated - the listed bits are the same.  (Never with the store epilogue.)  The float32 result is compared with the query's K-th
// entry, kept in a register; a tile that offers something goes through LDS, transposed, into the wave's sorted 32-entry lists
// (list_take<32>); exclusion is audience_kernel's cursor, the query's own row a compare of the row index.  The waves' lists meet in
// LDS (block_lists_fold); with slices they go to partial lists that topk_slices_merge_kernel folds.  The order is total and a pair's
// similarity does not depend on the slice, the wave, the block or the query's place in it: every grid gives the same bits.
//
// ROWS: the same walk with a store epilogue - rows_out[q * ld + j] = sim(queries[q], j), -inf at the query's own column and in the row
// of a rejected query.
//
// similar_nearest_kernel: one wave per row, lane i owns entry i of the row's list (k <= 32) with a running (best similarity, position).
// The list's item rows are staged once in LDS as float32 (32 rows, row stride dim + 4 floats, as the re-rank stages its pool); the
// history rows stream through one more LDS row, the next one requested while this one is compared.  Everything in float64, the
// formulas of poi_diverse_rerank to the operation (pair_sim.h).
//
// Bytes: per query block the slice of the table once (4 dim n, half of it on a half table) + 8 n (inv), + 24 n with the geographic part;
// flops 2 * 32 * n * dim per query block on the f32 matrix pipe, + the float64 epilogue per pair.
#include "poi_common.h"
#include "poi_kernels.h"
#include "pair_sim.h"
#include "launch_common.h"
#include "tile_walk.h"
#include "topk_list.h"
#include <limits.h>

namespace poi {

namespace {
constexpr int SIM_LD = 33;                  // row stride of the LDS score tile: rows and columns both fall on 32 different banks
constexpr int Q_REJECTED = -1, Q_NONE = -2; // s_q: a query that was rejected; a position of the block behind the call's last query
constexpr int NORM_COLS = 64;               // columns the norm prepass stages at a time
constexpr int NORM_LD = NORM_COLS + 4;
constexpr int NEAREST_ROWS = 32;            // list entries (item rows staged) of the nearest-visited kernel
}  // namespace

// one wave per 64 rows: the rows' columns go through LDS 64 at a time (coalesced loads), lane l sums row l in dot_rows_f64's order
__global__ __launch_bounds__(64) void row_inv_norms_kernel(const void* x, int f16, int n, int D, double* inv) {
#pragma clang fp contract(off)
  __shared__ __align__(16) float s_x[64 * NORM_LD];
  const int lane = lane_id(), grp = lane >> 4, gl = lane & 15;
  const int r0 = blockIdx.x * 64;
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
  for (int c0 = 0; c0 < D; c0 += NORM_COLS) {
    const int cw = min(NORM_COLS, D - c0);
    for (int t = 0; t < 16; ++t) {                  // 16 lanes per row, four rows at a time
      const int p = 4 * t + grp;
      const int row = min(r0 + p, n - 1);
      if (gl * 4 < cw) *reinterpret_cast<float4*>(s_x + p * NORM_LD + gl * 4) = ld4t(x, (size_t)row * D + c0 + gl * 4, f16);
    }
    wave_fence();
    const float* xr = s_x + lane * NORM_LD;
    for (int c = 0; c < cw; c += 4) {
      const float4 u = *reinterpret_cast<const float4*>(xr + c);
      a0 = fma((double)u.x, (double)u.x, a0); a1 = fma((double)u.y, (double)u.y, a1);
      a2 = fma((double)u.z, (double)u.z, a2); a3 = fma((double)u.w, (double)u.w, a3);
    }
    wave_fence();                                   // the chunk is read before the next one overwrites it
  }
  const double s = (a0 + a1) + (a2 + a3);
  if (r0 + lane < n) inv[r0 + lane] = s == 0.0 ? 0.0 : 1.0 / sqrt(s);
}

template <int D8, bool DB, bool GEO, bool ROWS>
__global__ __launch_bounds__(POI_BLOCK) void similar_kernel(SimilarArgs A) {
#pragma clang fp contract(off)
  __shared__ float l_s[POI_NWAVE][32][SIMILAR_K_MAX];
  __shared__ int l_i[POI_NWAVE][32][SIMILAR_K_MAX];
  __shared__ float s_sc[POI_NWAVE][32 * SIM_LD];
  __shared__ unsigned s_exm[POI_NWAVE][32];
  __shared__ int s_q[32], s_e0[32], s_e1[32], s_self[32];      // the query's row (or Q_REJECTED / Q_NONE), its exclusion list, is it on that list
  __shared__ double s_uinv[POI_NWAVE][32];                     // per wave: the tile's rows' inv; their latitude, longitude, cos(latitude)
  __shared__ double s_ulat[GEO ? POI_NWAVE : 1][32], s_ulon[GEO ? POI_NWAVE : 1][32], s_ucp[GEO ? POI_NWAVE : 1][32];
  const int lane = lane_id(), w = wave_id(), li = lane & 31, h = lane >> 5;
  const int S = A.n_split, qb = blockIdx.x / S, sl = blockIdx.x - qb * S;
  const int D = A.dim, n = A.n, K = A.k;

  // the block's queries: the row inside [0, n), the list's offsets in order and its rows ascending inside [0, n)
  for (int i = w; i < 32; i += POI_NWAVE) {         // (wave-uniform)
    const int q = qb * 32 + i;
    int id = Q_NONE, e0 = 0, e1 = 0, self = 0;
    if (q < A.n_q) {
      id = A.queries[q];
      int bad = (unsigned)id >= (unsigned)n;
      if (!ROWS && A.ex) bad |= check_ex_row(A.ex_off, A.ex, q, n, lane, e0, e1);
      if (__any(bad)) { id = Q_REJECTED; e0 = 0; e1 = 0; }
      else if (!ROWS && A.ex && lane == 0) self = listed(A.ex, e0, e1, id);      // (a list that names the query is not subtracted twice)
    }
    if (lane == 0) {
      s_q[i] = id; s_e0[i] = e0; s_e1[i] = e1; s_self[i] = self;
      if (id == Q_REJECTED && sl == 0 && A.count_bad) atomicAdd(A.bad, 1);
    }
  }
  if (!ROWS) {                                      // (every wave clears its own 32 lists)
    for (int e = lane; e < 32 * SIMILAR_K_MAX; e += 64) { (&l_s[w][0][0])[e] = neg_inf(); (&l_i[w][0][0])[e] = PAD_ID; }
  }
  __syncthreads();

  int ntile, tb, te;
  wave_tile_range(n, sl, S, w, ntile, tb, te);
  const int myq = s_q[li];
  const bool qlive = myq >= 0;
  const double g = A.g, omg = A.omg, scale_km = A.scale_km;

  if (tb < te) {                                    // (wave-uniform; a wave without tiles keeps its empty lists)
    const int qc = max(myq, 0);
    float4 bf[D8];
    load_frag<D8>(bf, A.x, A.x_f16, (size_t)qc, D, h);
    const double qinv = A.inv[qc];
    double qlat = 0.0, qlon = 0.0, qcp = 0.0;
    if (GEO) { qlat = A.coords[2 * (size_t)qc]; qlon = A.coords[2 * (size_t)qc + 1]; qcp = A.cphi[qc]; }

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

    // the streamed side's inv and coordinates: row li of tile t, direct loads, requested one tile ahead
    {
      const size_t u = (size_t)min(tb * 32 + li, n - 1);
      if (lane < 32) {
        s_uinv[w][lane] = A.inv[u];
        if (GEO) { s_ulat[w][lane] = A.coords[2 * u]; s_ulon[w][lane] = A.coords[2 * u + 1]; s_ucp[w][lane] = A.cphi[u]; }
      }
    }
    wave_fence();

    float ths = neg_inf();                          // the K-th entry of this lane's query in this wave's list
    int thi = PAD_ID;
    float4 a0[D8], a1[DB ? D8 : 1];
    load_frag<D8>(a0, A.x, A.x_f16, (size_t)min(tb * 32 + li, n - 1), D, h);

    for (int tile = tb; tile < te; ++tile) {
      if constexpr (DB) { if (tile + 1 < te) load_frag<D8>(a1, A.x, A.x_f16, (size_t)min((tile + 1) * 32 + li, n - 1), D, h); }
      double n_inv = 0.0, n_lat = 0.0, n_lon = 0.0, n_cp = 0.0;
      if (tile + 1 < te) {                          // (requested here, parked in LDS behind this tile's epilogue)
        const size_t u = (size_t)min((tile + 1) * 32 + li, n - 1);
        n_inv = A.inv[u];
        if (GEO) { n_lat = A.coords[2 * u]; n_lon = A.coords[2 * u + 1]; n_cp = A.cphi[u]; }
      }
      // (tile_walk.h: the walk's contract - not met here, the mask branch stands behind the product: DESIGN.md section 1)
      const f32x16 acc = tile_product<D8>(a0, bf);
      // one buffer: the next tile's rows are requested as soon as the product has read this tile's, behind them the whole epilogue
      if constexpr (!DB) { if (tile + 1 < te) load_frag<D8>(a0, A.x, A.x_f16, (size_t)min((tile + 1) * 32 + li, n - 1), D, h); }
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
        const double e = (double)acc[r] * (s_uinv[w][ul] * qinv);
        const bool live = ROWS || (qlive && u < n && u != myq && !((xm >> ul) & 1u));
        float s = quiet_nan();                      // compares false with everything: never offered
        if (GEO) {
          bool need = live;
          if (!ROWS && live) need = better((float)(g + omg * e) + 0.f, u, ths, thi);      // geo <= 1: the pair cannot do better than this
          if (need) {
            const double d = sin2_dist_km(s_ulat[w][ul], s_ulon[w][ul], s_ucp[w][ul], qlat, qlon, qcp);
            s = (float)sim_mix<true, true>(geo_part(g, d, scale_km), omg, e) + 0.f;
          }
        } else {
          if (live) s = (float)sim_mix<false, true>(0.0, omg, e) + 0.f;
        }
        if (!ROWS) cm |= better(s, u, ths, thi) ? 1u << r : 0u;
        sv[r] = s;
        if (GEO) __builtin_amdgcn_sched_barrier(0); // one row's transcendental chain in flight at a time
      }
      if (ROWS) {
#pragma unroll
        for (int r = 0; r < 16; ++r) s_sc[w][acc_tile_row(r, 4 * h) * SIM_LD + li] = sv[r];
        wave_fence();
        const int u = tile * 32 + li;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const int q = 2 * i + h, id = s_q[q];
          if (id != Q_NONE && u < n) A.rows_out[(size_t)(qb * 32 + q) * (size_t)A.ld + u] = (id >= 0 && u != id) ? s_sc[w][li * SIM_LD + q] : neg_inf();
        }
        wave_fence();                               // the tile is read before the next one overwrites it
      } else {
        const unsigned long long offers = __ballot(cm != 0u);
        if (offers) {                               // (wave-uniform; rare once the lists have warmed up)
#pragma unroll
          for (int r = 0; r < 16; ++r) s_sc[w][acc_tile_row(r, 4 * h) * SIM_LD + li] = sv[r];
          wave_fence();
          unsigned qs = (unsigned)(offers | (offers >> 32));
          const int u = tile * 32 + li;
          while (qs) {
            const int q = __ffs(qs) - 1;
            qs &= qs - 1u;
            float* ls = l_s[w][q];
            int* lx = l_i[w][q];
            const float v = s_sc[w][li * SIM_LD + q];
            const bool cand = h == 0 && better(v, u, ls[K - 1], lx[K - 1]);
            const unsigned long long bal = __ballot(cand);
            if (bal) list_take<SIMILAR_K_MAX>(ls, lx, bal, cand, v, u, K);
          }
          wave_fence();
          ths = l_s[w][li][K - 1]; thi = l_i[w][li][K - 1];
          wave_fence();                             // the tile is read before the next one overwrites it
        }
      }
      wave_fence();                                 // this tile's rows are read before the next tile's replace them
      if (lane < 32) {
        s_uinv[w][lane] = n_inv;
        if (GEO) { s_ulat[w][lane] = n_lat; s_ulon[w][lane] = n_lon; s_ucp[w][lane] = n_cp; }
      }
      wave_fence();
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
    block_lists_fold<SIMILAR_K_MAX>(&l_s[0][i][0], &l_i[0][i][0], 32 * SIMILAR_K_MAX, as, ai);
    const int cnt = (s_q[i] >= 0 && sl == 0) ? n - 1 - (s_e1[i] - s_e0[i]) + s_self[i] : 0;
    list_emit<SIMILAR_K_MAX>(A, A.part_s != nullptr, q, sl, as, ai, cnt);
  }
}

// after poi_topk_select over the score rows (the rows + select route): the selection counted [0, n) minus the list - the query's own
// row leaves the count unless the list named it; a query outside [0, n) lists nothing (its row is -inf), counts 0 and is counted once
// (the selection has counted a broken list already)
__global__ __launch_bounds__(64) void similar_fix_counts_kernel(SimilarArgs A) {
  const int q = blockIdx.x, lane = lane_id();
  const int id = A.queries[q];
  const bool idbad = (unsigned)id >= (unsigned)A.n;
  int e0 = 0, e1 = 0, lbad = 0;
  if (A.ex) lbad = __any(check_ex_row(A.ex_off, A.ex, q, A.n, lane, e0, e1)) ? 1 : 0;
  if (lane != 0) return;
  if (idbad) {
    if (!lbad) atomicAdd(A.bad, 1);
    if (A.count_out) A.count_out[q] = 0;
  } else if (!lbad && A.count_out) {
    const int self = A.ex ? (int)listed(A.ex, e0, e1, id) : 0;
    A.count_out[q] -= 1 - self;
  }
}

template <bool GEO, bool EMB>
__global__ __launch_bounds__(64) void similar_nearest_kernel(NearestArgs A) {
#pragma clang fp contract(off)
  extern __shared__ __align__(16) float s_x[];      // EMB: the list's item rows, 32 x (dim + 4), then the history row
  const int r = blockIdx.x, lane = lane_id();
  const int K = A.k, N = A.n_item, D = A.dim, LD = D + 4;
  float* const s_h = s_x + NEAREST_ROWS * LD;
  const int id = lane < K ? A.lists[(size_t)r * K + lane] : -1;
  const int h0 = A.h_off[r];
  int h1 = A.h_off[r + 1];
  // a listed id outside [-1, n_item), offsets out of order or a history id outside the table: the row is rejected, counted once
  bool rej = __any(id < -1 || id >= N) || h0 < 0 || h1 < h0;      // (wave-uniform)
  if (!rej) {
    int bad = 0;
    for (int p = h0 + lane; p < h1; p += 64) bad |= (unsigned)A.h_ids[p] >= (unsigned)N;
    rej = __any(bad);
  }
  if (rej) {
    if (lane == 0) atomicAdd(A.bad, 1);
    h1 = h0;
  }
  const bool live = !rej && id >= 0;
  const int idc = live ? id : 0;
  const double g = A.geo_weight, omg = 1.0 - A.geo_weight;
  double lat = 0.0, lon = 0.0, cp = 0.0, nrm = 0.0;
  const int lr = min(lane, NEAREST_ROWS - 1);       // (the lanes behind the list read its last row and keep nothing)
  if (h0 < h1) {                                    // (wave-uniform)
    if (GEO) { lat = A.coords[2 * (size_t)idc]; lon = A.coords[2 * (size_t)idc + 1]; cp = A.cphi[idc]; }
    if (EMB) {
      // 16 lanes per row, four rows at a time
      const int grp = lane >> 4, gl = lane & 15;
      for (int t = 0; t < NEAREST_ROWS / 4; ++t) {
        const int p = 4 * t + grp;
        const int pid = __shfl(idc, p, 64);
        const int pl = __shfl((int)live, p, 64);
        for (int c = gl * 4; c < D; c += 64)
          *reinterpret_cast<float4*>(s_x + p * LD + c) = pl ? ld4t(A.items, (size_t)pid * D + c, A.items_f16) : make_float4(0.f, 0.f, 0.f, 0.f);
      }
      wave_fence();
      nrm = sqrt(dot_rows_f64(s_x + lr * LD, s_x + lr * LD, D));
    }
  }

  double best = -__builtin_huge_val();
  int pos = -1;
  float4 nx = make_float4(0.f, 0.f, 0.f, 0.f);
  int hid = 0;
  if (h0 < h1) {
    hid = A.h_ids[h0];
    if (EMB && lane * 4 < D) nx = ld4t(A.items, (size_t)hid * D + lane * 4, A.items_f16);
  }
  for (int p = h0; p < h1; ++p) {
    const int cur = hid;
    if (EMB) {
      if (lane * 4 < D) *reinterpret_cast<float4*>(s_h + lane * 4) = nx;
      wave_fence();
    }
    if (p + 1 < h1) {                               // the next history row is requested while this one is compared
      hid = A.h_ids[p + 1];
      if (EMB && lane * 4 < D) nx = ld4t(A.items, (size_t)hid * D + lane * 4, A.items_f16);
    }
    double sim = 0.0, e = 0.0;
    if (GEO) {
      const double wlat = A.coords[2 * (size_t)cur], wlon = A.coords[2 * (size_t)cur + 1], wcp = A.cphi[cur];
      sim = geo_part(g, sin2_dist_km(lat, lon, cp, wlat, wlon, wcp), A.scale_km);
    }
    if (EMB) {
      const double wn = sqrt(dot_rows_f64(s_h, s_h, D));
      const double dt = dot_rows_f64(s_x + lr * LD, s_h, D);
      e = (nrm == 0.0 || wn == 0.0) ? 0.0 : dt / (nrm * wn);
    }
    sim = sim_mix<GEO, EMB>(sim, omg, e);
    if (live && sim > best) { best = sim; pos = p - h0; }      // (strict: ties go to the lower position)
    if (EMB) wave_fence();                          // the row is read before the next one replaces it
  }
  if (lane < K) {
    const size_t at = (size_t)r * K + lane;
    A.pos_out[at] = pos;
    if (A.sim_out) A.sim_out[at] = pos >= 0 ? best : -__builtin_huge_val();
  }
}

hipError_t launch_row_inv_norms(const void* x, int x_f16, int n, int dim, double* inv_out, hipStream_t st, Timing* tm) {
  tm->begin("similar_norms", st);
  hipLaunchKernelGGL(row_inv_norms_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, st, x, x_f16, n, dim, inv_out);
  tm->end(st);
  return hipGetLastError();
}

template <bool GEO, bool ROWS>
static hipError_t launch_similar_g(const SimilarArgs& A, hipStream_t st) {
  return by_dim<64>(A.dim, [&](auto d8, auto db) -> hipError_t {
    const unsigned n_qblock = (unsigned)((A.n_q + 31) / 32);
    hipLaunchKernelGGL((similar_kernel<decltype(d8)::value, decltype(db)::value, GEO, ROWS>), dim3(n_qblock * (unsigned)A.n_split), dim3(POI_BLOCK), 0, st, A);
    return hipSuccess;
  });
}

hipError_t launch_similar(const SimilarArgs& A, hipStream_t st, Timing* tm) {
  tm->begin("similar_walk", st);
  const hipError_t e = A.coords ? launch_similar_g<true, false>(A, st) : launch_similar_g<false, false>(A, st);
  tm->end(st);
  if (e != hipSuccess) return e;
  if (A.part_s) {
    tm->begin("similar_merge", st);
    launch_topk_slices_merge(slice_lists(A), SIMILAR_K_MAX, A.n_q, st);
    tm->end(st);
  }
  return hipGetLastError();
}

hipError_t launch_similar_rows(const SimilarArgs& A, hipStream_t st, Timing* tm) {
  Timing::Scope rec(tm, "similar_rows", st);
  const hipError_t e = A.coords ? launch_similar_g<true, true>(A, st) : launch_similar_g<false, true>(A, st);
  if (e != hipSuccess) return e;
  return rec.close();
}

hipError_t launch_similar_fix_counts(const SimilarArgs& A, hipStream_t st) {
  hipLaunchKernelGGL(similar_fix_counts_kernel, dim3((unsigned)A.n_q), dim3(64), 0, st, A);
  return hipGetLastError();
}

template <bool GEO, bool EMB>
static hipError_t launch_nearest_t(const NearestArgs& A, hipStream_t st) {
  const size_t lds = EMB ? sizeof(float) * (NEAREST_ROWS + 1) * (size_t)(A.dim + 4) : 0;
  hipLaunchKernelGGL((similar_nearest_kernel<GEO, EMB>), dim3((unsigned)A.n), dim3(64), lds, st, A);
  return hipGetLastError();
}

hipError_t launch_similar_nearest(const NearestArgs& A, hipStream_t st, Timing* tm) {
  if (A.k > NEAREST_ROWS || (A.dim > 256 && A.geo_weight < 1.0)) return hipErrorInvalidValue;
  const bool geo = A.geo_weight > 0.0, emb = A.geo_weight < 1.0;
  tm->begin("similar_nearest", st);
  const hipError_t e = geo ? (emb ? launch_nearest_t<true, true>(A, st) : launch_nearest_t<true, false>(A, st)) : launch_nearest_t<false, true>(A, st);
  tm->end(st);
  return e;
}

}  // namespace poi
