// GeoIE (prog_geoie.py, public/GeoIE.py, public/Load_Data_GeoIE.py): the batched pairwise geo-influence step, the packed pair distances
// and the user vectors of the scoring.
//
// Step (GeoIE.__theano_train__, GeoIE.py:129-188), for a user with train POIs p_0 .. p_{L-1} and negatives q_0 .. q_{L-1}, rows
// i = 0 .. L-2 (targets P_i = p_{i+1}, Q_i = q_{i+1}) and columns j <= i:
//   dp_ij = f32(cal_dis(p_j, P_i)),  dq_ij = f32(cal_dis(p_j, Q_i)),  d_eff = max(d, d_min),  f(d) = a d_eff^b (float64)
//   x_ij = g[p_j].h[P_i],  y_ij = g[p_j].h[Q_i],  diff_i = (1 / (i + 1)) sum_j (x_ij fp_ij - y_ij fq_ij)   (t[u].z[P_i] cancels)
//   loss = sum_i log sigmoid(diff_i),  c_i = sigmoid(-diff_i) / (i + 1)
//   d cost / d h[P_i] = -c_i sum_j fp_ij g[p_j]      d cost / d h[Q_i] = c_i sum_j fq_ij g[p_j]
//   d cost / d g[p_j] = -sum_{i >= j} c_i (fp_ij h[P_i] - fq_ij h[Q_i])
//   d cost / d a = -sum_i c_i sum_j (x_ij dp^b - y_ij dq^b)      d cost / d b = -sum_i c_i sum_j a (x_ij dp^b ln dp - y_ij dq^b ln dq)
// plus the L2 term lambda row for every gathered occurrence (g[p_0 .. p_{L-2}], h and z at P_i and Q_i; z has no loss gradient, t none).
// A pair at d_eff = 0 with b > 0 gives f = 0 and df/db = 0; with b <= 0 the user is rejected (as is any user with a non-finite value or an
// id out of range): it moves nothing, its loss is NaN and it is counted once (poi_ctx_take_bad_ids).
//
// Kernels: geoie_plan (one block: exclusive scans of the launch users' rows and tiles), geoie_row (one workgroup per GI_TR rows of a user:
// the distances in float64 in cal_dis's operation order with cphi / cos_small of poi_common.h, f, the two dot products and the per-row
// scalars; the h gradients as c_i (f . G) over 64-column tiles staged in LDS), geoie_col (one workgroup per GI_TC columns: recomputes
// f over 64-row tiles and sums c_i f h[.] into the g gradients), geoie_user (a wave per user: loss, d a, d b in a fixed order),
// geoie_keys + te_scatter's radix sort of the 5 touches per row keyed (table, row) over [g | h | z], the run sums of fpmc.hip / prme.hip
// (64-touch windows joined across window boundaries) with k = the number of distinct users in a run, geoie_commit, geoie_ab.  No float
// atomics: identical launches give bitwise identical tables and a, b.
#include "geoie_pair.h"      // gi_dist, gi_f: shared with geoie_score.hip
#include "poi_kernels.h"

namespace poi {

#define GI_TR 16        // rows per work item of geoie_row
#define GI_JT 64        // columns per LDS tile of geoie_row
#define GI_TC 16        // columns per work item of geoie_col
#define GI_IT 64        // rows per LDS tile of geoie_col

__device__ __forceinline__ int gi_id(int v, int hi) { return (unsigned)v < (unsigned)hi ? v : 0; }

// last k in [0, n) with a[k] <= w (a ascending, a[0] = 0 <= w)
__device__ __forceinline__ int gi_find(const int* a, int n, int w) {
  int lo = 0, hi = n;
  while (hi - lo > 1) {
    const int m = (lo + hi) >> 1;
    if (a[m] <= w) lo = m; else hi = m;
  }
  return lo;
}

// launch row position of touch e (layout [g: P][h: 2 P][z: 2 P])
__device__ __forceinline__ int gi_touch_row(int P, int e) { return e < P ? e : e < 3 * P ? (e - P) >> 1 : (e - 3 * P) >> 1; }

__device__ __forceinline__ float* gi_row_ptr(const GeoieArgs& A, int key) {
  const int R = A.n_item + 1;
  if (key < R) return A.g + (size_t)key * A.dim;
  if (key < 2 * R) return A.h + (size_t)(key - R) * A.dim;
  return A.z + (size_t)(key - 2 * R) * A.dim;
}

template <typename T>
__device__ T gi_block_scan(T v, T* wsum, T& total) {      // exclusive scan over a 256-thread block
  const int lane = lane_id(), w = wave_id();
  T inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) { const T t = __shfl_up(inc, o, 64); if (lane >= o) inc += t; }
  if (lane == 63) wsum[w] = inc;
  __syncthreads();
  T pre = 0, tot = 0;
  for (int i = 0; i < 4; ++i) { if (i < w) pre += wsum[i]; tot += wsum[i]; }
  __syncthreads();
  total = tot;
  return pre + inc - v;
}

// one block of 256: per launch user k the rows max(L - 1, 0), its tiles of both passes, its pairs; tot = {rows, row tiles, column tiles,
// -, totals mismatch}.  A user id outside [0, n_user) gets no rows and is rejected.  Rows (or pairs) that do not add up to the host totals
// set the mismatch flag: every kernel then does nothing and every user is rejected.
__global__ __launch_bounds__(256) void geoie_plan_kernel(GeoieArgs A) {
  __shared__ int s_w[3][4];
  __shared__ long long s_wl[4];
  const int tid = threadIdx.x, n = A.n;
  int cr = 0, ct = 0, cc = 0;
  long long cp = 0;
  for (int b0 = 0; b0 < n; b0 += 256) {
    const int k = b0 + tid;
    int rows = 0, bad = 0;
    if (k < n) {
      const int u = A.users[k];
      if ((unsigned)u >= (unsigned)A.n_user) bad = 1;
      else rows = max(A.off[u + 1] - A.off[u] - 1, 0);
      A.ubad[k] = bad;
    }
    int tr, tt, tc;
    long long tl;
    const int er = gi_block_scan<int>(rows, s_w[0], tr);
    const int et = gi_block_scan<int>((rows + GI_TR - 1) / GI_TR, s_w[1], tt);
    const int ec = gi_block_scan<int>((rows + GI_TC - 1) / GI_TC, s_w[2], tc);
    const long long ep = gi_block_scan<long long>((long long)rows * (rows + 1) / 2, s_wl, tl);
    if (k < n) { A.rowoff[k] = cr + er; A.troff[k] = ct + et; A.tcoff[k] = cc + ec; if (A.pairoff) A.pairoff[k] = cp + ep; }
    cr += tr; ct += tt; cc += tc; cp += tl;
  }
  if (tid == 0) {
    A.rowoff[n] = cr; A.troff[n] = ct; A.tcoff[n] = cc;
    if (A.pairoff) A.pairoff[n] = cp;
    const int mism = cr != A.P || (A.n_pairs >= 0 && cp != A.n_pairs);
    A.tot[0] = cr; A.tot[1] = mism ? 0 : ct; A.tot[2] = mism ? 0 : cc; A.tot[4] = mism;
    A.cnt[0] = 5 * A.P;
  }
}

// ---- row pass -----------------------------------------------------------------------------------------------------------------
template <int MAXD>
__global__ __launch_bounds__(256) void geoie_row_kernel(GeoieArgs A) {
  __shared__ __align__(16) float sG[GI_JT][MAXD];
  __shared__ __align__(16) float sHP[GI_TR][MAXD], sHQ[GI_TR][MAXD];
  __shared__ float sFP[GI_TR][GI_JT], sFQ[GI_TR][GI_JT];
  __shared__ double sC[3][GI_JT], sT[6][GI_TR];
  __shared__ float sCoef[GI_TR];
  constexpr int NSLOT = (GI_TR * MAXD / 4 + 255) / 256;
  const int tid = threadIdx.x, D = A.dim, D4 = D / 4, NI = A.n_item;
  const int r = tid >> 4, l16 = tid & 15;
  const double ca = A.ab[0], cb = A.ab[1], dmin = A.d_min;
  const int n_work = A.tot[1];
  for (int w = blockIdx.x; w < n_work; w += gridDim.x) {
    const int k = gi_find(A.troff, A.n, w);
    const int u = A.users[k], base = A.off[u], rows = A.rowoff[k + 1] - A.rowoff[k];
    const int i0 = (w - A.troff[k]) * GI_TR, nr = min(GI_TR, rows - i0), r0 = A.rowoff[k];
    bool bad = false;
    __syncthreads();
    for (int x = tid; x < GI_TR * D; x += 256) {
      const int rr = x / D, c = x - rr * D;
      float vp = 0.f, vq = 0.f;
      if (rr < nr) {
        const int pp = gi_id(A.p[base + i0 + rr + 1], NI), qq = gi_id(A.q[base + i0 + rr + 1], NI);
        vp = A.h[(size_t)pp * D + c]; vq = A.h[(size_t)qq * D + c];
      }
      sHP[rr][c] = vp; sHQ[rr][c] = vq;
    }
    if (tid < GI_TR && tid < nr) {
      const int pv = A.p[base + i0 + tid + 1], qv = A.q[base + i0 + tid + 1];
      if ((unsigned)pv >= (unsigned)NI || (unsigned)qv >= (unsigned)NI) bad = true;
      const int pp = gi_id(pv, NI), qq = gi_id(qv, NI);
      sT[0][tid] = A.coords[2 * (size_t)pp]; sT[1][tid] = A.coords[2 * (size_t)pp + 1]; sT[2][tid] = A.cphi[pp];
      sT[3][tid] = A.coords[2 * (size_t)qq]; sT[4][tid] = A.coords[2 * (size_t)qq + 1]; sT[5][tid] = A.cphi[qq];
    }
    if (tid == 0 && i0 == 0 && (unsigned)A.p[base] >= (unsigned)NI) bad = true;
    double sf = 0.0, sa = 0.0, sb = 0.0;
    float4 up[NSLOT], uq[NSLOT];
#pragma unroll
    for (int m = 0; m < NSLOT; ++m) { up[m] = make_float4(0.f, 0.f, 0.f, 0.f); uq[m] = up[m]; }
    const int i = i0 + r, ncols = i0 + nr;
    for (int j0 = 0; j0 < ncols; j0 += GI_JT) {
      const int nc = min(GI_JT, ncols - j0);
      __syncthreads();
      for (int x = tid; x < GI_JT * D; x += 256) {
        const int jj = x / D, c = x - jj * D;
        sG[jj][c] = jj < nc ? A.g[(size_t)gi_id(A.p[base + j0 + jj], NI) * D + c] : 0.f;
      }
      if (tid < GI_JT && tid < nc) {
        const int pj = gi_id(A.p[base + j0 + tid], NI);
        sC[0][tid] = A.coords[2 * (size_t)pj]; sC[1][tid] = A.coords[2 * (size_t)pj + 1]; sC[2][tid] = A.cphi[pj];
      }
      __syncthreads();
      // phase A: thread (r, l16) owns the columns l16 + 16 kk of row r
      float x[4] = {0.f, 0.f, 0.f, 0.f}, y[4] = {0.f, 0.f, 0.f, 0.f};
      if (r < nr) {
        for (int c = 0; c < D; c += 4) {
          const float4 hp = *reinterpret_cast<const float4*>(&sHP[r][c]), hq = *reinterpret_cast<const float4*>(&sHQ[r][c]);
#pragma unroll
          for (int kk = 0; kk < 4; ++kk) {
            const float4 gv = *reinterpret_cast<const float4*>(&sG[l16 + 16 * kk][c]);
            x[kk] = fmaf(gv.w, hp.w, fmaf(gv.z, hp.z, fmaf(gv.y, hp.y, fmaf(gv.x, hp.x, x[kk]))));
            y[kk] = fmaf(gv.w, hq.w, fmaf(gv.z, hq.z, fmaf(gv.y, hq.y, fmaf(gv.x, hq.x, y[kk]))));
          }
        }
      }
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) {
        const int jj = l16 + 16 * kk;
        float fpv = 0.f, fqv = 0.f;
        if (r < nr && jj < nc && j0 + jj <= i) {
          const float dp = gi_dist(sC[0][jj], sC[1][jj], sC[2][jj], sT[0][r], sT[1][r], sT[2][r]);
          const float dq = gi_dist(sC[0][jj], sC[1][jj], sC[2][jj], sT[3][r], sT[4][r], sT[5][r]);
          double fp, fpa, fpb, fq, fqa, fqb;
          gi_f(dp, dmin, ca, cb, fp, fpa, fpb, bad);
          gi_f(dq, dmin, ca, cb, fq, fqa, fqb, bad);
          const double xd = x[kk], yd = y[kk];
          sf += xd * fp - yd * fq; sa += xd * fpa - yd * fqa; sb += xd * fpb - yd * fqb;
          fpv = (float)fp; fqv = (float)fq;
        }
        sFP[r][jj] = fpv; sFQ[r][jj] = fqv;
      }
      __syncthreads();
      // phase B: slot (rB, c4) sums f G over the tile's columns
#pragma unroll
      for (int m = 0; m < NSLOT; ++m) {
        const int s = tid + 256 * m, rB = s / D4, c4 = s - rB * D4;
        if (s < GI_TR * D4 && rB < nr) {
          float4 ap = up[m], aq = uq[m];
          for (int jj = 0; jj < nc; ++jj) {
            const float4 gv = *reinterpret_cast<const float4*>(&sG[jj][4 * c4]);
            const float a1 = sFP[rB][jj], a2 = sFQ[rB][jj];
            ap.x = fmaf(a1, gv.x, ap.x); ap.y = fmaf(a1, gv.y, ap.y); ap.z = fmaf(a1, gv.z, ap.z); ap.w = fmaf(a1, gv.w, ap.w);
            aq.x = fmaf(a2, gv.x, aq.x); aq.y = fmaf(a2, gv.y, aq.y); aq.z = fmaf(a2, gv.z, aq.z); aq.w = fmaf(a2, gv.w, aq.w);
          }
          up[m] = ap; uq[m] = aq;
        }
      }
    }
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) {
      sf += __shfl_xor(sf, o, 64); sa += __shfl_xor(sa, o, 64); sb += __shfl_xor(sb, o, 64);
    }
    if (l16 == 0 && r < nr) {
      const double inv = 1.0 / (double)(i + 1), diff = sf * inv;
      const double s = 1.0 / (1.0 + exp(diff));
      const double ls = diff >= 0.0 ? -log1p(exp(-diff)) : diff - log1p(exp(diff));
      const double cf = s * inv;
      const int row = r0 + i;
      A.rloss[row] = ls; A.rda[row] = -cf * sa; A.rdb[row] = -cf * sb;
      A.coef[row] = (float)cf; A.tuser[row] = k;
      sCoef[r] = (float)cf;
      if (!isfinite(diff) || !isfinite(sa) || !isfinite(sb)) bad = true;
    }
    __syncthreads();
#pragma unroll
    for (int m = 0; m < NSLOT; ++m) {
      const int s = tid + 256 * m, rB = s / D4, c4 = s - rB * D4;
      if (s < GI_TR * D4 && rB < nr) {
        const float cf = sCoef[rB];
        const size_t row = (size_t)r0 + i0 + rB;
        const float4 gp = make_float4(-cf * up[m].x, -cf * up[m].y, -cf * up[m].z, -cf * up[m].w);
        const float4 gq = make_float4(cf * uq[m].x, cf * uq[m].y, cf * uq[m].z, cf * uq[m].w);
        if (!isfinite(gp.x + gp.y + gp.z + gp.w) || !isfinite(gq.x + gq.y + gq.z + gq.w)) bad = true;
        *reinterpret_cast<float4*>(A.G + ((size_t)A.P + 2 * row) * D + 4 * c4) = gp;
        *reinterpret_cast<float4*>(A.G + ((size_t)A.P + 2 * row + 1) * D + 4 * c4) = gq;
      }
    }
    if (__syncthreads_or(bad) && tid == 0) A.ubad[k] = 1;
  }
}

// ---- column pass --------------------------------------------------------------------------------------------------------------
template <int MAXD>
__global__ __launch_bounds__(256) void geoie_col_kernel(GeoieArgs A) {
  __shared__ __align__(16) float sHP[GI_IT][MAXD], sHQ[GI_IT][MAXD];
  __shared__ float sWP[GI_TC][GI_IT], sWQ[GI_TC][GI_IT];
  __shared__ double sT[6][GI_IT], sC[3][GI_TC];
  __shared__ float sCf[GI_IT];
  constexpr int NSLOT = (GI_TC * MAXD / 4 + 255) / 256;
  const int tid = threadIdx.x, D = A.dim, D4 = D / 4, NI = A.n_item;
  const int cA = tid >> 4, l16 = tid & 15;
  const double ca = A.ab[0], cb = A.ab[1], dmin = A.d_min;
  const int n_work = A.tot[2];
  for (int w = blockIdx.x; w < n_work; w += gridDim.x) {
    const int k = gi_find(A.tcoff, A.n, w);
    const int u = A.users[k], base = A.off[u], rows = A.rowoff[k + 1] - A.rowoff[k];
    const int j0 = (w - A.tcoff[k]) * GI_TC, nc = min(GI_TC, rows - j0), r0 = A.rowoff[k];
    bool bad = false;
    __syncthreads();
    if (tid < GI_TC && tid < nc) {
      const int pj = gi_id(A.p[base + j0 + tid], NI);
      sC[0][tid] = A.coords[2 * (size_t)pj]; sC[1][tid] = A.coords[2 * (size_t)pj + 1]; sC[2][tid] = A.cphi[pj];
    }
    float4 v[NSLOT];
#pragma unroll
    for (int m = 0; m < NSLOT; ++m) v[m] = make_float4(0.f, 0.f, 0.f, 0.f);
    const int j = j0 + cA;
    for (int ib = j0; ib < rows; ib += GI_IT) {
      const int nrw = min(GI_IT, rows - ib);
      __syncthreads();
      for (int x = tid; x < GI_IT * D; x += 256) {
        const int ii = x / D, c = x - ii * D;
        float vp = 0.f, vq = 0.f;
        if (ii < nrw) {
          const int pp = gi_id(A.p[base + ib + ii + 1], NI), qq = gi_id(A.q[base + ib + ii + 1], NI);
          vp = A.h[(size_t)pp * D + c]; vq = A.h[(size_t)qq * D + c];
        }
        sHP[ii][c] = vp; sHQ[ii][c] = vq;
      }
      if (tid < GI_IT && tid < nrw) {
        const int pp = gi_id(A.p[base + ib + tid + 1], NI), qq = gi_id(A.q[base + ib + tid + 1], NI);
        sT[0][tid] = A.coords[2 * (size_t)pp]; sT[1][tid] = A.coords[2 * (size_t)pp + 1]; sT[2][tid] = A.cphi[pp];
        sT[3][tid] = A.coords[2 * (size_t)qq]; sT[4][tid] = A.coords[2 * (size_t)qq + 1]; sT[5][tid] = A.cphi[qq];
        sCf[tid] = A.coef[r0 + ib + tid];
      }
      __syncthreads();
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) {
        const int ii = l16 + 16 * kk;
        float wp = 0.f, wq = 0.f;
        if (cA < nc && ii < nrw && j <= ib + ii) {
          const float dp = gi_dist(sC[0][cA], sC[1][cA], sC[2][cA], sT[0][ii], sT[1][ii], sT[2][ii]);
          const float dq = gi_dist(sC[0][cA], sC[1][cA], sC[2][cA], sT[3][ii], sT[4][ii], sT[5][ii]);
          double fp, fa, fb, fq;
          gi_f(dp, dmin, ca, cb, fp, fa, fb, bad);
          gi_f(dq, dmin, ca, cb, fq, fa, fb, bad);
          const double cf = sCf[ii];
          wp = (float)(cf * fp); wq = (float)(cf * fq);
        }
        sWP[cA][ii] = wp; sWQ[cA][ii] = wq;
      }
      __syncthreads();
#pragma unroll
      for (int m = 0; m < NSLOT; ++m) {
        const int s = tid + 256 * m, cB = s / D4, c4 = s - cB * D4;
        if (s < GI_TC * D4 && cB < nc) {
          float4 acc = v[m];
          for (int ii = 0; ii < nrw; ++ii) {
            const float4 hp = *reinterpret_cast<const float4*>(&sHP[ii][4 * c4]), hq = *reinterpret_cast<const float4*>(&sHQ[ii][4 * c4]);
            const float a1 = sWP[cB][ii], a2 = sWQ[cB][ii];
            acc.x = fmaf(a1, hp.x, fmaf(-a2, hq.x, acc.x)); acc.y = fmaf(a1, hp.y, fmaf(-a2, hq.y, acc.y));
            acc.z = fmaf(a1, hp.z, fmaf(-a2, hq.z, acc.z)); acc.w = fmaf(a1, hp.w, fmaf(-a2, hq.w, acc.w));
          }
          v[m] = acc;
        }
      }
    }
#pragma unroll
    for (int m = 0; m < NSLOT; ++m) {
      const int s = tid + 256 * m, cB = s / D4, c4 = s - cB * D4;
      if (s < GI_TC * D4 && cB < nc) {
        const float4 gg = make_float4(-v[m].x, -v[m].y, -v[m].z, -v[m].w);
        if (!isfinite(gg.x + gg.y + gg.z + gg.w)) bad = true;
        *reinterpret_cast<float4*>(A.G + ((size_t)r0 + j0 + cB) * D + 4 * c4) = gg;
      }
    }
    if (__syncthreads_or(bad) && tid == 0) A.ubad[k] = 1;
  }
}

// ---- per-user scalars, keys ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void geoie_user_kernel(GeoieArgs A) {
  const int lane = lane_id();
  const int mism = A.tot[4];
  for (int k = blockIdx.x * 4 + wave_id(); k < A.n; k += gridDim.x * 4) {
    double sl = 0.0, sa = 0.0, sb = 0.0;
    if (!mism) {
      for (int r = A.rowoff[k] + lane; r < A.rowoff[k + 1]; r += 64) { sl += A.rloss[r]; sa += A.rda[r]; sb += A.rdb[r]; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { sl += __shfl_xor(sl, o, 64); sa += __shfl_xor(sa, o, 64); sb += __shfl_xor(sb, o, 64); }
    if (lane == 0) {
      const bool bad = mism || A.ubad[k] || !isfinite(sl) || !isfinite(sa) || !isfinite(sb);
      if (bad) { A.ubad[k] = 1; atomicAdd(A.bad, 1); }
      A.loss[k] = bad ? __int_as_float(0x7fc00000) : (float)sl;
      A.uda[k] = bad ? 0.0 : sa; A.udb[k] = bad ? 0.0 : sb;
    }
  }
}

__global__ __launch_bounds__(256) void geoie_keys_kernel(GeoieArgs A) {
  const int P = A.P, R = A.n_item + 1, S = A.sentinel, mism = A.tot[4];
  for (int r = blockIdx.x * 256 + threadIdx.x; r < P; r += gridDim.x * 256) {
    bool ok = false;
    int pj = 0, pp = 0, qq = 0;
    if (!mism) {
      const int k = A.tuser[r];
      if (!A.ubad[k]) {
        const int i = r - A.rowoff[k], base = A.off[A.users[k]];
        ok = true; pj = A.p[base + i]; pp = A.p[base + i + 1]; qq = A.q[base + i + 1];
      }
    }
    A.keys0[r] = ok ? pj : S;
    A.keys0[P + 2 * r] = ok ? R + pp : S;
    A.keys0[P + 2 * r + 1] = ok ? R + qq : S;
    A.keys0[3 * P + 2 * r] = ok ? 2 * R + pp : S;
    A.keys0[3 * P + 2 * r + 1] = ok ? 2 * R + qq : S;
  }
}

// ---- write-back: runs of equal keys in sorted order (prme.hip's windows), k = distinct users of the run --------------------------
__device__ __forceinline__ float4 gi_grad(const GeoieArgs& A, int e, int col) {
  return e < 3 * A.P ? ld4(A.G + (size_t)e * A.dim + col) : make_float4(0.f, 0.f, 0.f, 0.f);
}

// row <- row - alpha min(k, cap) / k (G + lambda mult row), into the slot of the run's first sorted position
__device__ __forceinline__ void gi_apply(const GeoieArgs& A, int key, float4 G, int k, int mult, int col, int slot) {
  const float4 rw = ld4(gi_row_ptr(A, key) + col);
  const float sc = A.alpha * fminf((float)k, A.bcap) / (float)k, lm = A.lambda * (float)mult;
  *reinterpret_cast<float4*>(A.slot + (size_t)slot * A.dim + col) =
      make_float4(rw.x - sc * (G.x + lm * rw.x), rw.y - sc * (G.y + lm * rw.y), rw.z - sc * (G.z + lm * rw.z), rw.w - sc * (G.w + lm * rw.w));
}

template <int LPR>
__global__ __launch_bounds__(256) void geoie_chunk_kernel(GeoieArgs A) {
  constexpr int EPW = 64 / LPR;
  const int lane = lane_id(), grp = lane / LPR, gl = lane % LPR;
  const int D = A.dim, N = 5 * A.P, col = gl * 4;
  const bool has = col < D;
  const int n_chunk = (N + 63) / 64;
  for (int c = blockIdx.x * 4 + wave_id(); c < n_chunk; c += gridDim.x * 4) {
    const int j0 = 64 * c, nv = min(64, N - j0);
    const bool valid = lane < nv;
    const int key = valid ? A.ks[j0 + lane] : -1;
    const int val = valid ? A.vs[j0 + lane] : 0;
    const int usr = valid ? A.tuser[gi_touch_row(A.P, val)] : -1;
    const int upk = __shfl_up(key, 1, 64), upu = __shfl_up(usr, 1, 64);
    int prevk = upk, prevu = upu;
    if (lane == 0) {
      prevk = c > 0 ? A.ks[j0 - 1] : -2;
      prevu = c > 0 ? A.tuser[gi_touch_row(A.P, A.vs[j0 - 1])] : -2;
    }
    const int nextk = (j0 + nv < N) ? A.ks[j0 + nv] : -3;
    const unsigned long long starts = __ballot(valid && key != prevk);
    const unsigned long long ustarts = __ballot(valid && (key != prevk || usr != prevu));
    int lead_cnt = 0, lead_more = 0, lead_k = 0, trail_cnt = 0, trail_row = -1, trail_k = 0;
    int a = 0;
    while (a < nv) {
      const unsigned long long above = a + 1 < 64 ? (starts >> (a + 1)) << (a + 1) : 0ull;
      const int b = above ? min(nv, (int)__builtin_ctzll(above)) : nv;
      const int row = __builtin_amdgcn_readfirstlane(__shfl(key, a, 64));
      if (row == A.sentinel) break;      // rejected users' touches sort last: nothing after them
      const unsigned long long seg = (b >= 64 ? ~0ull : ((1ull << b) - 1ull)) & ~((1ull << a) - 1ull);
      const int ku = __popcll(ustarts & seg);
      const bool cont_before = a == 0 && !(starts & 1ull);
      const bool cont_after = b == nv && nextk == row;
      float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
      for (int e0 = a; e0 < b; e0 += EPW) {
        const int idx = e0 + grp;
        const int e = __shfl(val, idx & 63, 64);
        if (idx < b && has) {
          const float4 v = gi_grad(A, e, col);
          acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
        }
      }
#pragma unroll
      for (int o = LPR; o < 64; o <<= 1) {
        acc.x += __shfl_xor(acc.x, o, 64); acc.y += __shfl_xor(acc.y, o, 64);
        acc.z += __shfl_xor(acc.z, o, 64); acc.w += __shfl_xor(acc.w, o, 64);
      }
      if (!cont_before && !cont_after) {
        if (grp == 0 && has) gi_apply(A, row, acc, ku, b - a, col, j0 + a);
      } else {
        if (grp == 0 && has) *reinterpret_cast<float4*>((cont_before ? A.lead : A.trail) + (size_t)c * D + col) = acc;
        if (cont_before) { lead_cnt = b - a; lead_more = cont_after ? 1 : 0; lead_k = ku; }
        else { trail_cnt = b - a; trail_row = row; trail_k = ku; }
      }
      a = b;
    }
    if (lane == 0) { A.meta[c] = make_int4(lead_cnt, lead_more, trail_cnt, trail_row); A.meta2[c] = make_int4(lead_k, trail_k, 0, 0); }
  }
}

// runs cut by window boundaries: the window where a run starts owns it and adds the following windows' opening runs in order
template <int LPR>
__global__ __launch_bounds__(256) void geoie_span_kernel(GeoieArgs A) {
  constexpr int EPW = 64 / LPR;
  const int lane = lane_id(), grp = lane / LPR, gl = lane % LPR;
  const int D = A.dim, col = gl * 4, n_chunk = (5 * A.P + 63) / 64;
  for (int c = (blockIdx.x * 4 + wave_id()) * EPW + grp; c < n_chunk; c += gridDim.x * 4 * EPW) {
    const int4 m = A.meta[c];
    if (m.z == 0 || col >= D) continue;
    float4 sum = ld4(A.trail + (size_t)c * D + col);
    int mult = m.z, k = A.meta2[c].y;
    for (int c2 = c + 1; c2 < n_chunk; ++c2) {
      const int4 m2 = A.meta[c2];
      const float4 v = ld4(A.lead + (size_t)c2 * D + col);
      sum = make_float4(sum.x + v.x, sum.y + v.y, sum.z + v.z, sum.w + v.w);
      mult += m2.x; k += A.meta2[c2].x;
      if (!m2.y) break;
    }
    gi_apply(A, m.w, sum, k, mult, col, 64 * c + 64 - m.z);
  }
}

// every run's new row (slot of its first sorted position) -> its table, after all gradients have read the entry values
template <int LPR>
__global__ __launch_bounds__(256) void geoie_commit_kernel(GeoieArgs A) {
  constexpr int EPW = 64 / LPR;
  const int lane = lane_id(), grp = lane / LPR, gl = lane % LPR;
  const int D = A.dim, col = gl * 4, N = 5 * A.P;
  for (int e = (blockIdx.x * 4 + wave_id()) * EPW + grp; e < N; e += gridDim.x * 4 * EPW) {
    const int key = A.ks[e];
    if (col >= D || key == A.sentinel || (e > 0 && A.ks[e - 1] == key)) continue;
    *reinterpret_cast<float4*>(gi_row_ptr(A, key) + col) = ld4(A.slot + (size_t)e * D + col);
  }
}

// a, b -= alpha min(n_acc, cap) / n_acc sum_u d cost_u / d (a, b) over the accepted users with rows.  The sum runs over the accepted users
// COMPACTED in launch order (the c-th goes to thread c mod 256, then a fixed tree): removing a rejected user gives the same bits.
__global__ __launch_bounds__(256) void geoie_ab_kernel(GeoieArgs A) {
  __shared__ double s_va[256], s_vb[256], s_a[4], s_b[4];
  __shared__ int s_w[4];
  const int tid = threadIdx.x, lane = lane_id(), w = wave_id();
  double sa = 0.0, sb = 0.0;
  int base = 0;
  for (int k0 = 0; k0 < A.n; k0 += 256) {
    const int k = k0 + tid;
    const int acc = k < A.n && !A.ubad[k] && A.rowoff[k + 1] > A.rowoff[k];
    int cnt;
    const int ex = gi_block_scan<int>(acc, s_w, cnt);
    if (acc) { s_va[(base + ex) & 255] = A.uda[k]; s_vb[(base + ex) & 255] = A.udb[k]; }
    __syncthreads();
    if (((tid - base) & 255) < cnt) { sa += s_va[tid]; sb += s_vb[tid]; }
    base += cnt;
    __syncthreads();
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { sa += __shfl_xor(sa, o, 64); sb += __shfl_xor(sb, o, 64); }
  if (lane == 0) { s_a[w] = sa; s_b[w] = sb; }
  __syncthreads();
  if (tid == 0) {
    const double ta = ((s_a[0] + s_a[1]) + s_a[2]) + s_a[3], tb = ((s_b[0] + s_b[1]) + s_b[2]) + s_b[3];
    const int tn = base;
    if (tn > 0) {
      const double sc = (double)A.alpha * fmin((double)tn, (double)A.bcap) / (double)tn;
      A.ab[0] = A.ab[0] - sc * ta;
      A.ab[1] = A.ab[1] - sc * tb;
    }
  }
}

template <int MAXD, int LPR>
static hipError_t launch_geoie_step_t(GeoieArgs& A, int num_cu, hipStream_t st, Timing* tm) {
  auto grid = [&](long long items, int per) { return dim3((unsigned)max(1ll, min((long long)num_cu * 16, (items + per - 1) / per))); };
  const long long P = A.P;
  tm->begin("geoie_plan", st);
  hipLaunchKernelGGL(geoie_plan_kernel, dim3(1), dim3(256), 0, st, A);
  tm->end(st);
  if (P > 0) {
    tm->begin("geoie_row", st);
    hipLaunchKernelGGL(geoie_row_kernel<MAXD>, grid(P / GI_TR + A.n, 1), dim3(256), 0, st, A);
    tm->end(st);
    tm->begin("geoie_col", st);
    hipLaunchKernelGGL(geoie_col_kernel<MAXD>, grid(P / GI_TC + A.n, 1), dim3(256), 0, st, A);
    tm->end(st);
  }
  tm->begin("geoie_user", st);
  hipLaunchKernelGGL(geoie_user_kernel, grid(A.n, 4), dim3(256), 0, st, A);
  tm->end(st);
  if (P > 0) {
    tm->begin("geoie_sort", st);
    hipLaunchKernelGGL(geoie_keys_kernel, grid(P, 256), dim3(256), 0, st, A);
    int bits = 1;
    while ((1ll << bits) <= (long long)A.sentinel) ++bits;
    const int *ks = nullptr, *vs = nullptr;
    hipError_t e = launch_radix_sort(A.keys0, A.keys1, A.vals0, A.vals1, A.cnt, bits, A.hist, st, &ks, &vs);
    if (e != hipSuccess) return e;
    A.ks = ks; A.vs = vs;
    tm->end(st);
    const long long chunks = (5 * P + 63) / 64;
    tm->begin("geoie_rows", st);
    hipLaunchKernelGGL(geoie_chunk_kernel<LPR>, grid(chunks, 4), dim3(256), 0, st, A);
    hipLaunchKernelGGL(geoie_span_kernel<LPR>, grid(chunks, 4 * (64 / LPR)), dim3(256), 0, st, A);
    tm->end(st);
    tm->begin("geoie_commit", st);
    hipLaunchKernelGGL(geoie_commit_kernel<LPR>, grid(5 * P, 4 * (64 / LPR)), dim3(256), 0, st, A);
    tm->end(st);
  }
  tm->begin("geoie_ab", st);
  hipLaunchKernelGGL(geoie_ab_kernel, dim3(1), dim3(256), 0, st, A);
  tm->end(st);
  return hipGetLastError();
}

hipError_t launch_geoie_step(GeoieArgs& A, int num_cu, hipStream_t st, Timing* tm) {
  if (A.dim <= 32) return launch_geoie_step_t<32, 8>(A, num_cu, st, tm);
  if (A.dim <= 64) return launch_geoie_step_t<64, 16>(A, num_cu, st, tm);
  if (A.dim <= 128) return launch_geoie_step_t<128, 32>(A, num_cu, st, tm);
  return hipErrorInvalidValue;
}

// ---- packed pair distances (tests / debugging) ------------------------------------------------------------------------------------
// user k's row i occupies pairs pairoff[k] + i (i + 1) / 2 + j, j = 0 .. i; NaN where an id is out of range, everything NaN when the
// host totals do not match
__global__ __launch_bounds__(256) void geoie_pairs_kernel(GeoieArgs A) {
  const int NI = A.n_item;
  const float nan = __int_as_float(0x7fc00000);
  if (A.tot[4]) {
    for (long long x = blockIdx.x * 256ll + threadIdx.x; x < A.n_pairs; x += gridDim.x * 256ll) { A.dp_out[x] = nan; A.dq_out[x] = nan; }
    return;
  }
  for (int r = blockIdx.x * 256 + threadIdx.x; r < A.P; r += gridDim.x * 256) {
    const int k = gi_find(A.rowoff, A.n, r);
    const int i = r - A.rowoff[k], base = A.off[A.users[k]];
    const long long o = A.pairoff[k] + (long long)i * (i + 1) / 2;
    const int pv = A.p[base + i + 1], qv = A.q[base + i + 1];
    const bool okp = (unsigned)pv < (unsigned)NI, okq = (unsigned)qv < (unsigned)NI;
    const int pp = gi_id(pv, NI), qq = gi_id(qv, NI);
    for (int j = 0; j <= i; ++j) {
      const int jv = A.p[base + j];
      const bool ok = (unsigned)jv < (unsigned)NI;
      const int pj = gi_id(jv, NI);
      const double la = A.coords[2 * (size_t)pj], lo = A.coords[2 * (size_t)pj + 1], cp = A.cphi[pj];
      A.dp_out[o + j] = ok && okp ? gi_dist(la, lo, cp, A.coords[2 * (size_t)pp], A.coords[2 * (size_t)pp + 1], A.cphi[pp]) : nan;
      A.dq_out[o + j] = ok && okq ? gi_dist(la, lo, cp, A.coords[2 * (size_t)qq], A.coords[2 * (size_t)qq + 1], A.cphi[qq]) : nan;
    }
  }
}

hipError_t launch_geoie_pairs(GeoieArgs& A, int num_cu, hipStream_t st) {
  hipLaunchKernelGGL(geoie_plan_kernel, dim3(1), dim3(256), 0, st, A);
  hipLaunchKernelGGL(geoie_pairs_kernel, dim3((unsigned)max(1, min(num_cu * 8, (A.P + 255) / 256))), dim3(256), 0, st, A);
  return hipGetLastError();
}

// ---- user vectors of the scoring: out[u] = [t[u] | sum_{j < L} g[p_j] / nH_u] ------------------------------------------------------
__global__ __launch_bounds__(256) void geoie_uvec_kernel(const float* __restrict__ g, const float* __restrict__ t, const int* __restrict__ off,
                                                         const int* __restrict__ p, int n_user, int n_item, int dim, int len_max, int norm,
                                                         float* __restrict__ out) {
  const long long N = (long long)n_user * dim;
  for (long long x = blockIdx.x * 256ll + threadIdx.x; x < N; x += gridDim.x * 256ll) {
    const int u = (int)(x / dim), d = (int)(x - (long long)u * dim);
    const int b = off[u], e = off[u + 1], L = e - b;
    double s = 0.0, ids = 0.0;
    bool bad = false;
    for (int j = b; j < e; ++j) {
      const int pj = p[j];
      if ((unsigned)pj > (unsigned)n_item) { bad = true; continue; }
      s += (double)g[(size_t)pj * dim + d];
      ids += (double)pj;
    }
    double m;
    if (norm == 0) m = s / (ids + (double)(len_max - L) * (double)n_item);      // GeoIE.py:119: the sum of the padded id row
    else m = L > 0 ? s / (double)L : 0.0;
    out[(size_t)u * 2 * dim + d] = t[(size_t)u * dim + d];
    out[(size_t)u * 2 * dim + dim + d] = bad ? __int_as_float(0x7fc00000) : (float)m;
  }
}

hipError_t launch_geoie_uvec(const float* g, const float* t, const int* off, const int* p, int n_user, int n_item, int dim, int len_max,
                             int norm, float* out, int num_cu, hipStream_t st) {
  const long long N = (long long)n_user * dim;
  hipLaunchKernelGGL(geoie_uvec_kernel, dim3((unsigned)max(1ll, min((long long)num_cu * 16, (N + 255) / 256))), dim3(256), 0, st, g, t, off, p,
                     n_user, n_item, dim, len_max, norm, out);
  return hipGetLastError();
}

}  // namespace poi
