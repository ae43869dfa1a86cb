// GeoIE scoring under the TRAINED rule (poi_geoie_score_all_geo / poi_geoie_score_topk_geo): the score the step of
// geoie.hip optimises, taken against every POI.  For a compacted history (distinct ids k ascending, multiplicities m_k, L = sum m_k) and a
// candidate l:
//   S(l) = tu . z[l] + (1 / L) sum_k m_k (g[k] . h[l]) f(max(d(k, l), d_min)),   f(d) = a exp(b ln d)
// with d = gi_dist and f = gi_f of geoie_pair.h - the bits the step sees for the same pair.  The two dot products are float32 fma chains,
// the sum over k and the user term are float64, the result is rounded once.  A pair at d_eff = 0 contributes 0 when b > 0 and makes the
// candidate's score NaN when b <= 0.
//
// One workgroup = one history and one span of candidates (A.span ids; the spans of a row tile [0, n_item)).  16 candidates at a time:
// h[l] of the 16 in LDS, thread (candidate, lane16) takes the history entries lane16 + 16 kk (kk < 4) of each 64-entry tile (g rows,
// coordinates, cos lat and m_k in LDS; a history of at most 64 distinct POIs is staged once per workgroup), and the 16 float64 partial
// sums meet in an xor butterfly - one fixed order per (history, candidate), whatever the span, the grid or the other rows of the call.
// Matrix mode writes the score.  Top-K mode (k <= 32) skips a row's excluded ids before the pair math, queues 64 scores per wave and folds
// a full queue into the wave's sorted best 64 (top64_merge, topk_list.h; a queue without an entry above the K-th best is dropped after one
// ballot); the four waves' lists meet in LDS and, when a row has several spans, a one-wave kernel per row folds the spans' lists.  The
// order (descending score, ascending id) is total, so every span size gives the same lists, and the scores are matrix mode's bits.
// No float atomics; a bad row (offsets, an id outside [0, n_item), ids not strictly ascending, a multiplicity < 1, a malformed exclusion
// list) gives NaN scores / an empty list and is counted once with one integer atomic.
#include "geoie_pair.h"
#include "poi_kernels.h"
#include "topk_list.h"

namespace poi {

#define GS_NC 16        // candidates per round
#define GS_KT 64        // history entries per LDS tile

template <int MAXD, bool TOPK>
__global__ __launch_bounds__(256) void geoie_score_kernel(GeoScoreArgs A) {
  constexpr int LD = MAXD + 4;      // row stride of the staged tables: 16-byte aligned, consecutive rows 4 banks apart
  __shared__ __align__(16) float sG[GS_KT][LD];
  __shared__ __align__(16) float sH[GS_NC][LD];
  __shared__ double sC[3][GS_KT], sM[GS_KT];
  __shared__ long long s_len[POI_NWAVE];
  __shared__ float m_s[POI_NWAVE][GEO_K_MAX];
  __shared__ int m_i[POI_NWAVE][GEO_K_MAX];
  __shared__ int m_cnt[POI_NWAVE];
  const int tid = threadIdx.x, lane = lane_id(), w = wave_id(), cg = tid >> 4, l16 = tid & 15;
  const int S = A.n_split, r = blockIdx.x / S, s = blockIdx.x - r * S;
  const int D = A.dim, D4 = D / 4, NI = A.n_item;
  const int lo = (int)min((long long)NI, (long long)s * A.span), hi = (int)min((long long)NI, (long long)lo + A.span);
  const int hist = A.rows ? A.rows[r] : r;
  const int hb = hist >= 0 ? A.off[hist] : -1, he = hist >= 0 ? A.off[hist + 1] : -1;
  const int e0 = TOPK && A.ex ? A.ex_off[r] : 0, e1 = TOPK && A.ex ? A.ex_off[r + 1] : 0;
  int bad = hb < 0 || he < hb || e1 < e0 || e0 < 0;
  long long len = 0;
  if (!bad) {
    for (int i = hb + tid; i < he; i += 256) {
      const int v = A.p[i], m = A.mult ? A.mult[i] : 1;
      bad |= (unsigned)v >= (unsigned)NI || m < 1 || (i > hb && A.p[i - 1] >= v);
      len += m;
    }
    for (int i = e0 + tid; i < e1; i += 256) bad |= (unsigned)A.ex[i] >= (unsigned)NI;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) len += __shfl_xor(len, o, 64);
  if (lane == 0) s_len[w] = len;
  if (__syncthreads_or(bad)) {      // a rejected row: NaN scores / an empty list, counted once
    if (s == 0 && tid == 0) atomicAdd(A.bad, 1);
    if (TOPK) {
      if (w == 0) list_emit<GEO_K_MAX>(A, A.n_split > 1, r, s, neg_inf(), PAD_ID, 0);
    } else {
      for (int l = lo + tid; l < hi; l += 256) A.out[(size_t)r * NI + l] = quiet_nan();
    }
    return;
  }
  const int nh = he - hb;
  const double Ld = (double)((s_len[0] + s_len[1]) + (s_len[2] + s_len[3]));
  const double ca = A.ab[0], cb = A.ab[1], dmin = A.d_min;
  const bool single = nh <= GS_KT;
  // the user row: lane16 owns the columns 4 lane16 + 64 j
  constexpr int NJ = (MAXD + 63) / 64;
  float4 tu[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int col = 4 * l16 + 64 * j;
    tu[j] = (A.tu && col < D) ? ld4(A.tu + (size_t)r * D + col) : make_float4(0.f, 0.f, 0.f, 0.f);
  }
  auto stage = [&](int j0, int nc) {
    for (int x = tid; x < GS_KT * D4; x += 256) {
      const int jj = x / D4, c4 = x - jj * D4;
      const float4 v = jj < nc ? ld4(A.g + (size_t)A.p[hb + j0 + jj] * D + 4 * c4) : make_float4(0.f, 0.f, 0.f, 0.f);
      *reinterpret_cast<float4*>(&sG[jj][4 * c4]) = v;
    }
    if (tid < GS_KT && tid < nc) {
      const int pj = A.p[hb + j0 + tid];
      sC[0][tid] = A.coords[2 * (size_t)pj]; sC[1][tid] = A.coords[2 * (size_t)pj + 1]; sC[2][tid] = A.cphi[pj];
      sM[tid] = A.mult ? (double)A.mult[hb + j0 + tid] : 1.0;
    }
  };
  if (single && nh > 0) stage(0, nh);
  float cs = neg_inf(), q_s = neg_inf();
  int ci = PAD_ID, q_id = PAD_ID, count = 0;      // the wave's best 64 so far, sorted over its lanes; its queue, one entry per lane
  for (int c0 = lo, round = 0; c0 < hi; c0 += GS_NC, ++round) {
    const int l = c0 + cg;
    bool active = l < hi;
    if (TOPK && active && e1 > e0) {      // ascending ids: first entry >= l
      int a = e0, b = e1;
      while (a < b) { const int md = (a + b) >> 1; if (A.ex[md] < l) a = md + 1; else b = md; }
      active = !(a < e1 && A.ex[a] == l);
    }
    __syncthreads();      // the previous round has read sH (and its last tile of sG)
    for (int x = tid; x < GS_NC * D4; x += 256) {
      const int rr = x / D4, c4 = x - rr * D4;
      const float4 v = c0 + rr < hi ? ld4(A.h + (size_t)(c0 + rr) * D + 4 * c4) : make_float4(0.f, 0.f, 0.f, 0.f);
      *reinterpret_cast<float4*>(&sH[rr][4 * c4]) = v;
    }
    double lat2 = 0.0, lon2 = 0.0, cp2 = 0.0;
    float tz = 0.f;
    if (active) {
      lat2 = A.coords[2 * (size_t)l]; lon2 = A.coords[2 * (size_t)l + 1]; cp2 = A.cphi[l];
      if (A.tu) {
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
          const int col = 4 * l16 + 64 * j;
          if (col < D) {
            const float4 zv = ld4(A.z + (size_t)l * D + col);
            tz = fmaf(tu[j].x, zv.x, tz); tz = fmaf(tu[j].y, zv.y, tz); tz = fmaf(tu[j].z, zv.z, tz); tz = fmaf(tu[j].w, zv.w, tz);
          }
        }
      }
    }
    double sum = 0.0;
    bool nanc = false;
    for (int j0 = 0; j0 < nh; j0 += GS_KT) {
      const int nc = min(GS_KT, nh - j0);
      if (!single) {
        if (j0 > 0) __syncthreads();      // the previous tile has been read
        stage(j0, nc);
      }
      __syncthreads();
      if (active) {
        float x[4] = {0.f, 0.f, 0.f, 0.f};
        for (int c = 0; c < D; c += 4) {
          const float4 hv = *reinterpret_cast<const float4*>(&sH[cg][c]);
#pragma unroll
          for (int kk = 0; kk < 4; ++kk) {
            const float4 gv = *reinterpret_cast<const float4*>(&sG[l16 + 16 * kk][c]);
            x[kk] = fmaf(gv.w, hv.w, fmaf(gv.z, hv.z, fmaf(gv.y, hv.y, fmaf(gv.x, hv.x, x[kk]))));
          }
        }
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
          const int jj = l16 + 16 * kk;
          if (jj < nc) {
            const float d = gi_dist(sC[0][jj], sC[1][jj], sC[2][jj], lat2, lon2, cp2);
            double f, fa, fb;
            gi_f(d, dmin, ca, cb, f, fa, fb, nanc);
            sum += (sM[jj] * (double)x[kk]) * f;
          }
        }
      }
    }
    int nn = nanc;
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) { sum += __shfl_xor(sum, o, 64); tz += __shfl_xor(tz, o, 64); nn |= __shfl_xor(nn, o, 64); }
    const double v = (double)tz + (nh > 0 ? sum / Ld : 0.0);
    const float sc = nn ? quiet_nan() : (float)v;
    if (!TOPK) {
      if (l16 == 0 && l < hi) A.out[(size_t)r * NI + l] = sc;
    } else {
      const bool sel = active && sc > neg_inf();      // NaN and -inf are never selected
      count += sel && l16 == 0;
      // candidate g of this round was summed by lane group g: queue lane 4 (round & 15) + g takes it
      const float vs = __shfl(sel ? sc : neg_inf(), (lane & 3) << 4, 64);
      const int vi = __shfl(sel ? l : PAD_ID, (lane & 3) << 4, 64);
      if ((lane >> 2) == (round & 15)) { q_s = vs; q_id = vi; }
      if ((round & 15) == 15 || c0 + GS_NC >= hi) {
        const float ts = __shfl(cs, A.k - 1, 64);
        const int ti = __shfl(ci, A.k - 1, 64);
        if (__ballot(q_id != PAD_ID && better(q_s, q_id, ts, ti))) top64_merge(cs, ci, q_s, q_id);
        q_s = neg_inf(); q_id = PAD_ID;
      }
    }
  }
  if (TOPK) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) count += __shfl_xor(count, o, 64);
    if (lane < GEO_K_MAX) { m_s[w][lane] = cs; m_i[w][lane] = ci; }
    if (lane == 0) m_cnt[w] = count;
    __syncthreads();
    if (w == 0) {
      float as;
      int ai;
      block_lists_fold<GEO_K_MAX>(&m_s[0][0], &m_i[0][0], GEO_K_MAX, as, ai);
      list_emit<GEO_K_MAX>(A, A.n_split > 1, r, s, as, ai, (m_cnt[0] + m_cnt[1]) + (m_cnt[2] + m_cnt[3]));
    }
  }
}

template <int MAXD>
static hipError_t launch_geoie_score_t(GeoScoreArgs& A, hipStream_t st, Timing* tm) {
  const dim3 grid((unsigned)A.n_rows * (unsigned)A.n_split);
  if (A.k > 0) {
    tm->begin("geoie_topk_geo", st);
    hipLaunchKernelGGL((geoie_score_kernel<MAXD, true>), grid, dim3(256), 0, st, A);
    if (A.n_split > 1) launch_topk_slices_merge(slice_lists(A), GEO_K_MAX, A.n_rows, st);
  } else {
    tm->begin("geoie_score_geo", st);
    hipLaunchKernelGGL((geoie_score_kernel<MAXD, false>), grid, dim3(256), 0, st, A);
  }
  tm->end(st);
  return hipGetLastError();
}

hipError_t launch_geoie_score(GeoScoreArgs& A, hipStream_t st, Timing* tm) {
  if (A.dim <= 32) return launch_geoie_score_t<32>(A, st, tm);
  if (A.dim <= 64) return launch_geoie_score_t<64>(A, st, tm);
  if (A.dim <= 128) return launch_geoie_score_t<128>(A, st, tm);
  return hipErrorInvalidValue;
}

}  // namespace poi
