// Fold-in for the successive-POI models (poi_foldin_terms_fpmc / poi_foldin_terms_prme / poi_foldin_pair): a row of FPMC-LR's ui or of
// PRME's du for a check-in history the model never trained on.  With the item side frozen, each model's per-transition rule on the
// user row (public/FPMC_LR.py:113-140, the ui part; public/PRME.py:173-214, the du part) is foldin.hip's chain with two per-step scalars
// that do not depend on the row - a weight a_s and an offset c_s:
//
//   dot form    (FPMC-LR, Y = iu):  d = Y[p_t] - Y[q],  x = w . d + c,                         w -= alpha (-sigmoid(-x) d + lambda w)
//   metric form (PRME,    Y = dp):  d = Y[p_t] - Y[q],  x = a (|w - Y[q]|^2 - |w - Y[p_t]|^2) + c,  w -= alpha (-sigmoid(-x) 2 a d + lambda w)
//   loss[e] += -log sigmoid(x) in both (PRME.py returns +log sigmoid; fold-in keeps poi_foldin_bpr's sign)
//
// Terms pass (foldin_terms_kernel): everything of a step that does not touch w, off the chain and embarrassingly parallel over
// epochs x positions.  One 16-lane row of a wave = one (epoch, CSR position), lane split as below; the gathered rows are float32, the
// sums float64 in one fixed order (per lane its columns ascending, then the 16-lane tree); nothing is shared, no atomics, the output
// does not depend on the grid.
//   FPMC-LR:  c = ai[prev] . (ia[p_t] - ia[q])
//   PRME:     far = gap_t > thd,  wgt = (1 + d_t)^0.25,  a = far ? 1 : wgt cw,  b = far ? 0 : wgt (1 - cw)   (a: once per position)
//             c = b (|ds[q] - ds[prev]|^2 - |ds[p_t] - ds[prev]|^2)
//             d_t = the caller's distance, or cal_dis(cordi[p_t], cordi[prev]) in float64 in cal_dis's operation order (contract off),
//             as prme_score_kernel computes its weight
// prev = p[pos - 1]; the first position of a history (found by a search in the offsets) is written as 0.  An id outside [0, n_item]
// (or a distance that is negative or not finite) makes the entry NaN - the chain kernel turns that into a bad user and counts it.  A
// negative of -1 ("no negative exists", poi_fpmc_sample_negatives) is a skipped step: its c is 0.
//
// Chain (foldin_pair_kernel<NJ, K, FORM>): foldin_kernel's layout.  One 16-lane DPP row = one user, four users per wave, one wave per
// workgroup; lane g of a row owns the columns 4 g + 64 j and keeps its slice of w in float64 registers.  K steps of rows and 2 K steps
// of ids are in flight while a step computes; the ring also carries each step's a / c doubles, fetched with the ids.  Every load of the
// loop is unconditional (selects on address and value), so the compiler counts the loads in flight and waits only for the ones a step
// consumes.  No LDS, no barrier, nothing shared between users, no spin-wait: a user's bits depend on its own history, negatives, terms
// and w0 alone.  The metric form evaluates (w - yq)^2 - (w - yp)^2 as d (2 w - (yp + yq)): d and yp + yq are exact in float64.
// With a = c = NULL and first = 0 the dot form performs poi_foldin_bpr's operations in its order: the same bits.
//
// Bytes per step: two item rows (2 x 4 dim) + 8 B of ids + 8 B of c (+ 8 B of a in the metric form); the terms pass reads three rows
// (+ 20 B of gap / distance or 32 B of coordinates for PRME) and writes 8 B per (epoch, position).
#include "poi_common.h"
#include "poi_kernels.h"

namespace poi {

namespace {

// cal_dis (Load_Data_prme.py:24-35) in float64 in its operation order: rad(x) = x pi / 180, sin^2 halves, R = 6378.137
__device__ __forceinline__ double fs_cal_dis(double lat1, double lon1, double lat2, double lon2) {
#pragma clang fp contract(off)
  const double r1 = lat1 * 3.141592653589793 / 180.0, r2 = lat2 * 3.141592653589793 / 180.0;
  const double a = r1 - r2, b = lon1 * 3.141592653589793 / 180.0 - lon2 * 3.141592653589793 / 180.0;
  const double sa = sin(a / 2), sb = sin(b / 2);
  return 2 * asin(sqrt(sa * sa + cos(r1) * cos(r2) * (sb * sb))) * 6378.137;
}

}  // namespace

// ---------------------------------------------------------------------------------------------
// terms pass
template <bool PRME>
__global__ __launch_bounds__(256) void foldin_terms_kernel(FoldinTermsArgs A) {
  const int gl = threadIdx.x & 15;
  const int D = A.dim, NI = A.n_item;
  const long long T = A.total, items = T * A.n_epoch;
  const double nan = __builtin_nan("");
  for (long long it = (long long)blockIdx.x * 16 + (threadIdx.x >> 4); it < items; it += (long long)gridDim.x * 16) {
    const long long e = it / T, pos = it - e * T;
    // the history that holds pos: the last r with off[r] <= pos (upper bound in the ascending offsets)
    int lo = 0, hi = A.n + 1;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if ((long long)A.off[mid] <= pos) lo = mid + 1; else hi = mid;
    }
    const bool start = lo >= 1 && (long long)A.off[lo - 1] == pos;
    double* const cdst = A.c_out + e * A.q_epoch_stride + pos;
    if (start || pos == 0) {                                   // position 0 of a history is no step
      if (gl == 0) { *cdst = 0.0; if (PRME && e == 0) A.a_out[pos] = 0.0; }
      continue;
    }
    const int ip = A.p[pos], iv = A.p[pos - 1], iq = A.q[e * A.q_epoch_stride + pos];
    const bool skip = iq == -1;
    bool bad = (unsigned)ip > (unsigned)NI || (unsigned)iv > (unsigned)NI || (!skip && (unsigned)iq > (unsigned)NI);
    double a = 1.0, b = 1.0;
    if (PRME) {
      double d = 0.0;
      if (A.dist) d = A.dist[pos];
      else if (!bad) d = fs_cal_dis(A.cordi[2 * (size_t)ip], A.cordi[2 * (size_t)ip + 1], A.cordi[2 * (size_t)iv], A.cordi[2 * (size_t)iv + 1]);
      bad = bad || !(d >= 0.0) || isinf(d);
      const bool far = A.gap[pos] > A.thd;
      const double wgt = sqrt(sqrt(1.0 + (bad ? 0.0 : d)));
      a = far ? 1.0 : wgt * (double)A.cw;
      b = far ? 0.0 : wgt * (1.0 - (double)A.cw);
      if (gl == 0 && e == 0) A.a_out[pos] = bad ? nan : a;
    }
    if (bad || skip) {
      if (gl == 0) *cdst = bad ? nan : 0.0;
      continue;
    }
    double s = 0.0;
    for (int col = gl * 4; col < D; col += 64) {
      const float4 yp = ld4(A.tab_pq + (size_t)ip * D + col), yq = ld4(A.tab_pq + (size_t)iq * D + col), yv = ld4(A.tab_prev + (size_t)iv * D + col);
      if (PRME) {
        // (yq - yv)^2 - (yp - yv)^2, the differences exact in float64
        const double q0 = (double)yq.x - (double)yv.x, q1 = (double)yq.y - (double)yv.y, q2 = (double)yq.z - (double)yv.z, q3 = (double)yq.w - (double)yv.w;
        const double p0 = (double)yp.x - (double)yv.x, p1 = (double)yp.y - (double)yv.y, p2 = (double)yp.z - (double)yv.z, p3 = (double)yp.w - (double)yv.w;
        s += q0 * q0 - p0 * p0; s += q1 * q1 - p1 * p1; s += q2 * q2 - p2 * p2; s += q3 * q3 - p3 * p3;
      } else {
        s = fma((double)yv.x, (double)yp.x - (double)yq.x, s); s = fma((double)yv.y, (double)yp.y - (double)yq.y, s);
        s = fma((double)yv.z, (double)yp.z - (double)yq.z, s); s = fma((double)yv.w, (double)yp.w - (double)yq.w, s);
      }
    }
    s = row_sum(s);
    if (gl == 0) *cdst = PRME ? b * s : s;
  }
}

hipError_t launch_foldin_terms(const FoldinTermsArgs& A, bool prme, int num_cu, hipStream_t st, Timing* tm) {
  const long long items = A.total * A.n_epoch, blocks = (items + 15) / 16;
  if (items <= 0) return hipSuccess;
  const long long cap = (long long)(num_cu > 0 ? num_cu : 256) * 32;
  const dim3 grid((unsigned)(blocks < cap ? blocks : cap));
  tm->begin("foldin_terms", st);
  if (prme) hipLaunchKernelGGL(foldin_terms_kernel<true>, grid, dim3(256), 0, st, A);
  else hipLaunchKernelGGL(foldin_terms_kernel<false>, grid, dim3(256), 0, st, A);
  tm->end(st);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// chain
template <int NJ, int K, int FORM>
__global__ __launch_bounds__(64) void foldin_pair_kernel(FoldinPairArgs A) {
  constexpr bool METRIC = FORM == FOLDIN_FORM_METRIC;
  const float* const Y = A.items;
  const int lane = lane_id(), gl = lane & 15;
  const int r = blockIdx.x * FOLDIN_USERS_PER_WAVE + (lane >> 4);
  const bool live = r < A.n;
  const int D = A.dim, NI = A.n_item, E = A.epochs, F = A.first;
  int base = 0, len = 0, bad = 0;
  if (live) {
    base = A.off[r];
    len = A.off[r + 1] - base;
    if (base < 0 || len < 0) { bad = 1; len = 0; base = 0; }
    // the first check-in of a history is no step when first = 1, so the loop never reads it: it is checked here
    if (F && len > 0 && (unsigned)A.p[base] > (unsigned)NI) bad = 1;
  }
  const int m = len > F ? len - F : 0;                  // steps of this user per epoch
  const long long total = (long long)m * E;             // steps of this user
  long long wave_total = total;
#pragma unroll
  for (int o = 32; o >= 16; o >>= 1) { const long long v = __shfl_xor(wave_total, o, 64); wave_total = v > wave_total ? v : wave_total; }
  wave_total = (long long)__builtin_amdgcn_readfirstlane((int)(wave_total >> 32)) << 32 | (unsigned)__builtin_amdgcn_readfirstlane((int)wave_total);

  // Every load of the loop is unconditional and straight-line: a lane without a column reads column 0, a step past the end reads row 0,
  // the offset table instead of ids and a dummy double instead of a / c; selects discard what they return.
  bool col_ok[NJ];
  int colc[NJ];
  double w[NJ][4];
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int col = gl * 4 + 64 * j;
    col_ok[j] = live && col < D;
    colc[j] = col < D ? col : 0;
    const float4 v = (col_ok[j] && A.w0) ? ld4(A.w0 + (size_t)r * D + col) : make_float4(0.f, 0.f, 0.f, 0.f);
    w[j][0] = v.x; w[j][1] = v.y; w[j][2] = v.z; w[j][3] = v.w;
  }
  const int* pp = A.p + base + F;
  const int* qq = A.q + base + F;
  const double* const dummy = A.dummy;
  const double* aa = A.a ? A.a + base + F : dummy;
  const double* cc = A.c ? A.c + base + F : dummy;
  const bool has_a = METRIC && A.a != nullptr, has_c = A.c != nullptr;
  const double alpha = (double)A.alpha, lambda = (double)A.lambda;

  // id cursor: (ti, qi, ci) = position and epoch offsets of the next ids / terms to fetch; those of step s + K + j wait in slot j
  int ti = 0;
  long long qi = 0, ci = 0, si = 0;
  int idp[K], idq[K];
  double ida[K], idc[K];                                 // the step's a / c, fetched with its ids ...
  double sa[K], sc[K];                                   // ... and kept beside its rows until the step computes
  int ssk[K];                                            // 1: the step is skipped (negative -1)
  float4 rp[K][NJ], rq[K][NJ];
  auto fetch_ids = [&](int j) {
    const bool on = si < total;
    idp[j] = *(on ? pp + ti : A.off);
    idq[j] = *(on ? qq + qi + ti : A.off);
    if (METRIC) ida[j] = *((on && has_a) ? aa + ti : dummy);
    idc[j] = *((on && has_c) ? cc + ci + ti : dummy);
    const bool wrap = on && ti + 1 == m;
    ti = wrap ? 0 : ti + (on ? 1 : 0);
    qi += wrap ? A.q_epoch_stride : 0;
    ci += wrap ? A.c_epoch_stride : 0;
    ++si;
  };
  long long sr = 0;                                      // next step whose rows are fetched
  auto fetch_rows = [&](int j) {
    int ip = idp[j], iq = idq[j];
    const bool on = sr < total;
    const bool skip = iq == -1;
    const bool bp = (unsigned)ip > (unsigned)NI, bq = !skip && (unsigned)iq > (unsigned)NI;
    const double av = (METRIC && on && has_a) ? ida[j] : 1.0, cv = (on && has_c) ? idc[j] : 0.0;
    // a non-finite term is the terms pass's mark of an id or a distance it rejected
    bad |= (on && (bp || bq || !(fabs(av) < __builtin_inf()) || !(fabs(cv) < __builtin_inf()))) ? 1 : 0;
    sa[j] = av; sc[j] = cv; ssk[j] = skip ? 1 : 0;
    ip = bp ? 0 : ip;
    iq = (bq || skip) ? 0 : iq;
#pragma unroll
    for (int c = 0; c < NJ; ++c) {
      rp[j][c] = ld4(Y + (size_t)ip * D + colc[c]);
      rq[j][c] = ld4(Y + (size_t)iq * D + colc[c]);
    }
    ++sr;
  };
  // prologue: ids of steps 0 .. K - 1, their rows, ids of steps K .. 2 K - 1
#pragma unroll
  for (int j = 0; j < K; ++j) fetch_ids(j);
#pragma unroll
  for (int j = 0; j < K; ++j) { fetch_rows(j); fetch_ids(j); }

  int tc = 0, ec = 0;                                    // position and epoch of the step being computed
  double loss = 0.0;
  for (long long s0 = 0; s0 < wave_total; s0 += K) {
#pragma unroll
    for (int j = 0; j < K; ++j) {
      const bool on = s0 + j < total;
      const bool act = on && !ssk[j];                    // a skipped step: no update, no decay, no loss
      const double av = sa[j], cv = sc[j];
      double d[NJ][4], sm[METRIC ? NJ : 1][4];
#pragma unroll
      for (int c = 0; c < NJ; ++c) {
        d[c][0] = col_ok[c] ? (double)rp[j][c].x - (double)rq[j][c].x : 0.0; d[c][1] = col_ok[c] ? (double)rp[j][c].y - (double)rq[j][c].y : 0.0;
        d[c][2] = col_ok[c] ? (double)rp[j][c].z - (double)rq[j][c].z : 0.0; d[c][3] = col_ok[c] ? (double)rp[j][c].w - (double)rq[j][c].w : 0.0;
        if (METRIC) {
          sm[c][0] = (double)rp[j][c].x + (double)rq[j][c].x; sm[c][1] = (double)rp[j][c].y + (double)rq[j][c].y;
          sm[c][2] = (double)rp[j][c].z + (double)rq[j][c].z; sm[c][3] = (double)rp[j][c].w + (double)rq[j][c].w;
        }
      }
      fetch_rows(j);
      fetch_ids(j);
      double x = 0.0;
#pragma unroll
      for (int c = 0; c < NJ; ++c)
#pragma unroll
        for (int i = 0; i < 4; ++i) x = METRIC ? fma(d[c][i], 2.0 * w[c][i] - sm[c][i], x) : fma(w[c][i], d[c][i], x);
      x = row_sum(x);
      x = METRIC ? fma(av, x, cv) : x + cv;
      // e = exp(-|x|):  sigmoid(-x) = x >= 0 ? e / (1 + e) : 1 / (1 + e),  -log sigmoid(x) = max(-x, 0) + log1p(e)
      const double e = exp(-fabs(x));
      const double sg = (x >= 0.0 ? e : 1.0) / (1.0 + e);
      const double g = METRIC ? sg * (2.0 * av) : sg;
      loss += act ? fmax(-x, 0.0) + log1p(e) : 0.0;
#pragma unroll
      for (int c = 0; c < NJ; ++c)
#pragma unroll
        for (int i = 0; i < 4; ++i) w[c][i] = act ? w[c][i] - alpha * (fma(lambda, w[c][i], -g * d[c][i])) : w[c][i];
      if (on && ++tc == m) {
        if (A.loss_out && gl == 0) A.loss_out[(size_t)r * E + ec] = (float)loss;
        loss = 0.0; tc = 0; ++ec;
      }
    }
  }
  if (!live) return;
  const float nan = __builtin_nanf("");
  if (A.loss_out && (bad || m == 0))
    for (int e = gl; e < E; e += 16) A.loss_out[(size_t)r * E + e] = bad ? nan : 0.f;
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    if (!col_ok[j]) continue;
    const float4 v = bad ? make_float4(nan, nan, nan, nan) : make_float4((float)w[j][0], (float)w[j][1], (float)w[j][2], (float)w[j][3]);
    st4(A.w_out + (size_t)r * D + gl * 4 + 64 * j, v);
  }
  if (bad && gl == 0) atomicAdd(A.bad, 1);
}

hipError_t launch_foldin_pair(const FoldinPairArgs& A, hipStream_t st, Timing* tm) {
  const dim3 grid((unsigned)((A.n + FOLDIN_USERS_PER_WAVE - 1) / FOLDIN_USERS_PER_WAVE));
  const int nj = (A.dim + 63) / 64;
  if (nj < 1 || nj > 4) return hipErrorInvalidValue;
  tm->begin("foldin_pair", st);
#define FOLDIN_PAIR_LAUNCH(NJ, KD, KM)                                                                                                   \
  if (A.form == FOLDIN_FORM_METRIC) hipLaunchKernelGGL((foldin_pair_kernel<NJ, KM, FOLDIN_FORM_METRIC>), grid, dim3(64), 0, st, A);      \
  else hipLaunchKernelGGL((foldin_pair_kernel<NJ, KD, FOLDIN_FORM_DOT>), grid, dim3(64), 0, st, A)
  // ring depth per form: the metric form keeps y_p + y_q beside the difference, so at dim 65 .. 128 its ring is shallower (K = 4 there
  // costs 268 registers and the second wave of the SIMD)
  switch (nj) {
    case 1: FOLDIN_PAIR_LAUNCH(1, 4, 4); break;
    case 2: FOLDIN_PAIR_LAUNCH(2, 4, 2); break;
    case 3: FOLDIN_PAIR_LAUNCH(3, 2, 2); break;
    default: FOLDIN_PAIR_LAUNCH(4, 2, 2); break;
  }
#undef FOLDIN_PAIR_LAUNCH
  tm->end(st);
  return hipGetLastError();
}

}  // namespace poi
