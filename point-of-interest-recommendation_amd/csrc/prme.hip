// PRME (prog_prme.py, public/PRME.py, public/PRPRM.py, public/Load_Data_prme.py): the batched metric-embedding step and the geo-weighted
// all-POI scoring with a fused top-K.
//
// Step (OboPrme.__theano_train__, PRME.py:173-214), per transition (u, p = POI at i, q = negative, prev = POI at i-1, d = dist[i], gap[i]):
//   far = gap > threshold,  w = (1 + d)^0.25 (float64),  a = far ? 1 : w cw,  b = far ? 0 : w (1 - cw)
//   Dp = a |du - dp_p|^2 + b |ds_p - ds_prev|^2,  Dq = a |du - dp_q|^2 + b |ds_q - ds_prev|^2,  x = Dq - Dp
//   loss = log sigmoid(x),  g = sigmoid(-x);  each of the 7 gathered rows: row += alpha (g dx/drow - lambda row)
//     dx/ddu = 2a (dp_p - dp_q)    dx/ddp_p = 2a (du - dp_p)     dx/ddp_q = -2a (du - dp_q)    dx/ddp_prev = 0
//     dx/dds_p = -2b (ds_p - ds_prev)    dx/dds_q = 2b (ds_q - ds_prev)    dx/dds_prev = 2b (ds_p - ds_q)
// set_subtensor with a repeated index keeps the LAST occurrence in the order (p, q, prev): the losing occurrence of a duplicate row is keyed
// as the sentinel here (it adds nothing, not even its multiplicity).  dp[prev] - and in the far branch all three ds rows - still get the L2
// decay.  The rest is fpmc.hip's design: 7 n touches keyed by (table, row) in one key space [du | dp | ds], te_scatter.hip's stable radix
// sort, every run of equal keys summed in sorted order (runs cut by a 64-touch window joined by prme_span), new rows into per-launch slots,
// copied into the tables by prme_commit after every gradient has read the launch-entry values.  No float atomics.  A rejected transition
// (an id outside its table, p == q, d not finite or < 0) keys all 7 touches as the sentinel, gets a NaN loss and is counted once.
//
// Scoring (PrmeBasic.compute_sub_all_scores, PRME.py:117-139) of a row (user u, query POI l) against a candidate j < n_item:
//   score = -(1 + cal_dis(l, j))^0.25 (cw |du_u - dp_j|^2 + (1 - cw) |ds_l - ds_j|^2)
// The squared distances are direct float32 differences (no dot-product expansion, which cancels for near rows); the weight is float64 in
// cal_dis's operation order (Load_Data_prme.py:24-35: rad(x) = x pi / 180, sin^2 halves, R = 6378.137), (.)^0.25 as two square roots.
// A block owns PS_ROWS rows staged in LDS; each thread one candidate at a time, its dp / ds rows read once for all the block's rows.  The
// fused top-K keeps, per (wave, row), a 64-entry list sorted by score_topk's rule (higher score, then lower id) in LDS: a wave's 64 new
// scores of a row are merged only when one of them beats the list's K-th entry (bitonic sort, then the half-cleaner merge of two sorted
// lists); at the end the block's 4 lists of a row are merged the same way.
#include "poi_common.h"
#include "poi_kernels.h"
#include "topk_list.h"

namespace poi {

__device__ __forceinline__ float pr_sq4(float4 a, float4 b, float acc) {
  const float x = a.x - b.x, y = a.y - b.y, z = a.z - b.z, w = a.w - b.w;
  return fmaf(w, w, fmaf(z, z, fmaf(y, y, fmaf(x, x, acc))));
}

__device__ __forceinline__ const float* prme_row(const PrmeArgs& A, int key) {
  const int D = A.dim, R = A.n_item + 1;
  if (key < A.n_user) return A.du + (size_t)key * D;
  const int k2 = key - A.n_user;
  return k2 < R ? A.dp + (size_t)k2 * D : A.ds + (size_t)(k2 - R) * D;
}

// one pass over the transitions at the launch-entry values: 2 a g, 2 b g, loss, the 7 keys (touch e = kind n + t, kinds
// 0 du[u], 1 dp[p], 2 dp[q], 3 dp[prev], 4 ds[p], 5 ds[q], 6 ds[prev])
template <int LPT>
__global__ __launch_bounds__(256) void prme_fwd_kernel(PrmeArgs A) {
  const int gl = threadIdx.x % LPT, gpb = 256 / LPT;
  const int D = A.dim, n = A.n, R = A.n_item + 1, nu = A.n_user;
  if (blockIdx.x == 0 && threadIdx.x == 0) A.cnt[0] = 7 * n;
  for (int t = blockIdx.x * gpb + threadIdx.x / LPT; t < n; t += gridDim.x * gpb) {
    const int u = A.u[t], p = A.p[t], q = A.q[t], pv = A.prev[t];
    const double d = A.d[t];
    const bool bad = (unsigned)u >= (unsigned)nu || (unsigned)p >= (unsigned)R || (unsigned)q >= (unsigned)R || (unsigned)pv >= (unsigned)R ||
                     p == q || !(d >= 0.0) || isinf(d);
    if (bad) {
      if (gl == 0) { atomicAdd(A.bad, 1); A.loss[t] = __int_as_float(0x7fc00000); A.ga[t] = 0.f; A.gb[t] = 0.f; }
      if (gl < 7) A.keys0[(size_t)gl * n + t] = A.sentinel;
      continue;
    }
    const bool far = A.gap[t] > A.thd;
    const double w = sqrt(sqrt(1.0 + d));
    const float a = far ? 1.f : (float)(w * (double)A.cw), b = far ? 0.f : (float)(w * (double)(1.f - A.cw));
    float dpp = 0.f, dpq = 0.f, dsp = 0.f, dsq = 0.f;
    for (int c = gl * 4; c < D; c += LPT * 4) {
      const float4 U = ld4(A.du + (size_t)u * D + c), Pp = ld4(A.dp + (size_t)p * D + c), Pq = ld4(A.dp + (size_t)q * D + c);
      const float4 Sp = ld4(A.ds + (size_t)p * D + c), Sq = ld4(A.ds + (size_t)q * D + c), Sv = ld4(A.ds + (size_t)pv * D + c);
      dpp = pr_sq4(U, Pp, dpp); dpq = pr_sq4(U, Pq, dpq); dsp = pr_sq4(Sp, Sv, dsp); dsq = pr_sq4(Sq, Sv, dsq);
    }
    dpp = xor_group_sum<LPT>(dpp); dpq = xor_group_sum<LPT>(dpq); dsp = xor_group_sum<LPT>(dsp); dsq = xor_group_sum<LPT>(dsq);
    const float x = (a * dpq + b * dsq) - (a * dpp + b * dsp);
    if (gl == 0) {
      const float g = sigmoidf_(-x);
      A.loss[t] = log_sigmoidf_(x); A.ga[t] = 2.f * a * g; A.gb[t] = 2.f * b * g;
    }
    if (gl < 7) {
      // last occurrence wins in (p, q, prev): p loses to prev, q loses to prev (p == q is rejected above)
      const int tb = gl == 0 ? 0 : gl < 4 ? 1 : 2, k = gl == 0 ? 0 : (gl - 1) % 3;
      const int row = gl == 0 ? u : k == 0 ? p : k == 1 ? q : pv;
      const bool lost = k < 2 && gl > 0 && row == pv;
      A.keys0[(size_t)gl * n + t] = lost ? A.sentinel : tb == 0 ? u : tb == 1 ? nu + row : nu + R + row;
    }
  }
}

// the loss-gradient part g dx/drow of touch e (component col .. col+3)
__device__ __forceinline__ float4 prme_grad(const PrmeArgs& A, int e, int col) {
  const int n = A.n, D = A.dim, kind = e / n, t = e - kind * n;
  if (kind == 3) return make_float4(0.f, 0.f, 0.f, 0.f);
  float s;
  float4 v;
  if (kind <= 2) {
    s = A.ga[t];
    const float4 U = ld4(A.du + (size_t)A.u[t] * D + col);
    if (kind == 0) v = sub4(ld4(A.dp + (size_t)A.p[t] * D + col), ld4(A.dp + (size_t)A.q[t] * D + col));
    else if (kind == 1) v = sub4(U, ld4(A.dp + (size_t)A.p[t] * D + col));
    else v = sub4(ld4(A.dp + (size_t)A.q[t] * D + col), U);
  } else {
    s = A.gb[t];
    const float4 Sp = ld4(A.ds + (size_t)A.p[t] * D + col), Sq = ld4(A.ds + (size_t)A.q[t] * D + col);
    if (kind == 6) v = sub4(Sp, Sq);
    else {
      const float4 Sv = ld4(A.ds + (size_t)A.prev[t] * D + col);
      v = kind == 4 ? sub4(Sv, Sp) : sub4(Sq, Sv);
    }
  }
  return make_float4(s * v.x, s * v.y, s * v.z, s * v.w);
}

// row <- row + alpha min(k, cap) (G / k - lambda row), into the slot of the run's first sorted position
__device__ __forceinline__ void prme_apply(const PrmeArgs& A, int key, float4 G, int k, int col, int slot) {
  const float4 r = ld4(prme_row(A, key) + col);
  const float sc = A.alpha * fminf((float)k, A.bcap), inv = 1.0f / (float)k, lm = A.lambda;
  *reinterpret_cast<float4*>(A.slot + (size_t)slot * A.dim + col) =
      make_float4(r.x + sc * (G.x * inv - lm * r.x), r.y + sc * (G.y * inv - lm * r.y), r.z + sc * (G.z * inv - lm * r.z), r.w + sc * (G.w * inv - lm * r.w));
}

// one wave per window of 64 sorted touches; LPR lanes per row (one float4 each, D <= 4 LPR), EPW = 64 / LPR touches of a run per pass
template <int LPR>
__global__ __launch_bounds__(256) void prme_chunk_kernel(PrmeArgs A) {
  constexpr int EPW = 64 / LPR;
  const int lane = lane_id(), grp = lane / LPR, gl = lane % LPR;
  const int D = A.dim, N = 7 * A.n, col = gl * 4;
  const bool has = col < D;
  const int n_chunk = (N + 63) / 64;
  for (int c = blockIdx.x * 4 + wave_id(); c < n_chunk; c += gridDim.x * 4) {
    const int j0 = 64 * c, nv = min(64, N - j0);
    const bool valid = lane < nv;
    const int key = valid ? A.ks[j0 + lane] : -1;
    const int val = valid ? A.vs[j0 + lane] : 0;
    const int up = __shfl_up(key, 1, 64);
    const int prev = lane == 0 ? (c > 0 ? A.ks[j0 - 1] : -2) : up;
    const int nextk = (j0 + nv < N) ? A.ks[j0 + nv] : -3;
    const unsigned long long starts = __ballot(valid && key != prev);
    int lead_cnt = 0, lead_more = 0, trail_cnt = 0, trail_row = -1;
    int a = 0;
    while (a < nv) {
      const unsigned long long above = a + 1 < 64 ? (starts >> (a + 1)) << (a + 1) : 0ull;
      const int b = above ? min(nv, (int)__builtin_ctzll(above)) : nv;
      const int row = __builtin_amdgcn_readfirstlane(__shfl(key, a, 64));
      if (row == A.sentinel) break;      // lost occurrences and rejected transitions sort last: nothing after them
      const bool cont_before = a == 0 && !(starts & 1ull);
      const bool cont_after = b == nv && nextk == row;
      float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
      for (int e0 = a; e0 < b; e0 += EPW) {
        const int idx = e0 + grp;
        const int e = __shfl(val, idx & 63, 64);
        if (idx < b && has) {
          const float4 v = prme_grad(A, e, col);
          acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
        }
      }
#pragma unroll
      for (int o = LPR; o < 64; o <<= 1) {
        acc.x += __shfl_xor(acc.x, o, 64); acc.y += __shfl_xor(acc.y, o, 64);
        acc.z += __shfl_xor(acc.z, o, 64); acc.w += __shfl_xor(acc.w, o, 64);
      }
      if (!cont_before && !cont_after) {
        if (grp == 0 && has) prme_apply(A, row, acc, b - a, col, j0 + a);
      } else {
        if (grp == 0 && has) *reinterpret_cast<float4*>((cont_before ? A.lead : A.trail) + (size_t)c * D + col) = acc;
        if (cont_before) { lead_cnt = b - a; lead_more = cont_after ? 1 : 0; }
        else { trail_cnt = b - a; trail_row = row; }
      }
      a = b;
    }
    if (lane == 0) A.meta[c] = make_int4(lead_cnt, lead_more, trail_cnt, trail_row);
  }
}

// runs cut by window boundaries: the window where a run starts owns it and adds the following windows' opening runs in order
template <int LPR>
__global__ __launch_bounds__(256) void prme_span_kernel(PrmeArgs A) {
  constexpr int EPW = 64 / LPR;
  const int lane = lane_id(), grp = lane / LPR, gl = lane % LPR;
  const int D = A.dim, col = gl * 4, n_chunk = (7 * A.n + 63) / 64;
  for (int c = (blockIdx.x * 4 + wave_id()) * EPW + grp; c < n_chunk; c += gridDim.x * 4 * EPW) {
    const int4 m = A.meta[c];
    if (m.z == 0 || col >= D) continue;
    float4 sum = ld4(A.trail + (size_t)c * D + col);
    int k = m.z;
    for (int c2 = c + 1; c2 < n_chunk; ++c2) {
      const int4 m2 = A.meta[c2];
      const float4 v = ld4(A.lead + (size_t)c2 * D + col);
      sum = make_float4(sum.x + v.x, sum.y + v.y, sum.z + v.z, sum.w + v.w);
      k += m2.x;
      if (!m2.y) break;
    }
    prme_apply(A, m.w, sum, k, col, 64 * c + 64 - m.z);
  }
}

// every run's new row (slot of its first sorted position) -> its table, after all gradients have read the entry values
template <int LPR>
__global__ __launch_bounds__(256) void prme_commit_kernel(PrmeArgs A) {
  constexpr int EPW = 64 / LPR;
  const int lane = lane_id(), grp = lane / LPR, gl = lane % LPR;
  const int D = A.dim, col = gl * 4, N = 7 * A.n;
  for (int e = (blockIdx.x * 4 + wave_id()) * EPW + grp; e < N; e += gridDim.x * 4 * EPW) {
    const int key = A.ks[e];
    if (col >= D || key == A.sentinel || (e > 0 && A.ks[e - 1] == key)) continue;
    *reinterpret_cast<float4*>(const_cast<float*>(prme_row(A, key)) + col) = ld4(A.slot + (size_t)e * D + col);
  }
}

template <int LPR>
static hipError_t launch_prme_step_t(PrmeArgs& A, int num_cu, hipStream_t st, Timing* tm) {
  const int n = A.n;
  auto grid = [&](long long items, int per) { return dim3((unsigned)max(1ll, min((long long)num_cu * 16, (items + per - 1) / per))); };
  tm->begin("prme_fwd", st);
  hipLaunchKernelGGL(prme_fwd_kernel<LPR>, grid(n, 256 / LPR), dim3(256), 0, st, A);
  tm->end(st);
  tm->begin("prme_sort", st);
  int bits = 1;
  while ((1ll << bits) <= (long long)A.sentinel) ++bits;
  const int *ks = nullptr, *vs = nullptr;
  hipError_t e = launch_radix_sort(A.keys0, A.keys1, A.vals0, A.vals1, A.cnt, bits, A.hist, st, &ks, &vs);
  if (e != hipSuccess) return e;
  A.ks = ks; A.vs = vs;
  tm->end(st);
  const long long chunks = (7ll * n + 63) / 64;
  tm->begin("prme_rows", st);
  hipLaunchKernelGGL(prme_chunk_kernel<LPR>, grid(chunks, 4), dim3(256), 0, st, A);
  hipLaunchKernelGGL(prme_span_kernel<LPR>, grid(chunks, 4 * (64 / LPR)), dim3(256), 0, st, A);
  tm->end(st);
  tm->begin("prme_commit", st);
  hipLaunchKernelGGL(prme_commit_kernel<LPR>, grid(7ll * n, 4 * (64 / LPR)), dim3(256), 0, st, A);
  tm->end(st);
  return hipGetLastError();
}

hipError_t launch_prme_step(PrmeArgs& A, int num_cu, hipStream_t st, Timing* tm) {
  if (A.dim <= 32) return launch_prme_step_t<8>(A, num_cu, st, tm);
  if (A.dim <= 64) return launch_prme_step_t<16>(A, num_cu, st, tm);
  if (A.dim <= 128) return launch_prme_step_t<32>(A, num_cu, st, tm);
  return hipErrorInvalidValue;
}

// ---------------------------------------------------------------------------------------------
// Scoring
// ---------------------------------------------------------------------------------------------
#define PS_ROWS 16        // rows per block
#define PS_SPAN 2048      // candidates per block of the full-matrix kernel (grid.y)
#define PS_MAXD 128

// rad(x) of Load_Data_prme.py:20-21: np.multiply(x, np.pi) / 180.0
__device__ __forceinline__ double pr_rad(double x) { return x * 3.141592653589793 / 180.0; }

// (1 + cal_dis)^0.25 for query (rl1, ro1, cl1 = cos rl1) and candidate (rl2, ro2, cl2), cal_dis's operation order
__device__ __forceinline__ double pr_weight(double rl1, double ro1, double cl1, double rl2, double ro2, double cl2) {
#pragma clang fp contract(off)
  const double a = rl1 - rl2, b = ro1 - ro2;
  const double sa = sin(a / 2), sb = sin(b / 2);
  const double s = 2 * asin(sqrt(sa * sa + cl1 * cl2 * (sb * sb))) * 6378.137;
  return sqrt(sqrt(1 + s));
}

template <bool TOPK>
__global__ __launch_bounds__(256) void prme_score_kernel(PrmeScoreArgs A) {
  __shared__ __align__(16) float s_u[PS_ROWS][PS_MAXD], s_s[PS_ROWS][PS_MAXD];
  __shared__ double s_rl[PS_ROWS], s_ro[PS_ROWS], s_rc[PS_ROWS];
  __shared__ int s_ok[PS_ROWS];
  __shared__ float s_f[PS_ROWS][256];      // cw |du - dp_j|^2 + (1 - cw) |ds_l - ds_j|^2 of the thread's candidate
  __shared__ float s_ls[TOPK ? 4 : 1][TOPK ? PS_ROWS : 1][64];
  __shared__ int s_li[TOPK ? 4 : 1][TOPK ? PS_ROWS : 1][64];
  const int D = A.dim, N = A.n_item, tid = threadIdx.x, lane = lane_id(), w = wave_id();
  const int row0 = blockIdx.x * PS_ROWS, nr = min(PS_ROWS, A.n_rows - row0);
  if (tid < PS_ROWS) {
    int ok = 0;
    if (tid < nr) {
      const int u = A.users[row0 + tid], l = A.qpoi[row0 + tid];
      ok = (unsigned)u < (unsigned)A.n_user && (unsigned)l <= (unsigned)N;
      if (ok) {
        const double rl = pr_rad(A.coords[2 * (size_t)l]);
        s_rl[tid] = rl; s_ro[tid] = pr_rad(A.coords[2 * (size_t)l + 1]); s_rc[tid] = cos(rl);
      }
    }
    s_ok[tid] = ok;
  }
  for (int x = tid; x < PS_ROWS * D; x += 256) {
    const int r = x / D, c = x - r * D;
    float vu = 0.f, vs = 0.f;
    if (r < nr) {
      const int u = A.users[row0 + r], l = A.qpoi[row0 + r];
      if ((unsigned)u < (unsigned)A.n_user && (unsigned)l <= (unsigned)N) { vu = A.du[(size_t)u * D + c]; vs = A.ds[(size_t)l * D + c]; }
    }
    s_u[r][c] = vu; s_s[r][c] = vs;
  }
  if (TOPK) {
    for (int x = tid; x < 4 * PS_ROWS * 64; x += 256) { (&s_ls[0][0][0])[x] = -INFINITY; (&s_li[0][0][0])[x] = PAD_ID; }
  }
  __syncthreads();
  const float cw = A.cw, cw1 = 1.f - A.cw;
  const int j_beg = TOPK ? 0 : blockIdx.y * PS_SPAN, j_end = TOPK ? N : min(N, j_beg + PS_SPAN);
  for (int jt = j_beg; jt < j_end; jt += 256) {
    const int j = jt + tid;
    const bool valid = j < j_end;
    float accp[PS_ROWS], accs[PS_ROWS];
#pragma unroll
    for (int r = 0; r < PS_ROWS; ++r) { accp[r] = 0.f; accs[r] = 0.f; }
    double rl2 = 0.0, ro2 = 0.0, cl2 = 1.0;
    if (valid) {
      for (int c = 0; c < D; c += 4) {
        const float4 P = ld4(A.dp + (size_t)j * D + c), S = ld4(A.ds + (size_t)j * D + c);
#pragma unroll
        for (int r = 0; r < PS_ROWS; ++r) {
          accp[r] = pr_sq4(*reinterpret_cast<const float4*>(&s_u[r][c]), P, accp[r]);
          accs[r] = pr_sq4(*reinterpret_cast<const float4*>(&s_s[r][c]), S, accs[r]);
        }
      }
      rl2 = pr_rad(A.coords[2 * (size_t)j]); ro2 = pr_rad(A.coords[2 * (size_t)j + 1]); cl2 = cos(rl2);
    }
#pragma unroll
    for (int r = 0; r < PS_ROWS; ++r) s_f[r][tid] = cw * accp[r] + cw1 * accs[r];      // own column: no barrier needed
    for (int r = 0; r < nr; ++r) {
      const float wf = (float)pr_weight(s_rl[r], s_ro[r], s_rc[r], rl2, ro2, cl2);
      const float sc = s_ok[r] ? -wf * s_f[r][tid] : __int_as_float(0x7fc00000);
      if (!TOPK) {
        if (valid) A.out[(size_t)(row0 + r) * N + j] = sc;
      } else {
        lds_list_merge(s_ls[w][r], s_li[w][r], valid && s_ok[r] ? sc : -INFINITY, valid && s_ok[r] ? j : PAD_ID, A.k);
      }
    }
  }
  if (!TOPK) return;
  __syncthreads();
  // the block's 4 lists of a row -> one, wave w takes rows w, w + 4, ...
  for (int r = w; r < nr; r += 4) {
    float s = s_ls[0][r][lane];
    int i = s_li[0][r][lane];
    for (int v = 1; v < 4; ++v) {
      float rs = s_ls[v][r][63 - lane];
      int ri = s_li[v][r][63 - lane];
      if (better(s, i, rs, ri)) { rs = s; ri = i; }
#pragma unroll
      for (int jj = 32; jj > 0; jj >>= 1) {
        const float ps = __shfl_xor(rs, jj, 64);
        const int pi = __shfl_xor(ri, jj, 64);
        const bool mine = better(rs, ri, ps, pi);
        if (((lane & jj) == 0) != mine) { rs = ps; ri = pi; }
      }
      s = rs; i = ri;
    }
    if (lane < A.k) {
      const size_t o = (size_t)(row0 + r) * A.k + lane;
      const bool ok = s_ok[r];
      A.idx_out[o] = ok ? i : -1;
      if (A.sc_out) A.sc_out[o] = ok ? s : __int_as_float(0x7fc00000);
    }
  }
}

hipError_t launch_prme_score(PrmeScoreArgs& A, hipStream_t st) {
  const unsigned gx = (unsigned)((A.n_rows + PS_ROWS - 1) / PS_ROWS);
  if (A.k > 0) {
    hipLaunchKernelGGL(prme_score_kernel<true>, dim3(gx), dim3(256), 0, st, A);
  } else {
    hipLaunchKernelGGL(prme_score_kernel<false>, dim3(gx, (unsigned)((A.n_item + PS_SPAN - 1) / PS_SPAN)), dim3(256), 0, st, A);
  }
  return hipGetLastError();
}

}  // namespace poi
