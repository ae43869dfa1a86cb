// VBPR (OboVBpr, public/BPR.py:245-335): BPR-MF plus a fixed per-item feature table fi (n_item + 1, F) and a trained projection ei (D, F).
//   d = fi[p] - fi[q],  v = ei d,  x = ux[u] . (lt[p] - lt[q]) + ue[u] . v,  g = -sigmoid(-x),  loss = -log sigmoid(x)
//   ux[u] -= a (g (lt[p] - lt[q]) + l ux[u])    ue[u] -= a (g v + l ue[u])    lt[p] -= a (g ux[u] + l lt[p])    lt[q] -= a (-g ux[u] + l lt[q])
//   ei    -= a (g ue[u] (x) d + l_ev ei)                                                      every right-hand side at the launch-entry values
// The feature rows are F = 1024 floats against D <= 128 of an embedding row: the step's bytes are 2 F e per triple and pass, and both
// passes are matrix products over the SAME gathered difference matrix Dmat (n x F), which is never written to memory:
//   vbpr_fwd     V = Dmat ei^T (n x F . F x D): a wave owns 16 triples, a workgroup 64; per 64 columns of F the workgroup stages that
//                slice of ei and each wave its 16 x 64 tile of fi[p] - fi[q] in LDS; 16 k-steps of the float64 MFMA per slice and
//                16-column block of D.  The epilogue closes x in float64 (the lt / ux / ue part straight from the tables), writes g, loss,
//                V (float32, n x D: the ue touch needs g v), the accepted flag and the 4 keys of the triple.
//   vbpr_ord     accepted triples in launch order -> a dense list (one workgroup: count, scan, fill).  The dense gradient is chunked over
//                this list, so a rejected triple changes no chunk boundary: removing it from the launch leaves every sum bitwise the same.
//   vbpr_wgrad   d ei = G^T Dmat (D x n . n x F), G_i = g_i ue[u_i]: workgroup (row chunk c, 64 columns of F), a wave per 16 columns, all
//                of D in its accumulators; 16 accepted triples per LDS stage (Dmat tile gathered again: the second and last read of the
//                feature rows).  Partials (n_chunk, D, F) in float64.  The chunk count is a function of n alone (vbpr_chunking).
//   vbpr_dense   partials added in chunk order + the SGD / L2 step on ei, rounded once.
//   vbpr_chunk / _span / _commit   the 4 n row touches ux[u], ue[u], lt[p], lt[q] in one key space [ux | ue | lt], te_scatter.hip's
//                stable radix sort, runs of equal keys summed in sorted order (prme.hip's scheme: runs cut by a 64-touch window are joined
//                in window order, new rows go to per-launch slots and are copied into the tables after every reader has seen the entry
//                values).  A rejected triple keys its 4 touches as the sentinel (sorts last, adds nothing).
// Matrix cores: v_mfma_f64_16x16x4_f64 on float32 operands widened in registers.  The float32-input MFMA runs twice as fast, but its
// k-ordered float32 fma chain leaves ~1e-7 sum|a b| in x; with the reference's init x is a sum of 1024 products of magnitude ~10 and
// g = -sigmoid(-x) ~ e^-12 takes the ABSOLUTE error of x as its RELATIVE error - a few 1e-5 against a bar of 1e-4 per row of the update,
// and worse on hot rows.  In float64 the products are exact and the sums carry 1e-16; the kernels are bound by the feature gathers either way.
// No float atomics anywhere: identical launches give bitwise identical tables on any grid (every work item is a function of the launch alone).
// Scoring side (vbpr_fwd<ITEMS>): items_out = [lt | fi ei^T], the same product over the table rows instead of triples.
#include "poi_common.h"
#include "poi_kernels.h"

namespace poi {

#define VB_LD 68      // LDS row stride (floats) of a 64-column tile: 16-byte aligned rows, the MFMA operand reads hit 64 distinct banks

typedef double vb_d4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ const float* vbpr_row(const VbprArgs& A, int key) {
  const int D = A.dim, nu = A.n_user;
  if (key < nu) return A.ux + (size_t)key * D;
  if (key < 2 * nu) return A.ue + (size_t)(key - nu) * D;
  return A.lt + (size_t)(key - 2 * nu) * D;
}

// MODE 0: the step's forward pass over triples.  MODE 1: items_out = [lt | fi ei^T] over the n_rows table rows.
template <int NB, int MODE>
__global__ __launch_bounds__(256) void vbpr_fwd_kernel(VbprArgs A) {
  __shared__ __align__(16) float s_e[NB * 16][VB_LD];
  __shared__ __align__(16) float s_d[4][16][VB_LD];
  const int tid = threadIdx.x, lane = lane_id(), w = wave_id();
  const int D = A.dim, F = A.n_img, nu = A.n_user, NI = A.n_item;
  const int R = MODE ? A.n_rows : A.n;
  const int n_tile = (R + 63) / 64;
  const int lr = lane & 15, lk = lane >> 4;
  if (MODE == 0 && blockIdx.x == 0 && tid == 0) A.cnt[0] = 4 * A.n;
  for (int tile = blockIdx.x; tile < n_tile; tile += gridDim.x) {
    const int r0 = tile * 64 + w * 16;
    // the four staging rows of this lane (pass * 4 + lk): feature-row offsets, -1 = no row
    long long po[4], qo[4];
#pragma unroll
    for (int ps = 0; ps < 4; ++ps) {
      const int row = r0 + ps * 4 + lk;
      po[ps] = -1; qo[ps] = -1;
      if (row < R) {
        if (MODE) po[ps] = (long long)row * F;
        else {
          po[ps] = (long long)min((unsigned)A.p[row], (unsigned)NI) * F;      // (ids clamped into the table: a rejected triple reads in bounds and moves nothing)
          qo[ps] = (long long)min((unsigned)A.q[row], (unsigned)NI) * F;
        }
      }
    }
    vb_d4 acc[NB];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) acc[nb] = (vb_d4){0.0, 0.0, 0.0, 0.0};
    for (int k0 = 0; k0 < F; k0 += 64) {
      __syncthreads();
      for (int x = tid; x < NB * 16 * 16; x += 256) {
        const int r = x >> 4, c4 = (x & 15) * 4;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (r < D && k0 + c4 < F) v = ld4(A.ei + (size_t)r * F + k0 + c4);
        *reinterpret_cast<float4*>(&s_e[r][c4]) = v;
      }
#pragma unroll
      for (int ps = 0; ps < 4; ++ps) {
        const int c4 = lr * 4;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (po[ps] >= 0 && k0 + c4 < F) {
          v = ld4(A.fi + po[ps] + k0 + c4);
          if (!MODE) {
            const float4 b = ld4(A.fi + qo[ps] + k0 + c4);
            v = make_float4(v.x - b.x, v.y - b.y, v.z - b.z, v.w - b.w);
          }
        }
        *reinterpret_cast<float4*>(&s_d[w][ps * 4 + lk][c4]) = v;
      }
      __syncthreads();
#pragma unroll 4
      for (int kk = 0; kk < 16; ++kk) {
        const double a = (double)s_d[w][lr][kk * 4 + lk];
#pragma unroll
        for (int nb = 0; nb < NB; ++nb)
          acc[nb] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, (double)s_e[nb * 16 + lr][kk * 4 + lk], acc[nb], 0, 0, 0);
      }
    }
    // acc[nb][r]: row r0 + lk + 4 r, column nb * 16 + lr
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = r0 + lk + 4 * r;
      const bool live = row < R;
      if (MODE) {
        if (live) {
#pragma unroll
          for (int nb = 0; nb < NB; ++nb) {
            const int col = nb * 16 + lr;
            if (col < D) {
              A.out[(size_t)row * 2 * D + D + col] = (float)acc[nb][r];
              A.out[(size_t)row * 2 * D + col] = A.lt[(size_t)row * D + col];
            }
          }
        }
        continue;
      }
      const int t = live ? row : 0;
      const int u = A.uidx[t], p = A.p[t], q = A.q[t];
      const bool bad = (unsigned)u >= (unsigned)nu || (unsigned)p > (unsigned)NI || (unsigned)q > (unsigned)NI || p == q;
      const size_t uo = (size_t)min((unsigned)u, (unsigned)(nu - 1)) * D, pr = (size_t)min((unsigned)p, (unsigned)NI) * D, qr = (size_t)min((unsigned)q, (unsigned)NI) * D;
      double x = 0.0;
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) {
        const int col = nb * 16 + lr;
        if (col < D) {
          x = fma((double)A.ue[uo + col], acc[nb][r], x);
          x = fma((double)A.ux[uo + col], (double)A.lt[pr + col] - (double)A.lt[qr + col], x);
          if (live) A.V[(size_t)row * D + col] = (float)acc[nb][r];
        }
      }
#pragma unroll
      for (int o = 1; o < 16; o <<= 1) x += __shfl_xor(x, o, 64);
      if (live && lr == 0) {
        if (bad) {
          atomicAdd(A.bad, 1);
          A.g[row] = 0.f; A.loss[row] = __int_as_float(0x7fc00000); A.okf[row] = 0;
        } else {
          A.g[row] = (float)(-1.0 / (1.0 + exp(x)));
          A.loss[row] = (float)(x >= 0.0 ? log1p(exp(-x)) : log1p(exp(x)) - x);
          A.okf[row] = 1;
        }
      }
      if (live && lr < 4) {      // touch kinds 0 ux[u], 1 ue[u], 2 lt[p], 3 lt[q]
        const int key = bad ? A.sentinel : lr == 0 ? u : lr == 1 ? nu + u : 2 * nu + (lr == 2 ? p : q);
        A.keys0[(size_t)lr * A.n + row] = key;
      }
    }
  }
}

// accepted triples, in launch order -> ord[0 .. n_acc), n_acc -> cnt[1].  One workgroup.
__global__ __launch_bounds__(256) void vbpr_ord_kernel(VbprArgs A) {
  __shared__ int s_c[256];
  const int tid = threadIdx.x, n = A.n;
  const int per = (n + 255) / 256, b = min(n, tid * per), e = min(n, b + per);
  int c = 0;
  for (int i = b; i < e; ++i) c += A.okf[i];
  s_c[tid] = c;
  __syncthreads();
  if (tid == 0) {
    int run = 0;
    for (int i = 0; i < 256; ++i) { const int t = s_c[i]; s_c[i] = run; run += t; }
    A.cnt[1] = run;
  }
  __syncthreads();
  int o = s_c[tid];
  for (int i = b; i < e; ++i) if (A.okf[i]) A.ord[o++] = i;
}

// d ei partial of (row chunk, 64 columns of F)
template <int NB>
__global__ __launch_bounds__(256) void vbpr_wgrad_kernel(VbprArgs A) {
  __shared__ __align__(16) float s_d[16][VB_LD];
  __shared__ __align__(16) float s_u[16][NB * 16 + 4];
  __shared__ float s_g[16];
  const int tid = threadIdx.x, lane = lane_id(), w = wave_id();
  const int D = A.dim, F = A.n_img;
  const int lr = lane & 15, lk = lane >> 4;
  const int n_ft = (F + 63) / 64, work = n_ft * A.n_chunk;
  const int n_acc = A.cnt[1];
  for (int wk = blockIdx.x; wk < work; wk += gridDim.x) {
    const int c = wk / n_ft, f0 = (wk - c * n_ft) * 64;
    const int j_beg = c * A.ch_rows, j_end = min(j_beg + A.ch_rows, n_acc);
    vb_d4 acc[NB];
#pragma unroll
    for (int mb = 0; mb < NB; ++mb) acc[mb] = (vb_d4){0.0, 0.0, 0.0, 0.0};
    for (int j0 = j_beg; j0 < j_end; j0 += 16) {
      __syncthreads();
      {
        const int rr = tid >> 4, c4 = (tid & 15) * 4, j = j0 + rr;
        const int t = j < j_end ? A.ord[j] : -1;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (t >= 0 && f0 + c4 < F) {
          const float4 a = ld4(A.fi + (size_t)A.p[t] * F + f0 + c4), b = ld4(A.fi + (size_t)A.q[t] * F + f0 + c4);
          v = make_float4(a.x - b.x, a.y - b.y, a.z - b.z, a.w - b.w);
        }
        *reinterpret_cast<float4*>(&s_d[rr][c4]) = v;
        if (tid < 16) { const int j2 = j0 + tid; s_g[tid] = j2 < j_end ? A.g[A.ord[j2]] : 0.f; }
      }
      for (int x = tid; x < 16 * NB * 4; x += 256) {
        const int rr = x / (NB * 4), c4 = (x - rr * NB * 4) * 4, j = j0 + rr;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (j < j_end && c4 < D) v = ld4(A.ue + (size_t)A.uidx[A.ord[j]] * D + c4);
        *reinterpret_cast<float4*>(&s_u[rr][c4]) = v;
      }
      __syncthreads();
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) {
        const int k = kk * 4 + lk;
        const double gk = (double)s_g[k], b = (double)s_d[k][w * 16 + lr];
#pragma unroll
        for (int mb = 0; mb < NB; ++mb)
          acc[mb] = __builtin_amdgcn_mfma_f64_16x16x4f64(gk * (double)s_u[k][mb * 16 + lr], b, acc[mb], 0, 0, 0);
      }
    }
    const int f = f0 + w * 16 + lr;
    if (f < F) {
#pragma unroll
      for (int mb = 0; mb < NB; ++mb)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int d = mb * 16 + lk + 4 * r;
          if (d < D) A.dpart[((size_t)c * D + d) * F + f] = acc[mb][r];
        }
    }
  }
}

// ei -= alpha min(n_acc, cap) (sum of the chunk partials in chunk order / n_acc + lambda_ev ei)
__global__ __launch_bounds__(256) void vbpr_dense_kernel(VbprArgs A) {
  const int n_acc = A.cnt[1];
  if (n_acc == 0) return;
  const size_t tot = (size_t)A.dim * A.n_img;
  const double sc = (double)A.alpha * fmin((double)n_acc, (double)A.bcap), inv = 1.0 / (double)n_acc, lm = (double)A.lambda_ev;
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < tot; e += (size_t)gridDim.x * 256) {
    double s = 0.0;
    for (int c = 0; c < A.n_chunk; ++c) s += A.dpart[(size_t)c * tot + e];
    const double v = (double)A.ei[e];
    A.ei[e] = (float)(v - sc * (s * inv + lm * v));
  }
}

// the loss-gradient part of touch e (components col .. col + 3)
__device__ __forceinline__ float4 vbpr_grad(const VbprArgs& A, int e, int col) {
  const int n = A.n, D = A.dim, kind = e / n, t = e - kind * n;
  float s = A.g[t];
  float4 v;
  if (kind == 0) {
    const float4 a = ld4(A.lt + (size_t)A.p[t] * D + col), b = ld4(A.lt + (size_t)A.q[t] * D + col);
    v = make_float4(a.x - b.x, a.y - b.y, a.z - b.z, a.w - b.w);
  } else if (kind == 1) v = ld4(A.V + (size_t)t * D + col);
  else { v = ld4(A.ux + (size_t)A.uidx[t] * D + col); if (kind == 3) s = -s; }
  return make_float4(s * v.x, s * v.y, s * v.z, s * v.w);
}

// row <- row - alpha min(k, cap) (G / k + lambda row), into the slot of the run's first sorted position
__device__ __forceinline__ void vbpr_apply(const VbprArgs& A, int key, float4 G, int k, int col, int slot) {
  const float4 r = ld4(vbpr_row(A, key) + col);
  const float sc = A.alpha * fminf((float)k, A.bcap), inv = 1.0f / (float)k, lm = A.lambda;
  *reinterpret_cast<float4*>(A.slot + (size_t)slot * A.dim + col) =
      make_float4(r.x - sc * (G.x * inv + lm * r.x), r.y - sc * (G.y * inv + lm * r.y), r.z - sc * (G.z * inv + lm * r.z), r.w - sc * (G.w * inv + lm * r.w));
}

// one wave per window of 64 sorted touches; LPR lanes per row (one float4 each, D <= 4 LPR), EPW = 64 / LPR touches of a run per pass
template <int LPR>
__global__ __launch_bounds__(256) void vbpr_chunk_kernel(VbprArgs A) {
  constexpr int EPW = 64 / LPR;
  const int lane = lane_id(), grp = lane / LPR, gl = lane % LPR;
  const int D = A.dim, N = 4 * A.n, col = gl * 4;
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
      if (row == A.sentinel) break;      // rejected triples sort last: nothing after them
      const bool cont_before = a == 0 && !(starts & 1ull);
      const bool cont_after = b == nv && nextk == row;
      float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
      for (int e0 = a; e0 < b; e0 += EPW) {
        const int idx = e0 + grp;
        const int e = __shfl(val, idx & 63, 64);
        if (idx < b && has) {
          const float4 v = vbpr_grad(A, e, col);
          acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
        }
      }
#pragma unroll
      for (int o = LPR; o < 64; o <<= 1) {
        acc.x += __shfl_xor(acc.x, o, 64); acc.y += __shfl_xor(acc.y, o, 64);
        acc.z += __shfl_xor(acc.z, o, 64); acc.w += __shfl_xor(acc.w, o, 64);
      }
      if (!cont_before && !cont_after) {
        if (grp == 0 && has) vbpr_apply(A, row, acc, b - a, col, j0 + a);
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
__global__ __launch_bounds__(256) void vbpr_span_kernel(VbprArgs A) {
  constexpr int EPW = 64 / LPR;
  const int lane = lane_id(), grp = lane / LPR, gl = lane % LPR;
  const int D = A.dim, col = gl * 4, n_chunk = (4 * A.n + 63) / 64;
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
    vbpr_apply(A, m.w, sum, k, col, 64 * c + 64 - m.z);
  }
}

// every run's new row (slot of its first sorted position) -> its table, after all gradients have read the entry values
template <int LPR>
__global__ __launch_bounds__(256) void vbpr_commit_kernel(VbprArgs A) {
  constexpr int EPW = 64 / LPR;
  const int lane = lane_id(), grp = lane / LPR, gl = lane % LPR;
  const int D = A.dim, col = gl * 4, N = 4 * A.n;
  for (int e = (blockIdx.x * 4 + wave_id()) * EPW + grp; e < N; e += gridDim.x * 4 * EPW) {
    const int key = A.ks[e];
    if (col >= D || key == A.sentinel || (e > 0 && A.ks[e - 1] == key)) continue;
    *reinterpret_cast<float4*>(const_cast<float*>(vbpr_row(A, key)) + col) = ld4(A.slot + (size_t)e * D + col);
  }
}

__global__ __launch_bounds__(256) void vbpr_users_kernel(const float* ux, const float* ue, int n_user, int D, float* out) {
  const size_t tot = (size_t)n_user * 2 * D;
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < tot; e += (size_t)gridDim.x * 256) {
    const size_t r = e / (2 * D);
    const int c = (int)(e - r * 2 * D);
    out[e] = c < D ? ux[r * D + c] : ue[r * D + c - D];
  }
}

// row chunks of the dense gradient: a function of n alone.  64-row leaves; up to VBPR_DENSE_CHUNKS chunks of equally many leaves.
void vbpr_chunking(int n, int* ch_rows, int* n_chunk) {
  const long long leaves = ((long long)n + 63) / 64;
  const long long per = (leaves + VBPR_DENSE_CHUNKS - 1) / VBPR_DENSE_CHUNKS;
  *ch_rows = (int)(64 * (per < 1 ? 1 : per));
  *n_chunk = (int)(leaves < 1 ? 1 : (leaves + per - 1) / (per < 1 ? 1 : per));
}

static int vbpr_grid(const VbprArgs& A, long long items, int num_cu, int per_cu) {
  long long g = items < 1 ? 1 : items;
  if (g > (long long)num_cu * per_cu) g = (long long)num_cu * per_cu;
  if (A.grid_cap > 0 && g > A.grid_cap) g = A.grid_cap;
  return (int)g;
}

template <int NB, int LPR>
static hipError_t launch_vbpr_step_t(VbprArgs& A, int num_cu, hipStream_t st, Timing* tm) {
  const int n = A.n;
  auto grid = [&](long long items, int per) { return dim3((unsigned)vbpr_grid(A, (items + per - 1) / per, num_cu, 16)); };
  tm->begin("vbpr_fwd", st);
  hipLaunchKernelGGL((vbpr_fwd_kernel<NB, 0>), grid(n, 64), dim3(256), 0, st, A);
  hipLaunchKernelGGL(vbpr_ord_kernel, dim3(1), dim3(256), 0, st, A);
  tm->end(st);
  tm->begin("vbpr_wgrad", st);
  hipLaunchKernelGGL(vbpr_wgrad_kernel<NB>, grid((long long)A.n_chunk * ((A.n_img + 63) / 64), 1), dim3(256), 0, st, A);
  tm->end(st);
  tm->begin("vbpr_sort", st);
  int bits = 1;
  while ((1ll << bits) <= (long long)A.sentinel) ++bits;
  const int *ks = nullptr, *vs = nullptr;
  hipError_t e = launch_radix_sort(A.keys0, A.keys1, A.vals0, A.vals1, A.cnt, bits, A.hist, st, &ks, &vs);
  if (e != hipSuccess) return e;
  A.ks = ks; A.vs = vs;
  tm->end(st);
  const long long chunks = (4ll * n + 63) / 64;
  tm->begin("vbpr_rows", st);
  hipLaunchKernelGGL(vbpr_chunk_kernel<LPR>, grid(chunks, 4), dim3(256), 0, st, A);
  hipLaunchKernelGGL(vbpr_span_kernel<LPR>, grid(chunks, 4 * (64 / LPR)), dim3(256), 0, st, A);
  tm->end(st);
  tm->begin("vbpr_commit", st);
  hipLaunchKernelGGL(vbpr_commit_kernel<LPR>, grid(4ll * n, 4 * (64 / LPR)), dim3(256), 0, st, A);
  hipLaunchKernelGGL(vbpr_dense_kernel, grid((long long)A.dim * A.n_img, 256), dim3(256), 0, st, A);
  tm->end(st);
  return hipGetLastError();
}

hipError_t launch_vbpr_step(VbprArgs& A, int num_cu, hipStream_t st, Timing* tm) {
  if (A.dim <= 16) return launch_vbpr_step_t<1, 8>(A, num_cu, st, tm);
  if (A.dim <= 32) return launch_vbpr_step_t<2, 8>(A, num_cu, st, tm);
  if (A.dim <= 64) return launch_vbpr_step_t<4, 16>(A, num_cu, st, tm);
  if (A.dim <= 128) return launch_vbpr_step_t<8, 32>(A, num_cu, st, tm);
  return hipErrorInvalidValue;
}

hipError_t launch_vbpr_items(VbprArgs& A, int num_cu, hipStream_t st, Timing* tm) {
  const dim3 g((unsigned)vbpr_grid(A, (A.n_rows + 63) / 64, num_cu, 16));
  tm->begin("vbpr_items", st);
  if (A.dim <= 16) hipLaunchKernelGGL((vbpr_fwd_kernel<1, 1>), g, dim3(256), 0, st, A);
  else if (A.dim <= 32) hipLaunchKernelGGL((vbpr_fwd_kernel<2, 1>), g, dim3(256), 0, st, A);
  else if (A.dim <= 64) hipLaunchKernelGGL((vbpr_fwd_kernel<4, 1>), g, dim3(256), 0, st, A);
  else if (A.dim <= 128) hipLaunchKernelGGL((vbpr_fwd_kernel<8, 1>), g, dim3(256), 0, st, A);
  else return hipErrorInvalidValue;
  tm->end(st);
  return hipGetLastError();
}

hipError_t launch_vbpr_users(const float* ux, const float* ue, int n_user, int dim, float* out, int num_cu, hipStream_t st, Timing* tm) {
  const long long tot = (long long)n_user * 2 * dim;
  long long g = (tot + 255) / 256;
  if (g > (long long)num_cu * 16) g = (long long)num_cu * 16;
  tm->begin("vbpr_users", st);
  hipLaunchKernelGGL(vbpr_users_kernel, dim3((unsigned)(g < 1 ? 1 : g)), dim3(256), 0, st, ux, ue, n_user, dim, out);
  tm->end(st);
  return hipGetLastError();
}

}  // namespace poi
