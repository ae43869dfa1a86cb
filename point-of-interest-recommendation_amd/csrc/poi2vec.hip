// POI2Vec (prog_poi2vec.py, public/POI2Vec.py, public/Load_Data_Poi2vec.py): the batched full-softmax + hierarchical-softmax step and the
// factorised scoring.
//
// Step (Poi2vec.__theano_train__, POI2Vec.py:127-177), one user u with targets t_0 .. t_{L-1} and contexts C_i:
//   s_j = xu_u . wl_j,  G_j = softmax_j - count_j / L;  c_i = sum_{k in C_i} wl_k,  ind_i = ceil(|mean_d c_i|)
//   z_ird = pb[routes[t_i][r][d]] . c_i,  sg = sigmoid(z lr),  P_ir = prod_d (sg ind_i),  S_i = sum_r probs[t_i][r] P_ir
//   paths_i = floor(1 - S_i) + S_i,  upq = -(1 / L) sum_i (s_{t_i} - lse + log paths_i)
//   d upq / d z_ird = -(1 / (L paths_i)) probs_ir (prod_{d' != d} sg ind) ind sg (1 - sg) lr =: gz_ird
//   d / d wl_j = G_j xu_u + lambda wl_j + sum over (i, k in C_i, k == j) of gc_i,  gc_i = sum_rd gz_ird pb[node_ird]
//   d / d xu_u = sum_j G_j wl_j + lambda xu_u;  pb[node] per occurrence: -alpha gz_ird c_i, last write in (i, r, d) order of the padded
//   bidx wins (a user shorter than len_max: the nodes of routes[0] keep their value).
//
// Kernels: p2v_plan (one block: offsets of the launch users' positions), p2v_lse (item tiles x all users: per-tile max / sum of the
// logits), p2v_pos (a wave per position: everything per position in float64 - the ceil / floor decisions cannot flip on a float32
// rounding), p2v_user (a wave per user: logsumexp from the tile partials in tile order, loss, acceptance, sum of the target rows),
// p2v_count (accepted users), p2v_win (a workgroup per user: which (i, r, d) occurrence is the last write on its node, from the
// left-to-right leaf index of each route: two routes share their ancestor at level l iff their indices agree on the top l bits),
// radix sort of the winning occurrences by node and of the target / context touches by wl row (te_scatter's sort), p2v_dense (item
// stationary: recomputes the logits of its 64-row tile for all users, finishes the softmax term and the decay of those rows, and sums
// its share of dXU into its own slot), p2v_pb / p2v_sparse (ordered run sums, a wave per run), p2v_xu.  No float atomics; every sum
// runs in launch order, and a rejected user contributes exact zeros: identical launches are bitwise identical and removing a rejected
// user leaves every other result bitwise equal.
#include "poi_common.h"
#include "poi_kernels.h"
#include "session_common.h"
#include "topk_list.h"

namespace poi {

#define P2V_TI 64          // items per tile
#define P2V_UC 32          // users per chunk of the dense pass
#define P2V_SLOTS 256      // dXU partial slots (independent of the launch size: the summation order must not depend on it)

__device__ __forceinline__ float wave_all_max_f(float v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ int p2v_find(const int* off, int n, int x) {      // largest k with off[k] <= x
  int lo = 0, hi = n;
  while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (off[mid] <= x) lo = mid; else hi = mid; }
  return lo;
}

// ---- plan: lpos = exclusive scan of the launch users' lengths; ubad[b] = 1 for an id out of range or L == 0 -------------------------
__global__ __launch_bounds__(256) void p2v_plan_kernel(P2vArgs A) {
  __shared__ int s_part[256];
  const int tid = threadIdx.x, per = (A.n + 255) / 256;
  const int b0 = min(A.n, tid * per), b1 = min(A.n, b0 + per);
  int sum = 0;
  for (int b = b0; b < b1; ++b) {
    const int u = A.users[b];
    const bool ok = (unsigned)u < (unsigned)A.n_user;
    const int L = ok ? A.off[u + 1] - A.off[u] : 0;
    A.ubad[b] = (!ok || L <= 0) ? 1 : 0;
    sum += max(L, 0);
  }
  s_part[tid] = sum;
  __syncthreads();
  if (tid == 0) {
    int run = 0;
    for (int t = 0; t < 256; ++t) { const int v = s_part[t]; s_part[t] = run; run += v; }
    A.lpos[A.n] = run;
    A.tot[0] = run == A.n_pos ? 0 : 1;                        // host total mismatch: every user rejected
    A.cnt[0] = run == A.n_pos ? run * 4 * A.depth : 0;        // pb occurrences
    A.cnt[1] = 0;                                             // wl touches: set by p2v_keys
  }
  __syncthreads();
  int run = s_part[tid];
  for (int b = b0; b < b1; ++b) {
    const int u = A.users[b];
    const bool ok = (unsigned)u < (unsigned)A.n_user;
    A.lpos[b] = run;
    run += ok ? max(A.off[u + 1] - A.off[u], 0) : 0;
  }
}

// ---- logits of a 64-item tile for every user: per (user, tile) max and sum of exp ----------------------------------------------------
// block = 64 items x 4 user lanes; the tile is staged transposed (tile[d][item], row stride 65)
__device__ __forceinline__ void p2v_stage_tile(const float* __restrict__ wl, int j0, int n_item, int D, float* tile) {
  for (int x = threadIdx.x; x < P2V_TI * D; x += 256) {
    const int i = x / D, d = x - i * D;
    tile[d * 65 + i] = (j0 + i < n_item) ? wl[(size_t)(j0 + i) * D + d] : 0.f;
  }
}

__global__ __launch_bounds__(256) void p2v_lse_kernel(P2vArgs A) {
  extern __shared__ float smem[];
  float* tile = smem;
  const int D = A.dim, i = threadIdx.x & 63, ul = threadIdx.x >> 6;
  for (int t = blockIdx.x; t < A.n_tile; t += gridDim.x) {
    const int j0 = t * P2V_TI;
    __syncthreads();
    p2v_stage_tile(A.wl, j0, A.n_item, D, tile);
    __syncthreads();
    const bool live = j0 + i < A.n_item;
    for (int b = ul; b < A.n; b += 4) {
      if (A.ubad[b]) continue;                                 // (wave-uniform)
      const float* x = A.xu + (size_t)A.users[b] * D;
      float s = 0.f;
      for (int d = 0; d < D; ++d) s = fmaf(tile[d * 65 + i], x[d], s);
      const float m = wave_all_max_f(live ? s : -INFINITY);
      const double e = wave_sum_d(live ? (double)__expf(s - m) : 0.0);
      if (i == 0) { A.pmax[(size_t)b * A.n_tile + t] = m; A.psum[(size_t)b * A.n_tile + t] = e; }
    }
  }
}

// ---- per position ------------------------------------------------------------------------------------------------------------------
// a wave per position; lane l owns the dimensions l and l + 64.  posval = s_t + log paths (float64); gz (4 depth) float64; c and gc (D)
__global__ __launch_bounds__(256) void p2v_pos_kernel(P2vArgs A) {
  __shared__ double s_sg[4][128];
  __shared__ double s_gz[4][128];
  const int D = A.dim, lane = threadIdx.x & 63, w = threadIdx.x >> 6, dep = A.depth, R = 4 * dep;
  if (A.tot[0]) return;
  for (int x = blockIdx.x * 4 + w; x < A.n_pos; x += gridDim.x * 4) {
    const int b = p2v_find(A.lpos, A.n, x);
    if (A.ubad[b]) continue;
    const int u = A.users[b], L = A.off[u + 1] - A.off[u], gp = A.off[u] + (x - A.lpos[b]);
    const int t = A.tgt[gp];
    if ((unsigned)t >= (unsigned)A.n_item) { if (lane == 0) atomicOr(&A.ubad[b], 2); continue; }
    const int d0 = lane, d1 = lane + 64;
    double c0 = 0.0, c1 = 0.0;
    for (int e = A.coff[gp]; e < A.coff[gp + 1]; ++e) {
      const int k = A.cidx[e];
      if ((unsigned)k >= (unsigned)A.n_item) continue;         // the reference's padding id adds the zero row
      if (d0 < D) c0 += (double)A.wl[(size_t)k * D + d0];
      if (d1 < D) c1 += (double)A.wl[(size_t)k * D + d1];
    }
    const double mean = wave_sum_d(c0 + c1) / (double)D;
    const double ind = ceil(fabs(mean));
    const float* xr = A.xu + (size_t)u * D;
    const float* wt = A.wl + (size_t)t * D;
    const double st = wave_sum_d((d0 < D ? (double)xr[d0] * (double)wt[d0] : 0.0) + (d1 < D ? (double)xr[d1] * (double)wt[d1] : 0.0));
    const int* rt = A.routes + (size_t)t * R;
    const signed char* lr = A.lrs + (size_t)t * R;
    for (int q = 0; q < R; ++q) {
      const float* pr = A.pb + (size_t)rt[q] * D;
      const double z = wave_sum_d((d0 < D ? (double)pr[d0] * c0 : 0.0) + (d1 < D ? (double)pr[d1] * c1 : 0.0));
      if (lane == 0) s_sg[w][q] = 1.0 / (1.0 + exp(-z * (double)lr[q]));
    }
    __builtin_amdgcn_wave_barrier();
    __threadfence_block();
    double S = 0.0;
    for (int r = 0; r < 4; ++r) {
      double pr = 1.0;
      for (int d = 0; d < dep; ++d) pr *= s_sg[w][r * dep + d] * ind;
      S += (double)A.probs[(size_t)t * 4 + r] * pr;
    }
    const double paths = floor(1.0 - S) + S;
    if (lane == 0) A.posval[x] = st + log(paths);
    const double dS = -1.0 / ((double)L * paths);
    for (int q = lane; q < R; q += 64) {
      const int r = q / dep, d = q - r * dep;
      double oth = 1.0;
      for (int d2 = 0; d2 < dep; ++d2) if (d2 != d) oth *= s_sg[w][r * dep + d2] * ind;
      const double sg = s_sg[w][q];
      const double g = dS * (double)A.probs[(size_t)t * 4 + r] * oth * (sg * (1.0 - sg) * ind) * (double)lr[q];
      s_gz[w][q] = g;
      A.gz[(size_t)x * R + q] = g;
    }
    __builtin_amdgcn_wave_barrier();
    __threadfence_block();
    double g0 = 0.0, g1 = 0.0;
    for (int q = 0; q < R; ++q) {
      const float* pr = A.pb + (size_t)rt[q] * D;
      const double g = s_gz[w][q];
      if (d0 < D) g0 += g * (double)pr[d0];
      if (d1 < D) g1 += g * (double)pr[d1];
    }
    if (d0 < D) { A.cbuf[(size_t)x * D + d0] = c0; A.gcbuf[(size_t)x * D + d0] = g0; }
    if (d1 < D) { A.cbuf[(size_t)x * D + d1] = c1; A.gcbuf[(size_t)x * D + d1] = g1; }
    __builtin_amdgcn_wave_barrier();
  }
}

// ---- per user: logsumexp, loss, acceptance, sum of the target rows ----------------------------------------------------------------------
__global__ __launch_bounds__(256) void p2v_user_kernel(P2vArgs A) {
  const int D = A.dim, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const float nanf_ = __int_as_float(0x7fc00000);
  for (int b = blockIdx.x * 4 + w; b < A.n; b += gridDim.x * 4) {
    if (A.ubad[b] || A.tot[0]) {
      if (lane == 0) { A.loss[b] = nanf_; A.acc[b] = 0; }
      continue;
    }
    const int u = A.users[b], L = A.off[u + 1] - A.off[u], x0 = A.lpos[b];
    float m = -INFINITY;
    for (int t = lane; t < A.n_tile; t += 64) m = fmaxf(m, A.pmax[(size_t)b * A.n_tile + t]);
    m = wave_all_max_f(m);
    double sum = 0.0;                                          // tile order
    for (int t = 0; t < A.n_tile; ++t) sum += A.psum[(size_t)b * A.n_tile + t] * exp((double)A.pmax[(size_t)b * A.n_tile + t] - (double)m);
    const double lse = (double)m + log(sum);
    double pv = 0.0;
    for (int i = 0; i < L; ++i) pv += A.posval[x0 + i] - lse;
    const double loss = -pv / (double)L;
    const bool ok = isfinite(loss) && isfinite((float)loss);
    double t0 = 0.0, t1 = 0.0;
    if (ok) {
      const int* tg = A.tgt + A.off[u];
      for (int i = 0; i < L; ++i) {
        const float* wt = A.wl + (size_t)tg[i] * D;
        if (lane < D) t0 += (double)wt[lane];
        if (lane + 64 < D) t1 += (double)wt[lane + 64];
      }
    }
    if (lane < D) A.tsum[(size_t)b * D + lane] = t0;
    if (lane + 64 < D) A.tsum[(size_t)b * D + lane + 64] = t1;
    if (lane == 0) { A.loss[b] = ok ? (float)loss : nanf_; A.acc[b] = ok ? 1 : 0; A.lse[b] = lse; }
  }
}

// accepted users k -> tot[1], the wl scale alpha min(k, cap) / k -> scale[0], rejected users counted once
__global__ __launch_bounds__(256) void p2v_count_kernel(P2vArgs A) {
  __shared__ int s_k[256];
  int k = 0;
  for (int b = threadIdx.x; b < A.n; b += 256) k += A.acc[b];
  s_k[threadIdx.x] = k;
  __syncthreads();
  if (threadIdx.x == 0) {
    int tk = 0;
    for (int t = 0; t < 256; ++t) tk += s_k[t];
    A.tot[1] = tk;
    A.scale[0] = tk > 0 ? A.alpha * fminf((float)tk, A.bcap) / (float)tk : 0.f;
    if (A.n - tk > 0) atomicAdd(A.bad, A.n - tk);
  }
}

// ---- winners of the last-wins collapse + sort keys ------------------------------------------------------------------------------------
// a workgroup per launch user.  Entry e = (i, r) (flattened 4 i + r, then the 4 padding routes of routes[0] when L < len_max) with leaf
// index rid; m_e = the longest common prefix (in levels) with any later entry, -1 when there is none.  The occurrence (i, r, d) is the
// last write on its node (level depth - 1 - d) iff that level > m_e.
__global__ __launch_bounds__(256) void p2v_win_kernel(P2vArgs A) {
  __shared__ int s_rid[1024];
  const int dep = A.depth, R = 4 * dep;
  for (int b = blockIdx.x; b < A.n; b += gridDim.x) {
    if (A.ubad[b] || A.tot[0]) continue;                       // (lengths of bad users are 0 in lpos or their keys are never read)
    const int u = A.users[b], L = A.off[u + 1] - A.off[u], x0 = A.lpos[b];
    const int* tg = A.tgt + A.off[u];
    const int ne = 4 * L, nt = ne + (L < A.len_max ? 4 : 0);
    const bool accepted = A.acc[b] != 0;
    for (int e0 = 0; e0 < ne; e0 += 256) {
      const int e = e0 + threadIdx.x;
      const int my = e < ne ? A.rid[(size_t)tg[e >> 2] * 4 + (e & 3)] : 0;
      int m = -1;
      for (int c0 = (e0 / 1024) * 1024; c0 < nt; c0 += 1024) {
        __syncthreads();
        for (int y = threadIdx.x; y < 1024 && c0 + y < nt; y += 256) {
          const int e2 = c0 + y;
          s_rid[y] = e2 < ne ? A.rid[(size_t)tg[e2 >> 2] * 4 + (e2 & 3)] : A.rid[e2 - ne];      // padding: routes[0]
        }
        __syncthreads();
        if (e < ne) {
          const int hi = min(1024, nt - c0);
          for (int y = max(0, e + 1 - c0); y < hi; ++y) {
            const unsigned xo = (unsigned)(my ^ s_rid[y]);
            const int cpl = xo == 0 ? dep - 1 : dep - 1 - (32 - __clz(xo));
            m = max(m, cpl);
          }
        }
      }
      if (e < ne) {
        const int t = tg[e >> 2];
        const int* rt = A.routes + ((size_t)t * 4 + (e & 3)) * dep;
        const size_t o = (size_t)x0 * R + (size_t)e * dep;
        for (int d = 0; d < dep; ++d) {
          const bool win = accepted && (dep - 1 - d) > m;
          A.keys0[o + d] = win ? rt[d] : A.n_node;
          A.vals0[o + d] = (int)(o + d);
        }
      }
    }
  }
}

// keys of rejected / bad users' occurrences (p2v_win skips them), and the wl touches: entry x < n_pos = target of position x (value
// -xu_u / L), entry n_pos + y = y-th context id of the launch (value gc of its position); key n_item = none
__global__ __launch_bounds__(256) void p2v_keys_kernel(P2vArgs A) {
  const int R = 4 * A.depth;
  if (A.tot[0]) { if (blockIdx.x == 0 && threadIdx.x == 0) A.cnt[1] = 0; return; }
  if (blockIdx.x == 0 && threadIdx.x == 0) A.cnt[1] = A.n_pos + A.n_ctx;
  for (int x = blockIdx.x * 256 + threadIdx.x; x < A.n_pos; x += gridDim.x * 256) {
    const int b = p2v_find(A.lpos, A.n, x);
    const int u = A.users[b], gp = A.off[u] + (x - A.lpos[b]);
    const bool ok = A.acc[b] != 0;
    if (A.ubad[b]) for (int q = 0; q < R; ++q) { A.keys0[(size_t)x * R + q] = A.n_node; A.vals0[(size_t)x * R + q] = (int)((size_t)x * R + q); }
    A.k2a[x] = ok ? A.tgt[gp] : A.n_item;
    A.v2a[x] = x;
  }
}
// context touches: a thread per launch position writes its contexts at lctx[x] ..; lctx = exclusive scan (p2v_ctxscan)
__global__ __launch_bounds__(256) void p2v_ctxscan_kernel(P2vArgs A) {
  // one block: per-user context totals are contiguous in the CSR (coff[off[u]] .. coff[off[u+1]]), so the scan runs over users
  __shared__ int s_part[256];
  const int tid = threadIdx.x, per = (A.n + 255) / 256;
  const int b0 = min(A.n, tid * per), b1 = min(A.n, b0 + per);
  int sum = 0;
  for (int b = b0; b < b1; ++b) {
    const int u = A.users[b];
    if ((unsigned)u < (unsigned)A.n_user) sum += A.coff[A.off[u + 1]] - A.coff[A.off[u]];
  }
  s_part[tid] = sum;
  __syncthreads();
  if (tid == 0) {
    int run = 0;
    for (int t = 0; t < 256; ++t) { const int v = s_part[t]; s_part[t] = run; run += v; }
    A.lctx[A.n] = run;
    if (run != A.n_ctx) { A.tot[0] = 1; A.cnt[0] = 0; }
  }
  __syncthreads();
  int run = s_part[tid];
  for (int b = b0; b < b1; ++b) {
    const int u = A.users[b];
    A.lctx[b] = run;
    if ((unsigned)u < (unsigned)A.n_user) run += A.coff[A.off[u + 1]] - A.coff[A.off[u]];
  }
}
__global__ __launch_bounds__(256) void p2v_ckeys_kernel(P2vArgs A) {
  if (A.tot[0]) return;
  for (int x = blockIdx.x * 256 + threadIdx.x; x < A.n_pos; x += gridDim.x * 256) {
    const int b = p2v_find(A.lpos, A.n, x);
    const int u = A.users[b], gp = A.off[u] + (x - A.lpos[b]);
    const bool ok = A.acc[b] != 0;
    const int base = A.n_pos + A.lctx[b] + (A.coff[gp] - A.coff[A.off[u]]);
    for (int e = A.coff[gp]; e < A.coff[gp + 1]; ++e) {
      const int k = A.cidx[e], y = base + (e - A.coff[gp]);
      A.k2a[y] = (ok && (unsigned)k < (unsigned)A.n_item) ? k : A.n_item;
      A.v2a[y] = y;
      A.epos[y - A.n_pos] = x;
    }
  }
}

// ---- item-stationary dense pass ----------------------------------------------------------------------------------------------------------
// workgroup g owns the tiles g, g + P2V_SLOTS, ..; per tile and chunk of 32 users: G = exp(s - lse) (0 for a rejected user), then
// dWL[i][:] += G[b][i] xu_b in launch order (thread = item x quarter of the dimensions) and dXU[b][:] += sum_i G[b][i] wl_i into the
// workgroup's slot.  The rows are finished here: wl += -scale (dWL + k lambda wl).
template <int DQ>      // dimensions per thread in the dWL phase: ceil(D / 4)
__global__ __launch_bounds__(256) void p2v_dense_kernel(P2vArgs A) {
  extern __shared__ float smem[];
  const int D = A.dim;
  float* tile = smem;                        // D x 65
  float* xs = tile + D * 65;                 // 32 x D
  float* gs = xs + P2V_UC * D;               // 32 x 64
  const int i = threadIdx.x & 63, q = threadIdx.x >> 6;
  const int k = A.tot[1];
  const float sc = A.scale[0];
  float* slot = A.dxu + (size_t)blockIdx.x * A.n * D;
  bool first = true;
  for (int t = blockIdx.x; t < A.n_tile; t += gridDim.x) {
    const int j0 = t * P2V_TI;
    __syncthreads();
    p2v_stage_tile(A.wl, j0, A.n_item, D, tile);
    float acc[DQ];
#pragma unroll
    for (int a = 0; a < DQ; ++a) acc[a] = 0.f;
    for (int c0 = 0; c0 < A.n; c0 += P2V_UC) {
      const int nc = min(P2V_UC, A.n - c0);
      __syncthreads();
      for (int x = threadIdx.x; x < nc * D; x += 256) {
        const int bl = x / D, d = x - bl * D, b = c0 + bl;
        xs[x] = A.acc[b] ? A.xu[(size_t)A.users[b] * D + d] : 0.f;
      }
      __syncthreads();
      for (int bl = q; bl < nc; bl += 4) {
        float g = 0.f;
        if (A.acc[c0 + bl] && j0 + i < A.n_item) {
          float s = 0.f;
          for (int d = 0; d < D; ++d) s = fmaf(tile[d * 65 + i], xs[bl * D + d], s);
          g = (float)exp((double)s - A.lse[c0 + bl]);
        }
        gs[bl * 64 + i] = g;
      }
      __syncthreads();
      for (int bl = 0; bl < nc; ++bl) {
        const float g = gs[bl * 64 + i];
#pragma unroll
        for (int a = 0; a < DQ; ++a) {
          const int d = q + 4 * a;
          if (d < D) acc[a] = fmaf(g, xs[bl * D + d], acc[a]);
        }
      }
      for (int x = threadIdx.x; x < nc * D; x += 256) {
        const int bl = x / D, d = x - bl * D;
        float s = 0.f;
        for (int ii = 0; ii < 64; ++ii) s = fmaf(gs[bl * 64 + ii], tile[d * 65 + ii], s);
        float* o = slot + (size_t)(c0 + bl) * D + d;
        *o = first ? s : *o + s;
      }
    }
    first = false;
    if (k > 0 && j0 + i < A.n_item) {
#pragma unroll
      for (int a = 0; a < DQ; ++a) {
        const int d = q + 4 * a;
        if (d < D) {
          const float w0 = tile[d * 65 + i];
          A.wl[(size_t)(j0 + i) * D + d] = w0 - sc * (acc[a] + (float)k * A.lambda * w0);
        }
      }
    }
  }
}

// ---- ordered run sums ---------------------------------------------------------------------------------------------------------------------
// a wave per 64 sorted entries: the lanes find the run heads of their window, then the wave walks each run (it may leave the window)
// with the lanes over the dimensions
__global__ __launch_bounds__(256) void p2v_pb_kernel(P2vArgs A) {
  const int D = A.dim, lane = threadIdx.x & 63, w = threadIdx.x >> 6, R = 4 * A.depth;
  const int E = A.cnt[0];
  for (int s0 = (blockIdx.x * 4 + w) * 64; s0 < E; s0 += gridDim.x * 256) {
    const int s = s0 + lane;
    const int key = s < E ? A.ks[s] : A.n_node;
    const bool head = s < E && key < A.n_node && (s == 0 || A.ks[s - 1] != key);
    unsigned long long hm = __ballot(head);
    while (hm) {
      const int hl = __ffsll((long long)hm) - 1;
      hm &= hm - 1;
      const int hs = s0 + hl, node = A.ks[hs];
      float a0 = 0.f, a1 = 0.f;
      int kk = 0;
      for (int y = hs; y < E && A.ks[y] == node; ++y) {      // one winning occurrence per accepted user, in launch order
        const int e = A.vs[y], x = e / R;
        const float g = (float)A.gz[e];
        if (lane < D) a0 += g * (float)A.cbuf[(size_t)x * D + lane];
        if (lane + 64 < D) a1 += g * (float)A.cbuf[(size_t)x * D + lane + 64];
        ++kk;
      }
      const float sc = A.alpha * fminf((float)kk, A.bcap) / (float)kk;
      float* pr = A.pb + (size_t)node * D;
      if (lane < D) pr[lane] = pr[lane] - sc * a0;
      if (lane + 64 < D) pr[lane + 64] = pr[lane + 64] - sc * a1;
    }
  }
}

__global__ __launch_bounds__(256) void p2v_sparse_kernel(P2vArgs A) {
  const int D = A.dim, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int E = A.cnt[1];
  const float sc = A.scale[0];
  for (int s0 = (blockIdx.x * 4 + w) * 64; s0 < E; s0 += gridDim.x * 256) {
    const int s = s0 + lane;
    const int key = s < E ? A.k2s[s] : A.n_item;
    const bool head = s < E && key < A.n_item && (s == 0 || A.k2s[s - 1] != key);
    unsigned long long hm = __ballot(head);
    while (hm) {
      const int hl = __ffsll((long long)hm) - 1;
      hm &= hm - 1;
      const int hs = s0 + hl, row = A.k2s[hs];
      float a0 = 0.f, a1 = 0.f;
      for (int y = hs; y < E && A.k2s[y] == row; ++y) {
        const int e = A.v2s[y];
        if (e < A.n_pos) {                                     // a target: -xu_u / L
          const int b = p2v_find(A.lpos, A.n, e);
          const int u = A.users[b];
          const float il = -1.0f / (float)(A.off[u + 1] - A.off[u]);
          if (lane < D) a0 += il * A.xu[(size_t)u * D + lane];
          if (lane + 64 < D) a1 += il * A.xu[(size_t)u * D + lane + 64];
        } else {                                               // a context occurrence: gc of its position
          const int x = A.epos[e - A.n_pos];
          if (lane < D) a0 += (float)A.gcbuf[(size_t)x * D + lane];
          if (lane + 64 < D) a1 += (float)A.gcbuf[(size_t)x * D + lane + 64];
        }
      }
      float* wr = A.wl + (size_t)row * D;
      if (lane < D) wr[lane] = wr[lane] - sc * a0;
      if (lane + 64 < D) wr[lane + 64] = wr[lane + 64] - sc * a1;
    }
  }
}

// xu rows: the first accepted occurrence of a user id sums every accepted occurrence of it (launch order); xu is read by p2v_sparse, which
// runs before
__global__ __launch_bounds__(128) void p2v_xu_kernel(P2vArgs A, int n_slot) {
  const int D = A.dim, d = threadIdx.x;
  for (int b = blockIdx.x; b < A.n; b += gridDim.x) {
    if (!A.acc[b]) continue;
    const int u = A.users[b];
    bool dup = false;
    for (int b2 = 0; b2 < b && !dup; ++b2) dup = A.acc[b2] && A.users[b2] == u;
    if (dup || d >= D) continue;
    const int L = A.off[u + 1] - A.off[u];
    const float x0 = A.xu[(size_t)u * D + d];
    float sum = 0.f;
    int kk = 0;
    for (int b2 = b; b2 < A.n; ++b2) {
      if (!A.acc[b2] || A.users[b2] != u) continue;
      float g = 0.f;
      for (int sl = 0; sl < n_slot; ++sl) g += A.dxu[((size_t)sl * A.n + b2) * D + d];
      sum += (float)((double)g - A.tsum[(size_t)b2 * D + d] / (double)L) + A.lambda * x0;
      ++kk;
    }
    A.xu[(size_t)u * D + d] = x0 - A.alpha * fminf((float)kk, A.bcap) / (float)kk * sum;
  }
}

size_t p2v_dense_lds(int D) { return sizeof(float) * ((size_t)D * 65 + (size_t)P2V_UC * D + (size_t)P2V_UC * 64); }

hipError_t launch_poi2vec_step(P2vArgs& A, int num_cu, hipStream_t st, Timing* tm) {
  auto grid = [&](long long items, int per) { return dim3((unsigned)max(1ll, min((long long)num_cu * 16, (items + per - 1) / per))); };
  const int D = A.dim, n_slot = min(A.n_tile, P2V_SLOTS);
  tm->begin("p2v_plan", st);
  hipLaunchKernelGGL(p2v_plan_kernel, dim3(1), dim3(256), 0, st, A);
  hipLaunchKernelGGL(p2v_ctxscan_kernel, dim3(1), dim3(256), 0, st, A);
  tm->end(st);
  tm->begin("p2v_lse", st);
  hipLaunchKernelGGL(p2v_lse_kernel, grid(A.n_tile, 1), dim3(256), sizeof(float) * D * 65, st, A);
  tm->end(st);
  tm->begin("p2v_pos", st);
  hipLaunchKernelGGL(p2v_pos_kernel, grid(A.n_pos, 4), dim3(256), 0, st, A);
  tm->end(st);
  tm->begin("p2v_user", st);
  hipLaunchKernelGGL(p2v_user_kernel, grid(A.n, 4), dim3(256), 0, st, A);
  hipLaunchKernelGGL(p2v_count_kernel, dim3(1), dim3(256), 0, st, A);
  tm->end(st);
  tm->begin("p2v_sort", st);
  hipLaunchKernelGGL(p2v_win_kernel, grid(A.n, 1), dim3(256), 0, st, A);
  hipLaunchKernelGGL(p2v_keys_kernel, grid(A.n_pos, 256), dim3(256), 0, st, A);
  hipLaunchKernelGGL(p2v_ckeys_kernel, grid(A.n_pos, 256), dim3(256), 0, st, A);
  {
    int bits = 1;
    while ((1ll << bits) <= (long long)A.n_node) ++bits;
    const int *ks = nullptr, *vs = nullptr;
    hipError_t e = launch_radix_sort(A.keys0, A.keys1, A.vals0, A.vals1, A.cnt, bits, A.hist, st, &ks, &vs);
    if (e != hipSuccess) return e;
    A.ks = ks; A.vs = vs;
    bits = 1;
    while ((1ll << bits) <= (long long)A.n_item) ++bits;
    e = launch_radix_sort(A.k2a, A.k2b, A.v2a, A.v2b, A.cnt + 1, bits, A.hist, st, &ks, &vs);
    if (e != hipSuccess) return e;
    A.k2s = ks; A.v2s = vs;
  }
  tm->end(st);
  tm->begin("p2v_pb", st);
  hipLaunchKernelGGL(p2v_pb_kernel, grid((long long)A.n_pos * 4 * A.depth, 256), dim3(256), 0, st, A);
  tm->end(st);
  tm->begin("p2v_dense", st);
  const size_t lds = p2v_dense_lds(D);
  if (D <= 32) hipLaunchKernelGGL(p2v_dense_kernel<8>, dim3(n_slot), dim3(256), lds, st, A);
  else if (D <= 64) hipLaunchKernelGGL(p2v_dense_kernel<16>, dim3(n_slot), dim3(256), lds, st, A);
  else hipLaunchKernelGGL(p2v_dense_kernel<32>, dim3(n_slot), dim3(256), lds, st, A);
  tm->end(st);
  tm->begin("p2v_sparse", st);
  hipLaunchKernelGGL(p2v_sparse_kernel, grid((long long)A.n_pos + A.n_ctx, 256), dim3(256), 0, st, A);
  tm->end(st);
  tm->begin("p2v_xu", st);
  hipLaunchKernelGGL(p2v_xu_kernel, grid(A.n, 1), dim3(128), 0, st, A, n_slot);
  tm->end(st);
  return hipGetLastError();
}

// ---- scoring (Poi2vecBasic.compute_sub_all_scores, POI2Vec.py:91-109) --------------------------------------------------------------------
// rows (user b, position t); cl = context sum (float64); zf (rows, n_node): the node products in float64 (ceil(|z|) is decided on
// them); rp (rows, n_leaf) float64 product along each distinct route; then 4 gathers per POI.
__global__ __launch_bounds__(256) void p2v_sc_ctx_kernel(P2vScoreArgs A) {
  const long long N = (long long)A.n_rows * A.dim;
  for (long long x = blockIdx.x * 256ll + threadIdx.x; x < N; x += gridDim.x * 256ll) {
    const int r = (int)(x / A.dim), d = (int)(x - (long long)r * A.dim);
    double c = 0.0;
    for (int e = A.coff[r]; e < A.coff[r + 1]; ++e) {
      const int k = A.cidx[e];
      if ((unsigned)k < (unsigned)A.n_item) c += (double)A.wl[(size_t)k * A.dim + d];
    }
    A.cl[x] = c;
  }
}
__global__ __launch_bounds__(256) void p2v_sc_node_kernel(P2vScoreArgs A) {
  const long long N = (long long)A.n_rows * A.n_node;
  for (long long x = blockIdx.x * 256ll + threadIdx.x; x < N; x += gridDim.x * 256ll) {
    const int r = (int)(x / A.n_node), n = (int)(x - (long long)r * A.n_node);
    const float* pr = A.pb + (size_t)n * A.dim;
    const double* c = A.cl + (size_t)r * A.dim;
    double z = 0.0;
    for (int d = 0; d < A.dim; ++d) z += (double)pr[d] * c[d];
    A.zf[x] = z;
  }
}
__global__ __launch_bounds__(256) void p2v_sc_route_kernel(P2vScoreArgs A) {
  const int dep = A.depth, NL = 1 << (dep - 1);
  const long long N = (long long)A.n_rows * NL;
  for (long long x = blockIdx.x * 256ll + threadIdx.x; x < N; x += gridDim.x * 256ll) {
    const int r = (int)(x / NL), lf = (int)(x - (long long)r * NL);
    const double* z = A.zf + (size_t)r * A.n_node;
    double p = 1.0;
    for (int d = 0; d < dep; ++d) {
      const double zz = z[A.leaf_nodes[(size_t)lf * dep + d]];
      const double lr = d == 0 ? 1.0 : (double)(1 - 2 * ((lf >> (d - 1)) & 1));
      p *= ceil(fabs(zz)) / (1.0 + exp(-zz * lr));
    }
    A.rp[x] = p;
  }
}
// logits and their softmax statistics: axis 0 (over the users of the batch; per POI) or axis 1 (over the POIs; per user)
__global__ __launch_bounds__(256) void p2v_sc_logit_kernel(P2vScoreArgs A) {
  const long long N = (long long)A.n_batch * A.n_item;
  for (long long x = blockIdx.x * 256ll + threadIdx.x; x < N; x += gridDim.x * 256ll) {
    const int b = (int)(x / A.n_item), j = (int)(x - (long long)b * A.n_item);
    const int u = A.users[b];
    float s = __int_as_float(0x7fc00000);
    if ((unsigned)u < (unsigned)A.n_user) {
      const float* xr = A.xu + (size_t)u * A.dim;
      const float* wr = A.wl + (size_t)j * A.dim;
      double a = 0.0;
      for (int d = 0; d < A.dim; ++d) a += (double)xr[d] * (double)wr[d];
      s = (float)a;
    }
    A.logit[x] = s;
  }
}
__global__ __launch_bounds__(256) void p2v_sc_stat_kernel(P2vScoreArgs A) {
  __shared__ double s_red[256];
  if (A.axis == 0) {
    for (int j = blockIdx.x * 256 + threadIdx.x; j < A.n_item; j += gridDim.x * 256) {
      float m = -INFINITY;
      for (int b = 0; b < A.n_batch; ++b) m = fmaxf(m, A.logit[(size_t)b * A.n_item + j]);      // (fmaxf skips a NaN logit)
      double s = 0.0;
      for (int b = 0; b < A.n_batch; ++b) {                    // a user id out of range has NaN logits: left out, only its own rows are NaN
        const float v = A.logit[(size_t)b * A.n_item + j];
        if (v == v) s += exp((double)v - (double)m);
      }
      A.smax[j] = m; A.ssum[j] = s;
    }
  } else {
    for (int b = blockIdx.x; b < A.n_batch; b += gridDim.x) {
      float m = -INFINITY;
      for (int j = threadIdx.x; j < A.n_item; j += 256) m = fmaxf(m, A.logit[(size_t)b * A.n_item + j]);
      s_red[threadIdx.x] = m;
      __syncthreads();
      for (int o = 128; o >= 1; o >>= 1) { if (threadIdx.x < o) s_red[threadIdx.x] = fmax(s_red[threadIdx.x], s_red[threadIdx.x + o]); __syncthreads(); }
      const float mm = (float)s_red[0];
      __syncthreads();
      double s = 0.0;
      for (int j = threadIdx.x; j < A.n_item; j += 256) s += exp((double)A.logit[(size_t)b * A.n_item + j] - (double)mm);
      s_red[threadIdx.x] = s;
      __syncthreads();
      for (int o = 128; o >= 1; o >>= 1) { if (threadIdx.x < o) s_red[threadIdx.x] += s_red[threadIdx.x + o]; __syncthreads(); }
      if (threadIdx.x == 0) { A.smax[b] = mm; A.ssum[b] = s_red[0]; }
      __syncthreads();
    }
  }
}
// the score of (row r, POI j): 4 gathers of the route products, floor on the float64 sum, times plu
__device__ __forceinline__ float p2v_score(const P2vScoreArgs& A, int r, int j) {
  const int NL = 1 << (A.depth - 1), b = r / A.length;
  const double* rp = A.rp + (size_t)r * NL;
  double S = 0.0;
  for (int q = 0; q < 4; ++q) S += (double)A.probs[(size_t)j * 4 + q] * rp[A.rid[(size_t)j * 4 + q]];
  const double paths = floor(1.0 - S) + S;
  const int si = A.axis == 0 ? j : b;
  const double plu = exp((double)A.logit[(size_t)b * A.n_item + j] - (double)A.smax[si]) / A.ssum[si];
  return (float)(paths * plu);
}
__global__ __launch_bounds__(256) void p2v_sc_out_kernel(P2vScoreArgs A) {
  const long long N = (long long)A.n_rows * A.n_item;
  for (long long x = blockIdx.x * 256ll + threadIdx.x; x < N; x += gridDim.x * 256ll) {
    const int r = (int)(x / A.n_item), j = (int)(x - (long long)r * A.n_item);
    A.out[x] = p2v_score(A, r, j);
  }
}

// fused top-K (K <= 64): a workgroup per row computes the scores of its POIs on the fly - the row of scores is never stored - and each
// wave keeps a sorted 64-entry list in LDS; the 4 lists are merged at the end.  Order: higher score, then lower id; a NaN score ranks
// as -inf (last) and is reported as NaN.
__global__ __launch_bounds__(256) void p2v_sc_topk_kernel(P2vScoreArgs A) {
  __shared__ float s_ls[4][64];
  __shared__ int s_li[4][64];
  __shared__ int s_nex;                                       // POIs of the row its exclusion list removed
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (int r = blockIdx.x; r < A.n_rows; r += gridDim.x) {
    if (threadIdx.x == 0) s_nex = 0;                          // (wave 0 has read the previous row's count)
    __syncthreads();
    s_ls[w][lane] = -INFINITY; s_li[w][lane] = PAD_ID;
    __builtin_amdgcn_wave_barrier();
    // exclusion list of the row (poi_poi2vec_topk_ex; ascending unique ids): an excluded POI enters the lists as an empty entry.  A
    // malformed list (descending offsets) is taken as empty
    const int e0 = A.ex ? A.ex_off[r] : 0, e1 = A.ex ? max(A.ex_off[r + 1], e0) : 0;
    int n_ex = 0;
    for (int j0 = 0; j0 < A.n_item; j0 += 256) {              // (wave-uniform trip count)
      const int j = j0 + threadIdx.x;
      bool on = j < A.n_item;
      if (on && e1 > e0) {                                    // first entry >= j
        int a = e0, b = e1;
        while (a < b) { const int md = (a + b) >> 1; if (A.ex[md] < j) a = md + 1; else b = md; }
        if (a < e1 && A.ex[a] == j) { on = false; ++n_ex; }
      }
      float s = -INFINITY;
      if (on) { s = p2v_score(A, r, j); if (!(s == s)) s = -INFINITY; }
      lds_list_merge(s_ls[w], s_li[w], s, on ? j : PAD_ID, A.k);
    }
    if (n_ex) atomicAdd(&s_nex, n_ex);                        // (an integer count in LDS: order-free)
    __syncthreads();
    if (w == 0) {
      float s = s_ls[0][lane];
      int i = s_li[0][lane];
      for (int v = 1; v < 4; ++v) {
        float rs = s_ls[v][63 - lane];
        int ri = s_li[v][63 - lane];
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
        const size_t o = (size_t)r * A.k + lane;
        const bool ok = i != PAD_ID;
        A.idx_out[o] = ok ? i : -1;
        if (A.score_out) A.score_out[o] = ok ? p2v_score(A, r, i) : __int_as_float(0x7fc00000);
      }
      if (lane == 0 && A.count_out) A.count_out[r] = A.n_item - s_nex;
    }
  }
}

hipError_t launch_poi2vec_scores(P2vScoreArgs& A, int num_cu, hipStream_t st, Timing* tm) {
  auto grid = [&](long long items) { return dim3((unsigned)max(1ll, min((long long)num_cu * 16, (items + 255) / 256))); };
  const long long NL = 1ll << (A.depth - 1);
  tm->begin("p2v_sc_node", st);
  hipLaunchKernelGGL(p2v_sc_ctx_kernel, grid((long long)A.n_rows * A.dim), dim3(256), 0, st, A);
  hipLaunchKernelGGL(p2v_sc_node_kernel, grid((long long)A.n_rows * A.n_node), dim3(256), 0, st, A);
  tm->end(st);
  tm->begin("p2v_sc_route", st);
  hipLaunchKernelGGL(p2v_sc_route_kernel, grid((long long)A.n_rows * NL), dim3(256), 0, st, A);
  tm->end(st);
  tm->begin("p2v_sc_plu", st);
  hipLaunchKernelGGL(p2v_sc_logit_kernel, grid((long long)A.n_batch * A.n_item), dim3(256), 0, st, A);
  hipLaunchKernelGGL(p2v_sc_stat_kernel, A.axis == 0 ? grid(A.n_item) : dim3((unsigned)min(A.n_batch, num_cu * 8)), dim3(256), 0, st, A);
  tm->end(st);
  if (A.k > 0) {
    tm->begin("p2v_sc_topk", st);
    hipLaunchKernelGGL(p2v_sc_topk_kernel, dim3((unsigned)min(A.n_rows, num_cu * 8)), dim3(256), 0, st, A);
    tm->end(st);
  } else {
    tm->begin("p2v_sc_out", st);
    hipLaunchKernelGGL(p2v_sc_out_kernel, grid((long long)A.n_rows * A.n_item), dim3(256), 0, st, A);
    tm->end(st);
  }
  return hipGetLastError();
}

}  // namespace poi
