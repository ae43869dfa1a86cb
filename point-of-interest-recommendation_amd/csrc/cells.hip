// Mini-batch Lstm / Rnn baselines (public/GRU.py:502-657 `Lstm`, :661-809 `Rnn`): one kernel family templated on the number of gate
// blocks G (1 = Rnn: h = sigmoid(a); 4 = Lstm: i, f, g, o and the cell state c).
//
// A launch is ONE mini-batch of n users.  Tables are float32 in HBM; gate sums, states, the BPTT chain and every
// gradient sum are float64 and round once at the write-back.  No float atomics: dense gradients are per-row-chunk partial sums added in
// chunk order (the chunking is a function of n and max_len alone), POI rows are (row, entry) pairs sorted with launch_radix_sort and
// summed in sorted order - identical launches give bitwise identical tables, whatever grid the recurrent kernel ran on.
//
// Layout: sequence k of the launch owns the L_k "position rows" poff[k] .. poff[k] + L_k - 1 (t = 0 .. L-1).  Row (k, t) holds
//   H    h_{t-1} (zero for t = 0): the state the loss term of position t and the cell step t read
//   gam  -sigmoid(-u_t), u_t = h_{t-1} . (lt[p_t] - lt[q_t])         (the factor 1 / n is applied at the write-back)
//   ACT  the gate activations of cell step t (t <= L-2), overwritten by d a_t in the backward pass; zero for t = L-1
//   CS   c_t (Lstm)
//   DX   ui^T d a_t (zero for t = L-1)
// A user needs L-1 cell steps: the reference scans to the batch's longest L and feeds pad rows to shorter users, but those steps carry
// no loss and nothing reads them.  The pad row's L2 multiplicity 2 (len_max - L) per user is analytic (one extra sorted entry).
//
// A launch with an id out of range (user outside [0, n_user), POI or negative outside [0, n_item], a length outside [1, max_len])
// moves NOTHING: the offending sequences get a NaN loss and are counted (poi_ctx_take_bad_ids), every write-back kernel returns.
#include "poi_common.h"
#include "poi_kernels.h"

namespace poi {

namespace {

constexpr int NT = CELL_NT;

// block sum in a fixed order: xor-butterfly inside each wave, the wave sums in wave order.  Contains barriers.
// (local: NT / 64 waves summed left to right - not the (0 + 1) + (2 + 3) of session_common.h's block_sum_d)
__device__ __forceinline__ double block_sum_d(double v, double* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  __syncthreads();
  if (lane_id() == 0) red[wave_id()] = v;
  __syncthreads();
  double s = red[0];
#pragma unroll
  for (int w = 1; w < NT / 64; ++w) s += red[w];
  return s;
}

// sum_{k4 in [k0, k1)} W[k4 * stride + col] . v[4 k4 .. 4 k4 + 3]: W holds four consecutive contraction indices of one output per
// float4 (cell_pack_kernel), so that the threads of a wave read consecutive float4s; v is LDS (broadcast reads)
__device__ __forceinline__ double dot_col(const float4* __restrict__ W, int stride, int col, const double* v, int k0, int k1) {
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
#pragma unroll 4
  for (int k4 = k0; k4 < k1; ++k4) {
    const float4 w = W[(size_t)k4 * stride + col];
    const double* x = v + 4 * k4;
    a0 = fma((double)w.x, x[0], a0); a1 = fma((double)w.y, x[1], a1);
    a2 = fma((double)w.z, x[2], a2); a3 = fma((double)w.w, x[3], a3);
  }
  return (a0 + a1) + (a2 + a3);
}

// contraction splits: NJ outputs on NT threads - with fewer outputs than threads the contraction is cut into ks slices whose partial
// sums meet in LDS in slice order (a function of the shape alone)
__device__ __forceinline__ int k_slices(int NJ, int K4) {
  if (NJ >= NT) return 1;
  const int ks = NT / NJ;
  return ks < K4 ? ks : K4;
}

struct Lds {
  double *xs, *hs, *cs, *dh, *dc, *av, *part, *red;
  __device__ Lds(double* sm, int D, int NO) {
    xs = sm; hs = xs + D; cs = hs + D; dh = cs + D; dc = dh + D; av = dc + D; part = av + NO; red = part + CELL_PART;
  }
};

// one cell step: reads x_t (S.xs) and h_{t-1} / c_{t-1} (S.hs / S.cs), leaves h_t / c_t there; row >= 0: records the activations
template <int G>
__device__ __forceinline__ void cell_forward(const CellArgs& A, const Lds& S, int row) {
  const int D = A.dim, NO = G * D, K4 = D >> 2, tid = threadIdx.x;
  const int ks = k_slices(NO, K4);
  for (int job = tid; job < NO * ks; job += NT) {
    const int j = job % NO, s = job / NO, k0 = s * K4 / ks, k1 = (s + 1) * K4 / ks;
    S.part[job] = dot_col(A.uiP, NO, j, S.xs, k0, k1) + dot_col(A.whP, NO, j, S.hs, k0, k1);
  }
  __syncthreads();
  if (tid < D) {
    double a[G];
#pragma unroll
    for (int g = 0; g < G; ++g) {
      double s = (double)A.bi[g * D + tid];
      for (int k = 0; k < ks; ++k) s += S.part[k * NO + g * D + tid];
      a[g] = s;
    }
    if (G == 1) {
      const double h = sigmoid_d(a[0]);
      S.hs[tid] = h;
      if (row >= 0) A.ACT[(size_t)row * NO + tid] = h;
    } else {
      const double i = sigmoid_d(a[0]), f = sigmoid_d(a[G > 1 ? 1 : 0]), g = tanh(a[G > 2 ? 2 : 0]), o = sigmoid_d(a[G > 3 ? 3 : 0]);
      const double c = f * S.cs[tid] + i * g;
      S.cs[tid] = c;
      S.hs[tid] = o * tanh(c);
      if (row >= 0) {
        double* act = A.ACT + (size_t)row * NO;
        act[tid] = i; act[D + tid] = f; act[2 * D + tid] = g; act[3 * D + tid] = o;
        A.CS[(size_t)row * D + tid] = c;
      }
    }
  }
  __syncthreads();
}

}  // namespace

// lengths, row offsets, totals; rejects users out of range.  One workgroup.
__global__ __launch_bounds__(256) void cell_plan_kernel(CellArgs A) {
  __shared__ int s_w[256];
  __shared__ int s_carry, s_bad;
  const int tid = threadIdx.x, n = A.n_seq;
  if (tid == 0) { s_carry = 0; s_bad = 0; }
  __syncthreads();
  for (int base = 0; base < n; base += 256) {
    const int k = base + tid;
    int L = 0;
    if (k < n) {
      const int u = A.uidx[k];
      bool bad = (unsigned)u >= (unsigned)A.n_user;
      if (!bad) { L = A.off[u + 1] - A.off[u]; bad = L < 1 || L > A.max_len; }
      if (bad) { L = 0; A.out[k] = __int_as_float(0x7fc00000); atomicAdd(&s_bad, 1); }
      A.slen[k] = L;
    }
    s_w[tid] = L;
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {
      const int v = tid >= o ? s_w[tid - o] : 0;
      __syncthreads();
      s_w[tid] += v;
      __syncthreads();
    }
    if (k < n) A.poff[k] = s_carry + s_w[tid] - L;
    __syncthreads();
    if (tid == 255) s_carry += s_w[255];
    __syncthreads();
  }
  if (tid == 0) {
    const int P = s_carry;
    const long long pad = 2ll * ((long long)A.len_max * (n - s_bad) - P);
    A.poff[n] = P;
    A.cnt[0] = 2 * P + 1; A.cnt[1] = P; A.cnt[2] = (int)pad; A.cnt[3] = s_bad;
    if (s_bad) atomicAdd(A.bad, s_bad);
    A.keys0[2 * P] = pad > 0 ? A.n_item : A.n_item + 1;      // the pad row's analytic touches (sentinel: no padding in this launch)
  }
}

// W (NO x D row-major: ui or wh) -> fwd[k4 * NO + o] = W[o][4 k4 ..] and bwd[o4 * D + d] = W[4 o4 ..][d]
__global__ __launch_bounds__(256) void cell_pack_kernel(CellArgs A) {
  const int D = A.dim, NO = A.G * D, n4 = NO * (D >> 2);
  for (int i = blockIdx.x * 256 + threadIdx.x; i < 2 * n4; i += gridDim.x * 256) {
    const int m = i / n4, e = i - m * n4;
    const float* W = m ? A.wh : A.ui;
    { const int k4 = e / NO, o = e - k4 * NO; (m ? A.whP : A.uiP)[e] = ld4(W + (size_t)o * D + 4 * k4); }
    { const int o4 = e / D, d = e - o4 * D;
      (m ? A.whT : A.uiT)[e] = make_float4(W[(size_t)(4 * o4) * D + d], W[(size_t)(4 * o4 + 1) * D + d], W[(size_t)(4 * o4 + 2) * D + d], W[(size_t)(4 * o4 + 3) * D + d]); }
  }
}

// forward recurrence + loss + BPTT of one sequence per workgroup; a persistent grid walks the launch
template <int G>
__global__ __launch_bounds__(CELL_NT) void cell_rec_kernel(CellArgs A) {
  extern __shared__ double cell_sm[];
  const int D = A.dim, NO = G * D, tid = threadIdx.x;
  const Lds S(cell_sm, D, NO);
  const int ksb = k_slices(2 * D, NO >> 2);
  for (int k = blockIdx.x; k < A.n_seq; k += gridDim.x) {
    const int L = A.slen[k];
    if (L == 0) continue;                                    // rejected by cell_plan_kernel
    const int base = A.off[A.uidx[k]], r0 = A.poff[k];
    int bad = 0;
    for (int t = tid; t < L; t += NT) {
      const int p = A.p[base + t], q = A.q[base + t];
      const bool b = (unsigned)p > (unsigned)A.n_item || (unsigned)q > (unsigned)A.n_item;
      bad |= b;
      A.rowp[r0 + t] = b ? 0 : p;
      A.keys0[2 * (r0 + t)] = b ? A.n_item + 1 : p;
      A.keys0[2 * (r0 + t) + 1] = b ? A.n_item + 1 : q;
    }
    if (__syncthreads_or(bad)) {
      if (tid == 0) { atomicAdd(A.bad, 1); atomicAdd(A.cnt + 3, 1); A.out[k] = __int_as_float(0x7fc00000); }
      continue;
    }
    if (tid < D) { S.hs[tid] = 0.0; S.cs[tid] = 0.0; }
    double loss = 0.0;
    for (int t = 0; t < L; ++t) {
      const int row = r0 + t;
      double prod = 0.0;
      if (tid < D) {
        const double x = (double)A.lt[(size_t)A.p[base + t] * D + tid], e = x - (double)A.lt[(size_t)A.q[base + t] * D + tid];
        S.xs[tid] = x;
        A.H[(size_t)row * D + tid] = S.hs[tid];
        prod = S.hs[tid] * e;
      }
      const double u = block_sum_d(prod, S.red);
      if (tid == 0) { loss -= log_sigmoid_d(u); A.gam[row] = -sigmoid_d(-u); }
      if (t < L - 1) cell_forward<G>(A, S, row);
    }
    if (tid == 0) A.out[k] = (float)loss;
    // BPTT: dh = d cost / d h_s (times n), complete when step s is reached
    __syncthreads();
    {
      const int row = r0 + L - 1;
      if (tid < D) {
        const double e = (double)A.lt[(size_t)A.p[base + L - 1] * D + tid] - (double)A.lt[(size_t)A.q[base + L - 1] * D + tid];
        S.dh[tid] = A.gam[row] * e;
        S.dc[tid] = 0.0;
        A.DX[(size_t)row * D + tid] = 0.0;
#pragma unroll
        for (int g = 0; g < G; ++g) A.ACT[(size_t)row * NO + g * D + tid] = 0.0;
      }
    }
    __syncthreads();
    for (int s = L - 2; s >= 0; --s) {
      const int row = r0 + s;
      if (tid < D) {
        double* act = A.ACT + (size_t)row * NO;
        const double dh = S.dh[tid];
        if (G == 1) {
          const double h = act[tid], da = dh * h * (1.0 - h);
          act[tid] = da; S.av[tid] = da;
        } else {
          const double i = act[tid], f = act[D + tid], g = act[2 * D + tid], o = act[3 * D + tid];
          const double tc = tanh(A.CS[(size_t)row * D + tid]), cp = s > 0 ? A.CS[(size_t)(row - 1) * D + tid] : 0.0;
          const double dc = S.dc[tid] + dh * o * (1.0 - tc * tc);
          const double dai = dc * g * i * (1.0 - i), daf = dc * cp * f * (1.0 - f), dag = dc * i * (1.0 - g * g), dao = dh * tc * o * (1.0 - o);
          S.dc[tid] = dc * f;
          act[tid] = dai; act[D + tid] = daf; act[2 * D + tid] = dag; act[3 * D + tid] = dao;
          S.av[tid] = dai; S.av[D + tid] = daf; S.av[2 * D + tid] = dag; S.av[3 * D + tid] = dao;
        }
      }
      __syncthreads();
      for (int job = tid; job < 2 * D * ksb; job += NT) {
        const int j = job % (2 * D), sl = job / (2 * D), k0 = sl * (NO >> 2) / ksb, k1 = (sl + 1) * (NO >> 2) / ksb;
        S.part[job] = j < D ? dot_col(A.uiT, D, j, S.av, k0, k1) : dot_col(A.whT, D, j - D, S.av, k0, k1);
      }
      __syncthreads();
      if (tid < D) {
        double dx = 0.0, dhp = 0.0;
        for (int sl = 0; sl < ksb; ++sl) { dx += S.part[sl * 2 * D + tid]; dhp += S.part[sl * 2 * D + D + tid]; }
        A.DX[(size_t)row * D + tid] = dx;
        const double e = (double)A.lt[(size_t)A.p[base + s] * D + tid] - (double)A.lt[(size_t)A.q[base + s] * D + tid];
        S.dh[tid] = dhp + A.gam[row] * e;
      }
      __syncthreads();
    }
  }
}

// seq_predict: the cell over all L positions of the snapshot, h_{L-1} to output row out_row[k] (or k)
template <int G>
__global__ __launch_bounds__(CELL_NT) void cell_predict_kernel(CellArgs A) {
  extern __shared__ double cell_sm[];
  const int D = A.dim, NO = G * D, tid = threadIdx.x;
  const Lds S(cell_sm, D, NO);
  for (int k = blockIdx.x; k < A.n_seq; k += gridDim.x) {
    const int u = A.uidx[k], orow = A.out_row ? A.out_row[k] : k;
    int L = 0, base = 0;
    bool ubad = (unsigned)u >= (unsigned)A.n_user;
    if (!ubad) { base = A.off[u]; L = A.off[u + 1] - base; ubad = L < 1; }
    int bad = ubad;
    for (int t = tid; t < L; t += NT) bad |= (unsigned)A.p[base + t] > (unsigned)A.n_item;
    if (__syncthreads_or(bad)) {
      if (tid == 0) atomicAdd(A.bad, 1);
      if (tid < D && (unsigned)orow < (unsigned)A.n_seq) A.hts[(size_t)orow * D + tid] = __int_as_float(0x7fc00000);
      continue;
    }
    if (tid < D) { S.hs[tid] = 0.0; S.cs[tid] = 0.0; }
    for (int t = 0; t < L; ++t) {
      if (tid < D) S.xs[tid] = (double)A.lt[(size_t)A.p[base + t] * D + tid];
      __syncthreads();
      cell_forward<G>(A, S, -1);
    }
    if (tid < D && (unsigned)orow < (unsigned)A.n_seq) A.hts[(size_t)orow * D + tid] = (float)S.hs[tid];
    __syncthreads();
  }
}

// dense gradients: block (c-tile, o-tile, chunk) sums d a_r (x) [x_r | h_{r-1}] over the chunk's position rows in row order, 64 x 64
// outputs per block, 4 x 4 per thread; the c-tile 0 blocks also sum d a_r (d bi).  dpart[chunk][o][2 D + 1].
__global__ __launch_bounds__(256) void cell_wgrad_kernel(CellArgs A) {
  if (A.cnt[3]) return;
  __shared__ double sa[8][64], sv[8][64];
  const int D = A.dim, NO = A.G * D, W2 = 2 * D, tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int c0 = blockIdx.x * 64, o0 = blockIdx.y * 64, z = blockIdx.z;
  const int P = A.cnt[1], rA = min(P, z * A.ch_rows), rB = min(P, rA + A.ch_rows);
  double acc[4][4] = {}, bacc[4] = {};
  for (int r = rA; r < rB; r += 8) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int i = tid + 256 * h, rr = i >> 6, cc = i & 63, row = r + rr, o = o0 + cc, c = c0 + cc;
      const bool live = row < rB;
      sa[rr][cc] = live && o < NO ? A.ACT[(size_t)row * NO + o] : 0.0;
      sv[rr][cc] = live && c < W2 ? (c < D ? (double)A.lt[(size_t)A.rowp[row] * D + c] : A.H[(size_t)row * D + c - D]) : 0.0;
    }
    __syncthreads();
#pragma unroll
    for (int rr = 0; rr < 8; ++rr) {
      double a[4], v[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) { a[i] = sa[rr][ty * 4 + i]; v[i] = sv[rr][tx * 4 + i]; }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = fma(a[i], v[j], acc[i][j]);
        bacc[i] += a[i];
      }
    }
    __syncthreads();
  }
  double* out = A.dpart + (size_t)z * NO * (W2 + 1);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int o = o0 + ty * 4 + i;
    if (o >= NO) continue;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int c = c0 + tx * 4 + j;
      if (c < W2) out[(size_t)o * (W2 + 1) + c] = acc[i][j];
    }
    if (blockIdx.x == 0 && tx == 0) out[(size_t)o * (W2 + 1) + W2] = bacc[i];
  }
}

// theta <- theta - alpha (G / n + lambda theta), G = the chunk partials in chunk order
__global__ __launch_bounds__(256) void cell_dense_kernel(CellArgs A) {
  if (A.cnt[3]) return;
  const int D = A.dim, NO = A.G * D, W2 = 2 * D, tot = NO * (W2 + 1);
  const double inv_n = 1.0 / (double)A.n_seq;
  for (int e = blockIdx.x * 256 + threadIdx.x; e < tot; e += gridDim.x * 256) {
    double g = 0.0;
    for (int z = 0; z < CELL_DENSE_CHUNKS; ++z) g += A.dpart[(size_t)z * tot + e];
    const int o = e / (W2 + 1), c = e - o * (W2 + 1);
    float* th = c < D ? A.ui + (size_t)o * D + c : c < W2 ? A.wh + (size_t)o * D + c - D : A.bi + o;
    const double v = (double)*th;
    *th = (float)(v - A.alpha * (g * inv_n + A.lambda * v));
  }
}

// new row of a run: row - alpha (G / n + lambda mult row), into the slot of the run's first sorted position
__device__ __forceinline__ void cell_apply(const CellArgs& A, int row, double g, int mult, int d, int slot) {
  const double v = (double)A.lt[(size_t)row * A.dim + d];
  A.slot[(size_t)slot * A.dim + d] = (float)(v - A.alpha * (g / (double)A.n_seq + A.lambda * (double)mult * v));
}

// one workgroup per window of 64 sorted entries, thread d owns component d; entry e: position row e >> 1, the positive (e & 1 == 0:
// + gam h_{t-1} + ui^T d a_t) or the negative (- gam h_{t-1}); e == 2 P: the pad row's multiplicity
__global__ __launch_bounds__(256) void cell_rows_kernel(CellArgs A) {
  if (A.cnt[3]) return;
  const int D = A.dim, d = threadIdx.x, N = A.cnt[0], P = A.cnt[1], sentinel = A.n_item + 1;
  const int n_chunk = (N + 63) / 64;
  for (int c = blockIdx.x; c < n_chunk; c += gridDim.x) {
    const int j0 = 64 * c, nv = min(64, N - j0);
    const int prev = c > 0 ? A.ks[j0 - 1] : -2, nextk = j0 + nv < N ? A.ks[j0 + nv] : -3;
    int lead_more = 0, trail_cnt = 0, trail_row = -1, lead_mult = 0, trail_mult = 0;
    int a = 0;
    while (a < nv) {
      const int row = A.ks[j0 + a];
      if (row == sentinel) break;                            // sorts last: nothing after it
      int b = a + 1;
      while (b < nv && A.ks[j0 + b] == row) ++b;
      const bool cont_before = a == 0 && row == prev, cont_after = b == nv && nextk == row;
      double acc = 0.0;
      int mult = 0;
      for (int j = a; j < b; ++j) {
        const int e = A.vs[j0 + j];
        if (e == 2 * P) { mult += A.cnt[2]; continue; }
        const int r = e >> 1;
        ++mult;
        if (d < D) {
          const double gh = A.gam[r] * A.H[(size_t)r * D + d];
          acc += (e & 1) ? -gh : gh + A.DX[(size_t)r * D + d];
        }
      }
      if (!cont_before && !cont_after) {
        if (d < D) cell_apply(A, row, acc, mult, d, j0 + a);
      } else {
        if (d < D) (cont_before ? A.lead : A.trail)[(size_t)c * D + d] = acc;
        if (cont_before) { lead_mult = mult; lead_more = cont_after ? 1 : 0; }
        else { trail_cnt = b - a; trail_mult = mult; trail_row = row; }
      }
      a = b;
    }
    if (d == 0) { A.meta[c] = make_int4(lead_mult, lead_more, trail_cnt, trail_row); A.mm[c] = trail_mult; }
  }
}

// runs cut by window boundaries: the window where a run starts owns it and adds the following windows' opening runs in order
__global__ __launch_bounds__(256) void cell_span_kernel(CellArgs A) {
  if (A.cnt[3]) return;
  const int D = A.dim, d = threadIdx.x, n_chunk = (A.cnt[0] + 63) / 64;
  for (int c = blockIdx.x; c < n_chunk; c += gridDim.x) {
    const int4 m = A.meta[c];
    if (m.z == 0 || d >= D) continue;
    double sum = A.trail[(size_t)c * D + d];
    int mult = A.mm[c];
    for (int c2 = c + 1; c2 < n_chunk; ++c2) {
      const int4 m2 = A.meta[c2];
      sum += A.lead[(size_t)c2 * D + d];
      mult += m2.x;
      if (!m2.y) break;
    }
    cell_apply(A, m.w, sum, mult, d, 64 * c + 64 - m.z);
  }
}

// every run's new row -> the table, after every kernel that reads the launch-entry values
__global__ __launch_bounds__(256) void cell_commit_kernel(CellArgs A) {
  if (A.cnt[3]) return;
  const int D = A.dim, d = threadIdx.x, N = A.cnt[0], sentinel = A.n_item + 1;
  for (int e = blockIdx.x; e < N; e += gridDim.x) {
    const int key = A.ks[e];
    if (d >= D || key == sentinel || (e > 0 && A.ks[e - 1] == key)) continue;
    A.lt[(size_t)key * D + d] = A.slot[(size_t)e * D + d];
  }
}

size_t cell_lds_bytes(int D, int G) { return sizeof(double) * ((size_t)5 * D + (size_t)G * D + CELL_PART + 8); }

int cell_grid(int n_seq, int cap) {
  int g = n_seq < CELL_GRID_MAX ? n_seq : CELL_GRID_MAX;
  if (cap > 0 && g > cap) g = cap;
  return g < 1 ? 1 : g;
}

// position rows per dense-gradient chunk: a function of the launch's n and max_len alone
int cell_chunk_rows(int n_seq, int max_len) {
  const long long bound = (long long)n_seq * max_len;
  long long ch = (bound + CELL_DENSE_CHUNKS - 1) / CELL_DENSE_CHUNKS;
  ch = (ch + 7) & ~7ll;
  return (int)(ch < 8 ? 8 : ch);
}

hipError_t launch_cell_step(CellArgs& A, hipStream_t st, Timing* tm) {
  const int D = A.dim, NO = A.G * D;
  const long long bound = (long long)A.n_seq * A.max_len;
  tm->begin("cell_plan", st);
  hipLaunchKernelGGL(cell_plan_kernel, dim3(1), dim3(256), 0, st, A);
  hipLaunchKernelGGL(cell_pack_kernel, dim3((2 * NO * (D / 4) + 255) / 256), dim3(256), 0, st, A);
  tm->end(st);
  tm->begin("cell_rec", st);
  const size_t lds = cell_lds_bytes(D, A.G);
  if (A.G == 1) hipLaunchKernelGGL(cell_rec_kernel<1>, dim3(A.grid), dim3(NT), lds, st, A);
  else hipLaunchKernelGGL(cell_rec_kernel<4>, dim3(A.grid), dim3(NT), lds, st, A);
  tm->end(st);
  tm->begin("cell_wgrad", st);
  hipLaunchKernelGGL(cell_wgrad_kernel, dim3((2 * D + 63) / 64, (NO + 63) / 64, CELL_DENSE_CHUNKS), dim3(256), 0, st, A);
  tm->end(st);
  tm->begin("cell_sort", st);
  int bits = 1;
  while ((1ll << bits) <= (long long)A.n_item + 1) ++bits;
  const int *ks = nullptr, *vs = nullptr;
  hipError_t e = launch_radix_sort(A.keys0, A.keys1, A.vals0, A.vals1, A.cnt, bits, A.hist, st, &ks, &vs);
  if (e != hipSuccess) return e;
  A.ks = ks; A.vs = vs;
  tm->end(st);
  const long long chunks = (2 * bound + 1 + 63) / 64;
  tm->begin("cell_rows", st);
  hipLaunchKernelGGL(cell_rows_kernel, dim3((unsigned)(chunks < 8192 ? chunks : 8192)), dim3(256), 0, st, A);
  hipLaunchKernelGGL(cell_span_kernel, dim3((unsigned)(chunks < 8192 ? chunks : 8192)), dim3(256), 0, st, A);
  tm->end(st);
  tm->begin("cell_commit", st);
  hipLaunchKernelGGL(cell_commit_kernel, dim3((unsigned)(2 * bound + 1 < 16384 ? 2 * bound + 1 : 16384)), dim3(256), 0, st, A);
  hipLaunchKernelGGL(cell_dense_kernel, dim3((NO * (2 * D + 1) + 255) / 256), dim3(256), 0, st, A);
  tm->end(st);
  return hipGetLastError();
}

hipError_t launch_cell_predict(CellArgs& A, hipStream_t st, Timing* tm) {
  const int D = A.dim, NO = A.G * D;
  tm->begin("cell_predict", st);
  hipLaunchKernelGGL(cell_pack_kernel, dim3((2 * NO * (D / 4) + 255) / 256), dim3(256), 0, st, A);
  const size_t lds = cell_lds_bytes(D, A.G);
  if (A.G == 1) hipLaunchKernelGGL(cell_predict_kernel<1>, dim3(A.grid), dim3(NT), lds, st, A);
  else hipLaunchKernelGGL(cell_predict_kernel<4>, dim3(A.grid), dim3(NT), lds, st, A);
  tm->end(st);
  return hipGetLastError();
}

}  // namespace poi
