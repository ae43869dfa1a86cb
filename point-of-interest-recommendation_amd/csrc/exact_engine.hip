// Exact engine (poi_ctx_set_engine(ctx, 4) / POI_ENGINE=exact): the Distance2Pre / plain GRU training step and the batched
// predict in FLOAT64 arithmetic end to end - the reference's Theano graphs run in float64 (floatX is never overridden:
// public/GRU.py:57, public/GRU_Spatial.py:52) and BASELINE.json asks for weights within 1e-5 of it after a step.  At the
// BASELINE shapes (D = 128, L <= 50, uniform(-0.5, 0.5) init) float32 BPTT misses that bar on ~0.1 % of the POI rows whatever
// the kernel does (conditioning, not implementation); this engine is the opt-in mode that meets it on
// every row.  Tables stay float32 in HBM (converted when they are gathered, rounded to nearest once when they are written
// back); every intermediate - gathered rows, gates, hidden states, softmax, losses, BPTT, the dense-gradient slabs, the
// sparse gradient tables and the SGD update itself - is float64.
//
// Structure: the per-sequence engine's (seq_engine.hip) - one 256-thread workgroup walks one sequence at a time over a
// persistent grid, GEMVs with one wavefront per weight row (rows streamed from L2 as float4, converted on the fly), BPTT,
// deferred outer products into the workgroup's float64 slab, sparse row gradients as float64 atomics into the float64
// gradient tables (order-dependent only at the 1e-16 level: the float32 result is reproducible except on exact rounding ties).
//
// Math: public/GRU_Spatial.py:127-229 (SPATIAL) and public/GRU.py:313-389 (plain), backward as derived in SURVEY.md 2.1.
#include "poi_common.h"
#include "poi_kernels.h"
#include "seq_common.h"

#include <hip/amd_detail/amd_hip_unsafe_atomics.h>

namespace poi {

namespace {

__device__ __forceinline__ double readlane_d(double v, int l) {
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), l), __builtin_amdgcn_readlane(__double2loint(v), l));
}
// DPP + readlane reductions: another summation order (other bits) than the xor-butterfly wave_sum_d of session_common.h
__device__ __forceinline__ double wave_sum_d(double v) {
  v += dpp_d<0xB1>(v);
  v += dpp_d<0x4E>(v);
  v += dpp_d<0x141>(v);
  v += dpp_d<0x140>(v);
  return (readlane_d(v, 0) + readlane_d(v, 16)) + (readlane_d(v, 32) + readlane_d(v, 48));
}
__device__ __forceinline__ double wave_max_d(double v) {
  v = fmax(v, dpp_d<0xB1>(v));
  v = fmax(v, dpp_d<0x4E>(v));
  v = fmax(v, dpp_d<0x141>(v));
  v = fmax(v, dpp_d<0x140>(v));
  return fmax(fmax(readlane_d(v, 0), readlane_d(v, 16)), fmax(readlane_d(v, 32), readlane_d(v, 48)));
}
__device__ __forceinline__ double block_sum_d(double v, double* red) {
  v = wave_sum_d(v);
  __syncthreads();
  if (lane_id() == 0) red[wave_id()] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}
__device__ __forceinline__ double block_max_d(double v, double* red) {
  v = wave_max_d(v);
  __syncthreads();
  if (lane_id() == 0) red[wave_id()] = v;
  __syncthreads();
  return fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
}

__device__ __forceinline__ double dot4d(const float4 w, const double* x) {
  return fma((double)w.x, x[0], fma((double)w.y, x[1], fma((double)w.z, x[2], (double)w.w * x[3])));
}

// out[r] = act(W1[r, :K1] . x1 + W2[r, :K2] . x2 + bias[r]); one wavefront per row, four rows in flight per wave.
template <int ACT>
__device__ __forceinline__ void gemv_rows_d(const float* __restrict__ W1, int K1, const double* x1, const float* __restrict__ W2, int K2,
                                            const double* x2, const float* __restrict__ bias, int nrows, double* out) {
  const int lane = lane_id(), w = wave_id();
  for (int r0 = w * 4; r0 < nrows; r0 += POI_NWAVE * 4) {
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int r = r0 + u;
      if (r < nrows) {
        const float* w1 = W1 + (size_t)r * K1;
        for (int j = lane * 4; j < K1; j += 256) acc[u] += dot4d(*reinterpret_cast<const float4*>(w1 + j), x1 + j);
        if (W2) {
          const float* w2 = W2 + (size_t)r * K2;
          for (int j = lane * 4; j < K2; j += 256) acc[u] += dot4d(*reinterpret_cast<const float4*>(w2 + j), x2 + j);
        }
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const double s = wave_sum_d(acc[u]);
      const int r = r0 + u;
      if (lane == 0 && r < nrows) {
        double v = s + (bias ? (double)bias[r] : 0.0);
        if (ACT == 1) v = sigmoid_d(v);
        if (ACT == 2) v = tanh(v);
        out[r] = v;
      }
    }
  }
}

// out[j] (+)= sum_i W[i, j] v[i]: thread t owns the float4 column t % (cols / 4) of row group t / (cols / 4); partial sums meet in `part`.
template <bool ACCUM>
__device__ __forceinline__ void gemv_cols_d(const float* __restrict__ W, int rows, int cols, const double* v, double* out, double* part) {
  const int c4n = cols >> 2;
  const int RG = POI_BLOCK / c4n > 0 ? POI_BLOCK / c4n : 1;
  const int tid = threadIdx.x;
  const int c = tid % c4n, rg = tid / c4n;
  if (rg < RG) {
    double a[4] = {0.0, 0.0, 0.0, 0.0};
    for (int i = rg; i < rows; i += RG) {
      const float4 w0 = *reinterpret_cast<const float4*>(W + (size_t)i * cols + 4 * c);
      const double v0 = v[i];
      a[0] = fma((double)w0.x, v0, a[0]); a[1] = fma((double)w0.y, v0, a[1]); a[2] = fma((double)w0.z, v0, a[2]); a[3] = fma((double)w0.w, v0, a[3]);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) part[rg * cols + 4 * c + u] = a[u];
  }
  __syncthreads();
  for (int j = tid; j < cols; j += POI_BLOCK) {
    double s = 0.0;
    for (int g = 0; g < RG; ++g) s += part[g * cols + j];
    if (ACCUM) out[j] += s; else out[j] = s;
  }
  __syncthreads();
}

struct LdsD {
  double *xs, *hcur, *rh, *act, *dh, *dacc, *mvec, *os, *part, *red;
  __device__ LdsD(double* q, int D, int XW, int NBpad) {
    xs = q; q += XW;
    hcur = q; q += D;
    rh = q; q += D;
    act = q; q += 3 * D;
    dh = q; q += D;
    dacc = q; q += XW;
    mvec = q; q += D;
    os = q; q += NBpad;
    part = q; q += 1024;
    red = q; q += 8;
  }
};
__host__ __device__ inline int ex_lds_doubles(int D, int XW, int NBpad) { return XW + D + D + 3 * D + D + XW + D + NBpad + 1024 + 8; }

__device__ __forceinline__ void load_row_d(double* dst, const float* __restrict__ src, int n) {
  for (int j = threadIdx.x * 4; j < n; j += POI_BLOCK * 4) {
    const float4 v = *reinterpret_cast<const float4*>(src + j);
    dst[j] = v.x; dst[j + 1] = v.y; dst[j + 2] = v.z; dst[j + 3] = v.w;
  }
}

// slab[row][col] += sum_t A[t * lda + row] * b(t, col)
template <typename BFN>
__device__ __forceinline__ void outer_acc_d(double* __restrict__ slab, int rows, int cols, const double* __restrict__ A, int lda, int nstep, BFN bfn) {
  const int c4n = cols >> 2;
  const int RG = POI_BLOCK / c4n > 0 ? POI_BLOCK / c4n : 1;
  const int tid = threadIdx.x;
  const int c = tid % c4n, rg = tid / c4n;
  if (rg >= RG) return;
  for (int r0 = rg; r0 < rows; r0 += 4 * RG) {
    double acc[4][4];
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int k = 0; k < 4; ++k) acc[u][k] = 0.0;
    for (int t = 0; t < nstep; ++t) {
      double b[4];
      bfn(t, c, b);
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int r = r0 + u * RG;
        const double a = r < rows ? A[(size_t)t * lda + r] : 0.0;
#pragma unroll
        for (int k = 0; k < 4; ++k) acc[u][k] = fma(a, b[k], acc[u][k]);
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int r = r0 + u * RG;
      if (r < rows) {
        double* o = slab + (size_t)r * cols + 4 * c;
#pragma unroll
        for (int k = 0; k < 4; ++k) o[k] += acc[u][k];
      }
    }
  }
}

__device__ __forceinline__ void cell_forward_d(const ExArgs& A, LdsD& S, int D, int XW, double* wsZ, double* wsR, double* wsC, double* wsH) {
  gemv_rows_d<1>(A.ui, XW, S.xs, A.wh, D, S.hcur, A.bi, 2 * D, S.act);
  __syncthreads();
  for (int j = threadIdx.x; j < D; j += POI_BLOCK) S.rh[j] = S.act[D + j] * S.hcur[j];
  __syncthreads();
  gemv_rows_d<2>(A.ui + (size_t)2 * D * XW, XW, S.xs, A.wh + (size_t)2 * D * D, D, S.rh, A.bi + 2 * D, D, S.act + 2 * D);
  __syncthreads();
  for (int j = threadIdx.x; j < D; j += POI_BLOCK) {
    const double z = S.act[j], r = S.act[D + j], c = S.act[2 * D + j], hp = S.hcur[j];
    const double hn = (1.0 - z) * hp + z * c;
    if (wsZ) { wsZ[j] = z; wsR[j] = r; wsC[j] = c; wsH[j] = hn; }
    S.hcur[j] = hn;
  }
  __syncthreads();
}

// softmax(vs . h + bs), max-subtracted (public/GRU_Spatial.py:31-37), into S.os
__device__ __forceinline__ void head_softmax_d(const ExArgs& A, LdsD& S, int D, int NB) {
  gemv_rows_d<0>(A.vs, D, S.hcur, nullptr, 0, nullptr, A.bs, NB, S.os);
  __syncthreads();
  double m = -INFINITY;
  for (int k = threadIdx.x; k < NB; k += POI_BLOCK) m = fmax(m, S.os[k]);
  m = block_max_d(m, S.red);
  double sum = 0.0;
  for (int k = threadIdx.x; k < NB; k += POI_BLOCK) { const double e = exp(S.os[k] - m); S.os[k] = e; sum += e; }
  sum = block_sum_d(sum, S.red);
  for (int k = threadIdx.x; k < NB; k += POI_BLOCK) S.os[k] /= sum;
  __syncthreads();
}

__device__ __forceinline__ void cell_backward_d(const ExArgs& A, LdsD& S, int D, int XW, const double* wsZ, const double* wsR, const double* wsC,
                                                const double* wsHp, double* wsDA) {
  const int j = threadIdx.x;          // dim <= 256: one hidden column per thread
  const bool on = j < D;
  double dz = 0.0, dhp = 0.0, z = 0.0, r = 0.0, hp = 0.0;
  if (on) {
    z = wsZ[j]; r = wsR[j]; hp = wsHp[j];
    const double c = wsC[j], d = S.dh[j];
    dz = d * (c - hp);
    dhp = d * (1.0 - z);
    S.act[2 * D + j] = d * z * (1.0 - c * c);
  }
  __syncthreads();
  gemv_cols_d<false>(A.wh + (size_t)2 * D * D, D, D, S.act + 2 * D, S.mvec, S.part);
  if (on) {
    const double m = S.mvec[j];
    const double dr = m * hp;
    dhp += m * r;
    S.act[j] = dz * z * (1.0 - z);
    S.act[D + j] = dr * r * (1.0 - r);
  }
  __syncthreads();
  gemv_cols_d<false>(A.wh, 2 * D, D, S.act, S.mvec, S.part);
  gemv_cols_d<false>(A.ui, 3 * D, XW, S.act, S.dacc, S.part);
  if (on) S.dh[j] = dhp + S.mvec[j];
  for (int i = threadIdx.x; i < 3 * D; i += POI_BLOCK) wsDA[i] = S.act[i];
  __syncthreads();
}

__device__ __forceinline__ void atomic_add_d(double* p, double v) { (void)unsafeAtomicAdd(p, v); }

template <bool SPATIAL>
__global__ __launch_bounds__(POI_BLOCK) void ex_train_kernel(ExArgs A) {
  extern __shared__ __align__(16) double lds_raw_d[];
  const int D = A.dim, XW = SPATIAL ? 2 * D : D, NB = SPATIAL ? A.n_dist + 1 : 0;
  const int NBpad = (NB + 3) & ~3;
  LdsD S(lds_raw_d, D, XW, NBpad);
  const int tid = threadIdx.x;
  const DenseLayout dl = dense_layout(D, XW, NB);

  double* ws = A.ws + (size_t)blockIdx.x * A.ws_stride;
  double* wsH = ws;
  double* wsZ = wsH + (size_t)(A.cap + 1) * D;
  double* wsR = wsZ + (size_t)A.cap * D;
  double* wsC = wsR + (size_t)A.cap * D;
  double* wsDA = wsC + (size_t)A.cap * D;
  double* wsS = wsDA + (size_t)A.cap * 3 * D;
  double* wsU = wsS + (size_t)A.cap * NBpad;
  double* slab = A.slab + (size_t)blockIdx.x * dl.total;

  double ls0 = 0.0, ls1 = 1.0, wd = 0.0;
  if (SPATIAL) {
    const double a = A.lw[0], b = A.lw[1], m = fmax(a, b);
    const double ea = exp(a - m), eb = exp(b - m);
    ls0 = ea / (ea + eb); ls1 = eb / (ea + eb);
    wd = A.wd[0];
  }

  for (int k = blockIdx.x; k < A.n_seq; k += gridDim.x) {
    const int u = A.uidx[k];
    const int base = A.off[u];
    const int L = A.off[u + 1] - base;
    const int* p = A.p + base;
    const int* q = A.q + base;
    const int* dp = SPATIAL ? A.dp + base : nullptr;
    const int* dq = SPATIAL ? A.dq + base : nullptr;
    const int nstep = SPATIAL ? (L > 0 ? L - 1 : 0) : L;

    count_rows<true>(p, q, L, A.n_item, 2 * (A.len_max - L), A.mult_lt, A.nseq_lt);
    if (SPATIAL) count_rows<false>(dp, dp, L, A.n_dist, A.len_max - L, A.mult_di, A.nseq_di);

    for (int j = tid; j < D; j += POI_BLOCK) { S.hcur[j] = 0.0; wsH[j] = 0.0; }
    double sur = 0.0, bpr = 0.0;
    __syncthreads();

    for (int t = 0; t < nstep; ++t) {
      const float* xp = A.lt + (size_t)p[t] * D;
      load_row_d(S.xs, xp, D);
      if (SPATIAL) load_row_d(S.xs + D, A.di + (size_t)dp[t] * D, D);
      if (!SPATIAL) {
        const float* xq = A.lt + (size_t)q[t] * D;
        double part = 0.0;
        for (int j = tid; j < D; j += POI_BLOCK) part += S.hcur[j] * ((double)xp[j] - (double)xq[j]);
        const double ut = block_sum_d(part, S.red);
        if (tid == 0) { wsU[t] = ut; bpr += log_sigmoid_d(ut); }
      }
      __syncthreads();
      cell_forward_d(A, S, D, XW, wsZ + (size_t)t * D, wsR + (size_t)t * D, wsC + (size_t)t * D, wsH + (size_t)(t + 1) * D);
      if (SPATIAL) {
        head_softmax_d(A, S, D, NB);
        const int a = dp[t + 1], b = dq[t + 1];
        const float* xp1 = A.lt + (size_t)p[t + 1] * D;
        const float* xq1 = A.lt + (size_t)q[t + 1] * D;
        double part = 0.0, cum = 0.0;
        for (int j = tid; j < D; j += POI_BLOCK) part += S.hcur[j] * ((double)xp1[j] - (double)xq1[j]);
        for (int kk = tid; kk < NB; kk += POI_BLOCK) { const double s = S.os[kk]; wsS[(size_t)t * NBpad + kk] = s; if (kk <= a) cum += s; }
        const double he = block_sum_d(part, S.red);
        const double cs = block_sum_d(cum, S.red);
        if (tid == 0) {
          const double sa = S.os[a], sb = S.os[b];
          const double ut = he + wd * (sa - sb);
          wsU[t] = ut;
          bpr += log_sigmoid_d(ut);
          sur += cs - log(sa);
        }
        __syncthreads();
      }
    }
    if (tid == 0) {
      if (SPATIAL) {
        const double upq = -bpr;
        float* o = A.out + (size_t)k * 5;
        o[0] = (float)(ls0 * sur + ls1 * upq); o[1] = (float)sur; o[2] = (float)upq; o[3] = (float)ls0; o[4] = (float)ls1;
        slab[dl.sur] += sur; slab[dl.upq] += upq;
      } else {
        A.out[k] = (float)(-bpr);
      }
    }

    for (int j = tid; j < D; j += POI_BLOCK) S.dh[j] = 0.0;
    __syncthreads();
    for (int t = nstep - 1; t >= 0; --t) {
      const double* h_t = wsH + (size_t)(t + 1) * D;
      const double* h_p = wsH + (size_t)t * D;
      double g_plain = 0.0;
      if (SPATIAL) {
        const int a = dp[t + 1], b = dq[t + 1];
        const double ut = wsU[t];
        const double g = -ls1 * sigmoid_d(-ut);
        double* st = wsS + (size_t)t * NBpad;
        const double sa = st[a], sb = st[b];
        double part = 0.0;
        for (int kk = tid; kk < NB; kk += POI_BLOCK) {
          const double s = st[kk];
          double ds = (kk <= a ? ls0 : 0.0);
          if (kk == a) ds += g * wd - ls0 / sa;
          if (kk == b) ds -= g * wd;
          S.os[kk] = ds;
          part += ds * s;
        }
        const double dot = block_sum_d(part, S.red);
        for (int kk = tid; kk < NB; kk += POI_BLOCK) {
          const double dlog = st[kk] * (S.os[kk] - dot);
          S.os[kk] = dlog;
          st[kk] = dlog;
          slab[dl.bs + kk] += dlog;
        }
        if (tid == 0) slab[dl.wd] += g * (sa - sb);
        const float* xp1 = A.lt + (size_t)p[t + 1] * D;
        const float* xq1 = A.lt + (size_t)q[t + 1] * D;
        double* gp = A.g_lt + (size_t)p[t + 1] * D;
        double* gq = A.g_lt + (size_t)q[t + 1] * D;
        for (int j = tid; j < D; j += POI_BLOCK) {
          const double hv = h_t[j];
          S.dh[j] += g * ((double)xp1[j] - (double)xq1[j]);
          atomic_add_d(gp + j, g * hv);
          atomic_add_d(gq + j, -g * hv);
        }
        __syncthreads();
        gemv_cols_d<true>(A.vs, NB, D, S.os, S.dh, S.part);
      } else {
        g_plain = -sigmoid_d(-wsU[t]);
      }
      cell_backward_d(A, S, D, XW, wsZ + (size_t)t * D, wsR + (size_t)t * D, wsC + (size_t)t * D, h_p, wsDA + (size_t)t * 3 * D);
      {
        double* gp = A.g_lt + (size_t)p[t] * D;
        for (int j = tid; j < D; j += POI_BLOCK) atomic_add_d(gp + j, S.dacc[j]);
        if (SPATIAL) {
          double* gd = A.g_di + (size_t)dp[t] * D;
          for (int j = tid; j < D; j += POI_BLOCK) atomic_add_d(gd + j, S.dacc[D + j]);
        } else {
          const float* xp = A.lt + (size_t)p[t] * D;
          const float* xq = A.lt + (size_t)q[t] * D;
          double* gq = A.g_lt + (size_t)q[t] * D;
          for (int j = tid; j < D; j += POI_BLOCK) {
            const double hv = h_p[j];
            atomic_add_d(gp + j, g_plain * hv);
            atomic_add_d(gq + j, -g_plain * hv);
            S.dh[j] += g_plain * ((double)xp[j] - (double)xq[j]);
          }
        }
      }
      __syncthreads();
    }

    if (nstep > 0) {
      const float* lt = A.lt; const float* di = A.di;
      outer_acc_d(slab + dl.ui, 3 * D, XW, wsDA, 3 * D, nstep, [&](int t, int c, double* b) {
        const int col = 4 * c;
        const float* src = (!SPATIAL || col < D) ? lt + (size_t)p[t] * D + col : di + (size_t)dp[t] * D + (col - D);
        const float4 v = *reinterpret_cast<const float4*>(src);
        b[0] = v.x; b[1] = v.y; b[2] = v.z; b[3] = v.w;
      });
      outer_acc_d(slab + dl.wh, 2 * D, D, wsDA, 3 * D, nstep, [&](int t, int c, double* b) {
        const double* h = wsH + (size_t)t * D + 4 * c;
        b[0] = h[0]; b[1] = h[1]; b[2] = h[2]; b[3] = h[3];
      });
      outer_acc_d(slab + dl.wh + (size_t)2 * D * D, D, D, wsDA + 2 * D, 3 * D, nstep, [&](int t, int c, double* b) {
        const double* h = wsH + (size_t)t * D + 4 * c;
        const double* r = wsR + (size_t)t * D + 4 * c;
        b[0] = h[0] * r[0]; b[1] = h[1] * r[1]; b[2] = h[2] * r[2]; b[3] = h[3] * r[3];
      });
      for (int r = tid; r < 3 * D; r += POI_BLOCK) {
        double s = 0.0;
        for (int t = 0; t < nstep; ++t) s += wsDA[(size_t)t * 3 * D + r];
        slab[dl.bi + r] += s;
      }
      if (SPATIAL)
        outer_acc_d(slab + dl.vs, NB, D, wsS, NBpad, nstep, [&](int t, int c, double* b) {
          const double* h = wsH + (size_t)(t + 1) * D + 4 * c;
          b[0] = h[0]; b[1] = h[1]; b[2] = h[2]; b[3] = h[3];
        });
    }
    __syncthreads();
  }
}

template <bool SPATIAL>
__global__ __launch_bounds__(POI_BLOCK) void ex_predict_kernel(ExArgs A) {
  extern __shared__ __align__(16) double lds_raw_d[];
  const int D = A.dim, XW = SPATIAL ? 2 * D : D, NB = SPATIAL ? A.n_dist + 1 : 0;
  const int NBpad = (NB + 3) & ~3;
  LdsD S(lds_raw_d, D, XW, NBpad);
  const int tid = threadIdx.x;
  for (int k = blockIdx.x; k < A.n_seq; k += gridDim.x) {
    const int u = A.uidx[k];
    const int base = A.off[u];
    const int L = A.off[u + 1] - base;
    for (int j = tid; j < D; j += POI_BLOCK) S.hcur[j] = 0.0;
    __syncthreads();
    for (int t = 0; t < L; ++t) {
      load_row_d(S.xs, A.lt + (size_t)A.p[base + t] * D, D);
      if (SPATIAL) load_row_d(S.xs + D, A.di + (size_t)A.dp[base + t] * D, D);
      __syncthreads();
      cell_forward_d(A, S, D, XW, nullptr, nullptr, nullptr, nullptr);
    }
    const int ko = A.out_row ? A.out_row[k] : k;
    for (int j = tid; j < D; j += POI_BLOCK) A.hts[(size_t)ko * D + j] = (float)S.hcur[j];
    if (SPATIAL && A.sts) {
      head_softmax_d(A, S, D, NB);
      for (int kk = tid; kk < NB; kk += POI_BLOCK) A.sts[(size_t)ko * NB + kk] = (float)S.os[kk];
    }
    __syncthreads();
  }
}

// Batch rule in float64 (rule_scales of poi_common.h): row -= sc (G + lm row)
__device__ __forceinline__ void rule_scales_d(double alpha, double lambda, int nseq, int mult, double cap, double& sc, double& lm) {
  if (cap < 0.0) { sc = alpha / -cap; lm = lambda * (double)mult * -cap; }
  else { sc = alpha * fmin((double)nseq, cap) / (double)max(nseq, 1); lm = lambda * (double)mult; }
}

__device__ __forceinline__ void apply_row_d(float* __restrict__ T, double* __restrict__ G, int* __restrict__ mult, int* __restrict__ nseq, int row,
                                            int D, double alpha, double lambda, double cap) {
  const int got = nseq[row];
  if (got <= 0) return;
  double sc, lm; rule_scales_d(alpha, lambda, got, mult[row], cap, sc, lm);
  float* t = T + (size_t)row * D;
  double* g = G + (size_t)row * D;
  for (int j = lane_id(); j < D; j += 64) {
    const double tv = (double)t[j];
    t[j] = (float)(tv - sc * (g[j] + lm * tv));
    g[j] = 0.0;
  }
  if (lane_id() == 0) { nseq[row] = 0; mult[row] = 0; }
}

template <bool SPATIAL>
__global__ __launch_bounds__(POI_BLOCK) void ex_rows_apply_kernel(ExArgs A, double alpha, double lambda) {
  const int D = A.dim;
  const int n_lt = A.n_item + 1, n_di = SPATIAL ? A.n_dist + 1 : 0;
  for (int r = blockIdx.x * POI_NWAVE + wave_id(); r < n_lt + n_di; r += gridDim.x * POI_NWAVE) {
    if (r < n_lt) apply_row_d(A.lt, A.g_lt, A.mult_lt, A.nseq_lt, r, D, alpha, lambda, (double)A.bcap);
    else apply_row_d(A.di, A.g_di, A.mult_di, A.nseq_di, r - n_lt, D, alpha, lambda, (double)A.bcap);
  }
}

// theta <- theta - alpha min(n, cap) (mean_k grad_k + lambda theta) in float64 (public/GRU_Spatial.py:210-211 for n == 1); slabs re-zeroed
template <bool SPATIAL>
__global__ __launch_bounds__(POI_BLOCK) void ex_dense_apply_kernel(ExArgs A, int n_slab, double alpha, double lambda) {
  const int D = A.dim, XW = SPATIAL ? 2 * D : D, NB = SPATIAL ? A.n_dist + 1 : 0;
  const DenseLayout dl = dense_layout(D, XW, NB);
  const double inv_n = 1.0 / (double)A.n_seq;
  alpha *= A.bcap < 0.f ? 1.0 : fmin((double)A.n_seq, (double)A.bcap);
  const int i = blockIdx.x * POI_BLOCK + threadIdx.x;
  if (i >= dl.total) return;
  if (SPATIAL && i == dl.upq) return;
  double g = 0.0;
  for (int s = 0; s < n_slab; ++s) { double* p0 = A.slab + (size_t)s * dl.total + i; g += *p0; *p0 = 0.0; }
  g *= inv_n;
  float* theta = nullptr;
  if (i < dl.wh) theta = A.ui + (i - dl.ui);
  else if (i < dl.bi) theta = A.wh + (i - dl.wh);
  else if (i < dl.vs) theta = A.bi + (i - dl.bi);
  else if (i < dl.bs) theta = A.vs + (i - dl.vs);
  else if (i < dl.wd) theta = A.bs + (i - dl.bs);
  else if (i == dl.wd) { if (SPATIAL) theta = A.wd; }
  if (theta) { const double v = (double)*theta; *theta = (float)(v - alpha * (g + lambda * v)); return; }
  if (SPATIAL && i == dl.sur) {
    double upq = 0.0;
    for (int s = 0; s < n_slab; ++s) { double* ptr = A.slab + (size_t)s * dl.total + dl.upq; upq += *ptr; *ptr = 0.0; }
    upq *= inv_n;
    const double a = A.lw[0], b = A.lw[1], m = fmax(a, b);
    const double ea = exp(a - m), eb = exp(b - m);
    const double ls0 = ea / (ea + eb), ls1 = eb / (ea + eb);
    const double d0 = g + lambda * ls0, d1 = upq + lambda * ls1;
    const double dot = d0 * ls0 + d1 * ls1;
    A.lw[0] = (float)(a - alpha * ls0 * (d0 - dot));
    A.lw[1] = (float)(b - alpha * ls1 * (d1 - dot));
  }
}

}  // namespace

size_t ex_ws_doubles(int D, int NB, int cap) {
  const int NBpad = (NB + 3) & ~3;
  return (size_t)(cap + 1) * D + (size_t)3 * cap * D + (size_t)cap * 3 * D + (size_t)cap * NBpad + (size_t)cap + 16;
}

hipError_t launch_ex_train(const ExArgs& A, bool spatial, int grid, double alpha, double lambda, hipStream_t st, Timing* tm) {
  const int D = A.dim, XW = spatial ? 2 * D : D, NB = spatial ? A.n_dist + 1 : 0;
  const size_t lds = sizeof(double) * ex_lds_doubles(D, XW, (NB + 3) & ~3);
  tm->begin("ex_train", st);
  if (spatial) hipLaunchKernelGGL(ex_train_kernel<true>, dim3(grid), dim3(POI_BLOCK), lds, st, A);
  else hipLaunchKernelGGL(ex_train_kernel<false>, dim3(grid), dim3(POI_BLOCK), lds, st, A);
  tm->end(st);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const int rows = A.n_item + 1 + (spatial ? A.n_dist + 1 : 0);
  int rgrid = (rows + POI_NWAVE - 1) / POI_NWAVE;
  if (rgrid > 8192) rgrid = 8192;
  tm->begin("ex_rows_apply", st);
  if (spatial) hipLaunchKernelGGL(ex_rows_apply_kernel<true>, dim3(rgrid), dim3(POI_BLOCK), 0, st, A, alpha, lambda);
  else hipLaunchKernelGGL(ex_rows_apply_kernel<false>, dim3(rgrid), dim3(POI_BLOCK), 0, st, A, alpha, lambda);
  tm->end(st);
  const DenseLayout dl = dense_layout(D, XW, NB);
  const int dgrid = (dl.total + POI_BLOCK - 1) / POI_BLOCK;
  tm->begin("ex_dense_apply", st);
  if (spatial) hipLaunchKernelGGL(ex_dense_apply_kernel<true>, dim3(dgrid), dim3(POI_BLOCK), 0, st, A, grid, alpha, lambda);
  else hipLaunchKernelGGL(ex_dense_apply_kernel<false>, dim3(dgrid), dim3(POI_BLOCK), 0, st, A, grid, alpha, lambda);
  tm->end(st);
  return hipGetLastError();
}

hipError_t launch_ex_predict(const ExArgs& A, bool spatial, int grid, hipStream_t st, Timing* tm) {
  const int D = A.dim, XW = spatial ? 2 * D : D, NB = spatial ? A.n_dist + 1 : 0;
  const size_t lds = sizeof(double) * ex_lds_doubles(D, XW, (NB + 3) & ~3);
  tm->begin("ex_predict", st);
  if (spatial) hipLaunchKernelGGL(ex_predict_kernel<true>, dim3(grid), dim3(POI_BLOCK), lds, st, A);
  else hipLaunchKernelGGL(ex_predict_kernel<false>, dim3(grid), dim3(POI_BLOCK), lds, st, A);
  tm->end(st);
  return hipGetLastError();
}

}  // namespace poi
