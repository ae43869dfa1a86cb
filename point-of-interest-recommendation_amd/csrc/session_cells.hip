// Online sessions of the baselines (poi_session_cell_advance / poi_session_carnn_advance): per-slot state of Lstm, Rnn and CA-RNN kept on
// the device and advanced ONE check-in at a time - the cell steps of poi_cell_predict (public/GRU.py:562-567, :720-722) and
// poi_carnn_predict (public/CA_RNN.py:172-217, literally) on the evaluation snapshots, for a batch of (slot, POI) events.
//
// State of slot s: h[s] (D float64), c[s] (D float64, Lstm only), last_poi[s] (-1: none yet), steps[s].  Tables are float32 at the
// model's own dim (these classes are never padded); every product, gate sum, sigmoid and tanh is float64.  No atomics on results: an
// event owns its slot rows, sums run in a fixed order - identical calls give bitwise identical state.
//
// One kernel family per regime, templated on the cell (G = gate blocks: 1 Rnn, 4 Lstm, 0 CA-RNN), in the shapes of session.hip:
//   event path  one workgroup per event: a wave takes four output rows at a time, the lanes stride a row in float4, a float64
//               xor-butterfly closes each dot product.  Lstm walks all 4 D rows in ONE pass (its gate products do not depend on each
//               other) and the thread that owns unit u combines i, f, g, o after one barrier.  CA-RNN sums the row of wd[d] in the same
//               walk that dots the row of M with x, and takes sum(h) as a block sum.
//   tile path   16 events per workgroup on v_mfma_f64_16x16x4_f64 with the operand layout of sess_tile_kernel: weights = A operand (one
//               float4 per lane and k-block, straight from the row-major tensors), gathered rows [x | h] = B operand, k-major in LDS at
//               stride 17 and rows swz(k).  A wave owns every gate of its unit tiles: c and h are finished in registers, no barrier sits
//               between the products.  CA-RNN has K = D only; rowsum(wd[d]) comes from a pre-pass (float64, rewritten on every call)
//               and sum(h) from 16 lanes per event.
//
// Bad ids and repeated slots behave as in poi_session_advance: slot untouched, NaN hts_out row, counted (poi_ctx_take_bad_ids).
#include "poi_common.h"
#include "poi_kernels.h"
#include "session_common.h"

namespace poi {

namespace {

// this lane's share of sum(w[0 .. K)): row_part's walk
__device__ __forceinline__ double row_sum_part(const float* __restrict__ w, int K, int lane) {
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
  for (int j = lane * 4; j < K; j += 256) {
    const float4 v = ld4(w + j);
    a0 += (double)v.x; a1 += (double)v.y; a2 += (double)v.z; a3 += (double)v.w;
  }
  return (a0 + a1) + (a2 + a3);
}

// acc[q] += W_q[16 rows][K] . S[K][16 events]: wrow[q] = this lane's row of W_q at column 4 g; S k-major in LDS at the swizzled rows
// (rows swz(k), session_common.h).  Not session.hip's sess_mma: this one keeps the next k-block's weights in flight - another schedule.
template <int NG, class T>
__device__ __forceinline__ void sc_mma(f64x4 (&acc)[NG], const float* (&wrow)[NG], int K, const T* sT, int i, int g) {
  const int nk = K >> 4;
  float4 an[NG];      // the next k-block's weights are in flight while this one's MFMAs issue (the last block reloads itself)
#pragma unroll
  for (int q = 0; q < NG; ++q) an[q] = ld4(wrow[q]);
  for (int kq = 0; kq < nk; ++kq) {
    float4 a[NG];
    const int kn = kq + 1 < nk ? kq + 1 : kq;
#pragma unroll
    for (int q = 0; q < NG; ++q) { a[q] = an[q]; an[q] = ld4(wrow[q] + 16 * kn); }
    const T* bp = sT + (size_t)(16 * kq + g) * RS + i;
    const double b0 = (double)bp[0], b1 = (double)bp[4 * RS], b2 = (double)bp[8 * RS], b3 = (double)bp[12 * RS];
#pragma unroll
    for (int q = 0; q < NG; ++q) acc[q] = __builtin_amdgcn_mfma_f64_16x16x4f64((double)a[q].x, b0, acc[q], 0, 0, 0);
#pragma unroll
    for (int q = 0; q < NG; ++q) acc[q] = __builtin_amdgcn_mfma_f64_16x16x4f64((double)a[q].y, b1, acc[q], 0, 0, 0);
#pragma unroll
    for (int q = 0; q < NG; ++q) acc[q] = __builtin_amdgcn_mfma_f64_16x16x4f64((double)a[q].z, b2, acc[q], 0, 0, 0);
#pragma unroll
    for (int q = 0; q < NG; ++q) acc[q] = __builtin_amdgcn_mfma_f64_16x16x4f64((double)a[q].w, b3, acc[q], 0, 0, 0);
  }
}

}  // namespace

// ---- CA-RNN pre-pass of the tile path: wrs[b][i] = sum_k wd[b][i][k] in float64, one workgroup per interval matrix ---------------------
__global__ __launch_bounds__(256) void sc_rowsum_kernel(const float* __restrict__ wd, int D, double* __restrict__ wrs) {
  const int b = blockIdx.x, lane = lane_id(), w = wave_id();
  for (int o0 = w * 4; o0 < D; o0 += 16) {
    double acc[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) acc[u] = row_sum_part(wd + ((size_t)b * D + o0 + u) * D, D, lane);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const double s = wave_sum_d(acc[u]);
      if (lane == 0) wrs[(size_t)b * D + o0 + u] = s;
    }
  }
}

// ---- event path: one workgroup per event ----------------------------------------------------------------------------------------------
template <int G>
__global__ __launch_bounds__(256) void sc_event_kernel(SessCellArgs A) {
  extern __shared__ __align__(16) unsigned char sc_sm[];
  constexpr int NGB = G == 4 ? 4 : 1;
  const int D = A.dim, NO = NGB * D, tid = threadIdx.x, lane = lane_id(), w = wave_id();
  double* xs = reinterpret_cast<double*>(sc_sm);      // [D]
  double* hs = xs + D;                                 // [D]
  double* cs = hs + D;                                 // [D] (Lstm; unused otherwise)
  double* act = cs + D;                                // [NO] gate activations
  double* red = act + NO;                              // [4]
  for (int e = blockIdx.x; e < A.n; e += gridDim.x) {
    const int s = A.slot[e], j = A.poi[e];
    int bad = (unsigned)s >= (unsigned)A.n_slot || (unsigned)j >= (unsigned)A.n_item;
    if (!bad) {
      if (A.owner) bad = A.owner[s] != e;
      else for (int o = tid; o < A.n; o += 256) bad |= o != e && A.slot[o] == s;
    }
    if (__syncthreads_or(bad)) {
      if (tid == 0) atomicAdd(A.bad, 1);
      if (A.hts_out) for (int u = tid; u < D; u += 256) A.hts_out[(size_t)e * D + u] = quiet_nan();
      continue;
    }
    double* hrow = A.h + (size_t)s * D;
    double* crow = G == 4 ? A.c + (size_t)s * D : nullptr;
    int d = 0;
    if (G == 0) { const int lp = A.last_poi[s]; d = lp >= 0 ? pos_bin(A, j, lp) : A.n_dist; }
    for (int u = tid; u < D; u += 256) {
      xs[u] = (double)A.lt[(size_t)j * D + u];
      hs[u] = hrow[u];
      if (G == 4) cs[u] = crow[u];
    }
    __syncthreads();
    double hsum = 0.0;
    if (G == 0) {
      double part = 0.0;
      for (int u = tid; u < D; u += 256) part += hs[u];
      hsum = block_sum_d(part, red);
    }
    // every gate row in one pass, four rows of a wave in flight (NO % 4 == 0)
    for (int o0 = w * 4; o0 < NO; o0 += 16) {
      double acc[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const size_t o = (size_t)(o0 + u);
        if (G == 0) acc[u] = row_part(A.ui + o * D, D, xs, lane) + row_sum_part(A.wh + ((size_t)d * D + o) * D, D, lane);
        else acc[u] = row_part(A.ui + o * D, D, xs, lane) + row_part(A.wh + o * D, D, hs, lane);
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const double a = wave_sum_d(acc[u]);
        const int o = o0 + u;
        if (lane == 0) {
          if (G == 0) act[o] = sigmoid_d(a + hsum);
          else if (G == 4 && o >= 2 * D && o < 3 * D) act[o] = tanh(a + (double)A.bi[o]);
          else act[o] = sigmoid_d(a + (double)A.bi[o]);
        }
      }
    }
    __syncthreads();
    for (int u = tid; u < D; u += 256) {
      double hn;
      if (G == 4) {
        const double cn = act[D + u] * cs[u] + act[u] * act[2 * D + u];
        hn = act[3 * D + u] * tanh(cn);
        crow[u] = cn;
      } else hn = act[u];
      hrow[u] = hn;
      if (A.hts_out) A.hts_out[(size_t)e * D + u] = (float)hn;
    }
    if (tid == 0) { A.last_poi[s] = j; A.steps[s] += 1; }
    __syncthreads();
  }
}

// ---- tile path: 16 events per workgroup, float64 MFMA ---------------------------------------------------------------------------------
size_t sess_cell_tile_lds(int G, int D) {
  return sizeof(float) * RS * (size_t)D + sizeof(double) * RS * (size_t)D * (G == 0 ? 1 : G == 1 ? 2 : 3);
}
size_t sess_cell_event_lds(int G, int D) { return sizeof(double) * ((size_t)(3 + (G == 4 ? 4 : 1)) * D + 4); }
bool sess_cell_tile_supported(int G, int D) { return D >= 16 && D % 16 == 0 && D <= 256 && sess_cell_tile_lds(G, D) <= SESS_TILE_LDS_MAX; }

template <int G>
__global__ __launch_bounds__(256) void sc_tile_kernel(SessCellArgs A) {
  extern __shared__ __align__(16) unsigned char sc_sm[];
  constexpr int NG = G == 4 ? 4 : 1;
  const int D = A.dim, NT = D >> 4;
  float* xT = reinterpret_cast<float*>(sc_sm);                                   // [D][RS] float32: table values are exact in it
  double* hT = reinterpret_cast<double*>(sc_sm + sizeof(float) * RS * (size_t)D); // [D][RS] (D % 16 == 0: 68 D bytes keep the alignment)
  double* nT = G == 0 ? hT : hT + (size_t)D * RS;                                // [D][RS] new state (CA-RNN: hT is no operand, a lane overwrites its own units)
  double* cT = nT + (size_t)D * RS;                                              // [D][RS] Lstm only
  __shared__ int s_slot[16], s_poi[16], s_d[16], s_ok[16];
  __shared__ double s_hsum[16];
  const int tid = threadIdx.x, lane = lane_id(), w = wave_id(), i = lane & 15, g = lane >> 4;
  const int e0 = blockIdx.x * 16;
  if (tid < 16) {
    const int e = e0 + tid;
    int ok = 0, s = 0, j = 0, d = A.n_dist;
    if (e < A.n) {
      s = A.slot[e]; j = A.poi[e];
      const bool bad = (unsigned)s >= (unsigned)A.n_slot || (unsigned)j >= (unsigned)A.n_item || (A.owner && A.owner[s] != e);
      if (bad) atomicAdd(A.bad, 1);
      else {
        ok = 1;
        if (G == 0) { const int lp = A.last_poi[s]; if (lp >= 0) d = pos_bin(A, j, lp); }
      }
    }
    s_slot[tid] = s; s_poi[tid] = j; s_d[tid] = d; s_ok[tid] = ok;
  }
  __syncthreads();
  for (int idx = tid; idx < 16 * D; idx += 256) {
    const int e = idx / D, u = idx - e * D, ok = s_ok[e], su = swz(u);
    xT[su * RS + e] = ok ? A.lt[(size_t)s_poi[e] * D + u] : 0.f;
    hT[su * RS + e] = ok ? A.h[(size_t)s_slot[e] * D + u] : 0.0;
    if (G == 4) cT[su * RS + e] = ok ? A.c[(size_t)s_slot[e] * D + u] : 0.0;
  }
  __syncthreads();
  if (G == 0) {      // sum(h) of event e on 16 lanes, fixed order
    const int e = tid >> 4, q = tid & 15;
    double s = 0.0;
    for (int u = q; u < D; u += 16) s += hT[u * RS + e];
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (q == 0) s_hsum[e] = s;
    __syncthreads();
  }
  // wave w owns the unit tiles w, w + 4, ... (D <= 256: at most four) of every gate; C layout of the f64 MFMA: register r of lane (i, g) =
  // unit 16 ut + g + 4 r of event i
#pragma unroll 1
  for (int t = 0; t < 4; ++t) {
    const int ut = w + 4 * t;
    if (ut >= NT) break;
    const int row = 16 * ut + i;
    f64x4 acc[NG];
    const float* wp[NG];
#pragma unroll
    for (int q = 0; q < NG; ++q) { acc[q] = f64x4{0.0, 0.0, 0.0, 0.0}; wp[q] = A.ui + ((size_t)q * D + row) * D + 4 * g; }
    sc_mma<NG>(acc, wp, D, xT, i, g);
    if (G != 0) {
#pragma unroll
      for (int q = 0; q < NG; ++q) wp[q] = A.wh + ((size_t)q * D + row) * D + 4 * g;
      sc_mma<NG>(acc, wp, D, hT, i, g);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int unit = 16 * ut + g + 4 * r, at = swz(unit) * RS + i;
      if constexpr (G == 0) {
        nT[at] = sigmoid_d(acc[0][r] + A.wrs[(size_t)s_d[i] * D + unit] + s_hsum[i]);
      } else if constexpr (G == 1) {
        nT[at] = sigmoid_d(acc[0][r] + (double)A.bi[unit]);
      } else {      // cT[at]: read and written by this lane only
        const double ig = sigmoid_d(acc[0][r] + (double)A.bi[unit]), fg = sigmoid_d(acc[1][r] + (double)A.bi[D + unit]);
        const double gg = tanh(acc[2][r] + (double)A.bi[2 * D + unit]), og = sigmoid_d(acc[3][r] + (double)A.bi[3 * D + unit]);
        const double cn = fg * cT[at] + ig * gg;
        cT[at] = cn;
        nT[at] = og * tanh(cn);
      }
    }
  }
  __syncthreads();
  for (int idx = tid; idx < 16 * D; idx += 256) {
    const int e = idx / D, u = idx - e * D;
    if (e0 + e >= A.n) break;
    const int at = swz(u) * RS + e;
    const double v = nT[at];
    if (s_ok[e]) {
      A.h[(size_t)s_slot[e] * D + u] = v;
      if (G == 4) A.c[(size_t)s_slot[e] * D + u] = cT[at];
    }
    if (A.hts_out) A.hts_out[(size_t)(e0 + e) * D + u] = s_ok[e] ? (float)v : quiet_nan();
  }
  if (tid < 16 && s_ok[tid]) { A.last_poi[s_slot[tid]] = s_poi[tid]; A.steps[s_slot[tid]] += 1; }
}

namespace {
template <int G>
hipError_t sc_launch(SessCellArgs& A, int tile, hipStream_t st) {
  if (tile) {
    static DeviceOnce once;      // the LDS opt-in is a per-device attribute of the function
    const hipError_t oe = once.run([&]() -> hipError_t {
      return hipFuncSetAttribute(reinterpret_cast<const void*>(&sc_tile_kernel<G>), hipFuncAttributeMaxDynamicSharedMemorySize, SESS_TILE_LDS_MAX);
    });
    if (oe != hipSuccess) return oe;
    if (G == 0) hipLaunchKernelGGL(sc_rowsum_kernel, dim3(A.n_dist + 1), dim3(256), 0, st, A.wh, A.dim, const_cast<double*>(A.wrs));
    hipLaunchKernelGGL(sc_tile_kernel<G>, dim3((A.n + 15) / 16), dim3(256), sess_cell_tile_lds(G, A.dim), st, A);
  } else {
    hipLaunchKernelGGL(sc_event_kernel<G>, dim3(A.n < SESS_EVENT_GRID_MAX ? A.n : SESS_EVENT_GRID_MAX), dim3(256), sess_cell_event_lds(G, A.dim), st, A);
  }
  return hipGetLastError();
}
}  // namespace

hipError_t launch_session_cells(SessCellArgs& A, int tile, hipStream_t st, Timing* tm) {
  tm->begin(A.G == 0 ? "session_carnn_advance" : "session_cell_advance", st);
  hipError_t e = hipSuccess;
  if (A.owner) e = launch_session_claims(A.slot, A.n, A.n_slot, A.owner, st);
  if (e == hipSuccess) e = A.G == 0 ? sc_launch<0>(A, tile, st) : A.G == 1 ? sc_launch<1>(A, tile, st) : sc_launch<4>(A, tile, st);
  tm->end(st);
  return e;
}

}  // namespace poi
