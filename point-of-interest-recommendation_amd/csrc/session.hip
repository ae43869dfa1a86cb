// Online sessions (poi_session_advance / poi_session_sts): per-slot recurrent state of the GRU family kept on the device and advanced
// ONE check-in at a time - the cell step of seq_predict (public/GRU_Spatial.py:231-288, public/GRU.py:154-202) on the evaluation
// snapshots, for a batch of (slot, POI) events.
//
// State of slot s: h[s] (D float64 - one rounding less per step than a float32 state, 8 D bytes per user), sts[s] (n_dist + 1 float32,
// spatial only), last_poi[s] (-1: none yet), steps[s].  Tables are float32 (the POI snapshot may be IEEE half); every product, gate sum
// and the softmax are float64.  No atomics on results: an event owns its slot row, sums run in a fixed order - identical calls give
// bitwise identical state.
//
// Two launch regimes (DESIGN.md "Sessions"):
//   event path  one workgroup per event: rows of ui / wh / vs streamed from L2, a wave per output row, float64 wave reductions.  Latency
//               bound - the regime of live traffic.
//   tile path   16 events per workgroup on the float64 matrix cores (v_mfma_f64_16x16x4_f64, as te_rec_fwdd): weights = A operand (16
//               units x 4 k, one float4 per lane and k-block of 16), gathered rows [x | h] and r * h = B operand, k-major in LDS.  The
//               candidate gate's wh[2] . (r * h) needs r, so a wave owns z, r and c of its unit tiles and both products sit in one kernel.
//               MFMA j of k-block kq contracts k = 16 kq + 4 g + j (g = lane >> 4: the lane's float4 of weights); the LDS rows are stored
//               at swz(k) = 16 kq + 4 j + g so that the four lane groups of a B fragment read four consecutive rows.
//
// A slot >= n_slot or a POI outside [0, n_item) leaves the slot untouched, gives NaN rows in the optional outputs and is counted
// (poi_ctx_take_bad_ids).  A slot named by more than one event of a call is REFUSED the same way, every event of it: the caller splits
// such a batch into successive calls (models.Session.advance does).
#include "poi_common.h"
#include "poi_kernels.h"
#include "session_common.h"

namespace poi {

namespace {

// softmax(vs . hs + bs) of one event by the whole workgroup: float32 rows to st (state, may be null) and out (may be null)
__device__ __forceinline__ void event_head(const SessArgs& A, const double* hs, double* lg, double* red, float* st, float* out) {
  const int D = A.dim, NB = A.n_dist + 1, lane = lane_id(), w = wave_id(), tid = threadIdx.x;
  for (int b0 = w * 4; b0 < NB; b0 += 16) {
    double acc[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) acc[u] = b0 + u < NB ? row_part(A.vs + (size_t)(b0 + u) * D, D, hs, lane) : 0.0;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const double s = wave_sum_d(acc[u]);
      if (lane == 0 && b0 + u < NB) lg[b0 + u] = s + (double)A.bs[b0 + u];
    }
  }
  __syncthreads();
  double m = -1.0e300;
  for (int b = tid; b < NB; b += 256) m = fmax(m, lg[b]);
  m = block_max_d(m, red);
  double s = 0.0;
  for (int b = tid; b < NB; b += 256) s += exp(lg[b] - m);
  s = block_sum_d(s, red);
  for (int b = tid; b < NB; b += 256) {
    const float v = (float)(exp(lg[b] - m) / s);
    if (st) st[b] = v;
    if (out) out[b] = v;
  }
}

}  // namespace

// ---- duplicate slots of a call (launches too large for the in-kernel scan): the last writer owns a slot, every other event of that
// slot then voids the claim - no event of a repeated slot finds its own index there
__global__ __launch_bounds__(256) void sess_claim_kernel(SessArgs A) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= A.n) return;
  const int s = A.slot[e];
  if ((unsigned)s < (unsigned)A.n_slot) A.owner[s] = e;
}
__global__ __launch_bounds__(256) void sess_mark_kernel(SessArgs A) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= A.n) return;
  const int s = A.slot[e];
  if ((unsigned)s < (unsigned)A.n_slot && A.owner[s] != e) A.owner[s] = -1;
}

// ---- event path: one workgroup per event (head_only: softmax(vs . h[slot] + bs) into sts_out, nothing else) -------------------------
__global__ __launch_bounds__(256) void sess_event_kernel(SessArgs A) {
  extern __shared__ __align__(16) unsigned char sess_sm[];
  const int D = A.dim, xw = A.xw, NB = A.n_dist + 1, tid = threadIdx.x, lane = lane_id(), w = wave_id();
  double* xs = reinterpret_cast<double*>(sess_sm);      // [xw]
  double* hs = xs + xw;                                  // [D]
  double* rh = hs + D;                                   // [D]
  double* zs = rh + D;                                   // [D]
  double* lg = zs + D;                                   // [NB]
  double* red = lg + (A.spatial ? NB : 0);               // [4]
  for (int e = blockIdx.x; e < A.n; e += gridDim.x) {
    const int s = A.slot[e], j = A.head_only ? 0 : A.poi[e];
    int bad = (unsigned)s >= (unsigned)A.n_slot || (unsigned)j >= (unsigned)A.n_item;
    if (!bad && !A.head_only) {
      if (A.owner) bad = A.owner[s] != e;
      else for (int o = tid; o < A.n; o += 256) bad |= o != e && A.slot[o] == s;
    }
    if (__syncthreads_or(bad)) {
      if (tid == 0) atomicAdd(A.bad, 1);
      if (A.hts_out) for (int u = tid; u < D; u += 256) A.hts_out[(size_t)e * D + u] = quiet_nan();
      if (A.sts_out && A.spatial) for (int b = tid; b < NB; b += 256) A.sts_out[(size_t)e * NB + b] = quiet_nan();
      continue;
    }
    double* hrow = A.h + (size_t)s * D;
    for (int u = tid; u < D; u += 256) hs[u] = hrow[u];
    if (A.head_only) {
      __syncthreads();
      event_head(A, hs, lg, red, nullptr, A.sts_out + (size_t)e * NB);
      __syncthreads();
      continue;
    }
    int d = A.n_dist;
    if (A.spatial) { const int lp = A.last_poi[s]; if (lp >= 0) d = pos_bin(A, j, lp); }
    for (int u = tid; u < D; u += 256) {
      xs[u] = (double)ld_tab(A.lt, (size_t)j * D + u, A.lt_f16);
      if (A.spatial) xs[D + u] = (double)A.di[(size_t)d * D + u];
    }
    __syncthreads();
    // z, r: rows 0 .. 2 D - 1 of ui / wh, four rows of a wave in flight
    for (int o0 = w * 4; o0 < 2 * D; o0 += 16) {
      double acc[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) acc[u] = row_part(A.ui + (size_t)(o0 + u) * xw, xw, xs, lane) + row_part(A.wh + (size_t)(o0 + u) * D, D, hs, lane);
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const double a = wave_sum_d(acc[u]);
        const int o = o0 + u;
        if (lane == 0) {
          const double v = sigmoid_d(a + (double)A.bi[o]);
          if (o < D) zs[o] = v; else rh[o - D] = v * hs[o - D];
        }
      }
    }
    __syncthreads();
    // c and the new state: hs[u] is read and written by the lane that owns row u only
    for (int o0 = w * 4; o0 < D; o0 += 16) {
      double acc[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) acc[u] = row_part(A.ui + (size_t)(2 * D + o0 + u) * xw, xw, xs, lane) + row_part(A.wh + (size_t)(2 * D + o0 + u) * D, D, rh, lane);
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const double a = wave_sum_d(acc[u]);
        const int o = o0 + u;
        if (lane == 0) {
          const double c = tanh(a + (double)A.bi[2 * D + o]), z = zs[o], hp = hs[o];
          hs[o] = (1.0 - z) * hp + z * c;
        }
      }
    }
    __syncthreads();
    for (int u = tid; u < D; u += 256) {
      hrow[u] = hs[u];
      if (A.hts_out) A.hts_out[(size_t)e * D + u] = (float)hs[u];
    }
    if (tid == 0) { A.last_poi[s] = j; A.steps[s] += 1; }
    if (A.spatial) event_head(A, hs, lg, red, A.sts + (size_t)s * NB, A.sts_out ? A.sts_out + (size_t)e * NB : nullptr);
    __syncthreads();
  }
}

// ---- tile path: 16 events per workgroup, float64 MFMA (sess_mma and the gate expressions: session_common.h) ---------------------------
size_t sess_tile_lds(int D, int xw, int NB, int spatial) {
  size_t r0 = sizeof(float) * RS * (size_t)xw;
  if (spatial && sizeof(double) * RS * (size_t)NB > r0) r0 = sizeof(double) * RS * (size_t)NB;
  r0 = (r0 + 15) & ~(size_t)15;
  return r0 + sizeof(double) * 2 * RS * (size_t)D;
}

__global__ __launch_bounds__(256) void sess_tile_kernel(SessArgs A, int r0_bytes) {
  extern __shared__ __align__(16) unsigned char sess_sm[];
  const int D = A.dim, xw = A.xw, NB = A.n_dist + 1, NT = D >> 4;
  float* xT = reinterpret_cast<float*>(sess_sm);         // [xw][RS] float32: table values are exact in it
  double* lg = reinterpret_cast<double*>(sess_sm);       // [NB][RS] logits: reuses xT once the gates are done
  double* hT = reinterpret_cast<double*>(sess_sm + r0_bytes);      // [D][RS]
  double* rhT = hT + (size_t)D * RS;                     // [D][RS]
  __shared__ int s_slot[16], s_poi[16], s_d[16], s_ok[16];
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
        if (A.spatial) { const int lp = A.last_poi[s]; if (lp >= 0) d = pos_bin(A, j, lp); }
      }
    }
    s_slot[tid] = s; s_poi[tid] = j; s_d[tid] = d; s_ok[tid] = ok;
  }
  __syncthreads();
  for (int idx = tid; idx < 16 * D; idx += 256) {
    const int e = idx / D, u = idx - e * D, ok = s_ok[e], su = swz(u);
    xT[su * RS + e] = ok ? ld_tab(A.lt, (size_t)s_poi[e] * D + u, A.lt_f16) : 0.f;
    if (A.spatial) xT[(D + su) * RS + e] = ok ? A.di[(size_t)s_d[e] * D + u] : 0.f;
    hT[su * RS + e] = ok ? A.h[(size_t)s_slot[e] * D + u] : 0.0;
  }
  __syncthreads();
  // wave w owns the unit tiles w, w + 4, ... (D <= 256: at most four) of z, r and c; C layout of the f64 MFMA: register r of lane (i, g) =
  // unit 16 ut + g + 4 r of event i
  double zr[4][4];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int ut = w + 4 * t;
    if (ut < NT) {
      const int row = 16 * ut + i;
      f64x4 acc[2] = {f64x4{0.0, 0.0, 0.0, 0.0}, f64x4{0.0, 0.0, 0.0, 0.0}};
      const float* const wu[2] = {A.ui + (size_t)row * xw + 4 * g, A.ui + (size_t)(D + row) * xw + 4 * g};
      sess_mma<2>(acc, wu, xw, xT, i, g);
      const float* const ww[2] = {A.wh + (size_t)row * D + 4 * g, A.wh + (size_t)(D + row) * D + 4 * g};
      sess_mma<2>(acc, ww, D, hT, i, g);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int unit = 16 * ut + g + 4 * r, at = swz(unit) * RS + i;
        zr[t][r] = sigmoid_d(acc[0][r] + (double)A.bi[unit]);
        rhT[at] = sigmoid_d(acc[1][r] + (double)A.bi[D + unit]) * hT[at];
      }
    }
  }
  __syncthreads();
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int ut = w + 4 * t;
    if (ut < NT) {
      const int row = 2 * D + 16 * ut + i;
      f64x4 acc[1] = {f64x4{0.0, 0.0, 0.0, 0.0}};
      const float* const wu[1] = {A.ui + (size_t)row * xw + 4 * g};
      sess_mma<1>(acc, wu, xw, xT, i, g);
      const float* const ww[1] = {A.wh + (size_t)row * D + 4 * g};
      sess_mma<1>(acc, ww, D, rhT, i, g);
#pragma unroll
      for (int r = 0; r < 4; ++r) {      // hT[unit] of event i: read and written by this lane only (the products above read xT and rhT)
        const int unit = 16 * ut + g + 4 * r, at = swz(unit) * RS + i;
        const double c = tanh(acc[0][r] + (double)A.bi[2 * D + unit]), z = zr[t][r], hp = hT[at];
        hT[at] = (1.0 - z) * hp + z * c;
      }
    }
  }
  __syncthreads();
  for (int idx = tid; idx < 16 * D; idx += 256) {
    const int e = idx / D, u = idx - e * D;
    if (e0 + e >= A.n) break;
    const double v = hT[swz(u) * RS + e];
    if (s_ok[e]) A.h[(size_t)s_slot[e] * D + u] = v;
    if (A.hts_out) A.hts_out[(size_t)(e0 + e) * D + u] = s_ok[e] ? (float)v : quiet_nan();
  }
  if (tid < 16 && s_ok[tid]) { A.last_poi[s_slot[tid]] = s_poi[tid]; A.steps[s_slot[tid]] += 1; }
  if (!A.spatial) return;
  // head: logits (NB x 16 events) = vs . h + bs on the matrix cores, then a softmax per event on 16 lanes
  for (int bt = w; bt < ((NB + 15) >> 4); bt += 4) {
    const int rowb = min(16 * bt + i, NB - 1);
    f64x4 acc[1] = {f64x4{0.0, 0.0, 0.0, 0.0}};
    const float* const wv[1] = {A.vs + (size_t)rowb * D + 4 * g};
    sess_mma<1>(acc, wv, D, hT, i, g);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int b = 16 * bt + g + 4 * r;
      if (b < NB) lg[b * RS + i] = acc[0][r] + (double)A.bs[b];
    }
  }
  __syncthreads();
  {
    const int e = tid >> 4, q = tid & 15;
    double m = -1.0e300, s = 0.0;
    for (int b = q; b < NB; b += 16) m = fmax(m, lg[b * RS + e]);
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) m = fmax(m, __shfl_xor(m, o, 64));
    for (int b = q; b < NB; b += 16) s += exp(lg[b * RS + e] - m);
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (e0 + e < A.n) {
      const int ok = s_ok[e];
      float* st = ok ? A.sts + (size_t)s_slot[e] * NB : nullptr;
      float* out = A.sts_out ? A.sts_out + (size_t)(e0 + e) * NB : nullptr;
      for (int b = q; b < NB; b += 16) {
        const float v = ok ? (float)(exp(lg[b * RS + e] - m) / s) : quiet_nan();
        if (st) st[b] = v;
        if (out) out[b] = v;
      }
    }
  }
}

size_t sess_event_lds(int D, int xw, int NB, int spatial) { return sizeof(double) * ((size_t)xw + 3 * (size_t)D + (spatial ? NB : 0) + 4); }

bool sess_tile_supported(int D, int xw, int NB, int spatial) {
  return D >= 16 && D % 16 == 0 && D <= 256 && sess_tile_lds(D, xw, NB, spatial) <= SESS_TILE_LDS_MAX;
}

hipError_t launch_session_claims(const int* slot, int n, int n_slot, int* owner, hipStream_t st) {
  SessArgs A = SessArgs{};
  A.slot = slot; A.n = n; A.n_slot = n_slot; A.owner = owner;
  hipLaunchKernelGGL(sess_claim_kernel, dim3((n + 255) / 256), dim3(256), 0, st, A);
  hipLaunchKernelGGL(sess_mark_kernel, dim3((n + 255) / 256), dim3(256), 0, st, A);
  return hipGetLastError();
}

hipError_t launch_session(SessArgs& A, int tile, hipStream_t st, Timing* tm) {
  const int NB = A.n_dist + 1;
  tm->begin(A.head_only ? "session_sts" : "session_advance", st);
  if (A.owner) {
    hipLaunchKernelGGL(sess_claim_kernel, dim3((A.n + 255) / 256), dim3(256), 0, st, A);
    hipLaunchKernelGGL(sess_mark_kernel, dim3((A.n + 255) / 256), dim3(256), 0, st, A);
  }
  if (tile) {
    static DeviceOnce once;      // the LDS opt-in is a per-device attribute of the function
    const hipError_t oe = once.run([&]() -> hipError_t {
      return hipFuncSetAttribute(reinterpret_cast<const void*>(&sess_tile_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, SESS_TILE_LDS_MAX);
    });
    if (oe != hipSuccess) return oe;
    const size_t lds = sess_tile_lds(A.dim, A.xw, NB, A.spatial);
    hipLaunchKernelGGL(sess_tile_kernel, dim3((A.n + 15) / 16), dim3(256), lds, st, A, (int)(lds - sizeof(double) * 2 * RS * (size_t)A.dim));
  } else {
    hipLaunchKernelGGL(sess_event_kernel, dim3(A.n < SESS_EVENT_GRID_MAX ? A.n : SESS_EVENT_GRID_MAX), dim3(256),
                       sess_event_lds(A.dim, A.xw, NB, A.spatial), st, A);
  }
  tm->end(st);
  return hipGetLastError();
}

}  // namespace poi
