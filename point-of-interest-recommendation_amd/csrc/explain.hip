// Leave-one-out attribution (poi_explain_loo, include/poi_hip.h): which past check-ins drove a recommendation.  For a row with history
// p[0 .. L) a VARIANT is the history with the positions of one group removed (a group: one check-in, or every visit of one POI); its
// state is what a fresh session slot holds after advancing through the kept positions - the step after a removed check-in is binned
// against the last KEPT POI.  delta[g][c] = score(whole history, j_c) - score(variant g, j_c), everything in float64.
//
// One persistent tile kernel.  A COLUMN is a (row, key, start) triple; a workgroup owns 16 of them - of any rows - and loops over steps
// until its longest column is through.  The state hT stays in LDS for the whole walk; per step the cell of session.hip's tile kernel
// runs on the float64 matrix cores (sess_mma), and a column that is finished or whose current position belongs to its removed group
// holds: its update is masked, every barrier is reached by every thread.  The table rows of step t + 1 do not depend on the state:
// their loads are issued before the gate chain of step t and land in the other xT buffer behind it; the ids and bins of step t + 2 are
// worked out by the 16 column threads meanwhile (three index slots).  After the last step: the head (spatial), the C <= 32 float64
// dot products per column, base or delta, optionally the variant's state.
//
// Two launches of that kernel.  The BASE pass walks the whole histories (key -1), writes base and keeps h after every 16th position
// in the context's workspace; the WALK starts a variant whose group first occurs at position f from the checkpoint 16 floor(f / 16)
// (option "explain_start" 0: from h = 0 at position 0).  Columns of an MFMA are independent and every sum has one fixed order, so
// the bits of a column do not depend on its tile, its neighbours, the grid or the start mode.
//
// A row with a history POI outside [0, n_item), a listed id outside [-1, n_item) or offsets outside the id array is counted once
// (poi_ctx_take_bad_ids) and gives NaN in base, in its deltas and in its states; nothing of it is gathered.
#include "poi_common.h"
#include "poi_kernels.h"
#include "session_common.h"

#include <limits.h>

namespace poi {

namespace {
// the two gate expressions of sess_tile_kernel, copied: as shared inline functions they left session.hip's results alone but not its
// instruction stream (other registers, another schedule), so that kernel keeps its own text
__device__ __forceinline__ double gru_gate(double a, float b) { return sigmoid_d(a + (double)b); }
__device__ __forceinline__ double gru_blend(double a, float b, double z, double hp) {
  const double c = tanh(a + (double)b);
  return (1.0 - z) * hp + z * c;
}
}  // namespace

// ---- rows: ids in range? -------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void explain_check_kernel(ExplainArgs A) {
  const int tid = threadIdx.x;
  for (int r = blockIdx.x; r < A.n; r += gridDim.x) {
    const int o0 = A.h_off[r], o1 = A.h_off[r + 1];
    int bad = o0 < 0 || o1 < o0 || (long long)o1 > A.total;
    if (!bad) for (int t = o0 + tid; t < o1; t += 256) bad |= (unsigned)A.h_ids[t] >= (unsigned)A.n_item;
    for (int c = tid; c < A.C; c += 256) { const int j = A.lists[(size_t)r * A.C + c]; bad |= j < -1 || j >= A.n_item; }
    bad = __syncthreads_or(bad);
    if (tid == 0) { A.rowbad[r] = bad; if (bad) atomicAdd(A.bad, 1); }
  }
}

size_t explain_lds(int D, int xw, int NB, int spatial, int* xbytes, int* r0_bytes) {
  const size_t xb = (sizeof(float) * RS * (size_t)xw + 15) & ~(size_t)15;
  size_t r0 = 2 * xb;
  if (spatial && sizeof(double) * RS * (size_t)NB > r0) r0 = sizeof(double) * RS * (size_t)NB;
  r0 = (r0 + 15) & ~(size_t)15;
  if (xbytes) *xbytes = (int)xb;
  if (r0_bytes) *r0_bytes = r0 > (size_t)INT_MAX ? INT_MAX : (int)r0;
  return r0 + sizeof(double) * 2 * RS * (size_t)D;
}

bool explain_supported(int D, int xw, int NB, int spatial) {
  return sess_tile_supported(D, xw, NB, spatial) && explain_lds(D, xw, NB, spatial, nullptr, nullptr) <= SESS_TILE_LDS_MAX;
}

// ---- the walk ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void explain_tile_kernel(ExplainArgs A, int base_pass, int xbytes, int r0_bytes) {
  extern __shared__ __align__(16) unsigned char ex_sm[];
  const int D = A.dim, xw = A.xw, NB = A.n_dist + 1, NT = D >> 4;
  float* const xbuf[2] = {reinterpret_cast<float*>(ex_sm), reinterpret_cast<float*>(ex_sm + xbytes)};      // [xw][RS] each
  double* lg = reinterpret_cast<double*>(ex_sm);         // [NB][RS] logits: reuses both xT buffers once the walk is done
  double* hT = reinterpret_cast<double*>(ex_sm + r0_bytes);        // [D][RS]
  double* rhT = hT + (size_t)D * RS;                     // [D][RS]
  __shared__ int s_row[16], s_out[16], s_len[16], s_ck[16], s_rem[16], s_nan[16], s_last[16];
  __shared__ int s_poi[3][16], s_d[3][16], s_upd[3][16];
  const int tid = threadIdx.x, lane = lane_id(), w = wave_id(), i0 = lane & 15, g = lane >> 4;
  const int ce = tid >> 4, cq = tid & 15;                // the copies and the scores: thread (column ce, part cq)
  // column thread tid < 16: the cursor of column tid lives in its registers
  int key = -1, pos = 0, end = 0, last = -1;
  if (tid < 16) {
    const int c = blockIdx.x * 16 + tid, ncol = base_pass ? A.n : A.n_var;
    int row = 0, out = -1, len = 0, ck = -1, nan = 0;
    if (c < ncol) {
      const int4 q = reinterpret_cast<const int4*>(base_pass ? A.base_cols : A.var_cols)[c];
      const int start = base_pass || !A.start_mode ? 0 : q.z;
      if ((unsigned)q.x < (unsigned)A.n) {
        const int g0 = A.g_off[q.x], ng = A.g_off[q.x + 1] - g0;
        bool ok = base_pass ? true : q.y >= 0 && q.y < ng && g0 >= 0 && (long long)g0 + q.y < A.n_group;
        if (ok && A.rowbad[q.x]) { row = q.x; out = base_pass ? q.x : g0 + q.y; nan = 1; ok = false; }
        if (ok) {
          const int o0 = A.h_off[q.x];
          len = A.h_off[q.x + 1] - o0;
          ok = start >= 0 && (start & 15) == 0 && (start == 0 || (start < len && (start >> 4) - 1 < A.nck));
          if (ok) {
            row = q.x; key = base_pass ? -1 : q.y; out = base_pass ? q.x : g0 + q.y;
            pos = o0 + start; end = o0 + len;
            if (start > 0) { last = A.h_ids[pos - 1]; ck = (start >> 4) - 1; }
          } else len = 0;
        }
      }
    }
    s_row[tid] = row; s_out[tid] = out; s_len[tid] = len; s_ck[tid] = ck; s_rem[tid] = end - pos; s_nan[tid] = nan;
  }
  // ids and bin of this column's next position into index slot `slot`; a removed or finished position holds
  auto plan = [&](int slot) {
    int upd = 0, j = 0, d = A.n_dist;
    if (pos < end) {
      const int cur = A.h_ids[pos];
      if (!(key >= 0 && A.grp[pos] == key)) {
        upd = 1; j = cur;
        if (A.spatial && last >= 0) d = pos_bin(A, cur, last);
        last = cur;
      }
      ++pos;
    }
    s_poi[slot][tid] = j; s_d[slot][tid] = d; s_upd[slot][tid] = upd;
  };
  if (tid < 16) { plan(0); plan(1); }
  __syncthreads();
  int nstep = 0;
#pragma unroll
  for (int e = 0; e < 16; ++e) nstep = max(nstep, s_rem[e]);
  // thread (ce, cq) moves the elements u = cq + 16 k of column ce: state in, table rows in, checkpoints and states out
  float xr[16], dr[16];
  auto fetch = [&](int slot) {
    const int upd = s_upd[slot][ce];
    const size_t jo = (size_t)s_poi[slot][ce] * D, bo = (size_t)s_d[slot][ce] * D;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      if (k < NT) {
        const int u = cq + 16 * k;
        xr[k] = upd ? ld_tab(A.lt, jo + u, A.lt_f16) : 0.f;
        if (A.spatial) dr[k] = upd ? A.di[bo + u] : 0.f;
      }
    }
  };
  auto stash = [&](float* xT) {
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      if (k < NT) {
        const int su = swz(cq + 16 * k);
        xT[su * RS + ce] = xr[k];
        if (A.spatial) xT[(D + su) * RS + ce] = dr[k];
      }
    }
  };
  {
    const int ck = s_ck[ce];
    const double* src = ck >= 0 ? A.ck + ((size_t)s_row[ce] * A.nck + ck) * D : nullptr;
    for (int k = 0; k < NT; ++k) { const int u = cq + 16 * k; hT[swz(u) * RS + ce] = src ? src[u] : 0.0; }
  }
  if (nstep > 0) { fetch(0); stash(xbuf[0]); }
  __syncthreads();
  for (int t = 0; t < nstep; ++t) {
    const float* xT = xbuf[t & 1];
    const int s0 = t % 3, s1 = (t + 1) % 3, s2 = (t + 2) % 3;
    // the lane's column through an empty asm once per step: with a column the compiler can see, every weight-row and LDS address of
    // a step's twelve products is loop-invariant and stays in registers across the walk (347 registers against 306 with this line)
    int i = i0;
    asm volatile("" : "+v"(i));
    if (t + 1 < nstep) fetch(s1);                        // in flight behind the gates; used by stash() below
    if (tid < 16) plan(s2);
    // wave w owns the unit tiles w, w + 4, ... of z, r and c (the layout of sess_tile_kernel)
    double zr[4][4];
#pragma unroll
    for (int tt = 0; tt < 4; ++tt) {
      const int ut = w + 4 * tt;
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
          zr[tt][r] = gru_gate(acc[0][r], A.bi[unit]);
          rhT[at] = gru_gate(acc[1][r], A.bi[D + unit]) * hT[at];
        }
      }
    }
    __syncthreads();
    const int upd = s_upd[s0][i];
#pragma unroll
    for (int tt = 0; tt < 4; ++tt) {
      const int ut = w + 4 * tt;
      if (ut < NT) {
        const int row = 2 * D + 16 * ut + i;
        f64x4 acc[1] = {f64x4{0.0, 0.0, 0.0, 0.0}};
        const float* const wu[1] = {A.ui + (size_t)row * xw + 4 * g};
        sess_mma<1>(acc, wu, xw, xT, i, g);
        const float* const ww[1] = {A.wh + (size_t)row * D + 4 * g};
        sess_mma<1>(acc, ww, D, rhT, i, g);
#pragma unroll
        for (int r = 0; r < 4; ++r) {      // hT[unit] of column i: read and written by this lane only
          const int unit = 16 * ut + g + 4 * r, at = swz(unit) * RS + i;
          const double hp = hT[at], hn = gru_blend(acc[0][r], A.bi[2 * D + unit], zr[tt][r], hp);
          hT[at] = upd ? hn : hp;
        }
      }
    }
    if (t + 1 < nstep) stash(xbuf[(t + 1) & 1]);         // last read in step t - 1, a barrier ago
    __syncthreads();
    if (base_pass && ((t + 1) & 15) == 0) {              // h after position t: where the variants that first differ in [t + 1, t + 17) start
      const int ck = ((t + 1) >> 4) - 1;
      if (t + 1 < s_len[ce] && ck < A.nck) {
        double* dst = A.ck + ((size_t)s_row[ce] * A.nck + ck) * D;
        for (int k = 0; k < NT; ++k) { const int u = cq + 16 * k; dst[u] = hT[swz(u) * RS + ce]; }
      }
    }
  }
  if (tid < 16) s_last[tid] = last;
  // head: logits (NB x 16 columns) = vs . h + bs on the matrix cores (sess_tile_kernel's), the softmax's max and sum per column
  const int i = i0;
  double m = -1.0e300, s = 1.0;
  if (A.spatial) {
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
    s = 0.0;
    for (int b = cq; b < NB; b += 16) m = fmax(m, lg[b * RS + ce]);
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) m = fmax(m, __shfl_xor(m, o, 64));
    for (int b = cq; b < NB; b += 16) s += exp(lg[b * RS + ce] - m);
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  } else {
    __syncthreads();
  }
  const int out = s_out[ce];
  if (out < 0) return;
  const int row = s_row[ce], nan = s_nan[ce], lp = s_last[ce];
  const double wd = A.spatial ? (double)A.wd[0] : 0.0;
  for (int c = cq; c < A.C; c += 16) {
    const int j = A.lists[(size_t)row * A.C + c];
    double sc = quiet_nan();
    if (!nan && j >= 0) {
      double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
      for (int u = 0; u < D; u += 4) {
        const float4 v = ld4t(A.lt, (size_t)j * D + u, A.lt_f16);
        a0 = fma((double)v.x, hT[swz(u) * RS + ce], a0); a1 = fma((double)v.y, hT[swz(u + 1) * RS + ce], a1);
        a2 = fma((double)v.z, hT[swz(u + 2) * RS + ce], a2); a3 = fma((double)v.w, hT[swz(u + 3) * RS + ce], a3);
      }
      sc = (a0 + a1) + (a2 + a3);
      if (A.spatial && lp >= 0) {
        const int b = pos_bin(A, j, lp);
        if (b < A.n_dist) sc += wd * (exp(lg[b * RS + ce] - m) / s);
      }
    }
    if (base_pass) A.base[(size_t)row * A.C + c] = sc;
    else A.delta[(size_t)out * A.C + c] = A.base[(size_t)row * A.C + c] - sc;
  }
  if (base_pass) return;
  if (A.h_out) for (int k = 0; k < NT; ++k) { const int u = cq + 16 * k; A.h_out[(size_t)out * D + u] = nan ? quiet_nan() : hT[swz(u) * RS + ce]; }
  if (A.sts_out && A.spatial) for (int b = cq; b < NB; b += 16) A.sts_out[(size_t)out * NB + b] = nan ? quiet_nan() : exp(lg[b * RS + ce] - m) / s;
  if (A.last_out && cq == 0) A.last_out[out] = nan ? -1 : lp;
}

hipError_t launch_explain(ExplainArgs& A, hipStream_t st, Timing* tm) {
  static DeviceOnce once;      // the LDS opt-in is a per-device attribute of the function
  const hipError_t oe = once.run([&]() -> hipError_t {
    return hipFuncSetAttribute(reinterpret_cast<const void*>(&explain_tile_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, SESS_TILE_LDS_MAX);
  });
  if (oe != hipSuccess) return oe;
  int xbytes = 0, r0 = 0;
  const size_t lds = explain_lds(A.dim, A.xw, A.n_dist + 1, A.spatial, &xbytes, &r0);
  tm->begin("explain_base", st);
  hipLaunchKernelGGL(explain_check_kernel, dim3(A.n < 4096 ? A.n : 4096), dim3(256), 0, st, A);
  hipLaunchKernelGGL(explain_tile_kernel, dim3((A.n + 15) / 16), dim3(256), lds, st, A, 1, xbytes, r0);
  tm->end(st);
  if (A.n_var > 0) {
    tm->begin("explain_walk", st);
    hipLaunchKernelGGL(explain_tile_kernel, dim3((A.n_var + 15) / 16), dim3(256), lds, st, A, 0, xbytes, r0);
    tm->end(st);
  }
  return hipGetLastError();
}

}  // namespace poi
