// Fold-in for the factorisation family (poi_foldin_bpr): a user row for a check-in history the model never trained on.  The item side
// is frozen; the model's own per-check-in SGD rule (public/BPR.py:216-230, and :287-306 for VBPR, whose pair [ux | ue] moves like one
// BPR-MF row against [lt | fi ei^T]) runs on ONE fresh row over the history, `epochs` times:
//
//   d = Y[p_t] - Y[q_{e,t}],  x = w . d,  loss[e] += -log sigmoid(x),  w -= alpha (-sigmoid(-x) d + lambda w)
//
// The problem is a latency chain of epochs x len steps per user; each step is two random row gathers, a reduction and an axpy.  Which
// rows a step gathers does not depend on w, so they are fetched ahead of the chain.
//
// One 16-lane row of a wave = one user, four users per wave, one wave per workgroup.  Lane g of a row owns the columns 4 g + 64 j
// (a float4 of an item row per j, as near.hip scores) and keeps its slice of w in float64 registers (32 VGPRs at dim 256).  A wave walks
// its users' flattened steps s = e len + t in a loop unrolled by the ring depth K; iteration s
//   (a) converts the two rows of step s - issued K steps earlier - to the float64 difference d,
//   (b) issues the 2 NJ row loads of step s + K from the ids that arrived in the meantime,
//   (c) issues the two id loads of step s + 2 K,
//   (d) runs the chain: per-lane fma over its columns in ascending order, four DPP adds inside the 16-lane row, one exp, the axpy.
// So K steps of rows and 2 K steps of ids are in flight while a step computes, and the only wait on the chain is for loads issued K
// steps ago.  The reduction never leaves the lane row, there is no LDS and nothing is shared between users: a user's bits depend on
// its own history, negatives and w0 alone - not on the other users of the call, its position or the grid.  Every lane of a row holds the
// same x (the DPP sum is symmetric), so the sigmoid and the loss are computed redundantly and lane 0 of the row writes the loss.
//
// The loads of the loop are unconditional (a lane without a column or a step past a user's end reads a valid dummy address and a select
// drops the value), so the compiler can count the loads in flight and wait for exactly the ones a step consumes; the kernel is
// instantiated per table element type for the same reason.
// Ids are checked where they are used: an id outside [0, n_item] is replaced by row 0 for the gather and flags the user; a flagged user
// (or one with off[r + 1] < off[r] or off[r] < 0) gets a NaN row and NaN losses and is counted once with one integer atomic.
//
// Bytes per step: two item rows (2 x 4 dim, or 2 x 2 dim from a half table) + 8 B of ids.
#include <type_traits>
#include "poi_common.h"
#include "poi_kernels.h"

namespace poi {

template <int NJ, int K, bool F16>
__global__ __launch_bounds__(64) void foldin_kernel(FoldinArgs A) {
  using elem_t = typename std::conditional<F16, __half, float>::type;
  const elem_t* const Y = reinterpret_cast<const elem_t*>(A.items);
  const int lane = lane_id(), gl = lane & 15;
  const int r = blockIdx.x * FOLDIN_USERS_PER_WAVE + (lane >> 4);
  const bool live = r < A.n;
  const int D = A.dim, NI = A.n_item, E = A.epochs;
  int base = 0, len = 0, bad = 0;
  if (live) {
    base = A.off[r];
    len = A.off[r + 1] - base;
    if (base < 0 || len < 0) { bad = 1; len = 0; base = 0; }
  }
  const long long total = (long long)len * E;           // steps of this user
  long long wave_total = total;
#pragma unroll
  for (int o = 32; o >= 16; o >>= 1) { const long long v = __shfl_xor(wave_total, o, 64); wave_total = v > wave_total ? v : wave_total; }
  wave_total = (long long)__builtin_amdgcn_readfirstlane((int)(wave_total >> 32)) << 32 | (unsigned)__builtin_amdgcn_readfirstlane((int)wave_total);

  // Every load of the loop is unconditional and straight-line (a load under a branch leaves the number of loads in flight unknown and
  // the compiler then waits for all of them): a lane without a column reads column 0 and a step past the end reads row 0 and the
  // offset table instead of ids; selects discard what they return.
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
  const int* pp = A.p + base;
  const int* qq = A.q + base;
  const double alpha = (double)A.alpha, lambda = (double)A.lambda;

  // id cursor: (ti, qi) = position and epoch offset of the next id pair to fetch; ids of step s + K + j wait in idp[j] / idq[j]
  int ti = 0;
  long long qi = 0, si = 0;
  int idp[K], idq[K];
  float4 rp[K][NJ], rq[K][NJ];
  auto fetch_ids = [&](int j) {
    const bool on = si < total;
    idp[j] = *(on ? pp + ti : A.off);
    idq[j] = *(on ? qq + qi + ti : A.off);
    const bool wrap = on && ti + 1 == len;
    ti = wrap ? 0 : ti + (on ? 1 : 0);
    qi += wrap ? A.q_epoch_stride : 0;
    ++si;
  };
  long long sr = 0;                                      // next step whose rows are fetched
  auto fetch_rows = [&](int j) {
    int ip = idp[j], iq = idq[j];
    const bool bp = (unsigned)ip > (unsigned)NI, bq = (unsigned)iq > (unsigned)NI;
    bad |= (sr < total && (bp || bq)) ? 1 : 0;
    ip = bp ? 0 : ip;
    iq = bq ? 0 : iq;
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
      double d[NJ][4];
#pragma unroll
      for (int c = 0; c < NJ; ++c) {
        d[c][0] = col_ok[c] ? (double)rp[j][c].x - (double)rq[j][c].x : 0.0; d[c][1] = col_ok[c] ? (double)rp[j][c].y - (double)rq[j][c].y : 0.0;
        d[c][2] = col_ok[c] ? (double)rp[j][c].z - (double)rq[j][c].z : 0.0; d[c][3] = col_ok[c] ? (double)rp[j][c].w - (double)rq[j][c].w : 0.0;
      }
      fetch_rows(j);
      fetch_ids(j);
      double x = 0.0;
#pragma unroll
      for (int c = 0; c < NJ; ++c)
#pragma unroll
        for (int i = 0; i < 4; ++i) x = fma(w[c][i], d[c][i], x);
      x = row_sum(x);
      // e = exp(-|x|):  sigmoid(-x) = x >= 0 ? e / (1 + e) : 1 / (1 + e),  -log sigmoid(x) = max(-x, 0) + log1p(e)
      const double e = exp(-fabs(x));
      const double sg = (x >= 0.0 ? e : 1.0) / (1.0 + e);
      // a step past the user's end changes nothing (selects, no branch)
      loss += on ? fmax(-x, 0.0) + log1p(e) : 0.0;
#pragma unroll
      for (int c = 0; c < NJ; ++c)
#pragma unroll
        for (int i = 0; i < 4; ++i) w[c][i] = on ? w[c][i] - alpha * (fma(lambda, w[c][i], -sg * d[c][i])) : w[c][i];
      if (on && ++tc == len) {
        if (A.loss_out && gl == 0) A.loss_out[(size_t)r * E + ec] = (float)loss;
        loss = 0.0; tc = 0; ++ec;
      }
    }
  }
  if (!live) return;
  const float nan = __builtin_nanf("");
  if (A.loss_out && (bad || len == 0))
    for (int e = gl; e < E; e += 16) A.loss_out[(size_t)r * E + e] = bad ? nan : 0.f;
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    if (!col_ok[j]) continue;
    const float4 v = bad ? make_float4(nan, nan, nan, nan) : make_float4((float)w[j][0], (float)w[j][1], (float)w[j][2], (float)w[j][3]);
    st4(A.w_out + (size_t)r * D + gl * 4 + 64 * j, v);
  }
  if (bad && gl == 0) atomicAdd(A.bad, 1);
}

hipError_t launch_foldin(const FoldinArgs& A, hipStream_t st, Timing* tm) {
  const dim3 grid((unsigned)((A.n + FOLDIN_USERS_PER_WAVE - 1) / FOLDIN_USERS_PER_WAVE));
  tm->begin("foldin", st);
  const int nj = (A.dim + 63) / 64;
  if (nj < 1 || nj > 4) return hipErrorInvalidValue;
#define FOLDIN_LAUNCH(NJ, K)                                                                                   \
  if (A.items_f16) hipLaunchKernelGGL((foldin_kernel<NJ, K, true>), grid, dim3(64), 0, st, A);                 \
  else hipLaunchKernelGGL((foldin_kernel<NJ, K, false>), grid, dim3(64), 0, st, A)
  switch (nj) {
    case 1: FOLDIN_LAUNCH(1, 4); break;
    case 2: FOLDIN_LAUNCH(2, 4); break;
    case 3: FOLDIN_LAUNCH(3, 2); break;
    default: FOLDIN_LAUNCH(4, 2); break;
  }
#undef FOLDIN_LAUNCH
  tm->end(st);
  return hipGetLastError();
}

}  // namespace poi
