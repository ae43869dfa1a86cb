// Fold-in for POI2Vec (poi_foldin_p2v): a user row for a check-in history the model never trained on.  In Poi2vec.seq_train
// (public/POI2Vec.py:140-163) the geographic factor paths_i depends on wl, pb and the contexts only; with the item side frozen the row
// xu[u] sees the full softmax over all POIs alone:
//
//   cost(w) = logsumexp_j (w . wl_j) - (1/L) sum_i w . wl_{t_i} + (lambda / 2) |w|^2,   j < n_item
//   w <- w - alpha (sum_j plu_j wl_j - tbar + lambda w),   plu = softmax_j (w . wl_j),  tbar = (1/L) sum_i wl_{t_i}      once per epoch
//
// Each epoch is one pass over the whole of wl per user - an attention-shaped product (Q = w, K = V = wl) with an online softmax - and a
// small combine.  Kernels:
//   foldin_p2v_prep   once: checks the user's offsets and ids, tbar in float64 (history order), the float64 running row from w0
//   foldin_p2v_pass   per epoch: a workgroup = 4 waves = 4 tiles of 16 users x one SPAN of P2V_FOLD_SPAN items.  The span is walked in
//                     tiles of 32 items staged in LDS, converted to float64 once for the four user tiles.  Per 16 x 16 block a wave
//                     takes the logits from v_mfma_f64_16x16x4_f64 TRANSPOSED (A = the item tile, B = w^T from registers): the result
//                     layout col = lane & 15, row = (lane >> 4) + 4 reg then gives lane (lk, lr) the items lk + 4 reg of user lr - which
//                     is exactly the A operand (row = user lr, k = lk) of the second product sum_j e_j wl_j, whose k-step s contracts the
//                     items lk + 4 s.  No transposition through LDS sits between the two products.  The running maximum m of a user
//                     is exact (two xor steps over the four lane groups); the accumulators are rescaled only when some user of the
//                     tile raised its maximum, by exp(m_old - m_new) for those users and by an exact 1.0 for the others.
//                     Output per (user, span): m, sum of exp, and the D exp-weighted column sums, float64.
//   foldin_p2v_upd    per epoch: a workgroup per user merges its span partials in span order, writes the loss, applies the update.
// Determinism: no atomics on results; an MFMA output element depends on its own row and column only, padding users carry w = 0 and
// are never written, every other sum runs in one fixed order (the lane's items ascending, the four lane groups by a symmetric xor
// tree, the spans ascending).  So a user's bits depend on its own history and w0 alone - not on the other users, its position, n or
// the grid.
// LDS: a staged row holds DP = 16 ceil(D / 16) doubles at stride RS = DP + 2 (+ 16 if DP is no multiple of 32): RS = 2 mod 32 doubles
// puts the 16 rows x 4 columns a half wave reads for the logits on 64 distinct 4-byte banks.  Columns D .. DP are zero.
#include "poi_common.h"
#include "poi_kernels.h"

namespace poi {

typedef double d4_t __attribute__((ext_vector_type(4)));

constexpr int P2F_IT = 32;                  // items per staged tile
constexpr double P2F_M0 = -1.0e300;         // below every logit of finite float32 operands (|s| <= 128 FLT_MAX^2 < 1.5e79)

__host__ __device__ constexpr int p2f_rs(int NC) { return 16 * NC + ((16 * NC) % 32 == 0 ? 2 : 18); }

__global__ __launch_bounds__(128) void foldin_p2v_prep_kernel(FoldP2vArgs A) {
  const int r = blockIdx.x, d = threadIdx.x, D = A.dim, NI = A.n_item, E = A.epochs;
  int base = A.off[r], len = A.off[r + 1] - base;
  int bad = base < 0 || len < 0;
  if (bad) { base = 0; len = 0; }
  for (int i = 0; i < len; ++i) bad |= (unsigned)A.tgt[base + i] >= (unsigned)NI;      // (every thread reads every id: uniform)
  const float nan = quiet_nan();
  if (d < D) {
    double t = 0.0;
    if (!bad)
      for (int i = 0; i < len; ++i) t += (double)A.wl[(size_t)A.tgt[base + i] * D + d];
    const float w0 = A.w0 ? A.w0[(size_t)r * D + d] : 0.f;
    A.tbar[(size_t)r * D + d] = len > 0 && !bad ? t / (double)len : 0.0;
    A.w[(size_t)r * D + d] = bad ? 0.0 : (double)w0;
    A.w_out[(size_t)r * D + d] = bad ? nan : w0;
  }
  const int skip = bad ? 1 : (len == 0 || E == 0 ? 2 : 0);
  if (skip && A.loss_out)
    for (int e = d; e < E; e += 128) A.loss_out[(size_t)r * E + e] = bad ? nan : 0.f;
  if (d == 0) {
    A.flag[r] = skip;
    if (bad) atomicAdd(A.bad, 1);
  }
}

template <int NC>
__global__ __launch_bounds__(256) void foldin_p2v_pass_kernel(FoldP2vArgs A) {
  constexpr int KK = 4 * NC, RS = p2f_rs(NC);
  extern __shared__ double s_tile[];                      // P2F_IT x RS
  const int lane = lane_id(), lr = lane & 15, lk = lane >> 4;
  const int D = A.dim, d4n = D >> 2;
  const int sp = blockIdx.x, u0 = blockIdx.y * P2V_FOLD_USERS + wave_id() * 16;
  const bool wave_on = u0 < A.n;
  const int j_lo = sp * P2V_FOLD_SPAN, j_hi = min(A.n_item, j_lo + P2V_FOLD_SPAN);

  // B operand of the logits: lane (lk, lr) holds w[u0 + lr][4 kk + lk]; zero for a padding user and for the columns D .. DP
  double wr[KK];
#pragma unroll
  for (int kk = 0; kk < KK; ++kk) {
    const int k = 4 * kk + lk, u = u0 + lr;
    wr[kk] = (u < A.n && k < D) ? A.w[(size_t)u * D + k] : 0.0;
  }
  for (int x = threadIdx.x; x < P2F_IT * RS; x += 256) s_tile[x] = 0.0;

  double m = P2F_M0, l = 0.0;
  d4_t acc[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) acc[c] = d4_t{0.0, 0.0, 0.0, 0.0};

  for (int j0 = j_lo; j0 < j_hi; j0 += P2F_IT) {
    __syncthreads();                                      // the previous tile has been read (first trip: the zero fill is done)
    for (int x = threadIdx.x; x < P2F_IT * d4n; x += 256) {
      const int row = x / d4n, c = (x - row * d4n) * 4, j = j0 + row;
      const float4 v = j < j_hi ? ld4(A.wl + (size_t)j * D + c) : make_float4(0.f, 0.f, 0.f, 0.f);
      double* dst = s_tile + row * RS + c;
      dst[0] = (double)v.x; dst[1] = (double)v.y; dst[2] = (double)v.z; dst[3] = (double)v.w;
    }
    __syncthreads();
    if (!wave_on) continue;
#pragma unroll
    for (int t = 0; t < P2F_IT / 16; ++t) {
      const int jb = j0 + 16 * t;
      if (jb >= j_hi) break;                              // (wave-uniform)
      const double* tp = s_tile + 16 * t * RS;
      // s[reg] = w[u0 + lr] . wl[jb + lk + 4 reg]
      d4_t s = d4_t{0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int kk = 0; kk < KK; ++kk) s = __builtin_amdgcn_mfma_f64_16x16x4f64(tp[lr * RS + 4 * kk + lk], wr[kk], s, 0, 0, 0);
      double tmax = P2F_M0;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        if (jb + lk + 4 * g >= j_hi) s[g] = -__builtin_huge_val();      // an item past the span's end: exp = 0
        tmax = fmax(tmax, s[g]);
      }
      tmax = fmax(tmax, __shfl_xor(tmax, 16, 64));
      tmax = fmax(tmax, __shfl_xor(tmax, 32, 64));
      const double mn = fmax(m, tmax);
      const bool up = mn > m;
      if (__any(up)) {
        const double sc = up ? exp(m - mn) : 1.0;
        l *= sc;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const double f = __shfl(sc, lk + 4 * g, 64);   // the factor of user u0 + lk + 4 g (row of the accumulators)
#pragma unroll
          for (int c = 0; c < NC; ++c) acc[c][g] *= f;
        }
        m = mn;
      }
      double e[4];
#pragma unroll
      for (int g = 0; g < 4; ++g) e[g] = exp(s[g] - m);
      l += (e[0] + e[1]) + (e[2] + e[3]);
      // acc[c][reg] (user u0 + lk + 4 reg, column 16 c + lr) += sum over the tile's items of e . wl; k-step g contracts the items lk + 4 g
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const double* bp = tp + (lk + 4 * g) * RS + lr;
#pragma unroll
        for (int c = 0; c < NC; ++c) acc[c] = __builtin_amdgcn_mfma_f64_16x16x4f64(e[g], bp[16 * c], acc[c], 0, 0, 0);
      }
    }
  }
  if (!wave_on) return;
  l += __shfl_xor(l, 16, 64);
  l += __shfl_xor(l, 32, 64);
  const size_t PS = (size_t)D + 2;
  if (lk == 0 && u0 + lr < A.n) {
    double* o = A.part + ((size_t)(u0 + lr) * A.n_span + sp) * PS;
    o[0] = m; o[1] = l;
  }
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const int u = u0 + lk + 4 * g;
    if (u >= A.n) continue;
    double* o = A.part + ((size_t)u * A.n_span + sp) * PS + 2;
#pragma unroll
    for (int c = 0; c < NC; ++c)
      if (16 * c + lr < D) o[16 * c + lr] = acc[c][g];
  }
}

// The exponentials of the merge do not depend on each other: a thread per span computes exp(m_sp - M) into LDS, then every thread walks the
// spans in order for its own column (plain fmas on loads that do not wait for an exp).
__global__ __launch_bounds__(128) void foldin_p2v_upd_kernel(FoldP2vArgs A) {
  constexpr int FC = 512;                                 // spans per LDS chunk of factors
  __shared__ double s_red[128];
  __shared__ double s_f[FC];
  const int r = blockIdx.x, d = threadIdx.x, D = A.dim;
  if (A.flag[r]) return;                                  // a bad user, an empty history: written by the prep kernel
  const size_t PS = (size_t)D + 2;
  const double* pp = A.part + (size_t)r * A.n_span * PS;
  double M = P2F_M0;
  for (int sp = d; sp < A.n_span; sp += 128) M = fmax(M, pp[sp * PS]);
  s_red[d] = M;
  __syncthreads();
  for (int o = 64; o > 0; o >>= 1) {
    if (d < o) s_red[d] = fmax(s_red[d], s_red[d + o]);
    __syncthreads();
  }
  M = s_red[0];
  __syncthreads();
  double ls = 0.0, g = 0.0;
  for (int c0 = 0; c0 < A.n_span; c0 += FC) {
    const int nc = min(FC, A.n_span - c0);
    for (int i = d; i < nc; i += 128) s_f[i] = exp(pp[(c0 + i) * PS] - M);
    __syncthreads();
    for (int i = 0; i < nc; ++i) {                        // span order
      const double f = s_f[i];
      ls = fma(pp[(c0 + i) * PS + 1], f, ls);
      if (d < D) g = fma(pp[(c0 + i) * PS + 2 + d], f, g);
    }
    __syncthreads();
  }
  const double wv = d < D ? A.w[(size_t)r * D + d] : 0.0, tb = d < D ? A.tbar[(size_t)r * D + d] : 0.0;
  s_red[d] = wv * tb;
  __syncthreads();
  if (d == 0 && A.loss_out) {
    double dot = 0.0;
    for (int k = 0; k < D; ++k) dot += s_red[k];          // column order
    A.loss_out[(size_t)r * A.epochs + A.epoch] = (float)((M + log(ls)) - dot);
  }
  if (d < D) {
    const double wn = wv - (double)A.alpha * ((g / ls - tb) + (double)A.lambda * wv);
    A.w[(size_t)r * D + d] = wn;
    if (A.epoch == A.epochs - 1) A.w_out[(size_t)r * D + d] = (float)wn;
  }
}

size_t foldin_p2v_lds(int dim) { return sizeof(double) * P2F_IT * (size_t)p2f_rs((dim + 15) / 16); }

hipError_t launch_foldin_p2v(FoldP2vArgs& A, hipStream_t st, Timing* tm) {
  const int nc = (A.dim + 15) / 16;
  if (nc < 1 || nc > 8 || A.n_span != (A.n_item + P2V_FOLD_SPAN - 1) / P2V_FOLD_SPAN) return hipErrorInvalidValue;
  tm->begin("foldin_p2v_prep", st);
  hipLaunchKernelGGL(foldin_p2v_prep_kernel, dim3((unsigned)A.n), dim3(128), 0, st, A);
  tm->end(st);
  const dim3 grid((unsigned)A.n_span, (unsigned)((A.n + P2V_FOLD_USERS - 1) / P2V_FOLD_USERS));
  const size_t lds = foldin_p2v_lds(A.dim);
  for (int e = 0; e < A.epochs; ++e) {
    A.epoch = e;
    tm->begin("foldin_p2v_pass", st);
    switch (nc) {
#define P2F_LAUNCH(NC) case NC: hipLaunchKernelGGL(foldin_p2v_pass_kernel<NC>, grid, dim3(256), lds, st, A); break
      P2F_LAUNCH(1); P2F_LAUNCH(2); P2F_LAUNCH(3); P2F_LAUNCH(4); P2F_LAUNCH(5); P2F_LAUNCH(6); P2F_LAUNCH(7); P2F_LAUNCH(8);
#undef P2F_LAUNCH
    }
    tm->end(st);
    tm->begin("foldin_p2v_upd", st);
    hipLaunchKernelGGL(foldin_p2v_upd_kernel, dim3((unsigned)A.n), dim3(128), 0, st, A);
    tm->end(st);
  }
  return hipGetLastError();
}

}  // namespace poi
