// FPMC-LR (prog_fpmc_lr.py, public/FPMC_LR.py, public/Load_Data_fpmc_lr.py): neighbour sets, neighbour-restricted negatives and the
// batched SGD step.
//
// Neighbour sets (fun_acquire_neighbors_for_each_poi, Load_Data_fpmc_lr.py:114-143): neighbours(i) = {k != i : cal_dis(i, k) <= UD}.  The
// reference makes N^2 scalar Haversine calls; here the POIs are visited in ascending latitude (order: a stable argsort made by the caller) and
// a query only scans the contiguous band |lat_k - lat_i| <= band_deg (the caller's band covers 2 asin(sqrt(c_ud)) with a margin; since
// c >= (1 - cos a) / 2 nothing outside it can be a neighbour).  Inside the band `c` is evaluated in float64 in cal_dis's operation order with
// the cphi / cos_small helpers of poi_dist_prob and compared with the exact host threshold c_ud (data.ud_threshold): c < c_ud <=> dist <= UD.
// One block = NB_Q consecutive queries (a wave each) sharing the band tiles staged in LDS.  Two passes: counts (then an in-place scan to int64
// offsets), fill (a wave-level ordered compaction, ballot + mbcnt: each row lists its neighbours in ascending latitude position, no atomics,
// the same output on every run).
//
// Step (FPMC_LR.py:113-151), per transition (u, a, i, j):
//   x = ui[u].(iu[i] - iu[j]) + ai[a].(ia[i] - ia[j]),  s = sigmoid(-x),  loss = log sigmoid(x)
//   ui[u] += alpha (s (iu[i] - iu[j]) - lambda ui[u])     ai[a] += alpha (s (ia[i] - ia[j]) - lambda ai[a])
//   iu[i] += alpha (s ui[u] - lambda iu[i])                iu[j] += alpha (-s ui[u] - lambda iu[j])
//   ia[i] += alpha (s ai[a] - lambda ia[i])                ia[j] += alpha (-s ai[a] - lambda ia[j])
// under the snapshot rule of include/poi_hip.h, as bpr.hip: 6 n touches keyed by (table, row) in one key space [ui | ai | iu | ia], sorted by
// te_scatter.hip's stable radix sort, every run of equal keys summed in sorted order (fixed order, no float atomics), runs cut by a 64-touch
// window joined as in bpr_span.  New rows go to a per-launch slot buffer and are copied into the tables by fpmc_commit after every gradient has
// read the launch-entry values.  A transition with an id outside its table, or with i == j, is keyed past the last row: it adds no gradient, no
// L2 decay and no multiplicity; its loss is NaN and it is counted once (poi_ctx_take_bad_ids).
#include "poi_common.h"
#include "poi_kernels.h"

namespace poi {

#define NB_Q 4          // queries per block of the neighbour passes (one wave each)
#define NB_TILE 256     // band candidates staged in LDS per round

template <bool FILL>
__global__ __launch_bounds__(256) void fpmc_nbr_kernel(FpmcNbrArgs A) {
  __shared__ double s_lat[NB_TILE], s_lon[NB_TILE], s_cp[NB_TILE];
  __shared__ int s_id[NB_TILE];
  __shared__ int s_band[2];
  const int w = wave_id(), lane = lane_id(), n = A.n;
  const int q0 = blockIdx.x * NB_Q, qpos = q0 + w;
  const bool active = qpos < n;
  if (threadIdx.x == 0) {      // the band of all NB_Q queries (ascending latitude: first - band .. last + band)
    const int ql = min(q0 + NB_Q, n) - 1;
    s_band[0] = lat_bound<false>(A.coords, A.order, n, A.coords[2 * (size_t)A.order[q0]] - A.band_deg);
    s_band[1] = lat_bound<true>(A.coords, A.order, n, A.coords[2 * (size_t)A.order[ql]] + A.band_deg);
  }
  const int qi = active ? A.order[qpos] : 0;
  const double lat1 = A.coords[2 * (size_t)qi], lon1 = A.coords[2 * (size_t)qi + 1], c1 = A.cphi[qi];
  __syncthreads();
  const int b0 = s_band[0], b1 = s_band[1];
  long long count = 0;
  const long long base = (FILL && active) ? A.off[qi] : 0;
  for (int t0 = b0; t0 < b1; t0 += NB_TILE) {
    __syncthreads();
    const int k = t0 + threadIdx.x;
    if (k < b1) {
      const int id = A.order[k];
      s_id[threadIdx.x] = id; s_lat[threadIdx.x] = A.coords[2 * (size_t)id]; s_lon[threadIdx.x] = A.coords[2 * (size_t)id + 1];
      s_cp[threadIdx.x] = A.cphi[id];
    }
    __syncthreads();
    if (!active) continue;
    const int m = min(NB_TILE, b1 - t0);
    for (int l0 = 0; l0 < m; l0 += 64) {
      const int l = l0 + lane;
      bool hit = false;
      if (l < m) {
        const double c = haversine_c(lat1, lon1, c1, s_lat[l], s_lon[l], s_cp[l]);
        hit = c < A.c_ud && s_id[l] != qi;
      }
      const unsigned long long bal = __ballot(hit);
      if (FILL && hit) {
        const int before = __builtin_amdgcn_mbcnt_hi((unsigned)(bal >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)bal, 0u));
        A.nbr[base + count + before] = s_id[l];
      }
      count += __popcll(bal);
    }
  }
  if (!FILL && active && lane == 0) A.off[qi + 1] = count;
}

// off[1..n] counts -> inclusive prefix sums, in place (one block)
__global__ __launch_bounds__(1024) void fpmc_scan_kernel(long long* x, int n) {
  __shared__ long long part[1024];
  const int per = (n + 1023) / 1024, b = min(n, (int)threadIdx.x * per), e = min(n, b + per);
  long long s = 0;
  for (int k = b; k < e; ++k) s += x[k];
  part[threadIdx.x] = s;
  __syncthreads();
  for (int o = 1; o < 1024; o <<= 1) {
    const long long v = threadIdx.x >= (unsigned)o ? part[threadIdx.x - o] : 0;
    __syncthreads();
    part[threadIdx.x] += v;
    __syncthreads();
  }
  long long run = threadIdx.x ? part[threadIdx.x - 1] : 0;
  for (int k = b; k < e; ++k) { run += x[k]; x[k] = run; }
}

hipError_t launch_fpmc_neighbors(FpmcNbrArgs& A, int fill, hipStream_t st) {
  const dim3 grid((A.n + NB_Q - 1) / NB_Q);
  if (!fill) {
    if (hipMemsetAsync(A.off, 0, sizeof(long long), st) != hipSuccess) return hipGetLastError();
    hipLaunchKernelGGL(fpmc_nbr_kernel<false>, grid, dim3(256), 0, st, A);
    hipLaunchKernelGGL(fpmc_scan_kernel, dim3(1), dim3(1024), 0, st, A.off + 1, A.n);
  } else {
    hipLaunchKernelGGL(fpmc_nbr_kernel<true>, grid, dim3(256), 0, st, A);
  }
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// Training negatives (prog_fpmc_lr.py:188-190, random.sample(negs[i+1], 1)): j = nbr[off[i] + floor(r cnt[i])], r from the counter-based RNG of
// poi_sample_negatives keyed on (seed, transition index).  A target outside [0, n_item) or without neighbours gets -1 (the step rejects it).
__global__ __launch_bounds__(256) void fpmc_sample_kernel(const long long* __restrict__ off, const int* __restrict__ nbr, const int* __restrict__ pos,
                                                          long long n, int n_item, unsigned long long seed, int* __restrict__ out) {
  for (long long t = blockIdx.x * 256ll + threadIdx.x; t < n; t += (long long)gridDim.x * 256) {
    const int i = pos[t];
    int j = -1;
    if ((unsigned)i < (unsigned)n_item) {
      const long long b = off[i], c = off[i + 1] - b;
      if (c > 0) {
        const unsigned long long r = splitmix64(splitmix64(seed ^ ((unsigned long long)t * 0xD1342543DE82EF95ull)));
        j = nbr[b + (long long)__umul64hi(r, (unsigned long long)c)];      // floor(r / 2^64 * c)
      }
    }
    out[t] = j;
  }
}

hipError_t launch_fpmc_sample(const long long* off, const int* nbr, const int* pos, long long n, int n_item, unsigned long long seed, int* out,
                              hipStream_t st) {
  const long long blocks = (n + 255) / 256;
  hipLaunchKernelGGL(fpmc_sample_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, st, off, nbr, pos, n, n_item, seed, out);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// Step
// ---------------------------------------------------------------------------------------------
// touch e of 6 n: kind e / n (0 ui[u], 1 ai[a], 2 iu[i], 3 iu[j], 4 ia[i], 5 ia[j]) of transition e % n
__device__ __forceinline__ const float* fpmc_row(const FpmcArgs& A, int key) {
  const int D = A.dim, R = A.n_item + 1;
  if (key < A.n_user) return A.ui + (size_t)key * D;
  const int k2 = key - A.n_user, tb = k2 / R, row = k2 - tb * R;
  return (tb == 0 ? A.ai : tb == 1 ? A.iu : A.ia) + (size_t)row * D;
}

// one pass over the transitions at the launch-entry values: s_t, loss_t, the 6 keys
template <int LPT>
__global__ __launch_bounds__(256) void fpmc_fwd_kernel(FpmcArgs A) {
  const int gl = threadIdx.x % LPT, gpb = 256 / LPT;
  const int D = A.dim, n = A.n, R = A.n_item + 1;
  if (blockIdx.x == 0 && threadIdx.x == 0) A.cnt[0] = 6 * n;
  for (int t = blockIdx.x * gpb + threadIdx.x / LPT; t < n; t += gridDim.x * gpb) {
    const int u = A.u[t], a = A.a[t], i = A.i[t], j = A.j[t];
    const bool bad = (unsigned)u >= (unsigned)A.n_user || (unsigned)a >= (unsigned)R || (unsigned)i >= (unsigned)R || (unsigned)j >= (unsigned)R || i == j;
    if (bad) {
      if (gl == 0) { atomicAdd(A.bad, 1); A.loss[t] = __int_as_float(0x7fc00000); A.s[t] = 0.f; }
      if (gl < 6) A.keys0[(size_t)gl * n + t] = A.sentinel;
      continue;
    }
    float dot = 0.f;
    for (int c = gl * 4; c < D; c += LPT * 4) {
      const float4 U = ld4(A.ui + (size_t)u * D + c), Aa = ld4(A.ai + (size_t)a * D + c);
      const float4 di = sub4(ld4(A.iu + (size_t)i * D + c), ld4(A.iu + (size_t)j * D + c));
      const float4 da = sub4(ld4(A.ia + (size_t)i * D + c), ld4(A.ia + (size_t)j * D + c));
      dot += dot4(U, di) + dot4(Aa, da);
    }
    dot = xor_group_sum<LPT>(dot);
    if (gl == 0) { A.s[t] = sigmoidf_(-dot); A.loss[t] = log_sigmoidf_(dot); }
    if (gl < 6) {
      const int nu = A.n_user;
      const int key = gl == 0 ? u : gl == 1 ? nu + a : gl == 2 ? nu + R + i : gl == 3 ? nu + R + j : gl == 4 ? nu + 2 * R + i : nu + 2 * R + j;
      A.keys0[(size_t)gl * n + t] = key;
    }
  }
}

// row <- row + alpha min(k, cap) (G / k - lambda row), into the slot of the run's first sorted position
__device__ __forceinline__ void fpmc_apply(const FpmcArgs& A, int key, float4 G, int k, int col, int slot) {
  const float4 r = ld4(fpmc_row(A, key) + col);
  const float sc = A.alpha * fminf((float)k, A.bcap), inv = 1.0f / (float)k, lm = A.lambda;
  *reinterpret_cast<float4*>(A.slot + (size_t)slot * A.dim + col) =
      make_float4(r.x + sc * (G.x * inv - lm * r.x), r.y + sc * (G.y * inv - lm * r.y), r.z + sc * (G.z * inv - lm * r.z), r.w + sc * (G.w * inv - lm * r.w));
}

// one wave per window of 64 sorted touches; LPR lanes per row (one float4 each, D <= 4 LPR), EPW = 64 / LPR touches of a run per pass
template <int LPR>
__global__ __launch_bounds__(256) void fpmc_chunk_kernel(FpmcArgs A) {
  constexpr int EPW = 64 / LPR;
  const int lane = lane_id(), grp = lane / LPR, gl = lane % LPR;
  const int n = A.n, D = A.dim, N = 6 * n, col = gl * 4;
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
      if (row == A.sentinel) break;      // the touches of rejected transitions sort last: nothing after them
      const bool cont_before = a == 0 && !(starts & 1ull);
      const bool cont_after = b == nv && nextk == row;
      float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
      for (int e0 = a; e0 < b; e0 += EPW) {
        const int idx = e0 + grp;
        const int e = __shfl(val, idx & 63, 64);
        if (idx < b && has) {
          const int kind = e / n, t = e - kind * n;
          const float s = A.s[t];
          float4 v;
          if (kind == 0) v = sub4(ld4(A.iu + (size_t)A.i[t] * D + col), ld4(A.iu + (size_t)A.j[t] * D + col));
          else if (kind == 1) v = sub4(ld4(A.ia + (size_t)A.i[t] * D + col), ld4(A.ia + (size_t)A.j[t] * D + col));
          else {
            v = ld4((kind < 4 ? A.ui + (size_t)A.u[t] * D : A.ai + (size_t)A.a[t] * D) + col);
            if (kind & 1) v = make_float4(-v.x, -v.y, -v.z, -v.w);      // kinds 3 / 5: the negative's row
          }
          acc.x = fmaf(s, v.x, acc.x); acc.y = fmaf(s, v.y, acc.y); acc.z = fmaf(s, v.z, acc.z); acc.w = fmaf(s, v.w, acc.w);
        }
      }
#pragma unroll
      for (int o = LPR; o < 64; o <<= 1) {
        acc.x += __shfl_xor(acc.x, o, 64); acc.y += __shfl_xor(acc.y, o, 64);
        acc.z += __shfl_xor(acc.z, o, 64); acc.w += __shfl_xor(acc.w, o, 64);
      }
      if (!cont_before && !cont_after) {
        if (grp == 0 && has) fpmc_apply(A, row, acc, b - a, col, j0 + a);
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
__global__ __launch_bounds__(256) void fpmc_span_kernel(FpmcArgs A) {
  constexpr int EPW = 64 / LPR;
  const int lane = lane_id(), grp = lane / LPR, gl = lane % LPR;
  const int D = A.dim, col = gl * 4, n_chunk = (6 * A.n + 63) / 64;
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
    fpmc_apply(A, m.w, sum, k, col, 64 * c + 64 - m.z);
  }
}

// every run's new row (slot of its first sorted position) -> its table, after all gradients have read the entry values
template <int LPR>
__global__ __launch_bounds__(256) void fpmc_commit_kernel(FpmcArgs A) {
  constexpr int EPW = 64 / LPR;
  const int lane = lane_id(), grp = lane / LPR, gl = lane % LPR;
  const int D = A.dim, col = gl * 4, N = 6 * A.n;
  for (int e = (blockIdx.x * 4 + wave_id()) * EPW + grp; e < N; e += gridDim.x * 4 * EPW) {
    const int key = A.ks[e];
    if (col >= D || key == A.sentinel || (e > 0 && A.ks[e - 1] == key)) continue;
    *reinterpret_cast<float4*>(const_cast<float*>(fpmc_row(A, key)) + col) = ld4(A.slot + (size_t)e * D + col);
  }
}

template <int LPR>
static hipError_t launch_fpmc_step_t(FpmcArgs& A, int num_cu, hipStream_t st, Timing* tm) {
  const int n = A.n;
  auto grid = [&](long long items, int per) { return dim3((unsigned)max(1ll, min((long long)num_cu * 16, (items + per - 1) / per))); };
  tm->begin("fpmc_fwd", st);
  hipLaunchKernelGGL(fpmc_fwd_kernel<LPR>, grid(n, 256 / LPR), dim3(256), 0, st, A);
  tm->end(st);
  tm->begin("fpmc_sort", st);
  int bits = 1;
  while ((1ll << bits) <= (long long)A.sentinel) ++bits;
  const int *ks = nullptr, *vs = nullptr;
  hipError_t e = launch_radix_sort(A.keys0, A.keys1, A.vals0, A.vals1, A.cnt, bits, A.hist, st, &ks, &vs);
  if (e != hipSuccess) return e;
  A.ks = ks; A.vs = vs;
  tm->end(st);
  const long long chunks = (6ll * n + 63) / 64;
  tm->begin("fpmc_rows", st);
  hipLaunchKernelGGL(fpmc_chunk_kernel<LPR>, grid(chunks, 4), dim3(256), 0, st, A);
  hipLaunchKernelGGL(fpmc_span_kernel<LPR>, grid(chunks, 4 * (64 / LPR)), dim3(256), 0, st, A);
  tm->end(st);
  tm->begin("fpmc_commit", st);
  hipLaunchKernelGGL(fpmc_commit_kernel<LPR>, grid(6ll * n, 4 * (64 / LPR)), dim3(256), 0, st, A);
  tm->end(st);
  return hipGetLastError();
}

hipError_t launch_fpmc_step(FpmcArgs& A, int num_cu, hipStream_t st, Timing* tm) {
  if (A.dim <= 32) return launch_fpmc_step_t<8>(A, num_cu, st, tm);
  if (A.dim <= 64) return launch_fpmc_step_t<16>(A, num_cu, st, tm);
  if (A.dim <= 128) return launch_fpmc_step_t<32>(A, num_cu, st, tm);
  return hipErrorInvalidValue;
}

}  // namespace poi
