// Shared by the per-slot session kernels (session.hip, session_cells.hip): the LDS tile layout of the float64 matrix-core path, the
// position bin of an event, and the float64 xor-butterfly reductions.  The butterfly sums in another order than the DPP + readlane
// wave_sum_d / block_*_d of exact_engine.hip - other bits; the two families are not interchangeable.
#pragma once
#include "poi_common.h"

namespace poi {

constexpr int RS = 17;      // LDS row stride of the k-major tiles (16 events + 1: the transposing copies stay conflict-free)

typedef double f64x4 __attribute__((ext_vector_type(4)));

// LDS row of contraction index k: MFMA j of k-block kq contracts k = 16 kq + 4 g + j, stored at row 16 kq + 4 j + g
__device__ __forceinline__ int swz(int k) { return (k & ~15) | ((k & 3) << 2) | ((k >> 2) & 3); }

// data.dist_pos_bins: bin(coords[cur], coords[prev]) through the exact thresholds (the expression order of neg_dist_kernel)
template <class Args>
__device__ __forceinline__ int pos_bin(const Args& A, int cur, int prev) {
#pragma clang fp contract(off)
  const double pr = 0.017453292519943295;
  const double a = (A.coords[2 * cur] - A.coords[2 * prev]) * pr;
  const double b = (A.coords[2 * cur + 1] - A.coords[2 * prev + 1]) * pr;
  const double c = (1.0 - cos_small(a)) / 2 + A.cphi[cur] * A.cphi[prev] * (1.0 - cos_small(b)) / 2;
  return bin_of_c(c, A.thr, A.n_dist, (float)(12742.0 * 1000.0 / A.dd));
}

__device__ __forceinline__ float ld_tab(const void* base, size_t off, int f16) {
  return f16 ? __half2float(reinterpret_cast<const __half*>(base)[off]) : reinterpret_cast<const float*>(base)[off];
}

// ---- the 16-column float64 matrix-core cell step (session.hip's tile kernel, explain.hip's walk) ------------------------------------
// acc[q] += W_q[16 rows][K] . S[K][16 events]: wrow[q] = this lane's row of W_q at column 4 g; S k-major in LDS at the swizzled rows
// (not merged with session_cells.hip's sc_mma, which prefetches the next k-block: unifying them would change one kernel's schedule)
template <int NG, class T>
__device__ __forceinline__ void sess_mma(f64x4 (&acc)[NG], const float* const (&wrow)[NG], int K, const T* sT, int i, int g) {
  for (int kq = 0; kq < (K >> 4); ++kq) {
    float4 a[NG];
#pragma unroll
    for (int q = 0; q < NG; ++q) a[q] = ld4(wrow[q] + 16 * kq);
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

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
// block reductions of a 256-thread workgroup in a fixed order.  Contain barriers; `red` holds 4 doubles.
__device__ __forceinline__ double block_sum_d(double v, double* red) {
  v = wave_sum_d(v);
  __syncthreads();
  if (lane_id() == 0) red[wave_id()] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}
__device__ __forceinline__ double block_max_d(double v, double* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  __syncthreads();
  if (lane_id() == 0) red[wave_id()] = v;
  __syncthreads();
  return fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
}

// this lane's share of w[0 .. K) . x (x: LDS doubles); the lanes stride the row in float4 (K % 4 == 0)
__device__ __forceinline__ double row_part(const float* __restrict__ w, int K, const double* x, int lane) {
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
  for (int j = lane * 4; j < K; j += 256) {
    const float4 v = ld4(w + j);
    a0 = fma((double)v.x, x[j], a0); a1 = fma((double)v.y, x[j + 1], a1);
    a2 = fma((double)v.z, x[j + 2], a2); a3 = fma((double)v.w, x[j + 3], a3);
  }
  return (a0 + a1) + (a2 + a3);
}

}  // namespace poi
