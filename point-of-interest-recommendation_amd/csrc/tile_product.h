// The 32 x 32 float32 tile product of the item-stationary serving kernels (rank.hip, group.hip, route.hip, diverse.hip) and the helpers
// that go with it: the fragment loader, the distance term's probability, the exclusion-list search and what a tile row's prologue reads.  One routine for every kernel that must score a
// (row, item) pair to the same bits as the others.
#pragma once
#include "poi_common.h"

namespace poi {

typedef float f32x16 __attribute__((ext_vector_type(16)));

// row `row` of a (rows, D) table in fragment order: lane half h holds the k-columns 8m + 4h .. 8m + 4h + 3, one float4 per m
template <int D8>
__device__ __forceinline__ void load_frag(float4 (&f)[D8], const void* base, int f16, size_t row, int D, int h) {
#pragma unroll
  for (int m = 0; m < D8; ++m) {
    const int k0 = 8 * m + 4 * h;
    f[m] = k0 < D ? ld4t(base, row * D + k0, f16) : make_float4(0.f, 0.f, 0.f, 0.f);
  }
}

// THE product: acc[item = lane & 31][row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)], one fixed k order
template <int D8>
__device__ __forceinline__ f32x16 tile_product(const float4 (&a)[D8], const float4 (&b)[D8]) {
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
  for (int m = 0; m < D8; ++m) {
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[m].x, b[m].x, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[m].y, b[m].y, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[m].z, b[m].z, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[m].w, b[m].w, acc, 0, 0, 0);
  }
  return acc;
}

// the distance term's probability of (row, item): sts[row][bin] for bin < n_dist, the bin from the float64 Haversine term through thr
template <class Args>
__device__ __forceinline__ float geo_prob(const Args& A, const double* thr, int row, double ulat, double ulon, double ucp, double jlat,
                                          double jlon, double jcp) {
  const int bin = bin_of_c(haversine_c(ulat, ulon, ucp, jlat, jlon, jcp), thr, A.n_dist, A.bin_scale);
  return bin < A.n_dist ? A.sts[(size_t)row * (A.n_dist + 1) + bin] : 0.f;
}

// ascending list ex[a .. b): does it hold id?
__device__ __forceinline__ bool listed(const int* ex, int a, int b, int id) {
  const int e1 = b;
  while (a < b) { const int md = (a + b) >> 1; if (ex[md] < id) a = md + 1; else b = md; }
  return a < e1 && ex[a] == id;
}

// one wave: exclusion list `list` of (ex_off, ex) into [e0, e1).  Nonzero on a lane that saw it broken - offsets out of order, an id
// outside [0, N) or not above the one before it; the caller joins the lanes
__device__ __forceinline__ int check_ex_row(const int* ex_off, const int* ex, int list, int N, int lane, int& e0, int& e1) {
  e0 = ex_off[list]; e1 = ex_off[list + 1];
  int bad = e0 < 0 || e1 < e0;
  if (!bad)
    for (int p = e0 + lane; p < e1; p += 64) { const int v = ex[p]; bad |= (unsigned)v >= (unsigned)N || (p > e0 && ex[p - 1] >= v); }
  return bad;
}

// the distance term's row side: has row `row` (-1: no such row) a last POI, and that POI's latitude, longitude and cos(latitude)
template <class Args>
__device__ __forceinline__ void load_row_geo(const Args& A, int row, int N, int& has, double& lat, double& lon, double& cp) {
  const int lp = row >= 0 ? A.last_poi[row] : -1;
  const int lc = min(max(lp, 0), N - 1);            // (an id outside the table reads no memory outside it)
  has = lp >= 0;
  lat = A.coords[2 * (size_t)lc]; lon = A.coords[2 * (size_t)lc + 1]; cp = A.cphi[lc];
}

__device__ __forceinline__ float pos_inf() { return __builtin_huge_valf(); }

}  // namespace poi
