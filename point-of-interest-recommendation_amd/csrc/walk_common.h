// What the bitmap walks share (filter.hip, capped.hip): the score every path ranks, the bitmap's untrusted tail, and the check of a
// row's exclusion list by a whole workgroup.
#pragma once
#include "poi_common.h"

namespace poi {

// the score every path ranks: one zero, and is it selectable (neither NaN nor -inf)
__device__ __forceinline__ float one_zero(float s) { return s == 0.f ? 0.f : s; }
__device__ __forceinline__ bool selectable(float s) { return s > neg_inf(); }
__device__ __forceinline__ unsigned tail_mask(int N) { return (N & 31) ? (1u << (N & 31)) - 1u : ~0u; }

// one thread of a workgroup: the part of [e0, e1) it checks - ids inside [0, N) and strictly ascending
__device__ __forceinline__ int ex_slice_bad(const int* ex, int e0, int e1, int N, int tid, int nthr) {
  int bad = 0;
  for (int i = e0 + tid; i < e1; i += nthr) { const int v = ex[i]; bad |= (unsigned)v >= (unsigned)N || (i > e0 && ex[i - 1] >= v); }
  return bad;
}

}  // namespace poi
