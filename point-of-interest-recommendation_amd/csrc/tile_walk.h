// The named steps of the item-stationary tile walk (rank.hip, select.hip, rerank.hip, route.hip, diverse.hip, filter.hip, capped.hip,
// labels.hip, group.hip; audience.hip and similar.hip walk the other axis): a workgroup owns 32 rows, a wave a range of 32-item tiles,
// the rows' fragments stay in registers and the item tiles stream past them through tile_product (tile_product.h).  Helpers only - no
// kernel and no loop lives here: every family's loop is its own, tuned for registers one by one, and each helper
// is in a kernel only where the kernel compiles to the instruction stream it had with the helper's text written out (tools/isa_same.py).
// Three steps failed that test as helpers in every form tried and stay each kernel's own text: the thresholds' copy into LDS, the
// exclusion cursor with its tile masks (rank, labels, audience, similar) and the passing-listed count (filter, capped).
//
// THE WALK'S CONTRACT.  tile_product stays in the kernel's own loop body, LAST before the epilogue, in one basic block with the first
// read of its result; no helper may put a branch between the two.  With a (mask) branch between them the taken path reached the read
// of accumulator register 15 some ten wait states behind the last MFMA instead of eighteen (hipcc, ROCm 7: the wait count of a 16-pass
// MFMA is not carried across the branch) and rows 27 / 31 of a tile read a stale value.  So the steps with a branch inside - the
// exclusion masks, a load under a condition - come BEFORE the product, and what follows it up to the first acc[r] is straight-line code:
// of the helpers here only item_tile_coords, opaque_half_base and acc_tile_row belong between the two.
#pragma once
#include "tile_product.h"

namespace poi {

// ---- carried over from walk_common.h, not steps of the walk: the score every path ranks, the bitmap's untrusted tail, a row's
// ---- exclusion list checked by a whole workgroup (filter.hip, capped.hip, labels.hip, rerank.hip) ----------------------------------------
// one zero, and is it selectable (neither NaN nor -inf)
__device__ __forceinline__ float one_zero(float s) { return s == 0.f ? 0.f : s; }
__device__ __forceinline__ bool selectable(float s) { return s > neg_inf(); }
__device__ __forceinline__ unsigned tail_mask(int N) { return (N & 31) ? (1u << (N & 31)) - 1u : ~0u; }

// one thread of a workgroup: the part of [e0, e1) it checks - ids inside [0, N) and strictly ascending
__device__ __forceinline__ int ex_slice_bad(const int* ex, int e0, int e1, int N, int tid, int nthr) {
  int bad = 0;
  for (int i = e0 + tid; i < e1; i += nthr) { const int v = ex[i]; bad |= (unsigned)v >= (unsigned)N || (i > e0 && ex[i - 1] >= v); }
  return bad;
}

// ---- which tiles a wave walks: two rules, both kept ----------------------------------------------------------------------------------
// the EVEN split (filter, capped, labels, diverse, group, audience, similar): slice sl of S takes tiles [ntile sl / S, ntile (sl + 1) / S),
// wave w of the workgroup a quarter of those - ranges differ by at most one tile, none is empty while there are tiles enough
__device__ __forceinline__ void wave_tile_range(int N, int sl, int S, int w, int& ntile, int& tb, int& te) {
  ntile = (N + 31) / 32;
  const int t0 = (int)((long long)ntile * sl / S), t1 = (int)((long long)ntile * (sl + 1) / S);
  tb = t0 + (int)((long long)(t1 - t0) * w / POI_NWAVE);
  te = t0 + (int)((long long)(t1 - t0) * (w + 1) / POI_NWAVE);
}
// the CEIL split (rank, score_rows, score_lists_shared): wave `split` of n_split takes ceil(ntile / n_split) tiles from its own start;
// the last ranges may be short or empty
__device__ __forceinline__ void wave_tile_chunk(int N, int n_split, int split, int& t_begin, int& t_end) {
  const int ntile = (N + 31) / 32;
  const int tps = (ntile + n_split - 1) / n_split;
  t_begin = min(ntile, split * tps);
  t_end = min(ntile, t_begin + tps);
}

// ---- the two sides of a tile ------------------------------------------------------------------------------------------------------------
// lane li's row of row tile ut in fragment order; the rows behind the call's last read that one (never emitted: row < n decides)
template <int D8, class Args>
__device__ __forceinline__ void load_row_tile(float4 (&a)[D8], const Args& A, int ut, int li, int h) {
  load_frag<D8>(a, A.users, 0, (size_t)min(ut * 32 + li, A.n - 1), A.dim, h);
}
// lane li's row of item tile `tile` in fragment order; the tile behind the table's end reads its last row (never ranked: j < N decides)
template <int D8, class Args>
__device__ __forceinline__ void load_item_tile(float4 (&b)[D8], const Args& A, int tile, int li, int h) {
  load_frag<D8>(b, A.items, A.items_f16, (size_t)min(tile * 32 + li, A.n_item - 1), A.dim, h);
}
// item j's latitude, longitude and cos(latitude) for the distance term; zeros without one
template <bool GEO, class Args>
__device__ __forceinline__ void item_tile_coords(const Args& A, int j, double& jlat, double& jlon, double& jcp) {
  jlat = 0.0; jlon = 0.0; jcp = 0.0;
  if (GEO) { const int jc = min(j, A.n_item - 1); jlat = A.coords[2 * (size_t)jc]; jlon = A.coords[2 * (size_t)jc + 1]; jcp = A.cphi[jc]; }
}

// ---- the row side: what the epilogue reads from LDS -------------------------------------------------------------------------------------
// accumulator register r of lane half h holds tile row (r & 3) + 8 (r >> 2) + 4 h (tile_product.h).  The half's base 4 h goes through
// an empty asm once per tile: a base the compiler can see is loop-invariant, and it hoists the LDS reads of all 16 rows (targets, list
// thresholds, coordinates) out of the tile loop - 100 to 256 registers
__device__ __forceinline__ int opaque_half_base(int h) {
  int hb = 4 * h;
  asm volatile("" : "+v"(hb));
  return hb;
}
__device__ __forceinline__ int acc_tile_row(int r, int hb) { return (r & 3) + 8 * (r >> 2) + hb; }

// acc[rr] for a register number known at run time only, without dynamic indexing (which would send the accumulators to scratch)
__device__ __forceinline__ float acc_row(const f32x16& acc, int rr) {
  float v = acc[0];
#pragma unroll
  for (int r = 1; r < 16; ++r) v = rr == r ? acc[r] : v;
  return v;
}

// the distance term on a score: s + wd * P(bin(row's anchor, item)), one fused multiply-add.  Row ul of row tile ut, its anchor's
// coordinates from LDS; the guard - rows without an anchor (s_has), bits that are off - is the caller's
template <class Args>
__device__ __forceinline__ float geo_add(const Args& A, float wd, const double* thr, int ut, int ul, const double* ulat, const double* ulon,
                                         const double* ucp, double jlat, double jlon, double jcp, float s) {
  return __fmaf_rn(wd, geo_prob(A, thr, min(ut * 32 + ul, A.n - 1), ulat[ul], ulon[ul], ucp[ul], jlat, jlon, jcp), s);
}

// ---- the rare part: row by row over the tile's 32 rows ----------------------------------------------------------------------------------
// tile row `row` lives in register rr of lane half (row >> 2) & 1; true on the lanes whose bit rr of cm is set there.  The caller's
// own `for (row ...)` skips the row when no lane holds one (a ballot: wave-uniform)
__device__ __forceinline__ bool rare_row(int row, int h, unsigned cm, int& rr) {
  rr = (row & 3) + 4 * (row >> 3);
  return h == ((row >> 2) & 1) && ((cm >> rr) & 1u);
}

}  // namespace poi
