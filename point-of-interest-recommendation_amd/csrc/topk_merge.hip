// The second kernel of every split path (near.hip, geoie_score.hip, group.hip, diverse.hip): a row's slices each left a sorted partial
// list and a count; one wave per row folds the lists in slice order (fold_slice_lists, topk_list.h) and adds the counts.
#include "poi_common.h"
#include "poi_kernels.h"
#include "topk_list.h"

namespace poi {

template <int KMAX>
__global__ __launch_bounds__(64) void topk_slices_merge_kernel(SliceLists L) {
  const int r = blockIdx.x, lane = lane_id(), S = L.n_split;
  const size_t base = (size_t)r * S;
  float cs;
  int ci, cnt = 0;
  fold_slice_lists<KMAX>(L.part_s, L.part_i, base, S, cs, ci);
  for (int s = lane; s < S; s += 64) cnt += L.part_cnt[base + s];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
  if (lane < L.k) {
    L.idx_out[(size_t)r * L.k + lane] = ci == PAD_ID ? -1 : ci;
    if (L.score_out) L.score_out[(size_t)r * L.k + lane] = ci == PAD_ID ? neg_inf() : cs;
  }
  if (lane == 0 && L.count_out) L.count_out[r] = cnt;
}

// the launch alone: the caller's hipGetLastError reports it with its own kernel's
void launch_topk_slices_merge(const SliceLists& L, int k_max, int n_rows, hipStream_t st) {
  if (k_max == 64) hipLaunchKernelGGL(topk_slices_merge_kernel<64>, dim3((unsigned)n_rows), dim3(64), 0, st, L);
  else hipLaunchKernelGGL(topk_slices_merge_kernel<32>, dim3((unsigned)n_rows), dim3(64), 0, st, L);
}

}  // namespace poi
