// What the launchers of the tile-walk families share: the dim bracket behind every <D8, DB> instantiation, and the LDS opt-in of a kernel
// instantiation.  The bracket rule is plain host arithmetic, no HIP: a test compiles it on its own.
#pragma once

// 0 .. 3 for dim <= 32 / 64 / 128 / 256 - the kernels' D8 = 4 << bracket float4 fragments per operand row; -1: no kernel takes this dim
// (dim <= 0 too: the entry points reject it before any launcher sees it)
inline int dim_bracket(int dim) { return dim <= 0 ? -1 : dim <= 32 ? 0 : dim <= 64 ? 1 : dim <= 128 ? 2 : dim <= 256 ? 3 : -1; }
// does a bracket stream its tiles through two fragment buffers?  Up to dim `upto`: 64 for most families, 128 for rank.hip, select.hip
// and rerank.hip - the choices as found; which is better at dim 128 has not been measured
constexpr bool two_buffers(int bracket, int upto) { return (32 << bracket) <= upto; }

#ifdef __HIPCC__
#include "poi_common.h"
#include <type_traits>

namespace poi {

// f(integral_constant<int, D8>, bool_constant<DB>) for the bracket of `dim`; UPTO is a template argument so that a family instantiates its
// own four (D8, DB) pairs and no other
template <int UPTO, class F>
hipError_t by_dim(int dim, F&& f) {
  switch (dim_bracket(dim)) {
    case 0: return f(std::integral_constant<int, 4>{}, std::bool_constant<two_buffers(0, UPTO)>{});
    case 1: return f(std::integral_constant<int, 8>{}, std::bool_constant<two_buffers(1, UPTO)>{});
    case 2: return f(std::integral_constant<int, 16>{}, std::bool_constant<two_buffers(2, UPTO)>{});
    case 3: return f(std::integral_constant<int, 32>{}, std::bool_constant<two_buffers(3, UPTO)>{});
  }
  return hipErrorInvalidValue;
}

// the opt-in to `bytes` of dynamic LDS: an attribute of one kernel instantiation on one device (DeviceOnce, poi_common.h)
template <auto KERNEL>
hipError_t lds_opt_in(int bytes) {
  static DeviceOnce once;
  return once.run([&]() -> hipError_t {
    return hipFuncSetAttribute(reinterpret_cast<const void*>(KERNEL), hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
  });
}

}  // namespace poi
#endif
