// dev_common.h -- what the .hip files of csrc/ share (private to csrc/): the launch dispatchers that turn a run-time
// element kind or group count into a compile-time one, and the few small helpers every file had a copy of.
#ifndef CSLICER_DEV_COMMON_H
#define CSLICER_DEV_COMMON_H

#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "cslicer_feat16.h"
#include "cslicer_hip.h"
#include "feat_elem.h"

namespace {

__device__ __forceinline__ void add4(float4& a, const float4 b) { a.x += b.x, a.y += b.y, a.z += b.z, a.w += b.w; }
__device__ __forceinline__ void fma4(float4& a, const float s, const float4 b) {
  a.x += s * b.x, a.y += s * b.y, a.z += s * b.z, a.w += s * b.w;
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
int done() { return hipGetLastError() == hipSuccess ? CSL_OK : CSL_E_HIP; }
inline int64_t up4(int64_t x) { return (x + 3) & ~(int64_t)3; }  // every buffer starts 16-byte aligned

// The launch dispatchers: a run-time group count G (element kind) to a compile-time one.  f is a generic lambda that
// names its kernel with its own template arguments, e.g.
//   with_groups<1, 64>(G, [&](auto g) { hipLaunchKernelGGL((k<g(), E>), ...); });
template <int V>
using int_c = std::integral_constant<int, V>;
template <typename E>
struct elem_c { typedef E type; };

// f(int_c<the power of two in [LO, HI] that G names>): below LO it is LO, above HI it is HI.  The bounds keep the set of
// instantiated kernels to the groups a caller can reach.
template <int LO, int HI, typename F>
void with_groups(int G, F&& f) {
  static_assert(LO > 0 && (LO & (LO - 1)) == 0 && (HI & (HI - 1)) == 0 && LO <= HI, "powers of two");
  if constexpr (LO < HI) {
    if (G > LO) return with_groups<2 * LO, HI>(G, f);
  }
  f(int_c<LO>{});
}

// a 16-bit table's element kind (checked by the caller: feat::table_ok) to its element type
template <typename F>
auto with_elem(int32_t kind, F&& f) {
  if (kind == CSL_FEAT_F16) return f(elem_c<feat::f16>{});
  return f(elem_c<feat::bf16>{});
}

// the same for a table that may also be float32 (kind 0)
template <typename F>
auto with_table(int32_t kind, F&& f) {
  if (kind == 0) return f(elem_c<float>{});
  return with_elem(kind, f);
}

}  // namespace
#endif
