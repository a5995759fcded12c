// feat_elem.h -- how an element of the resident feature table reaches fp32 registers (device side of cslicer_feat16.h).
//
// A lane always moves FOUR consecutive elements of a row: one 16-byte load of a float32 table, one 8-byte load of a
// float16 / bfloat16 table, upcast in registers.  Both upcasts are exact (every float16 and every bfloat16 value is a
// float32 value), so a kernel templated on the element type computes on a 16-bit table bitwise what it computes on the
// table converted to float32 beforehand.  The all-zero bit pattern is 0.0 in all three formats (the zero row).
#ifndef CSLICER_FEAT_ELEM_H
#define CSLICER_FEAT_ELEM_H

#include <hip/hip_runtime.h>

#include <cstdint>

#include "cslicer_feat16.h"

namespace feat {

struct f16 { unsigned short bits; };    // IEEE binary16
struct bf16 { unsigned short bits; };   // the upper half of a float32

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));

template <typename E>
struct Elem;

template <>
struct Elem<float> {
  typedef float4 Raw;   // four elements as loaded
  static constexpr unsigned SIZE = 4;
  // an address that went through LDS as an integer is loaded from as GLOBAL memory, said explicitly (sage_mfma.hip)
  static __device__ __forceinline__ Raw ldg(unsigned long long addr) {
    const f32x4 v = *reinterpret_cast<const f32x4 __attribute__((address_space(1)))*>((uintptr_t)addr);
    return make_float4(v.x, v.y, v.z, v.w);
  }
  static __device__ __forceinline__ Raw ld(const float* p) { return *reinterpret_cast<const float4*>(p); }
  static __device__ __forceinline__ float4 up(const Raw r) { return r; }
  static __device__ __forceinline__ Raw zero() { return make_float4(0.f, 0.f, 0.f, 0.f); }
};

struct Elem16 {
  typedef u32x2 Raw;   // element 0 in the low half of .x (little endian)
  static constexpr unsigned SIZE = 2;
  static __device__ __forceinline__ Raw ldg(unsigned long long addr) {
    return *reinterpret_cast<const u32x2 __attribute__((address_space(1)))*>((uintptr_t)addr);
  }
  static __device__ __forceinline__ Raw ldp(const void* p) { return *reinterpret_cast<const u32x2*>(p); }
  static __device__ __forceinline__ Raw zero() {
    Raw r = {0u, 0u};
    return r;
  }
};

template <>
struct Elem<f16> : Elem16 {
  static __device__ __forceinline__ Raw ld(const f16* p) { return ldp(p); }
  static __device__ __forceinline__ float h2f(unsigned bits) {
    return (float)__builtin_bit_cast(_Float16, (unsigned short)bits);
  }
  // v_cvt_f32_f16 per element (the upper halves by its word select): exact, subnormals included.  (Element by element
  // on purpose: ROCm 7.2's clang folds a bit_cast of the two words to two half2 vectors into ONE word used twice.)
  static __device__ __forceinline__ float4 up(const Raw r) {
    return make_float4(h2f(r.x & 0xffffu), h2f(r.x >> 16), h2f(r.y & 0xffffu), h2f(r.y >> 16));
  }
};

template <>
struct Elem<bf16> : Elem16 {
  static __device__ __forceinline__ Raw ld(const bf16* p) { return ldp(p); }
  static __device__ __forceinline__ float4 up(const Raw r) {   // a shift or a mask per element
    return make_float4(__uint_as_float(r.x << 16), __uint_as_float(r.x & 0xffff0000u), __uint_as_float(r.y << 16),
                       __uint_as_float(r.y & 0xffff0000u));
  }
};

// what every 16-bit entry point checks about its table before any HIP call
inline bool kind_ok(int32_t kind) { return kind == CSL_FEAT_F16 || kind == CSL_FEAT_BF16; }
inline bool table_ok(const void* x, int32_t kind, int64_t ldx) {
  return kind_ok(kind) && x && ldx % 4 == 0 && (reinterpret_cast<uintptr_t>(x) & 7u) == 0;
}

}  // namespace feat
#endif
