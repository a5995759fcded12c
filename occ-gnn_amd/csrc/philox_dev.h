// philox_dev.h -- the counter-based generator behind every dropout mask (private to csrc/): Philox4x32-10 as
// cslicer_dropout.h and cslicer_gat_dropout.h define it, shared by dropout.hip and the attention kernels'
// dropout policies (gat_dev.h).
#ifndef CSLICER_PHILOX_DEV_H
#define CSLICER_PHILOX_DEV_H

#include <hip/hip_runtime.h>

#include <cstdint>

namespace {

// one round: (hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0) with (hi0, lo0) = M0 * c0, (hi1, lo1) = M1 * c2; the key moves by
// its increments between rounds.  Fully unrolled: ten rounds, two 32 x 32 -> 64 multiplies each.
__device__ __forceinline__ uint4 philox4x32_10(uint4 c, uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; r++) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c.x, p1 = (uint64_t)0xCD9E8D57u * c.z;
    c = make_uint4((uint32_t)(p1 >> 32) ^ c.y ^ k0, (uint32_t)p1, (uint32_t)(p0 >> 32) ^ c.w ^ k1, (uint32_t)p0);
    k0 += 0x9E3779B9u, k1 += 0xBB67AE85u;
  }
  return c;
}

// the mask on one quad: element j is kept and scaled by s where the quad's word j reaches the threshold
__device__ __forceinline__ float4 drop4(float4 a, const uint4 w, uint32_t thr, float s) {
  a.x = w.x >= thr ? a.x * s : 0.f;
  a.y = w.y >= thr ? a.y * s : 0.f;
  a.z = w.z >= thr ? a.z * s : 0.f;
  a.w = w.w >= thr ? a.w * s : 0.f;
  return a;
}

}  // namespace
#endif
