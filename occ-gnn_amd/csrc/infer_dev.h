// infer_dev.h -- what csrc/infer.hip and csrc/infer_parts.hip share beyond csrc/dev_common.h (private to csrc/): the
// launch constants, the float4 element helpers, the ROW ENDS of both models and the host helpers of their entry points.  A row is finished by the
// same code whether one process summed it or the ranks' partials were merged, so with one part the rank path rounds as
// the single-process path does: the bitwise promise of include/cslicer_infer_parts.h rests on this file being the only
// home of these functions.
#ifndef CSLICER_INFER_DEV_H
#define CSLICER_INFER_DEV_H

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <type_traits>

#include "cslicer_hip.h"
#include "cslicer_infer.h"
#include "cslicer_infer16.h"
#include "dev_common.h"
#include "feat_elem.h"

namespace {

constexpr int BLK = 256;
constexpr int WPB = BLK / 64;   // waves (items) per block
constexpr int SEG = CSL_INFER_SEG;
constexpr int U = 8;            // row loads in flight per lane and step (the attention kernels' steps depend on it)
constexpr int GAT_LAST_MAX_C = 4096;  // H * D of a last layer: its head mean stages a row per wave in LDS (64 KiB a block)
constexpr long long GAT_MAX_C = 1ll << 24;  // H * D of a hidden layer (nothing staged; column indices stay int)

__device__ __forceinline__ float4 f4zero() { return make_float4(0.f, 0.f, 0.f, 0.f); }
__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void st4(float* p, const float4 v) { *reinterpret_cast<float4*>(p) = v; }
__device__ __forceinline__ void scale4(float4& a, const float s) { a.x *= s, a.y *= s, a.z *= s, a.w *= s; }
__device__ __forceinline__ float4 shfl_xor4(const float4 v, const int d) {
  return make_float4(__shfl_xor(v.x, d), __shfl_xor(v.y, d), __shfl_xor(v.z, d), __shfl_xor(v.w, d));
}
__device__ __forceinline__ float elu1(const float v) { return v > 0.f ? v : expm1f(v); }

// ---------------------------------------------------------------- GraphSAGE

// the end of a row: aggregate-first writes the operand [x[v] | mean], project-first act(x[v, :W) + mean + bias)
template <typename E>
__device__ __forceinline__ void sage_finish(const E* __restrict__ x, long long ldx, int W, int proj,
                                            const float* __restrict__ bias, int relu, float* __restrict__ out, long long ldo,
                                            long long k, int row, int deg, int c4, float4 acc) {
  const float d = (float)(deg > 0 ? deg : 1);
  acc.x /= d, acc.y /= d, acc.z /= d, acc.w /= d;
  const float4 self = feat::Elem<E>::up(feat::Elem<E>::ld(x + (long long)row * ldx + 4 * c4));
  if (!proj) {
    st4(out + k * ldo + 4 * c4, self);
    st4(out + k * ldo + W + 4 * c4, acc);
    return;
  }
  float4 y = self;
  add4(y, acc);
  if (bias) add4(y, ld4(bias + 4 * c4));
  if (relu) y.x = fmaxf(y.x, 0.f), y.y = fmaxf(y.y, 0.f), y.z = fmaxf(y.z, 0.f), y.w = fmaxf(y.w, 0.f);
  st4(out + k * ldo + 4 * c4, y);
}

// ---------------------------------------------------------------- GAT

// merge softmax state (m2, s2, n2) into (m, s, n)
__device__ __forceinline__ void lse_merge(float& m, float& s, float4& n, const float m2, const float s2, const float4 n2) {
  const float M = fmaxf(m, m2);
  const float a = expf(m - M), b = expf(m2 - M);
  s = s * a + s2 * b;
  scale4(n, a);
  fma4(n, b, n2);
  m = M;
}

// the hub merge of csrc/infer.hip's k_infer_gat_hubs with its rounding spelled out: there the compiler forms
// s = s a + s2 b from two rounded products, n.xyz = fma(n, a, b n2) and n.w = fma(b, n2.w, n.w a) (gfx950, as
// contracted and paired by its vectoriser).  Left to contract freely, the same expression compiles differently in a
// kernel that stores the state instead of finishing the row, and a hub row with one part would differ in its last bit.
// (Only the hub pass needs it: a merge into the zero state, as the owner's first, is exact in every form.)
__device__ __forceinline__ void lse_merge_hub(float& m, float& s, float4& n, const float m2, const float s2,
                                              const float4 n2) {
#pragma clang fp contract(off)
  const float M = fmaxf(m, m2);
  const float a = expf(m - M), b = expf(m2 - M);
  s = s * a + s2 * b;
  n.x = __builtin_fmaf(n.x, a, b * n2.x);
  n.y = __builtin_fmaf(n.y, a, b * n2.y);
  n.z = __builtin_fmaf(n.z, a, b * n2.z);
  n.w = __builtin_fmaf(b, n2.w, n.w * a);
  m = M;
}

// the end of a row: hidden layers ELU(n / s + bias) in place of the output row; the last layer stages n / s + bias of the
// row in the wave's LDS region (the head mean follows once every column tile is there)
__device__ __forceinline__ void gat_finish(const float* __restrict__ bias, int last, float* __restrict__ out, long long ldo,
                                           float* stage, long long k, int c4, float s, float4 n) {
  float4 y = s > 0.f ? make_float4(n.x / s, n.y / s, n.z / s, n.w / s) : f4zero();
  if (bias) add4(y, ld4(bias + 4 * c4));
  if (last) {
    st4(stage + 4 * c4, y);
    return;
  }
  st4(out + k * ldo + 4 * c4, make_float4(elu1(y.x), elu1(y.y), elu1(y.z), elu1(y.w)));
}

__device__ __forceinline__ void gat_head_mean(const float* stage, int H, int D, int n_cls, float* __restrict__ out,
                                              long long ldo, long long k, int lane) {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  for (int j = lane; j < n_cls; j += 64) {
    float t = 0.f;
    for (int h = 0; h < H; h++) t += stage[h * D + j];
    out[k * ldo + j] = t / (float)H;
  }
}

// ---------------------------------------------------------------- host side

unsigned blocks_of(long long n, int per_wave = 1) {
  return (unsigned)((n + (long long)WPB * per_wave - 1) / ((long long)WPB * per_wave));
}

// G groups of 64 / G lanes: the smallest group that holds a column tile of min(C4, 64) float4s (at most 16 groups)
int groups_for(int C4) {
  int lg = 4;
  while (lg < 64 && lg < C4) lg <<= 1;
  return 64 / lg;
}

// the checks shared by every kernel that walks a work list: a plan slice that is there when it is used.
// hubs_read_indptr: the caller's hub pass reads indptr (csrc/infer.hip: a row's degree; csrc/infer_parts.hip's does not)
bool plan_ok(const int32_t* indptr, const int32_t* indices, const int32_t* items, int64_t n_items, const int32_t* hubs,
             int64_t n_hubs, int64_t pos0, int64_t part0, const void* partial, bool hubs_read_indptr) {
  if (n_items < 0 || n_hubs < 0 || pos0 < 0 || part0 < 0 || n_items >= (1ll << 31) * WPB || n_hubs >= (1ll << 31) * WPB)
    return false;
  if (n_items && (!indptr || !indices || !items || !aligned16(items))) return false;
  if (n_hubs && ((hubs_read_indptr && !indptr) || !hubs || !aligned16(hubs) || !partial || !aligned16(partial))) return false;
  return true;
}

// a group count G and the rows per wave R to compile-time ones (int_c and with_groups for G alone: csrc/dev_common.h):
// the (G, R) pairs in which a group keeps at least 4 lanes (pack_for): R <= 4, 2 and 1 for G <= 4, 8 and 16
template <typename F>
void with_groups_rows(int G, int R, F&& f) {
  with_groups<1, 16>(G, [&](auto g) {
    constexpr int RMAX = g() <= 4 ? 4 : 16 / g();
    with_groups<1, RMAX>(R, [&](auto r) { f(g, r); });
  });
}

}  // namespace
#endif
