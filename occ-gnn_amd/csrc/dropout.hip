// dropout.hip -- dropout between the GraphSAGE layers behind the C ABI (cslicer_dropout.h): the mask is
// Philox4x32-10 of (column quad, node id, layer, step) under the run's seed, recomputed wherever it is needed -- forward,
// backward (the same map on the gradient), any rank -- and never stored.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "cslicer_dropout.h"
#include "dev_common.h"
#include "philox_dev.h"

namespace {

constexpr int DBLK = 256;

// A row is walked by 2^lg lanes (the power of two that covers its H / 4 quads, 64 at the most), 256 >> lg rows per
// workgroup: the row and the lane come out of shifts, a lane reads its node id once.  x and y may be the same matrix
// (every lane reads its quad before it writes it; no quad is touched by two lanes), hence no __restrict__.
__global__ __launch_bounds__(DBLK) void k_dropout(const float* x, long long ldx, float* y, long long ldy, const int32_t* ids,
                                                  long long n, int hq, int lg, uint32_t thr, float s, uint32_t k0,
                                                  uint32_t k1, uint32_t layer, uint32_t step) {
  const long long row = (long long)blockIdx.x * (DBLK >> lg) + (threadIdx.x >> lg);
  if (row >= n) return;
  const uint32_t v = ids ? (uint32_t)ids[row] : (uint32_t)row;
  const float* xr = x + row * ldx;
  float* yr = y + row * ldy;
  for (int q = threadIdx.x & ((1 << lg) - 1); q < hq; q += 1 << lg) {
    const float4 a = *reinterpret_cast<const float4*>(xr + 4 * q);
    const uint4 w = philox4x32_10(make_uint4((uint32_t)q, v, layer, step), k0, k1);
    *reinterpret_cast<float4*>(yr + 4 * q) = drop4(a, w, thr, s);
  }
}

struct ScaleArgs {
  float* seg[CSL_SCALE_SEGMENTS_MAX];
  long long n[CSL_SCALE_SEGMENTS_MAX];
  float factor[CSL_SCALE_SEGMENTS_MAX];
  int first_block[CSL_SCALE_SEGMENTS_MAX + 1];   // blocks of SCALE_CHUNK elements, segments back to back
  int count;
};
constexpr int SCALE_CHUNK = 1024;

// (a segment of the flat gradient buffer starts wherever the parameters before it end: scalar accesses)
__global__ __launch_bounds__(DBLK) void k_scale_segments(ScaleArgs a) {
  int j = 0;
  while (j + 1 < a.count && (int)blockIdx.x >= a.first_block[j + 1]) j++;
  const long long base = ((long long)blockIdx.x - a.first_block[j]) * SCALE_CHUNK;
  float* p = a.seg[j];
  const float f = a.factor[j];
  for (long long i = base + threadIdx.x; i < base + SCALE_CHUNK && i < a.n[j]; i += DBLK) p[i] *= f;
}

}  // namespace

extern "C" {

int csl_dropout_f32(const float* x, int64_t ldx, float* y, int64_t ldy, const int32_t* ids, int64_t n, int32_t H, float p,
                    int64_t seed, int32_t layer, int64_t step, void* stream) {
  if (!(p > 0.f && p < 1.f) || n < 0 || H < 4 || H % 4 != 0 || ldx < H || ldy < H || ldx % 4 != 0 || ldy % 4 != 0)
    return CSL_E_INVALID;
  if (n == 0) return CSL_OK;
  if (!x || !y || !aligned16(x) || !aligned16(y)) return CSL_E_INVALID;
  const int hq = H / 4;
  int lg = 0;
  while (lg < 6 && (1 << lg) < hq) lg++;
  const long long rows = DBLK >> lg, blocks = (n + rows - 1) / rows;
  if (blocks > 0x7fffffffLL) return CSL_E_INVALID;
  const uint32_t thr = (uint32_t)((double)p * 4294967296.0);   // (p < 1 in float32: below 2^32; the cast floors)
  const float s = (float)(1.0 / (1.0 - (double)p));
  const uint64_t sd = (uint64_t)seed;
  hipLaunchKernelGGL(k_dropout, dim3((unsigned)blocks), dim3(DBLK), 0, (hipStream_t)stream, x, (long long)ldx, y,
                     (long long)ldy, ids, (long long)n, hq, lg, thr, s, (uint32_t)sd, (uint32_t)(sd >> 32), (uint32_t)layer,
                     (uint32_t)(uint64_t)step);
  return done();
}

int csl_scale_segments_f32(int32_t count, float* const* seg, const int64_t* n, const float* factor, void* stream) {
  if (count < 0 || count > CSL_SCALE_SEGMENTS_MAX || (count > 0 && (!seg || !n || !factor))) return CSL_E_INVALID;
  ScaleArgs a;
  a.count = 0;
  long long blocks = 0;
  for (int j = 0; j < count; j++) {
    if (n[j] < 0 || (n[j] > 0 && !seg[j])) return CSL_E_INVALID;
    if (n[j] == 0) continue;
    a.seg[a.count] = seg[j], a.n[a.count] = n[j], a.factor[a.count] = factor[j];
    a.first_block[a.count] = (int)blocks;
    blocks += (n[j] + SCALE_CHUNK - 1) / SCALE_CHUNK;
    if (blocks > 0x7fffffffLL) return CSL_E_INVALID;
    a.count++;
  }
  if (a.count == 0) return CSL_OK;
  a.first_block[a.count] = (int)blocks;
  for (int j = a.count; j < CSL_SCALE_SEGMENTS_MAX; j++) a.seg[j] = nullptr, a.n[j] = 0, a.factor[j] = 1.f;
  hipLaunchKernelGGL(k_scale_segments, dim3((unsigned)blocks), dim3(DBLK), 0, (hipStream_t)stream, a);
  return done();
}

}  // extern "C"
