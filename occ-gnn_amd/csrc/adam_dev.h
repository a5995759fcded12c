// adam_dev.h -- what the two optimizer kernels share (private to csrc/): k_adam (aggregate.hip, csl_adam_f32) and k_adamw
// (optim.hip, csl_adamw_f32) walk the same chunk layout and run the SAME per-element update, so that with no clipping
// and no decay the second is bitwise the first (tests/test_gpu_optim_edges.py holds them to it).
#ifndef CSLICER_ADAM_DEV_H
#define CSLICER_ADAM_DEV_H

#include <hip/hip_runtime.h>

namespace {

constexpr int ADAM_MAX = 24;
constexpr int ADAM_CHUNK = 1024;
struct AdamArgs {
  float* p[ADAM_MAX];
  const float* g[ADAM_MAX];
  float* m[ADAM_MAX];
  float* v[ADAM_MAX];
  long long first_block[ADAM_MAX + 1];  // blocks of ADAM_CHUNK elements, tensors back to back
  long long n[ADAM_MAX];
  int count;
};

// the tensor a chunk (a block of k_adam) belongs to; empty tensors share their successor's first chunk and are passed over
__device__ __forceinline__ int adam_tensor_of(const AdamArgs& a, long long chunk) {
  int t = 0;
  while (t + 1 < a.count && chunk >= a.first_block[t + 1]) t++;
  return t;
}

//   m = b1 m + (1-b1) g;  v = b2 v + (1-b2) g^2;  p -= (lr / (1-b1^t)) * m / (sqrt(v) / sqrt(1-b2^t) + eps)
__device__ __forceinline__ void adam_update(float& p, const float gi, float& m, float& v, float b1, float b2,
                                            float step_size, float inv_sqrt_bc2, float eps) {
  const float mi = b1 * m + (1.f - b1) * gi;
  const float vi = b2 * v + (1.f - b2) * gi * gi;
  m = mi;
  v = vi;
  p -= step_size * mi / (sqrtf(vi) * inv_sqrt_bc2 + eps);
}

}  // namespace
#endif
