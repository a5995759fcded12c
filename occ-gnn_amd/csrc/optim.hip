// optim.hip -- the optimizer step with weight decay, global-norm gradient clipping and the non-finite guard behind the C
// ABI (cslicer_optim.h).  k_adamw is k_adam (aggregate.hip) with a prologue per element: both walk
// AdamArgs' chunks and run adam_update (adam_dev.h).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "adam_dev.h"
#include "cslicer_optim.h"
#include "dev_common.h"

namespace {

constexpr int BLK = 256;
constexpr int NORM_BLOCKS = BLK;   // most blocks (= float64 partials) of the norm pass: one per thread of an update block

struct AdamwArgs {
  float decay[ADAM_MAX];     // per tensor: wd (coupled), or the factor 1 - lr wd (decoupled); read where decay_mask says so
  unsigned decay_mask;       // bit j: tensor j has wd > 0
  int decoupled;
  int nparts;                // float64 partials of the norm pass (CLIP only)
  float max_norm;
  const double* partial;
  float* grad_norm;
  int* skipped;
};

// the block's sum of its 256 threads' values, the same bits in every thread: a butterfly within each wave (a + b and
// b + a are the same float64), then the four waves' sums in one order
__device__ __forceinline__ double block_sum(double x, double* s_w) {
  for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);
  if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = x;
  __syncthreads();
  return (s_w[0] + s_w[1]) + (s_w[2] + s_w[3]);
}

// First stage of the norm: block b sums g^2 in float64 over chunks b, b + gridDim.x, ... of the update's chunk layout;
// a thread takes elements threadIdx.x, + 256, ... of a chunk in that order.  partial[b] depends on (count, numel) and the
// gradients alone.  An Inf or NaN gradient makes its partial, and so the norm, Inf or NaN: that is the guard's signal.
__global__ __launch_bounds__(BLK) void k_grad_sqsum(AdamArgs a, double* __restrict__ partial) {
  __shared__ double s_w[BLK / 64];
  const long long chunks = a.first_block[a.count];
  double acc = 0.0;
  for (long long c = blockIdx.x; c < chunks; c += gridDim.x) {
    const int t = adam_tensor_of(a, c);
    const long long base = (c - a.first_block[t]) * ADAM_CHUNK;
    const float* __restrict__ g = a.g[t];
    for (long long i = base + threadIdx.x; i < base + ADAM_CHUNK && i < a.n[t]; i += BLK) {
      const double gi = (double)g[i];
      acc += gi * gi;
    }
  }
  const double s = block_sum(acc, s_w);
  if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// The update: k_adam's walk (one block per chunk).  CLIP: every block sums the nparts <= 256 partials itself, thread i
// holding partial[i], in block_sum's fixed order, so that all blocks form the same n and the same c; a norm that is not
// finite ends the block before it has written anything.  Block 0 reports the norm and counts the skipped step.
template <bool CLIP>
__global__ __launch_bounds__(BLK) void k_adamw(AdamArgs a, AdamwArgs x, float b1, float b2, float step_size,
                                                float inv_sqrt_bc2, float eps) {
  float c = 1.f;
  if constexpr (CLIP) {
    __shared__ double s_w[BLK / 64];
    const double n = sqrt(block_sum((int)threadIdx.x < x.nparts ? x.partial[threadIdx.x] : 0.0, s_w));
    const bool finite = fabs(n) <= 1.7976931348623157e308;   // false for Inf and NaN
    if (blockIdx.x == 0 && threadIdx.x == 0) {
      if (x.grad_norm) *x.grad_norm = (float)n;
      if (!finite && x.skipped) *x.skipped = *x.skipped + 1;
    }
    if (!finite) return;
    c = (float)fmin(1.0, (double)x.max_norm / (n + 1e-6));
  }
  const int t = adam_tensor_of(a, (long long)blockIdx.x);
  const long long base = ((long long)blockIdx.x - a.first_block[t]) * ADAM_CHUNK;
  float* __restrict__ p = a.p[t];
  const float* __restrict__ g = a.g[t];
  float* __restrict__ m = a.m[t];
  float* __restrict__ v = a.v[t];
  const bool decay = (x.decay_mask >> t) & 1u;
  const float d = x.decay[t];
  for (long long i = base + threadIdx.x; i < base + ADAM_CHUNK && i < a.n[t]; i += BLK) {
    float gi = g[i], pi = p[i];
    if constexpr (CLIP) gi *= c;
    if (decay) {
      if (x.decoupled) pi *= d;
      else gi += d * pi;
    }
    adam_update(pi, gi, m[i], v[i], b1, b2, step_size, inv_sqrt_bc2, eps);
    p[i] = pi;
  }
}

// chunks of ADAM_CHUNK elements over the tensors, or -1 for sizes the kernels do not take
long long chunks_of(int32_t count, const int64_t* numel) {
  if (count < 0 || count > ADAM_MAX || (count > 0 && !numel)) return -1;
  long long chunks = 0;
  for (int t = 0; t < count; t++) {
    if (numel[t] < 0) return -1;
    chunks += (numel[t] + ADAM_CHUNK - 1) / ADAM_CHUNK;
    if (chunks > 0x7fffffffLL) return -1;
  }
  return chunks;
}

}  // namespace

extern "C" {

int64_t csl_adamw_scratch(int32_t count, const int64_t* numel) {
  const long long chunks = chunks_of(count, numel);
  if (chunks < 0) return CSL_E_INVALID;
  return (int64_t)sizeof(double) * (chunks < NORM_BLOCKS ? chunks : NORM_BLOCKS);
}

int csl_adamw_f32(int32_t count, float* const* params, const float* const* grads, float* const* exp_avg,
                  float* const* exp_avg_sq, const int64_t* numel, const float* weight_decay, int32_t decoupled,
                  float max_norm, float lr, float beta1, float beta2, float eps, int64_t step, float* grad_norm,
                  int32_t* skipped, void* scratch, void* stream) {
  if (count < 0 || count > ADAM_MAX || step < 1 || max_norm != max_norm) return CSL_E_INVALID;
  if (count == 0) return CSL_OK;
  if (!params || !grads || !exp_avg || !exp_avg_sq || !numel) return CSL_E_INVALID;
  const long long chunks = chunks_of(count, numel);
  if (chunks < 0) return CSL_E_INVALID;
  AdamArgs a;
  AdamwArgs x;
  x.decay_mask = 0;
  x.decoupled = decoupled != 0;
  long long at = 0;
  for (int t = 0; t < count; t++) {
    if (numel[t] > 0 && (!params[t] || !grads[t] || !exp_avg[t] || !exp_avg_sq[t])) return CSL_E_INVALID;
    const float wd = weight_decay ? weight_decay[t] : 0.f;
    if (!(wd >= 0.f)) return CSL_E_INVALID;   // negative or NaN
    a.p[t] = params[t];
    a.g[t] = grads[t];
    a.m[t] = exp_avg[t];
    a.v[t] = exp_avg_sq[t];
    a.n[t] = numel[t];
    a.first_block[t] = at;
    at += (numel[t] + ADAM_CHUNK - 1) / ADAM_CHUNK;
    x.decay[t] = x.decoupled ? (float)(1.0 - (double)lr * (double)wd) : wd;
    if (wd > 0.f) x.decay_mask |= 1u << t;
  }
  a.first_block[count] = chunks;
  a.count = count;
  const bool clip = max_norm > 0.f;
  x.nparts = clip ? (int)(chunks < NORM_BLOCKS ? chunks : NORM_BLOCKS) : 0;
  if (x.nparts > 0 && (!scratch || (reinterpret_cast<uintptr_t>(scratch) & 7u))) return CSL_E_INVALID;
  if (chunks == 0) return CSL_OK;
  x.max_norm = max_norm;
  x.partial = static_cast<const double*>(scratch);
  x.grad_norm = grad_norm;
  x.skipped = skipped;
  const double bc1 = 1.0 - pow((double)beta1, (double)step), bc2 = 1.0 - pow((double)beta2, (double)step);
  const float step_size = (float)((double)lr / bc1), inv_sqrt_bc2 = (float)(1.0 / sqrt(bc2));
  hipStream_t st = (hipStream_t)stream;
  if (clip) {
    hipLaunchKernelGGL(k_grad_sqsum, dim3((unsigned)x.nparts), dim3(BLK), 0, st, a, static_cast<double*>(scratch));
    hipLaunchKernelGGL(k_adamw<true>, dim3((unsigned)chunks), dim3(BLK), 0, st, a, x, beta1, beta2, step_size,
                       inv_sqrt_bc2, eps);
  } else {
    hipLaunchKernelGGL(k_adamw<false>, dim3((unsigned)chunks), dim3(BLK), 0, st, a, x, beta1, beta2, step_size,
                       inv_sqrt_bc2, eps);
  }
  return done();
}

}  // extern "C"
