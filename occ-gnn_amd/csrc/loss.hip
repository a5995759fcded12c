// loss.hip -- the single-label loss with its options behind the C ABI (cslicer_loss.h): class-weighted,
// label-smoothed softmax cross-entropy, forward, gradient and block partials in one pass -- k_softmax_ce (aggregate.hip)
// with a target distribution q in place of the one-hot row.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "cslicer_loss.h"
#include "dev_common.h"

namespace {

constexpr int BLK = 256;
constexpr int RPB = BLK / 64;   // rows per block: one wave each (the block count the step's Layout is laid out for)
constexpr int CW_CMAX = 256;    // widest row whose per-block column sums fit the LDS tile below (k_softmax_ce's SM_CMAX)
constexpr int CW_CLASSES = 4096;

// One wave per row, RPB rows per block, as k_softmax_ce: the step's partial layout (ceil(n_pad / 4) blocks) is fixed, and
// at its sizes (10^3 rows of 40-170 classes) the pass is one short launch.  Lane j walks columns j, j + 64, ... three
// times (max; sum of exponentials, and with smoothing the sum of the targets; loss terms and gradient): a row is at most
// 16 KB and the second and third walk hit the cache, the weights (<= 16 KB, read by every row) stay there.
//   q_c = w_c ((1 - eps) [c == y] + eps / C),   Q = sum_c q_c
//   loss = scale sum_c q_c ((m - z_c) + log s),  grad_c = scale (p_c Q - q_c)
// Q is the fp32 sum of the very q_c the gradient subtracts (w_c scaled, not w_c: the weights' sum times eps / C plus the
// label's term rounds differently), so a row whose softmax is one class -- C == 1 -- has the gradient 0 it should have,
// not a rounding of Q against q.  Without smoothing q is w_y at the label and 0 elsewhere: Q = w_y, nothing to sum.
// (m - z_c) + log s >= 0 term by term: a difference of two logits is exact up to its own rounding, so the loss keeps its
// relative accuracy at any offset of the row (k_softmax_ce's finding), and a sum of non-negative terms does not cancel.
// A class with q_c == 0 is skipped in the loss: a masked class adds nothing whatever its logit.
__global__ __launch_bounds__(BLK) void k_softmax_ce_w(const float* __restrict__ logits, long long ldl, long long n,
                                                      long long n_pad, int C, const int* __restrict__ ids,
                                                      const int* __restrict__ rowmap, const long long* __restrict__ labels,
                                                      const float* __restrict__ cw, float eps, float scale,
                                                      float* __restrict__ partial, float* __restrict__ grad,
                                                      long long ldgr, float* __restrict__ colpart) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const long long r = (long long)blockIdx.x * RPB + w;
  __shared__ float s_l[RPB];
  __shared__ float s_c[RPB][CW_CMAX];
  float mine = 0.f;
  if (r < n) {
    const float* z = logits + r * ldl;
    float m = -__builtin_inff();
    for (int c = lane; c < C; c += 64) m = fmaxf(m, z[c]);
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    const long long node = ids[r];
    const long long lab = labels[rowmap ? (long long)rowmap[node] : node];
    // a label outside [0, C) (a broken label file) is never used as an index: the row's loss and its gradient row are NaN
    const bool ok = lab >= 0 && lab < C;
    const float on = 1.0f - eps, off = eps / (float)C;
    // sum of the exponentials and, where smoothing spreads mass over every class, of the targets: strided partials, then
    // the xor tree -- one fixed order per (C, lane), the same in every wave
    const bool spread = eps > 0.f;
    float s = 0.f, qsum = 0.f;
    for (int c = lane; c < C; c += 64) {
      s += expf(z[c] - m);
      if (spread) qsum += (cw ? cw[c] : 1.0f) * ((c == lab ? on : 0.f) + off);
    }
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o), qsum += __shfl_xor(qsum, o);
    const float Q = spread ? qsum : (ok && cw ? cw[lab] : 1.0f);
    const float inv = 1.0f / s, logs = logf(s);
    float acc = 0.f;
    for (int c = lane; c < C; c += 64) {
      const float zc = z[c];
      const float q = (cw ? cw[c] : 1.0f) * ((c == lab ? on : 0.f) + off);
      const float gv = ok ? scale * (expf(zc - m) * inv * Q - q) : NAN;
      grad[r * ldgr + c] = gv;
      if (colpart) s_c[w][c] = gv;
      if (q != 0.f) acc += q * ((m - zc) + logs);
    }
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
    mine = ok ? scale * acc : NAN;
  } else if (r < n_pad) {
    // padding rows of the GEMM operand the gradient becomes
    for (int c = lane; c < C; c += 64) grad[r * ldgr + c] = 0.f;
  }
  if (colpart && r >= n)
    for (int c = lane; c < C; c += 64) s_c[w][c] = 0.f;
  if (lane == 0) s_l[w] = mine;
  __syncthreads();
  if (threadIdx.x == 0) partial[blockIdx.x] = s_l[0] + s_l[1] + s_l[2] + s_l[3];
  // the block's column sums of the gradient (the bias gradient's first stage)
  if (colpart)
    for (int c = threadIdx.x; c < C; c += BLK)
      colpart[(long long)blockIdx.x * C + c] = (s_c[0][c] + s_c[1][c]) + (s_c[2][c] + s_c[3][c]);
}

bool shape_ok(int64_t n, int64_t n_pad, int32_t C, float eps) {
  return n >= 0 && n_pad >= n && C >= 1 && C <= CW_CLASSES && eps >= 0.f && eps < 1.f &&   // (a NaN compares false)
         (n_pad + RPB - 1) / RPB <= 0x7fffffffLL;
}

}  // namespace

extern "C" {

int csl_softmax_ce_w_f32(const float* logits, int64_t ldl, int64_t n, int32_t C, const int32_t* ids, const int32_t* rowmap,
                         const int64_t* labels, const float* class_weight, float label_smoothing, float scale, float* loss,
                         float* grad, int64_t ldgr, float* scratch, void* stream) {
  if (!shape_ok(n, n, C, label_smoothing) || !loss) return CSL_E_INVALID;
  const long long blocks = (n + RPB - 1) / RPB;
  if (blocks > 0) {
    if (!logits || !ids || !labels || !grad || !scratch || ldl < C || ldgr < C) return CSL_E_INVALID;
    hipLaunchKernelGGL(k_softmax_ce_w, dim3((unsigned)blocks), dim3(BLK), 0, (hipStream_t)stream, logits, (long long)ldl,
                       (long long)n, (long long)n, (int)C, ids, rowmap, (const long long*)labels, class_weight,
                       label_smoothing, scale, scratch, grad, (long long)ldgr, (float*)nullptr);
    if (done() != CSL_OK) return CSL_E_HIP;
  }
  // the blocks' losses -> *loss (zero blocks: 0)
  const float* src[1] = {scratch};
  const int64_t nblk[1] = {blocks};
  const int32_t h[1] = {1};
  float* dst[1] = {loss};
  return csl_reduce_multi_f32(1, src, nblk, h, dst, stream);
}

int csl_softmax_ce_w_partial_f32(const float* logits, int64_t ldl, int64_t n, int64_t n_pad, int32_t C, const int32_t* ids,
                                 const int32_t* rowmap, const int64_t* labels, const float* class_weight,
                                 float label_smoothing, float scale, float* grad, int64_t ldgr, float* loss_partial,
                                 float* col_partial, void* stream) {
  if (!shape_ok(n, n_pad, C, label_smoothing) || (col_partial && C > CW_CMAX)) return CSL_E_INVALID;
  const long long blocks = (n_pad + RPB - 1) / RPB;
  if (blocks == 0) return CSL_OK;   // no rows, no padding: nothing to launch
  if (!grad || !loss_partial || ldgr < C || (n > 0 && (!logits || !ids || !labels || ldl < C))) return CSL_E_INVALID;
  hipLaunchKernelGGL(k_softmax_ce_w, dim3((unsigned)blocks), dim3(BLK), 0, (hipStream_t)stream, logits, (long long)ldl,
                     (long long)n, (long long)n_pad, (int)C, ids, rowmap, (const long long*)labels, class_weight,
                     label_smoothing, scale, loss_partial, grad, (long long)ldgr, col_partial);
  return done();
}

}  // extern "C"
