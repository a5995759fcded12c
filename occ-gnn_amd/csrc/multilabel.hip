// multilabel.hip -- multi-label node classification behind the C ABI (cslicer_multilabel.h): the fused
// sigmoid + binary cross-entropy pass of a training step (forward, gradient, block partials: the twin of k_softmax_ce in
// aggregate.hip) and the micro-F1 evaluation head.  Labels are packed bits, 32 classes per int32 word.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "cslicer_multilabel.h"
#include "dev_common.h"

namespace {

constexpr int BLK = 256;
constexpr int RPB = BLK / 64;   // rows per block: one wave each (the block count the step's Layout is laid out for)
constexpr int ML_CMAX = 256;    // widest row whose per-block column sums fit the LDS tile below (k_softmax_ce's SM_CMAX)
constexpr int ML_CLASSES = 4096;

// l = max(z, 0) - (y ? z : 0) + log1p(exp(-|z|)) and sigma(z), from one exponential: e <= 1, so nothing overflows, and
// the first two terms are one of z, 0 and -z, exact.  z >= 0 ? 1 / (1 + e) : e / (1 + e) keeps sigma's relative accuracy
// on both tails.
__device__ __forceinline__ void bce_elem(float z, bool y, float& l, float& sig) {
  const float e = expf(-fabsf(z));
  const float r = 1.0f / (1.0f + e);
  l = (fmaxf(z, 0.f) - (y ? z : 0.f)) + log1pf(e);
  sig = z >= 0.f ? r : e * r;
}

// One wave per row, RPB rows per block, as k_softmax_ce: the step's partial layout (ceil(n_pad / 4) blocks) is fixed, and
// at its sizes (10^3 rows of 40-170 classes) the pass is one short launch whose time is its launch and the latency of one
// row walk, not its lanes' use -- a row of 5 classes leaves 59 lanes idle for the length of ONE element's arithmetic.  Lane
// j walks columns j, j + 64, ...: the two halves of a wave read one label word each per 64 columns (a broadcast load), so
// a row's words are read once per 32 columns.
__global__ __launch_bounds__(BLK) void k_sigmoid_bce(const float* __restrict__ logits, long long ldl, long long n,
                                                     long long n_pad, int C, const int* __restrict__ ids,
                                                     const int* __restrict__ rowmap, const int* __restrict__ words,
                                                     long long ldw, float scale, float* __restrict__ partial,
                                                     float* __restrict__ grad, long long ldgr, float* __restrict__ colpart) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const long long r = (long long)blockIdx.x * RPB + w;
  __shared__ float s_l[RPB];
  __shared__ float s_c[RPB][ML_CMAX];
  float mine = 0.f;
  if (r < n) {
    const float* z = logits + r * ldl;
    const long long node = ids[r];
    const int* lw = words + (rowmap ? (long long)rowmap[node] : node) * ldw;
    float* g = grad + r * ldgr;
    float sum = 0.f;
    int bad = 0;
    for (int c = lane; c < C; c += 64) {
      const float zc = z[c];
      const bool y = ((unsigned)lw[c >> 5] >> (c & 31)) & 1u;
      float l, sig;
      bce_elem(zc, y, l, sig);
      bad |= !(fabsf(zc) <= 3.402823466e+38f);   // Inf or NaN
      sum += l;
      const float gv = scale * (sig - (y ? 1.f : 0.f));
      g[c] = gv;
      if (colpart) s_c[w][c] = gv;
    }
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o), bad |= __shfl_xor(bad, o);
    mine = scale * sum;
    if (bad) {
      // a non-finite logit: the row's loss and its WHOLE gradient row are NaN (an infinite logit alone would leave a
      // finite gradient and an infinite or finite loss), so the step shows up as a NaN loss; every lane rewrites what
      // it wrote itself
      mine = NAN;
      for (int c = lane; c < C; c += 64) {
        g[c] = NAN;
        if (colpart) s_c[w][c] = NAN;
      }
    }
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

// Evaluation, one wave per row: the 64 lanes' predictions of columns 64 j .. 64 j + 63 are one ballot = two words of the
// row's prediction; tp / fp / fn of the row are population counts of those words against the label words (lane 0).
__global__ __launch_bounds__(BLK) void k_eval_multilabel_rows(const float* __restrict__ logits, long long ld, long long n,
                                                              int C, const int* __restrict__ words, long long ldw,
                                                              int* __restrict__ pred, float* __restrict__ loss_row) {
  const int lane = threadIdx.x & 63;
  const long long r = (long long)blockIdx.x * RPB + (threadIdx.x >> 6);
  if (r >= n) return;
  const int W = (C + 31) >> 5;
  const float* z = logits + r * ld;
  const int* lw = words + r * ldw;
  float sum = 0.f;
  for (int c0 = 0; c0 < C; c0 += 64) {
    const int c = c0 + lane;
    bool pos = false;
    if (c < C) {
      const float zc = z[c];
      const bool y = ((unsigned)lw[c >> 5] >> (c & 31)) & 1u;
      float l, sig;
      bce_elem(zc, y, l, sig);
      sum += l;
      pos = zc > 0.f;
    }
    const unsigned long long m = __ballot(pos);
    if (lane == 0) {
      pred[r * W + (c0 >> 5)] = (int)(unsigned)m;
      if ((c0 >> 5) + 1 < W) pred[r * W + (c0 >> 5) + 1] = (int)(unsigned)(m >> 32);
    }
  }
  for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
  if (lane == 0) loss_row[r] = sum;
}

// *loss_sum in float64 and {tp, fp, fn} in a fixed order by ONE block (k_infer_eval_sum's shape): thread t takes rows t,
// t + 256, ..., then a tree.  The last word's bits at and above C are masked out of the labels (the predictions have none).
__global__ __launch_bounds__(BLK) void k_eval_multilabel_sum(const int* __restrict__ pred, const int* __restrict__ words,
                                                             long long ldw, const float* __restrict__ loss_row, long long n,
                                                             int C, double* __restrict__ loss_sum,
                                                             long long* __restrict__ counts) {
  __shared__ double sl[BLK];
  __shared__ long long sc[3][BLK];
  const int W = (C + 31) >> 5;
  const unsigned last = (C & 31) ? (1u << (C & 31)) - 1u : 0xffffffffu;
  double l = 0.0;
  long long tp = 0, fp = 0, fn = 0;
  for (long long k = threadIdx.x; k < n; k += BLK) {
    l += (double)loss_row[k];
    for (int j = 0; j < W; j++) {
      const unsigned p = (unsigned)pred[k * W + j];
      const unsigned y = (unsigned)words[k * ldw + j] & (j + 1 == W ? last : 0xffffffffu);
      tp += __popc(p & y), fp += __popc(p & ~y), fn += __popc(~p & y);
    }
  }
  sl[threadIdx.x] = l;
  sc[0][threadIdx.x] = tp, sc[1][threadIdx.x] = fp, sc[2][threadIdx.x] = fn;
  __syncthreads();
  for (int w = BLK / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) {
      sl[threadIdx.x] += sl[threadIdx.x + w];
      for (int j = 0; j < 3; j++) sc[j][threadIdx.x] += sc[j][threadIdx.x + w];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) *loss_sum = sl[0], counts[0] = sc[0][0], counts[1] = sc[1][0], counts[2] = sc[2][0];
}

bool shape_ok(int64_t n, int64_t n_pad, int32_t C) {
  return n >= 0 && n_pad >= n && C >= 1 && C <= ML_CLASSES && (n_pad + RPB - 1) / RPB <= 0x7fffffffLL;
}

}  // namespace

extern "C" {

int64_t csl_sigmoid_bce_scratch(int64_t n) { return (n + RPB - 1) / RPB; }

int csl_sigmoid_bce_f32(const float* logits, int64_t ldl, int64_t n, int32_t C, const int32_t* ids, const int32_t* rowmap,
                        const int32_t* label_words, int64_t ldw, float scale, float* loss, float* grad, int64_t ldgr,
                        float* scratch, void* stream) {
  if (!shape_ok(n, n, C) || !loss) return CSL_E_INVALID;
  const long long blocks = (n + RPB - 1) / RPB;
  if (blocks > 0) {
    if (!logits || !ids || !label_words || !grad || !scratch || ldl < C || ldgr < C || ldw < (C + 31) / 32)
      return CSL_E_INVALID;
    hipLaunchKernelGGL(k_sigmoid_bce, dim3((unsigned)blocks), dim3(BLK), 0, (hipStream_t)stream, logits, (long long)ldl,
                       (long long)n, (long long)n, (int)C, ids, rowmap, label_words, (long long)ldw, scale, scratch, grad,
                       (long long)ldgr, (float*)nullptr);
    if (done() != CSL_OK) return CSL_E_HIP;
  }
  // the blocks' losses -> *loss (zero blocks: 0)
  const float* src[1] = {scratch};
  const int64_t nblk[1] = {blocks};
  const int32_t h[1] = {1};
  float* dst[1] = {loss};
  return csl_reduce_multi_f32(1, src, nblk, h, dst, stream);
}

int csl_sigmoid_bce_partial_f32(const float* logits, int64_t ldl, int64_t n, int64_t n_pad, int32_t C, const int32_t* ids,
                                const int32_t* rowmap, const int32_t* label_words, int64_t ldw, float scale, float* grad,
                                int64_t ldgr, float* loss_partial, float* col_partial, void* stream) {
  if (!shape_ok(n, n_pad, C) || (col_partial && C > ML_CMAX)) return CSL_E_INVALID;
  const long long blocks = (n_pad + RPB - 1) / RPB;
  if (blocks == 0) return CSL_OK;   // no rows, no padding: nothing to launch
  if (!grad || !loss_partial || ldgr < C || (n > 0 && (!logits || !ids || !label_words || ldl < C || ldw < (C + 31) / 32)))
    return CSL_E_INVALID;
  hipLaunchKernelGGL(k_sigmoid_bce, dim3((unsigned)blocks), dim3(BLK), 0, (hipStream_t)stream, logits, (long long)ldl,
                     (long long)n, (long long)n_pad, (int)C, ids, rowmap, label_words, (long long)ldw, scale, loss_partial,
                     grad, (long long)ldgr, col_partial);
  return done();
}

int csl_infer_eval_multilabel_f32(const float* logits, int64_t ld, int64_t n, int32_t C, const int32_t* label_words,
                                  int64_t ldw, int32_t* pred_words, float* loss_row, double* loss_sum, int64_t* counts,
                                  void* stream) {
  if (!shape_ok(n, n, C) || ld < C || ldw < (C + 31) / 32 || !loss_sum || !counts) return CSL_E_INVALID;
  if (n > 0 && (!logits || !label_words || !pred_words || !loss_row)) return CSL_E_INVALID;
  hipStream_t st = (hipStream_t)stream;
  if (n > 0)
    hipLaunchKernelGGL(k_eval_multilabel_rows, dim3((unsigned)((n + RPB - 1) / RPB)), dim3(BLK), 0, st, logits,
                       (long long)ld, (long long)n, (int)C, label_words, (long long)ldw, pred_words, loss_row);
  hipLaunchKernelGGL(k_eval_multilabel_sum, dim3(1), dim3(BLK), 0, st, pred_words, label_words, (long long)ldw, loss_row,
                     (long long)n, (int)C, loss_sum, reinterpret_cast<long long*>(counts));
  return done();
}

}  // extern "C"
