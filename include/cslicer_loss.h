/* cslicer_loss.h -- the single-label loss with its options: class-weighted, label-smoothed softmax cross-entropy, forward
 * and backward in one pass, and the native GraphSAGE steps with that loss (csrc/loss.hip, csrc/sage_step.hip).
 *
 * Per row with logits z[0..C), label y, class weights w[0..C) (class_weight == NULL: all 1) and smoothing eps in [0, 1):
 *   q_c  = w_c * ((1 - eps) * [c == y] + eps / C),      Q = sum_c q_c
 *   m = max_c z_c,  s = sum_c exp(z_c - m),  p_c = exp(z_c - m) / s
 *   loss of the row = scale * sum_c q_c * ((m - z_c) + log s)      (every term >= 0: nothing cancels)
 *   grad[r, c]      = scale * (p_c * Q - q_c)
 * which is scale * torch.nn.functional.cross_entropy(z, y, weight=w, label_smoothing=eps, reduction="sum").  `scale` is the
 * caller's, 1 / seeds of the whole minibatch in the trainers: torch's SUM over the seeds divided by their count, NOT
 * torch's weighted "mean", which divides by sum_r w[y_r].  A class with q_c == 0 adds nothing to the loss whatever its
 * logit: weight 0 with eps == 0 masks a class (no loss, a zero gradient row for the rows that carry it).
 * A label outside [0, C) is never used as an index: that row's loss and its gradient row are NaN (csl_softmax_ce_f32's
 * rule), every other row is unaffected. */
#ifndef CSLICER_LOSS_H
#define CSLICER_LOSS_H

#include <stdint.h>

#include "cslicer_aggr.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The twins of csl_softmax_ce_f32 / csl_softmax_ce_partial_f32 (cslicer_aggr.h), same contract: logits [n, C] (row stride
 * ldl), label of row r = labels[rowmap ? rowmap[ids[r]] : ids[r]] (int64 labels, int32 node ids), grad [n, C] (row stride
 * ldgr), class_weight [C] float32 on the device or NULL.
 *   csl_softmax_ce_w_f32: *loss = the sum of the rows' losses; scratch: csl_softmax_ce_scratch(n) floats.
 *   csl_softmax_ce_w_partial_f32: grad rows [n, n_pad) are zeroed (the padding of the GEMM operand the gradient becomes);
 *     blocks = ceil(n_pad / 4); loss_partial[blocks]: the loss of each block's four rows; col_partial (optional, C <= 256
 *     only) [blocks][C]: each block's column sums of the gradient, the bias gradient's first stage.
 * 1 <= C <= 4096.  Refused before any HIP call (CSL_E_INVALID): n < 0, n_pad < n, C outside [1, 4096], label_smoothing
 * outside [0, 1) or NaN, col_partial with C > 256, a leading dimension below its width, and where there are rows a null
 * logits, ids, labels, grad, scratch or loss_partial; a null loss always.  One wave per row, four rows per block, the
 * partial layout of csl_softmax_ce_partial_f32; Q is summed per wave in a fixed order (deterministic) from the fp32 q_c the
 * gradient subtracts, so a row of one class (C == 1) has a gradient of exactly 0. */
int csl_softmax_ce_w_f32(const float* logits, int64_t ldl, int64_t n, int32_t C, const int32_t* ids, const int32_t* rowmap,
                         const int64_t* labels, const float* class_weight, float label_smoothing, float scale, float* loss,
                         float* grad, int64_t ldgr, float* scratch, void* stream);
int csl_softmax_ce_w_partial_f32(const float* logits, int64_t ldl, int64_t n, int64_t n_pad, int32_t C, const int32_t* ids,
                                 const int32_t* rowmap, const int64_t* labels, const float* class_weight,
                                 float label_smoothing, float scale, float* grad, int64_t ldgr, float* loss_partial,
                                 float* col_partial, void* stream);

/* csl_sage_fwd_bwd_dropout (cslicer_dropout.h) with the loss above in place of the plain cross-entropy: class_weight
 * (device, [dims[n_layers]], or NULL) and label_smoothing follow `labels`; the launch sequence, the workspace
 * (csl_sage_fwd_bwd_workspace) and every other kernel of the step are the same.  p == 0 with out_ids == NULL: no dropout
 * (kind 0: a float32 table, else CSL_FEAT_F16 / CSL_FEAT_BF16).  A refusal names the argument in csl_sage_last_error. */
int csl_sage_fwd_bwd_ce(int32_t n_layers, const int32_t* dims, const csl_sage_slice* slices, const float* const* weights,
                        const float* const* biases, const void* feat, int32_t kind, int64_t ldf, const int32_t* feat_rows,
                        const int32_t* seed_ids, const int64_t* labels, const float* class_weight, float label_smoothing,
                        float scale, int64_t row_pad, int32_t n_slabs, float* grads, float* loss, float* workspace,
                        int64_t workspace_floats, const int32_t* const* out_ids, float p, int64_t seed, int64_t step,
                        void* stream);

/* csl_sage_rank_fwd_bwd_x16 (cslicer_feat16.h; kind 0: a float32 table) with the loss above: the same exchanges, the same
 * workspace (csl_sage_rank_workspace).  No dropout: the rank sequencer has none. */
int csl_sage_rank_fwd_bwd_ce(int32_t n_layers, const int32_t* dims, const csl_sage_rank_slice* slices,
                             const float* const* weights, const float* const* biases, const void* feat, int32_t kind,
                             int64_t ldf, const int32_t* feat_rows, const int32_t* seed_ids, const int32_t* label_rows,
                             const int64_t* labels, const float* class_weight, float label_smoothing, float scale,
                             int64_t row_pad, int32_t n_slabs, csl_exchange_fn exchange, csl_exchange_wait_fn wait,
                             void* user, float* grads, float* loss, float* workspace, int64_t workspace_floats,
                             void* stream);

#ifdef __cplusplus
}
#endif
#endif
