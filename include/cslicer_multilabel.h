/* cslicer_multilabel.h -- multi-label node classification (PPI, ogbn-proteins, Yelp, Amazon: a node carries a SET of
 * classes): the fused sigmoid + binary cross-entropy pass, the micro-F1 evaluation head and the native GraphSAGE step with
 * that loss (csrc/multilabel.hip, csrc/sage_step.hip).
 *
 * Labels are packed bits: W = ceil(C / 32) 32-bit words per node, class c = bit c % 32 of word c / 32, carried as int32.
 * No reader looks at a bit at or above C in the last word: whatever is there changes no output.
 *
 * Per element, with y in {0, 1} and e = exp(-|z|) (the overflow-free form; max(z, 0) - (y ? z : 0) is exact):
 *   l     = max(z, 0) - (y ? z : 0) + log1p(e)
 *   sigma = z >= 0 ? 1 / (1 + e) : e / (1 + e)
 *   grad  = scale * (sigma - y),      loss of a row = scale * sum_c l
 * A non-finite logit makes its row's loss and gradient row NaN and touches no other row. */
#ifndef CSLICER_MULTILABEL_H
#define CSLICER_MULTILABEL_H

#include <stdint.h>

#include "cslicer_aggr.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The twins of csl_softmax_ce_f32 / csl_softmax_ce_partial_f32 (cslicer_aggr.h), same contract: logits [n, C] (row stride
 * ldl), the label row of logits row r is label_words + ldw * (rowmap ? rowmap[ids[r]] : ids[r]) (ldw >= W words),
 * grad [n, C] (row stride ldgr).
 *   csl_sigmoid_bce_f32: *loss = the sum of the rows' losses; scratch: csl_sigmoid_bce_scratch(n) floats.
 *   csl_sigmoid_bce_partial_f32: grad rows [n, n_pad) are zeroed (the padding of the GEMM operand the gradient becomes);
 *     blocks = ceil(n_pad / 4); loss_partial[blocks]: the loss of each block's four rows; col_partial (optional, C <= 256
 *     only) [blocks][C]: each block's column sums of the gradient, the bias gradient's first stage.
 * 1 <= C <= 4096.  Refused before any HIP call (CSL_E_INVALID): n < 0, n_pad < n, C outside [1, 4096], col_partial with
 * C > 256, a leading dimension below its width, and where there are rows a null logits, ids, label_words, grad, scratch
 * or loss_partial; a null loss always.  One wave per row, four rows per block: plain loads and stores, the column sums
 * through the LDS tile csl_softmax_ce_partial_f32 uses, no scratch memory. */
int64_t csl_sigmoid_bce_scratch(int64_t n);
int csl_sigmoid_bce_f32(const float* logits, int64_t ldl, int64_t n, int32_t C, const int32_t* ids, const int32_t* rowmap,
                        const int32_t* label_words, int64_t ldw, float scale, float* loss, float* grad, int64_t ldgr,
                        float* scratch, void* stream);
int csl_sigmoid_bce_partial_f32(const float* logits, int64_t ldl, int64_t n, int64_t n_pad, int32_t C, const int32_t* ids,
                                const int32_t* rowmap, const int32_t* label_words, int64_t ldw, float scale, float* grad,
                                int64_t ldgr, float* loss_partial, float* col_partial, void* stream);

/* Evaluation head over logits [n, C] (row stride ld) and the packed labels of the same rows (row stride ldw >= W words):
 *   pred_words[k, w] (dense [n, W]): bit c % 32 of word c / 32 = logits[k, c] > 0 (a logit of exactly 0 predicts
 *     negative, NaN too), bits at and above C zero,
 *   loss_row[k] = sum_c l (unscaled),   *loss_sum = sum_k loss_row[k] (float64, fixed order),
 *   counts[3] (int64) = {tp, fp, fn} over all n * C elements.
 * pred_words: [n, W]; loss_row: [n]; loss_sum, counts: device elements, written also for n == 0.  1 <= C <= 4096. */
int csl_infer_eval_multilabel_f32(const float* logits, int64_t ld, int64_t n, int32_t C, const int32_t* label_words,
                                  int64_t ldw, int32_t* pred_words, float* loss_row, double* loss_sum, int64_t* counts,
                                  void* stream);

/* csl_sage_fwd_bwd_dropout (cslicer_dropout.h) with the sigmoid-BCE loss in place of the softmax cross-entropy: `labels`
 * becomes (label_words, ldw), indexed by the seeds' node ids; the launch sequence, the workspace
 * (csl_sage_fwd_bwd_workspace) and every other kernel of the step are the same.  p == 0 with out_ids == NULL: no dropout
 * (kind 0: a float32 table, else CSL_FEAT_F16 / CSL_FEAT_BF16). */
int csl_sage_fwd_bwd_multilabel(int32_t n_layers, const int32_t* dims, const csl_sage_slice* slices,
                                const float* const* weights, const float* const* biases, const void* feat, int32_t kind,
                                int64_t ldf, const int32_t* feat_rows, const int32_t* seed_ids, const int32_t* label_words,
                                int64_t ldw, float scale, int64_t row_pad, int32_t n_slabs, float* grads, float* loss,
                                float* workspace, int64_t workspace_floats, const int32_t* const* out_ids, float p,
                                int64_t seed, int64_t step, void* stream);

#ifdef __cplusplus
}
#endif
#endif
