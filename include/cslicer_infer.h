/* cslicer_infer.h -- C ABI of full-neighbour, layer-wise inference (csrc/infer.hip).  Part of libcslicer_hip.so.
 *
 * The trained model applied with EVERY neighbour instead of a sample, one layer at a time over all nodes (the
 * `inference()` of DGL-style trainers; the reference evaluates this way, python/no_cache_multi_gpu.py:24-40).  The caller
 * (cslicer/infer.py) uploads the graph's NEIGHBOUR CSR: the int32 CSR with self loops removed (a self loop does not
 * count as a neighbour, duplicate edges count with multiplicity), so that a row's length is its degree.
 *
 * Work list.  Full rows are power-law: one row of 10^4 edges walked by one wave would set a kernel's time.  The caller
 * builds, once per graph (on the host, in numpy: a few vectorised passes over indptr, no device round trip), a work list
 * of ITEMS, int32 x 4 each:
 *     {row, pos, e0, part}
 * row: the CSR row; pos: the output position of the row; e0: the first edge of the item; the item's edges are
 * [e0, min(e0 + CSL_INFER_SEG, indptr[row + 1])).  A row of at most CSL_INFER_SEG edges is one item with part = -1 and
 * is finished by the wave that sums it.  A longer row (a hub) is cut into CSL_INFER_SEG-edge items with consecutive
 * part numbers; their partial results go to `partial`, and one HUB entry per hub row, int32 x 4:
 *     {row, pos, part_first, n_parts}
 * makes a second pass add the partials in part order and finish the row.  No float atomics anywhere: every output is
 * bitwise reproducible from call to call.
 *
 * A call covers the items and hubs it is given (a chunk of positions): out row = pos - pos0, partial row = part - part0.
 * All pointers are DEVICE pointers, `stream` a hipStream_t; fp32, row offsets are 64-bit.  Returns CSL_OK or
 * CSL_E_INVALID (arguments checked before anything is launched) / CSL_E_HIP (cslicer_hip.h).
 */
#ifndef CSLICER_INFER_H
#define CSLICER_INFER_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CSL_INFER_SEG 512

/* CSL_INFER_SEG: the edges of one work item */
int32_t csl_infer_seg(void);

/* GraphSAGE layer (DistSageConv) over full rows, deg[v] = indptr[v + 1] - indptr[v], mean over zero rows = 0:
 *   proj == 0, aggregate first:  out[k, 0:W) = x[v, 0:W),  out[k, W:2W) = mean_u x[u, 0:W)        (the Linear's operand)
 *   proj != 0, project first:    out[k, 0:W) = act(x[v, 0:W) + mean_u x[u, W:2W) + bias)
 *                                (x = h . [W_self; W_neigh]^T, [N, 2W]; act = ReLU if relu; bias may be NULL)
 * k = pos - pos0.  W % 4 == 0; ldx, ldo multiples of 4 (ldx >= 2W for proj, ldo >= 2W for !proj); x, out, partial
 * 16-byte aligned.  partial: [parts in this call, W] floats (NULL when there are no hubs). */
int csl_infer_sage_f32(const int32_t* indptr, const int32_t* indices, const int32_t* items, int64_t n_items,
                       const int32_t* hubs, int64_t n_hubs, int64_t pos0, int64_t part0, const float* x, int64_t ldx,
                       int32_t W, int32_t proj, const float* bias, int32_t relu, float* partial, float* out, int64_t ldo,
                       void* stream);

/* GAT layer (DistGATConv) over full rows from z [N, H*D] (dense), el / er [N, H] (csl_gat_logits_fwd_f32):
 *   score(u -> v, h) = LeakyReLU(el[u, h] + er[v, h]; slope), softmax over v's neighbours (no self term),
 *   n[v, h] = sum_u softmax * z[u, h],  a row without neighbours: n = 0.
 *   last == 0: out[k, h*D + j] = ELU(n[v, h, j] + bias[h*D + j])              (heads concatenated), ldo % 4 == 0
 *   last != 0: out[k, j] = mean_h (n[v, h, j] + bias[h*D + j])  for j < n_cls (head mean, class slice), any ldo
 * Hub rows: each item writes its partial softmax state (m, s, n), merged in part order with the log-sum-exp rescale.
 * D % 4 == 0; H * D <= 4096 for last != 0 (the head mean stages a row in LDS), H * D <= 2^24 otherwise; z, out, partial
 * 16-byte aligned.  partial: [parts in this call, csl_infer_gat_partial_ld(H, D)]
 * floats. */
int64_t csl_infer_gat_partial_ld(int32_t H, int32_t D);
int csl_infer_gat_f32(const int32_t* indptr, const int32_t* indices, const int32_t* items, int64_t n_items,
                      const int32_t* hubs, int64_t n_hubs, int64_t pos0, int64_t part0, const float* z, const float* el,
                      const float* er, int32_t H, int32_t D, float slope, const float* bias, int32_t last, int32_t n_cls,
                      float* partial, float* out, int64_t ldo, void* stream);

/* Evaluation head over logits [n, C] (row stride ld) and labels [n] (int64):
 *   pred[k] = argmax_j logits[k, j] (ties: the lowest j, as torch.argmax),
 *   loss_row[k] = logsumexp_j logits[k, j] - logits[k, labels[k]]  (NaN for a label outside [0, C)),
 *   *loss_sum = sum_k loss_row[k] (float64, fixed order),  *correct = #{k : pred[k] == labels[k]}.
 * pred, loss_row: [n]; loss_sum, correct: one device element each (written, also for n == 0). */
int csl_infer_eval_f32(const float* logits, int64_t ld, int64_t n, int32_t C, const int64_t* labels, int64_t* pred,
                       float* loss_row, double* loss_sum, int64_t* correct, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* CSLICER_INFER_H */
