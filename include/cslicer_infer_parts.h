/* cslicer_infer_parts.h -- C ABI of full-neighbour inference split over the parts of the graph (csrc/infer_parts.hip).
 * Part of libcslicer_hip.so.  The same layers as cslicer_infer.h, on ranks that each hold only the rows of the nodes
 * they own (cslicer/infer.py, full_inference_parts).
 *
 * A layer is cut where the training step cuts it: every rank sums, for each destination v, the neighbours of v that it
 * owns (a PARTIAL), the partials travel to the owner of v, and the owner merges them in rank order and finishes the row.
 *   GraphSAGE  partial S_q(v) = sum of y[u] over the neighbours u of v owned by q (no division, no self term);
 *              mean(v) = (S_0(v) + ... + S_{P-1}(v)) / max(deg v, 1), absent terms skipped, added from zero.
 *   GAT        partial = the online-softmax state (m, s, n) of v over q's neighbours of v, er[v] sent by the owner;
 *              the owner merges at most P states with the log-sum-exp rule of the hub merge of cslicer_infer.h.
 *
 * Each rank's LOCAL-SOURCE SUB-CSR holds one row per destination that has at least one neighbour it owns; its indices
 * are LOCAL rows (the source's row in the rank's own tables).  Its work list has the layout of cslicer_infer.h: items
 * {row, pos, e0, part} of at most CSL_INFER_SEG edges (row = sub-CSR row, pos = send row), hubs {row, pos, part_first,
 * n_parts}; the partials of a hub's items are merged in part order.  A call covers a slice of the list:
 * send row = pos - pos0, partial row = part - part0.
 *
 * The owner's MERGE LIST of a destination is P int32 row indices into the received buffer, one per rank in rank order,
 * -1 where that rank sent nothing.  dst records (GraphSAGE) are int32 x 2: {self row in x, full neighbour degree}.
 *
 * With one part the results are bitwise those of csl_infer_sage_f32 / csl_infer_gat_f32: a row's edges are summed in
 * the same order, and a merge of one partial into the zero state is exact.  No float atomics: every result is bitwise
 * reproducible.  fp32, float4 columns, 64-bit row offsets.  All pointers are DEVICE pointers, `stream` a hipStream_t.
 * Returns CSL_OK, or CSL_E_INVALID (arguments checked before anything is launched) / CSL_E_HIP (cslicer_hip.h).
 */
#ifndef CSLICER_INFER_PARTS_H
#define CSLICER_INFER_PARTS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* GraphSAGE partial sums: send[pos - pos0, 0:W) = sum_e y[indices[e], 0:W) over the item's edges (row stride ldy).
 * pack: sub-CSR rows per wave (1, 2 or 4; fewer where 64 / pack lanes cannot hold the width's lane groups).  W % 4 == 0,
 * ldy % 4 == 0, ldy >= W; y, send, partial 16-byte aligned; send: [rows, W] dense, partial: [parts in this call, W]
 * (NULL when there are no hubs). */
int csl_infer_sage_part_f32(const int32_t* indptr, const int32_t* indices, const int32_t* items, int64_t n_items,
                            const int32_t* hubs, int64_t n_hubs, int64_t pos0, int64_t part0, const float* y, int64_t ldy,
                            int32_t W, int32_t pack, float* partial, float* send, void* stream);

/* GraphSAGE merge of n destinations: mean = (sum of recv[lists[i, p]] over p in rank order) / max(deg, 1), then as
 * csl_infer_sage_f32 with self row x[dst[i].self]:
 *   proj == 0:  out[i, 0:W) = x[self, 0:W),  out[i, W:2W) = mean                      (the Linear's operand)
 *   proj != 0:  out[i, 0:W) = act(x[self, 0:W) + mean + bias)
 * recv: [rows, W] dense; lists: int32 [n, P]; dst: int32 [n, 2].  W, ldx, ldo multiples of 4, ldx >= W,
 * ldo >= (proj ? W : 2W). */
int csl_infer_sage_merge_f32(const int32_t* dst, const int32_t* lists, int64_t n, int32_t P, const float* recv,
                             const float* x, int64_t ldx, int32_t W, int32_t proj, const float* bias, int32_t relu,
                             float* out, int64_t ldo, void* stream);

/* GAT partial states: per item the online-softmax state of its row over its edges, from z [n_own, H*D] (dense),
 * el [n_own, H] of the sources and er_rows [send rows in this call, H] (row pos - pos0: the destination's er, received
 * from its owner).  send / partial rows have csl_infer_gat_partial_ld(H, D) floats: n at [0, H*D), m at H*D + h,
 * s at H*D + H + h.  D % 4 == 0, H * D <= 2^24; z, send, partial 16-byte aligned. */
int csl_infer_gat_part_f32(const int32_t* indptr, const int32_t* indices, const int32_t* items, int64_t n_items,
                           const int32_t* hubs, int64_t n_hubs, int64_t pos0, int64_t part0, const float* z,
                           const float* el, const float* er_rows, int32_t H, int32_t D, float slope, int32_t pack,
                           float* partial, float* send, void* stream);

/* GAT merge of n destinations: the states recv[lists[i, p]] merged in rank order into the zero state, then as
 * csl_infer_gat_f32:  last == 0: out[i, h*D + j] = ELU(n / s + bias)  (ldo % 4 == 0, ldo >= H*D)
 *                     last != 0: out[i, j] = mean_h (n / s + bias) for j < n_cls  (H * D <= 4096) */
int csl_infer_gat_merge_f32(const int32_t* lists, int64_t n, int32_t P, const float* recv, int32_t H, int32_t D,
                            const float* bias, int32_t last, int32_t n_cls, float* out, int64_t ldo, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* CSLICER_INFER_PARTS_H */
