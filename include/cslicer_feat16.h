/* cslicer_feat16.h -- C ABI of the readers of a 16-bit feature table (float16 or bfloat16 rows resident in HBM).
 * Part of libcslicer_hip.so; kernels in csrc/sage_mfma.hip, csrc/aggregate.hip, sequencers in csrc/sage_step.hip.
 *
 * The input layer takes no gradient, so of the GraphSAGE readers only the FORWARD ones have a 16-bit form (the attention
 * input layer reads the table in its backward too: its twins are in cslicer_gat_in16.h): each entry point here
 * is the twin of an fp32 entry point of cslicer_aggr.h whose table argument `x` / `feat` / `src` holds 16-bit elements
 * of kind `kind` instead of floats.  A row is upcast in registers (both conversions to float32 are exact) and everything
 * after the load -- the order of the sums, the operand kept for the weight gradient, the GEMMs, the backward -- is the
 * fp32 twin's: the results are BITWISE those of the twin on the table upcast to float32.
 *
 * Every entry point checks its arguments before any HIP call and returns CSL_E_INVALID for an unknown kind, a null
 * table, a row stride (in elements) that is not a multiple of 4, a table base that is not 8-byte aligned (a lane loads
 * four elements = 8 bytes at once), and for whatever its fp32 twin refuses.  Strides are in ELEMENTS of the table.
 * All other arguments, and the return values, are those of the twin (cslicer_aggr.h).
 */
#ifndef CSLICER_FEAT16_H
#define CSLICER_FEAT16_H

#include <stdint.h>

#include "cslicer_aggr.h"

#ifdef __cplusplus
extern "C" {
#endif

/* element kinds */
#define CSL_FEAT_F16 1  /* IEEE binary16 */
#define CSL_FEAT_BF16 2 /* bfloat16: the upper 16 bits of a float32 */

/* twin of csl_sage_fwd_mfma_f32 (same widths, same scratch: csl_sage_fwd_mfma_scratch) */
int csl_sage_fwd_mfma_x16(const int32_t* indptr, const int32_t* indices, const int32_t* self_ids, const int32_t* rowmap,
                          const void* x, int32_t kind, int64_t ldx, const float* W, int64_t ldw, const float* bias,
                          int64_t n, int64_t n_pad, int32_t H, int32_t out, int32_t relu_in, int32_t relu_out, float* cat,
                          int64_t ldc, float* y, int64_t ldy, float* wpack, void* stream);

/* twin of csl_sage_cat_f32: x is the 16-bit table (agg, the merged sums of the several-parts form, stays fp32) */
int csl_sage_cat_x16(const int32_t* indptr, const int32_t* indices, const int32_t* self_ids, const int32_t* owned,
                     const int32_t* deg, const int32_t* rowmap, const void* x, int32_t kind, int64_t ldx, const float* agg,
                     int64_t lda, int64_t n, int64_t n_pad, float* cat, int64_t ldc, int32_t H, int32_t relu_in,
                     void* stream);

/* twin of csl_spmm_sum_map_f32 */
int csl_spmm_sum_map_x16(const int32_t* indptr, const int32_t* indices, const int32_t* rows, int64_t n_rows, const void* x,
                         int32_t kind, int64_t ldx, const int32_t* rowmap, float* out, int64_t ldo, int32_t H,
                         int32_t compact, void* stream);

/* twin of csl_gather_rows_f32: dst[k, 0:H) = float32(src[idx[k], 0:H)) (a zero row for idx -1); dst may be a block of
 * a wider or row-padded matrix (ldd >= H) */
int csl_gather_rows_x16(const void* src, int32_t kind, int64_t lds, const int32_t* idx, int64_t n, float* dst, int64_t ldd,
                        int32_t H, void* stream);

/* twins of csl_sage_fwd_bwd_f32 / csl_sage_rank_fwd_bwd_f32 (same workspaces: csl_sage_fwd_bwd_workspace,
 * csl_sage_rank_workspace).  Only the deepest layer's forward differs: the fused kernel where the fp32 step runs it,
 * csl_sage_cat_x16 / csl_spmm_sum_map_x16 elsewhere; the rank step enters the same exchanges. */
int csl_sage_fwd_bwd_x16(int32_t n_layers, const int32_t* dims, const csl_sage_slice* slices, const float* const* weights,
                         const float* const* biases, const void* feat, int32_t kind, int64_t ldf, const int32_t* feat_rows,
                         const int32_t* seed_ids, const int64_t* labels, float scale, int64_t row_pad, int32_t n_slabs,
                         float* grads, float* loss, float* workspace, int64_t workspace_floats, void* stream);

int csl_sage_rank_fwd_bwd_x16(int32_t n_layers, const int32_t* dims, const csl_sage_rank_slice* slices,
                              const float* const* weights, const float* const* biases, const void* feat, int32_t kind,
                              int64_t ldf, const int32_t* feat_rows, const int32_t* seed_ids, const int32_t* label_rows,
                              const int64_t* labels, float scale, int64_t row_pad, int32_t n_slabs,
                              csl_exchange_fn exchange, csl_exchange_wait_fn wait, void* user, float* grads, float* loss,
                              float* workspace, int64_t workspace_floats, void* stream);

#ifdef __cplusplus
}
#endif
#endif
