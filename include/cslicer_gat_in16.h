/* cslicer_gat_in16.h -- C ABI of the attention model's input layer (aggregate-then-project, csrc/gat_input.hip) over a
 * 16-bit feature table (float16 or bfloat16 rows resident in HBM).  Part of libcslicer_hip.so.
 *
 * The layer reads the table in its two edge passes: the forward (attention logits and the weighted sum of raw rows) and
 * the backward, which reads the same rows again for dalpha and the sums behind g_vl / g_vr.  So, unlike the GraphSAGE
 * readers of cslicer_feat16.h, this layer has a 16-bit BACKWARD as well.  Each entry point here is the twin of the
 * csl_gat_in_*_f32 entry point of cslicer_aggr.h whose table argument `x` holds 16-bit elements of kind `kind`
 * (CSL_FEAT_F16 / CSL_FEAT_BF16, cslicer_feat16.h): `const void* x, int32_t kind, int64_t ldx` stand where the twin has
 * `const float* x, int64_t ldx`, every other argument and the return values are the twin's.  A lane loads four elements
 * (8 bytes) and upcasts them in registers (both conversions to float32 are exact); v_l, v_r, alpha, agg, dagg and every
 * partial sum stay float32, and everything behind the upcast -- the order of every sum, the softmax, the sign bit kept in
 * alpha, the NaN of an over-long row, the two-stage sums, the projection and its gradients -- is the twin's: the results
 * are BITWISE those of the twin on the table upcast to float32.
 *
 * As in cslicer_feat16.h, strides are in ELEMENTS of the table, and every entry point returns CSL_E_INVALID before any
 * HIP call, whatever the row count, for an unknown kind, a null table, a row stride that is not a multiple of 4 or is
 * below F, and a table base that is not 8-byte aligned (the float32 twins want 16 bytes), and for whatever its twin
 * refuses.  Scratch sizes are the twins': csl_gat_in_bwd_scratch, csl_gat_in_layer_fwd_scratch,
 * csl_gat_in_layer_bwd_scratch.
 */
#ifndef CSLICER_GAT_IN16_H
#define CSLICER_GAT_IN16_H

#include <stdint.h>

#include "cslicer_aggr.h"
#include "cslicer_feat16.h"

#ifdef __cplusplus
extern "C" {
#endif

/* twin of csl_gat_in_fwd_f32 */
int csl_gat_in_fwd_x16(const int32_t* indptr, const int32_t* indices, const int32_t* self_ids, const int32_t* rowmap,
                       const void* x, int32_t kind, int64_t ldx, int32_t F, const float* vl, const float* vr, int32_t H,
                       float slope, int64_t n_out, int64_t n_edges, int32_t max_deg, float* agg, float* alpha, void* stream);

/* twin of csl_gat_in_bwd_f32 (alpha: what csl_gat_in_fwd_x16 or the layer's forward wrote for the same max_deg) */
int csl_gat_in_bwd_x16(const int32_t* indptr, const int32_t* indices, const int32_t* self_ids, const int32_t* rowmap,
                       const void* x, int32_t kind, int64_t ldx, int32_t F, const float* alpha, const float* dagg,
                       int64_t ld_r, int64_t ld_h, int32_t H, float slope, int64_t n_out, int64_t n_edges, int32_t max_deg,
                       float* g_vl, float* g_vr, float* scratch, void* stream);

/* twins of csl_gat_in_layer_fwd_f32 / csl_gat_in_layer_bwd_f32: only the edge pass of each direction reads the table */
int csl_gat_in_layer_fwd_x16(const int32_t* indptr, const int32_t* indices, const int32_t* self_ids, const int32_t* rowmap,
                             const void* x, int32_t kind, int64_t ldx, int32_t F, const float* W, const float* attn_l,
                             const float* attn_r, const float* bias, int32_t H, int32_t D, float slope, int32_t elu,
                             int64_t n_out, int64_t n_edges, int32_t max_deg, float* agg, float* alpha, float* out, int64_t ldo,
                             float* scratch, void* stream);

int csl_gat_in_layer_bwd_x16(const int32_t* indptr, const int32_t* indices, const int32_t* self_ids, const int32_t* rowmap,
                             const void* x, int32_t kind, int64_t ldx, int32_t F, const float* W, const float* attn_l,
                             const float* attn_r, int32_t H, int32_t D, float slope, int32_t elu, int64_t n_out,
                             int64_t n_edges, int32_t max_deg, const float* agg, const float* alpha, const float* out,
                             int64_t ldo, const float* g, int64_t ldg, float* gg, float* dagg, float* gW, float* g_al,
                             float* g_ar, float* g_bias, float* scratch, void* stream);

#ifdef __cplusplus
}
#endif
#endif
