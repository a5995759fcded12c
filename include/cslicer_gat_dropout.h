/* cslicer_gat_dropout.h -- dropout for the attention model (csrc/aggregate.hip): feature dropout on the
 * output of every attention layer but the last, and attention dropout on the normalised coefficients of the edge softmax
 * (GAT as published drops both).  Two independent probabilities p_f and p_a, one seed, the step's counter; both masks are
 * pure functions of a counter exactly as in cslicer_dropout.h: Philox4x32-10, key = (seed mod 2^32, seed >> 32),
 * T = (uint32) floor((double) p * 4294967296.0), keep = w >= T, s = (float)(1.0 / (1.0 - (double) p)).  Nothing is
 * stored, there is no generator state.
 *
 * Feature dropout is cslicer_dropout.h's own map (csl_dropout_f32) on the layer's output AFTER its ELU, keyed by the
 * out-node's id v, the model layer k (0 = the deepest) and the column c over all H * D columns:
 *   ctr = (c >> 2, v, k, t mod 2^32), word c & 3;   y = keep ? act(n / s + b) * s_f : 0.
 * The backward is the same map on the incoming gradient, THEN the layer's own ELU' -- which needs the undropped output
 * (out > 0 ? 1 : out + 1), so a layer keeps `out` and hands `y` on; dropping in place would lose the kept negative
 * entries' derivative.  The feature table is never dropped.
 *
 * Attention dropout acts on alpha_h(u -> v), head h, SOURCE NODE ID u, DESTINATION NODE ID v, layer k, step t:
 *   ctr = (u, v, 0x80000000 | (h >> 2) << 8 | k, t mod 2^32), word h & 3;   kappa = keep ? s_a : 0.
 * The high bit of the third word keeps this counter space disjoint from the feature mask's, whose third word is a layer
 * number below CSL_MAX_LAYERS; k takes the low 8 bits, the head quad the bits above them (0 <= k < 256, H <= 2^24).
 * In the split-parallel (m, s, n) form of cslicer_aggr.h only the NUMERATOR is dropped:
 *   n[h, :] = sum_e kappa_e p_e z[u_e, h, :],   s = sum_e p_e and the stabiliser m as without dropout,
 * so n / s = sum_e kappa_e alpha_e z[u_e] whatever the number of parts, and the partial states of several parts still
 * merge by the log-sum-exp code that merges them today.  A row whose edges are all dropped has n = 0: its output is
 * act(bias).  Backward:  g_z[u] += kappa_e p_e g_n,   g_logit_e = (g_s + kappa_e <g_n, z_u>) p_e lrelu'.
 * The key is the pair of NODE IDS, not the edge's position: the mask is the same in the by-destination and the
 * by-source kernels, on any number of parts and under any partition -- and two sampled copies of the same edge (u, v)
 * (sampling with replacement) share one draw. */
#ifndef CSLICER_GAT_DROPOUT_H
#define CSLICER_GAT_DROPOUT_H

#include <stdint.h>

#include "cslicer_aggr.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The four aggregation entry points of cslicer_aggr.h with attention dropout: csl_gat_fwd_f32, csl_gat_bwd_f32,
 * csl_gat_bwd_t_f32 and csl_gat_bwd_t_fused_f32 argument for argument (same layouts, same zeroing contracts, the same
 * dispatch inside), then
 *   src_ids[n_src]   node id of every source row (the slice's in_nodes),
 *   dst_ids[n_rows]  node id of every destination row (the slice's out_nodes),
 *   p_a in (0, 1) (p_a == 0 is the caller's "call the parent"), seed, layer (0 <= layer < 256), step.
 * Refused before any HIP call (CSL_E_INVALID): p_a outside (0, 1), layer outside [0, 256), null src_ids or dst_ids
 * where there are rows, and whatever the parent refuses.  By source, the self entries (r < 0) are skipped and rows
 * [n_src, n_pad) of g_z are zeroed as in the parent.  csl_gat_drop_bwd_t_fused_f32 takes scratch of
 * csl_gat_bwd_t_fused_scratch floats and runs the parent's second stage over the destinations unchanged. */
int csl_gat_drop_fwd_f32(const int32_t* indptr, const int32_t* indices, int64_t n_rows, const float* el, const float* er,
                         const float* z, int32_t H, int32_t D, float slope, float* m_out, float* s_out, float* n_out,
                         const int32_t* src_ids, const int32_t* dst_ids, float p_a, int64_t seed, int32_t layer,
                         int64_t step, void* stream);

int csl_gat_drop_bwd_f32(const int32_t* indptr, const int32_t* indices, int64_t n_rows, const float* el, const float* er,
                         const float* z, int32_t H, int32_t D, float slope, const float* m_in, const float* g_s,
                         const float* g_n, float* g_el, float* g_er, float* g_z, const int32_t* src_ids,
                         const int32_t* dst_ids, float p_a, int64_t seed, int32_t layer, int64_t step, void* stream);

int csl_gat_drop_bwd_t_f32(const int32_t* t_indptr, const int32_t* t_indices, int64_t n_src, int64_t n_pad,
                           const float* el, const float* er, const float* z, int32_t H, int32_t D, float slope,
                           const float* m_in, const float* g_s, const float* g_n, float* g_el, float* g_er, float* g_z,
                           const int32_t* src_ids, const int32_t* dst_ids, float p_a, int64_t seed, int32_t layer,
                           int64_t step, void* stream);

int csl_gat_drop_bwd_t_fused_f32(const int32_t* t_indptr, const int32_t* t_indices, int64_t n_src, int64_t n_pad,
                                 const float* el, const float* er_out, const float* z, int32_t H, int32_t D, float slope,
                                 const float* m_in, const float* g_s, const float* g_n, const float* attn_l,
                                 const float* attn_r, const int32_t* self_ids_in, int64_t n_out, float* g_er_out,
                                 float* g_z, float* g_attn_l, float* g_attn_r, float* scratch, const int32_t* src_ids,
                                 const int32_t* dst_ids, float p_a, int64_t seed, int32_t layer, int64_t step,
                                 void* stream);

/* The layer's epilogue (csl_gat_finish_fwd_f32 / csl_gat_finish_bwd_f32 of cslicer_aggr.h) with feature dropout.
 * Forward: out[r] = act(n / s + bias) as the parent writes it (the layer keeps it for ELU') AND y[r] = the dropped out[r],
 * keyed by out_ids[r], in one pass: one more store, no more load.  y has out's layout [n, H*D]; it may be the first n rows
 * of a row-padded buffer, whose other rows are not touched.  Backward: the parent with the mask applied to g as it is
 * loaded; g_n, g_s, g_bias and scratch (csl_gat_finish_bwd_scratch floats) as the parent's.  By construction the pair is,
 * bit for bit, the parent followed (forward) or preceded (backward, on g) by csl_dropout_f32.  Refused before any HIP
 * call: p_f outside (0, 1), null out_ids or y with rows, and what the parent refuses. */
int csl_gat_finish_drop_fwd_f32(const float* n_in, const float* s_in, const float* bias, int64_t n, int32_t H, int32_t D,
                                int32_t elu, float* out, float* y, const int32_t* out_ids, float p_f, int64_t seed,
                                int32_t layer, int64_t step, void* stream);

int csl_gat_finish_drop_bwd_f32(const float* g, int64_t ldg, const float* out, const float* n_in, const float* s_in,
                                int64_t n, int32_t H, int32_t D, int32_t elu, float* g_n, float* g_s, float* g_bias,
                                float* scratch, const int32_t* out_ids, float p_f, int64_t seed, int32_t layer,
                                int64_t step, void* stream);

#ifdef __cplusplus
}
#endif
#endif
