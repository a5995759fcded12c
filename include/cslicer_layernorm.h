/* cslicer_layernorm.h -- layer normalisation between the GraphSAGE layers (SAGEConv's `norm`, applied to the layer's
 * result before the model's dropout(activation(x))), as two row-wise kernels (csrc/layernorm.hip) and the
 * native single-GPU step that runs them (csrc/sage_step.hip).  For a row z of width H (torch.nn.LayerNorm, biased variance):
 *
 *   mean = sum(z) / H                    var = sum((z - mean)^2) / H        (two passes: the mean, then the centred squares)
 *   rstd = 1 / sqrt(var + eps)           xhat = (z - mean) * rstd
 *   n    = gamma * xhat + beta           y = relu ? max(n, 0) : n
 *
 * and for the gradient dn w.r.t. n (the ReLU mask applied by the caller), a = gamma * dn:
 *
 *   dz     = rstd * (a - mean_row(a) - xhat * mean_row(a * xhat))
 *   dgamma = sum over rows of dn * xhat,   dbeta = sum over rows of dn   (the caller has it: the mask pass's column sums)
 *
 * A function of one row only: no cross-rank statistics, no running averages, the same numbers under any partition. */
#ifndef CSLICER_LAYERNORM_H
#define CSLICER_LAYERNORM_H

#include <stdint.h>

#include "cslicer_aggr.h"

#ifdef __cplusplus
extern "C" {
#endif

/* y[r, 0:H) = the map above of z[r, 0:H), r < n.  y may be z (in place).  xhat [n, ldh] and rstd [n] are stored for the
 * backward; both NULL: the forward-only form of inference (one of them NULL alone is refused).  H % 4 == 0; ldz / ldy /
 * ldh >= H and multiples of 4; z, y, xhat, gamma and beta 16-byte aligned; eps > 0.  Refused before any HIP call
 * (CSL_E_INVALID): anything that breaks the above, n < 0, and for n > 0 a null z, y, gamma or beta.
 * A row is walked by the power-of-two group of lanes that covers its H / 4 quads (a wave at the most) and stays in
 * registers between the passes up to H = 1024; wider rows are read again.  Reductions stay inside the lane group. */
int csl_layernorm_relu_fwd_f32(const float* z, int64_t ldz, const float* gamma, const float* beta, float eps, int64_t n,
                               int32_t H, float* y, int64_t ldy, float* xhat, int64_t ldh, float* rstd, int32_t relu,
                               void* stream);

/* floats of gpart and of bpart each: [blocks][H], blocks = csl_layernorm_bwd_scratch(n_pad, H) / H (0 for n_pad == 0);
 * CSL_E_INVALID for n_pad < 0 or a width the kernel refuses */
int64_t csl_layernorm_bwd_scratch(int64_t n_pad, int32_t H);

/* In place on dn [n_pad, ldd]: rows r < n become dz (above) from xhat [n, ldh], rstd [n] and gamma [H]; rows [n, n_pad) are
 * neither read nor written (the zeros they are stay).  gpart[b][0:H) / bpart[b][0:H) receive block b's column sums of
 * dn * xhat (first stage of dgamma) and of dz (first stage of the bias gradient of the layer whose result was normalised);
 * every block of the scratch is written, with zeros where it has no row below n.  Second stage: csl_reduce_multi_f32 over
 * the blocks -- two stages, no atomics, a fixed order.  Alignment and widths as for the forward; refused before any HIP
 * call: n < 0, n_pad < n, a bad width or leading dimension, for n_pad > 0 a null or misaligned gpart, bpart or gamma, for
 * n > 0 a null or misaligned dn or xhat or a null rstd. */
int csl_layernorm_bwd_f32(float* dn, int64_t ldd, const float* xhat, int64_t ldh, const float* rstd, const float* gamma,
                          int64_t n, int64_t n_pad, int32_t H, float* gpart, float* bpart, void* stream);

/* csl_sage_fwd_bwd_ce (cslicer_loss.h: table kind, class weights, label smoothing, dropout) with layer normalisation on the
 * result of every layer but the last, and optionally the multi-label loss (label_words != NULL: the packed words of
 * cslicer_multilabel.h in place of `labels`, class_weight / label_smoothing unused).  Forward, k < L-1: the layer's GEMM (or
 * the fused deepest layer) runs with its ReLU off, csl_layernorm_relu_fwd_f32 runs in place on y_k and stores xhat_k and
 * rstd_k in the workspace (csl_sage_fwd_bwd_norm_workspace: csl_sage_fwd_bwd_workspace plus those), dropout as before.
 * Backward: the gather by source of layer k+1 leaves mask * gradient in gy_k and its column sums are now dbeta_k;
 * csl_layernorm_bwd_f32 turns gy_k into dz in place and leaves the first stages of dgamma_k and gb_k.
 * gammas[k], betas[k]: [dims[k + 1]], k < L-1.  The flat gradient is W_0, b_0, ..., W_{L-1}, b_{L-1} followed by
 * gamma_0, beta_0, gamma_1, beta_1, ...; under dropout gamma_j and beta_j take W_j's factor s^(L-1-j).
 * L == 1 has nothing to normalise: the call is csl_sage_fwd_bwd_ce's (or csl_sage_fwd_bwd_multilabel's). */
int64_t csl_sage_fwd_bwd_norm_workspace(int32_t n_layers, const int32_t* dims, const csl_sage_slice* slices, int64_t row_pad,
                                        int32_t n_slabs);
int csl_sage_fwd_bwd_norm(int32_t n_layers, const int32_t* dims, const csl_sage_slice* slices, const float* const* weights,
                          const float* const* biases, const void* feat, int32_t kind, int64_t ldf, const int32_t* feat_rows,
                          const int32_t* seed_ids, const int64_t* labels, const float* class_weight, float label_smoothing,
                          float scale, int64_t row_pad, int32_t n_slabs, float* grads, float* loss, float* workspace,
                          int64_t workspace_floats, const int32_t* const* out_ids, float p, int64_t seed, int64_t step,
                          const int32_t* label_words, int64_t ldw, const float* const* gammas, const float* const* betas,
                          float eps, void* stream);

#ifdef __cplusplus
}
#endif
#endif
