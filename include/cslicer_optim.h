/* cslicer_optim.h -- the optimizer step with what a long run tunes: weight decay (decoupled, AdamW, or as an L2 term of
 * the gradient), clipping of the gradient's global norm, and a guard that skips the step when a gradient is not finite
 * (csrc/optim.hip).  csl_adam_f32 (cslicer_aggr.h) stays what the default trainer calls; with no clipping
 * and no decay csl_adamw_f32 gives bitwise its result -- both kernels run one per-element update (csrc/adam_dev.h).
 *
 * One step, float32 unless float64 is named, over `count` <= 24 tensors (params, grads, exp_avg, exp_avg_sq: HOST arrays
 * of device pointers, numel: HOST array; a tensor's start needs no more than float alignment):
 *   1. max_norm > 0 only: n = sqrt(sum g^2) over every tensor, the squares and their sum in float64 (a float32 square
 *      overflows at |g| = 1.8e19 and vanishes at 1e-23), in an order that depends on count and numel alone: no atomics,
 *      the same bits on every call.  *grad_norm = (float)n.
 *   2. c = min(1, max_norm / (n + 1e-6)) in float64, rounded to float32 (torch.nn.utils.clip_grad_norm_); without
 *      clipping c = 1 and no multiplication takes place.  max_norm = +inf never clips but runs 1 and 3.
 *   3. n not finite (a NaN or an Inf anywhere in any gradient): the step is SKIPPED on the device: no element of params,
 *      exp_avg, exp_avg_sq is written, and *skipped += 1 (one writer, in stream order).  The host is not told: the
 *      caller's step count `step` has advanced all the same, so after a skipped step the bias corrections run one step
 *      ahead of the moments (1 - beta^t is a little closer to 1 than the moments warrant; the effect fades as beta^t does).
 *   4. g1 = g c.  Tensor j with wd = weight_decay[j] > 0:  decoupled: p <- p (1 - lr wd) (the factor formed in float64 on
 *      the host, rounded once), g2 = g1;  coupled: g2 = g1 + wd p.  wd == 0: no decay arithmetic.
 *      Then csl_adam_f32's update on (p, g2, m, v):
 *        m = b1 m + (1-b1) g2;  v = b2 v + (1-b2) g2^2;  p -= (lr / (1-b1^t)) m / (sqrt(v) / sqrt(1-b2^t) + eps)
 *
 * Launches: the update kernel alone without clipping (as csl_adam_f32); with clipping one more in front of it, the
 * gradients' sums of squares: min(chunks, 256) blocks (chunks of 1,024 elements, tensors back to back as the update
 * walks them), block b takes chunks b, b + 256, ... and writes one float64 partial into `scratch`; every block of the
 * update kernel then sums the partials in one fixed order, so that all of them hold the same c.
 *
 * Refused before any HIP call (CSL_E_INVALID): count outside [0, 24], step < 1, a NaN max_norm, a null array, a negative
 * numel, a null tensor pointer of a non-empty tensor, a negative or NaN weight_decay[j], more than 2^31 - 1 chunks, and
 * with max_norm > 0 a scratch that is null (or not 8-byte aligned) where csl_adamw_scratch is above 0.  count == 0 or
 * only empty tensors: CSL_OK, nothing launched, nothing written. */
#ifndef CSLICER_OPTIM_H
#define CSLICER_OPTIM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* bytes of `scratch` a clipping step over these tensors needs (0: none, no element); CSL_E_INVALID for a count outside
 * [0, 24], a null numel with count > 0 or a negative numel */
int64_t csl_adamw_scratch(int32_t count, const int64_t* numel);

/* weight_decay: HOST array [count], or NULL = all 0.  decoupled: 1 AdamW, 0 the L2 term (torch.optim.Adam's
 * weight_decay).  max_norm <= 0: no clipping, no norm pass, no guard.  grad_norm (device, 1 float) and skipped (device,
 * 1 int32 counter) may be NULL; they are touched only when max_norm > 0. */
int csl_adamw_f32(int32_t count, float* const* params, const float* const* grads, float* const* exp_avg,
                  float* const* exp_avg_sq, const int64_t* numel, const float* weight_decay, int32_t decoupled,
                  float max_norm, float lr, float beta1, float beta2, float eps, int64_t step, float* grad_norm,
                  int32_t* skipped, void* scratch, void* stream);

#ifdef __cplusplus
}
#endif
#endif
