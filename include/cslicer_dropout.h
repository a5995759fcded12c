/* cslicer_dropout.h -- dropout between the GraphSAGE layers (models/factory.py:41: x = dropout(activation(x))), with a
 * mask that is a pure function of a counter: no generator state, no stored mask (csrc/dropout.hip).
 *
 * Philox4x32-10 (multipliers 0xD2511F53 / 0xCD9E8D57, key increments 0x9E3779B9 / 0xBB67AE85; after each round the
 * words are (hi1^c1^k0, lo1, hi0^c3^k1, lo0)).  For the row of node id v (a non-negative int32 read as uint32), column
 * c, model layer k (the layer whose output is dropped; 0 = the deepest hop) and step t:
 *
 *   (w0, w1, w2, w3) = philox4x32_10(ctr = (c >> 2, v, k, t mod 2^32), key = (seed mod 2^32, (seed >> 32) mod 2^32))
 *   keep(v, c) = w[c & 3] >= T,   T = (uint32) floor((double) p * 4294967296.0)
 *   y = keep ? x * s : 0,         s = (float)(1.0 / (1.0 - (double) p))
 *
 * One multiplication and one rounding per element.  The map is linear in x: its backward is the same call on the
 * gradient.  The key is the NODE id, not the row position, so a node's mask is the same on one GPU, on any number of
 * parts and under any partition. */
#ifndef CSLICER_DROPOUT_H
#define CSLICER_DROPOUT_H

#include <stdint.h>

#include "cslicer_aggr.h"

#ifdef __cplusplus
extern "C" {
#endif

/* y[r, 0:H) = the map above of x[r, 0:H), r < n, keyed by ids[r] (ids == NULL: by r mod 2^32).  y may be x (in place).
 * H % 4 == 0, ldx / ldy >= H and multiples of 4, x and y 16-byte aligned, 0 < p < 1 (p == 0 is the caller's "no call").
 * Refused before any HIP call (CSL_E_INVALID): p outside (0, 1), n < 0, a width or leading dimension that breaks the
 * above, and for n > 0 a null or misaligned x or y.  One Philox call, one 16-byte load and one 16-byte store per lane. */
int csl_dropout_f32(const float* x, int64_t ldx, float* y, int64_t ldy, const int32_t* ids, int64_t n, int32_t H, float p,
                    int64_t seed, int32_t layer, int64_t step, void* stream);

/* seg[j][0:n[j]) *= factor[j] for count <= 2 * CSL_MAX_LAYERS segments in ONE launch (seg / n / factor are HOST
 * arrays): what brings the weight and bias gradients below a dropped layer to scale (see below). */
#define CSL_SCALE_SEGMENTS_MAX (2 * CSL_MAX_LAYERS)
int csl_scale_segments_f32(int32_t count, float* const* seg, const int64_t* n, const float* factor, void* stream);

/* csl_sage_fwd_bwd_f32 / csl_sage_fwd_bwd_x16 (kind 0: a float32 table, else CSL_FEAT_F16 / CSL_FEAT_BF16) with dropout
 * of probability p on the output of every layer but the last: after layer k's forward (k < L-1; the fused deepest layer
 * included) rows [0, n_out) of y_k are dropped IN PLACE, keyed by out_ids[k][r] (the layer's out-node list), layer k,
 * `step`.  y_k is stored after its ReLU and the backward's ReLU mask is y_k > 0, so the dropped y_k carries
 * relu' * mask by itself: no stored mask, no extra workspace (csl_sage_fwd_bwd_workspace, unchanged), no other kernel
 * changed.  The factor s the backward then lacks per dropped layer it crosses commutes with everything downstream (the
 * backward is linear in gy): after the step's last reduction gW_j and gb_j are multiplied by s^(L-1-j), j < L-1, in one
 * launch.  L == 1 has nothing to drop: the call is csl_sage_fwd_bwd_f32's. */
int csl_sage_fwd_bwd_dropout(int32_t n_layers, const int32_t* dims, const csl_sage_slice* slices,
                             const float* const* weights, const float* const* biases, const void* feat, int32_t kind,
                             int64_t ldf, const int32_t* feat_rows, const int32_t* seed_ids, const int64_t* labels,
                             float scale, int64_t row_pad, int32_t n_slabs, float* grads, float* loss, float* workspace,
                             int64_t workspace_floats, const int32_t* const* out_ids, float p, int64_t seed, int64_t step,
                             void* stream);

#ifdef __cplusplus
}
#endif
#endif
