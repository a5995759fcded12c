/* cslicer_smooth.h -- C ABI of one label-propagation step over full rows (csrc/smooth.hip).  Part of libcslicer_hip.so.
 *
 * Correct and Smooth (cslicer/smooth.py) iterates X <- clamp(alpha S X + (1 - alpha) X0, lo, hi) with
 * S = D^-1/2 A D^-1/2 over the NEIGHBOUR CSR of cslicer_infer.h (self loops removed, duplicates counted, deg[v] the length
 * of row v, dinv[v] = deg[v] > 0 ? 1 / sqrt(deg[v]) : 0).  The iterate travels PRE-SCALED, xs = dinv (.) X: the gather is
 * then a plain row sum (no 4-byte dinv[u] load per edge), and the row end writes the next step's operand itself.
 *
 * The work list (items, hubs, pos0, part0, partial) is the one of cslicer_infer.h, built by the same build_plan /
 * plan_chunks: a row longer than CSL_INFER_SEG edges is summed in parts by separate waves and finished by a hub pass
 * that adds the partials in part order.  No atomics: two calls with the same arguments give the same bits.
 */
#ifndef CSLICER_SMOOTH_H
#define CSLICER_SMOOTH_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* For the item row v at position k = pos - pos0 and every column j < W:
 *   acc = sum over the row's edges e of xs[indices[e], j]
 *   y   = alpha * dinv[v] * acc + (base ? beta * base[k, j] : 0)
 *   y   = y < lo ? lo : (y > hi ? hi : y)                    (a NaN stays a NaN)
 *   out[k, j] = y (if out)      out_s[k, j] = dinv[v] * y (if out_s)
 * xs: [N, ldx] indexed by graph row; base, out, out_s: indexed by position, row strides ldb, ldo, ldos; columns [W, ld)
 * of an output row are left untouched.  Rounding: alpha * dinv[v] once, times acc once, the base term one fused
 * multiply-add, dinv[v] * y once; the row sum in a fixed order.
 * W > 0, W % 4 == 0; ldx, and the ld of every non-null matrix, a multiple of 4 and >= W; every non-null matrix 16-byte
 * aligned; lo <= hi, neither a NaN; alpha, beta finite; neither output may be xs.  Without items and hubs the call
 * returns CSL_OK and launches nothing; with them dinv and xs must be there, and out or out_s (or both).
 * partial: [parts in this call, W] floats (NULL when there are no hubs).  All pointers are DEVICE pointers, `stream` a
 * hipStream_t.  Returns CSL_OK, CSL_E_INVALID (checked before any HIP call) or CSL_E_HIP (cslicer_hip.h). */
int csl_prop_f32(const int32_t* indptr, const int32_t* indices, const int32_t* items, int64_t n_items,
                 const int32_t* hubs, int64_t n_hubs, int64_t pos0, int64_t part0, const float* xs, int64_t ldx, int32_t W,
                 const float* dinv, float alpha, const float* base, int64_t ldb, float beta, float lo, float hi,
                 float* partial, float* out, int64_t ldo, float* out_s, int64_t ldos, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* CSLICER_SMOOTH_H */
