/* cslicer_infer16.h -- C ABI of full-neighbour inference over a 16-bit feature table (float16 or bfloat16 rows resident
 * in HBM).  Part of libcslicer_hip.so; kernels in csrc/infer.hip and csrc/infer_parts.hip.
 *
 * Only the FIRST layer of an inference call reads the feature table; every later layer reads float32 activations.  The
 * first layer reads the table in one of two ways, and each has its entry points here:
 *
 *   a gather kernel reads table rows (GraphSAGE aggregate-first): csl_infer_sage_x16, csl_infer_sage_part_x16 and
 *   csl_infer_sage_merge_x16 are the twins of the float32 entry points of cslicer_infer.h / cslicer_infer_parts.h whose
 *   table argument holds 16-bit elements of kind `kind` (CSL_FEAT_F16 / CSL_FEAT_BF16, cslicer_feat16.h).  A lane loads
 *   four elements (8 bytes) and upcasts them in registers (both conversions to float32 are exact); the order of every
 *   sum, the hub split, the partial buffers, the outputs and the divide are the twin's: the results are BITWISE those of
 *   the twin on the table upcast to float32.
 *
 *   the library GEMM reads the table (GraphSAGE project-first, the attention model's projections): the caller upcasts
 *   each chunk of rows into one reusable float32 buffer with csl_upcast_rows_x16 and hands that buffer to the GEMM.
 *
 * As in cslicer_feat16.h, `kind` comes directly after the table pointer, strides are in ELEMENTS of the table, and every
 * entry point returns CSL_E_INVALID before any HIP call for an unknown kind, a null table, a row stride that is not a
 * multiple of 4, a table base that is not 8-byte aligned, and for whatever its float32 twin refuses.  All other
 * arguments, and the return values, are those of the twin.
 */
#ifndef CSLICER_INFER16_H
#define CSLICER_INFER16_H

#include <stdint.h>

#include "cslicer_feat16.h"
#include "cslicer_infer.h"
#include "cslicer_infer_parts.h"

#ifdef __cplusplus
extern "C" {
#endif

/* twin of csl_infer_sage_f32 for proj == 0 (the aggregate-first form: out row = [x[v] | mean x[u]]); proj != 0 is
 * CSL_E_INVALID, the projected operand is always float32 */
int csl_infer_sage_x16(const int32_t* indptr, const int32_t* indices, const int32_t* items, int64_t n_items,
                       const int32_t* hubs, int64_t n_hubs, int64_t pos0, int64_t part0, const void* x, int32_t kind,
                       int64_t ldx, int32_t W, int32_t proj, const float* bias, int32_t relu, float* partial, float* out,
                       int64_t ldo, void* stream);

/* twin of csl_infer_sage_part_f32: y is the 16-bit table (partial and send stay float32) */
int csl_infer_sage_part_x16(const int32_t* indptr, const int32_t* indices, const int32_t* items, int64_t n_items,
                            const int32_t* hubs, int64_t n_hubs, int64_t pos0, int64_t part0, const void* y, int32_t kind,
                            int64_t ldy, int32_t W, int32_t pack, float* partial, float* send, void* stream);

/* twin of csl_infer_sage_merge_f32 for proj == 0: x (the self rows) is the 16-bit table, recv stays float32 */
int csl_infer_sage_merge_x16(const int32_t* dst, const int32_t* lists, int64_t n, int32_t P, const float* recv,
                             const void* x, int32_t kind, int64_t ldx, int32_t W, int32_t proj, const float* bias,
                             int32_t relu, float* out, int64_t ldo, void* stream);

/* dst[k, 0:H) = float32(src[k, 0:H)) for the n consecutive rows k of src (8-byte loads, 16-byte stores, no index array).
 * H % 4 == 0, lds >= H, ldd >= H, ldd % 4 == 0, dst 16-byte aligned; n == 0 is CSL_OK.  src may be a block of rows of a
 * table (src = table + r0 * lds), dst a column block of a wider or row-padded matrix. */
int csl_upcast_rows_x16(const void* src, int32_t kind, int64_t lds, int64_t n, float* dst, int64_t ldd, int32_t H,
                        void* stream);

#ifdef __cplusplus
}
#endif
#endif
