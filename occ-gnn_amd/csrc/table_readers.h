// table_readers.h -- the kernels' host paths that read the resident feature table in either form (private to csrc/).
//
// Each is the ONE implementation behind a csl_*_f32 entry point (kind 0: x is float32) and its csl_*_x16 twin
// (CSL_FEAT_F16 / CSL_FEAT_BF16, cslicer_feat16.h, cslicer_gat_in16.h), so the twin refuses what the float32 form refuses by construction;
// csrc/sage_step.hip calls them with the kind its caller gave.  Arguments are those of the _x16 entry points.  What still
// differs by kind, on purpose: a 16-bit table is checked first and whatever the row count is (kind, null, stride % 4,
// 8-byte base, ld < H); a float32 table is not looked at when there is nothing to do, and keeps its element-wise path
// for unaligned rows or H % 4 != 0 where it has one.
#ifndef CSLICER_TABLE_READERS_H
#define CSLICER_TABLE_READERS_H

#include <cstdint>

#include "feat_elem.h"

#define CSL_HIDDEN __attribute__((visibility("hidden")))

namespace rd {

// a 16-bit table no reader takes, whatever the row count (kind 0: nothing is said about a float32 table here)
inline bool table16_bad(const void* x, int32_t kind, int64_t ldx, int32_t H) {
  return kind != 0 && (!feat::table_ok(x, kind, ldx) || ldx < H);
}

// csrc/aggregate.hip
CSL_HIDDEN int spmm_sum_map(const int32_t* indptr, const int32_t* indices, const int32_t* rows, int64_t n_rows, const void* x,
                            int32_t kind, int64_t ldx, const int32_t* rowmap, float* out, int64_t ldo, int32_t H,
                            int32_t compact, void* stream);
CSL_HIDDEN int gather_rows(const void* src, int32_t kind, int64_t lds, const int32_t* idx, int64_t n, float* dst, int64_t ldd,
                           int32_t H, void* stream);
CSL_HIDDEN int sage_cat(const int32_t* indptr, const int32_t* indices, const int32_t* self_ids, const int32_t* owned,
                        const int32_t* deg, const int32_t* rowmap, const void* x, int32_t kind, int64_t ldx, const float* agg,
                        int64_t lda, int64_t n, int64_t n_pad, float* cat, int64_t ldc, int32_t H, int32_t relu_in,
                        void* stream);
// csrc/sage_mfma.hip
CSL_HIDDEN int sage_fwd_mfma(const int32_t* indptr, const int32_t* indices, const int32_t* self_ids, const int32_t* rowmap,
                             const void* x, int32_t kind, int64_t ldx, const float* W, int64_t ldw, const float* bias, int64_t n,
                             int64_t n_pad, int32_t H, int32_t out, int32_t relu_in, int32_t relu_out, float* cat, int64_t ldc,
                             float* y, int64_t ldy, float* wpack, void* stream);

// csrc/gat_input.hip: the two edge passes of the attention input layer (its layer sequencers call them with their kind)
CSL_HIDDEN int gat_in_fwd(const int32_t* indptr, const int32_t* indices, const int32_t* self_ids, const int32_t* rowmap,
                          const void* x, int32_t kind, int64_t ldx, int32_t F, const float* vl, const float* vr, int32_t H,
                          float slope, int64_t n_out, int64_t n_edges, int32_t max_deg, float* agg, float* alpha, void* stream);
CSL_HIDDEN int gat_in_bwd(const int32_t* indptr, const int32_t* indices, const int32_t* self_ids, const int32_t* rowmap,
                          const void* x, int32_t kind, int64_t ldx, int32_t F, const float* alpha, const float* dagg,
                          int64_t ld_r, int64_t ld_h, int32_t H, float slope, int64_t n_out, int64_t n_edges, int32_t max_deg,
                          float* g_vl, float* g_vr, float* scratch, void* stream);

}  // namespace rd
#endif
