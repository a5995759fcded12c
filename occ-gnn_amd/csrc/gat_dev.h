// gat_dev.h -- what gat_dropout.hip takes from aggregate.hip (private to csrc/): the grid rules of the by-source attention
// backward and of the epilogue's backward, and the launches of their second stages, so that the dropped twins run them as
// they are.
#ifndef CSLICER_GAT_DEV_H
#define CSLICER_GAT_DEV_H

#include <cstdint>

namespace gatx {

// source (or destination) rows per workgroup of k_gat_bwd_t2 / k_gat_logits_bwd_dst (csl_gat_bwd_t_fused_scratch's rule)
long long t_rows(long long n);

// k_gat_logits_bwd_dst on `stream`: the er half of the logits' backward over the n_out destination rows, part_r one row of
// H * D partial sums per workgroup of rows_per_block rows.  No argument check: the caller's.
void logits_bwd_dst(const float* z, const float* attn_r, const int32_t* self_ids_in, const float* g_er_out, int64_t n_out,
                    int32_t H, int32_t D, float* g_z, float* part_r, long long rows_per_block, void* stream);

// rows per workgroup of k_gat_finish_bwd (csl_gat_finish_bwd_scratch's rule), and its second stage: k_colsum_finish adds
// the `blocks` rows of per-block column sums in `partial` into g_bias[0:C)
long long finish_rows(long long n);
void colsum_finish(const float* partial, long long blocks, int32_t C, float* g_bias, void* stream);

}  // namespace gatx
#endif
