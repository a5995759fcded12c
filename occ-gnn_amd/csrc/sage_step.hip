// sage_step.hip -- forward, loss and backward of the GraphSAGE model for one minibatch as ONE call behind the C ABI: the
// sequence of this library's fused kernels and plain GEMMs that python/train.py:56-88 + python/layers/dist_sageconv.py:42-84
// amount to, on ONE part that holds every node (cslicer_aggr.h: csl_sage_fwd_bwd_f32, its _x16, _dropout, _multilabel, _ce
// and _norm forms) and on one RANK of the split-parallel job (csl_sage_rank_fwd_bwd_f32 / _x16 / _ce).  No kernels here, only
// sequencing.
//
// Why a native sequencer: the step is ~25 kernel launches and 8 GEMMs of 5-90 us each.  Issued from Python (one ctypes
// call or torch op each, an autograd graph around them) they cost 0.55-0.75 ms of host time per step, more than the
// 0.6 ms the GPU needs, and the rate then follows the host's speed (1.2-1.8 k minibatches/s from box to box).  Issued
// from here a step is ~0.15 ms of host time and the GPU sets the pace (a rank: the 2 L callbacks plus ~0.25 ms instead of
// ~1.2 ms of interpreter + autograd work, which is what bounds a rank once the GPU work is split N ways).
//
// ONE layout (Layout, lay_out) and ONE body (sage_step) serve both; the nine entry points check their own arguments and
// call it.  Per model layer k (deepest hop first; slice k = the engine's layer n_layers-1-k, graph mode):
//   forward   cat_k = [x[self] | mean_{CSR row} x[src]]       csl_sage_cat_f32 (k = 0 reads the resident feature table
//             y_k   = cat_k W_k^T + b_k (ReLU for k < L-1)     through the slice's in_nodes)      + csl_gemm_f32
//             (k = 0, widths allowing: both as csl_sage_fwd_mfma_f32); dropout on y_k in place (k < L-1)
//             normalised (csl_sage_fwd_bwd_norm): the ReLU above off, y_k = relu(gamma_k * layer_norm(y_k) + beta_k) in place
//   loss      csl_softmax_ce_partial_f32 / csl_sigmoid_bce_partial_f32 / csl_softmax_ce_w_partial_f32 (class weights,
//             label smoothing: the _ce entry points) on y_{L-1} (forward, gradient = the top layer's padded gy, bias
//             column sums)
//   backward  gW_k  = gy_k^T cat_k (row slabs)                 csl_gemm_f32 (batched)
//             gcat  = gy_k W_k                                 csl_gemm_f32
//             gy_{k-1}, gb_{k-1} = gather of gcat over the slice by source, ReLU mask of y_{k-1}, row padding and
//                                  bias column sums in the same pass                   csl_sage_cat_bwd_t_f32
//   the second stage of every reduction above (bias sums, slab sums, the loss): ONE launch (csl_reduce_multi_f32)
// Rows are padded to a multiple of `row_pad` so that GEMM shapes repeat from minibatch to minibatch.
//
// A RANK (Layer::rank set; part g of P) differs from this in the places marked "rank" below and nowhere else:
//   - its rows are the out rows it OWNS (n_owned <= n_out, n_in of a layer = n_owned of the layer below);
//   - forward, the partial sums of the boundary rows go to their owners and come back merged (pull_for_remotes /
//     push_from_remotes, dist_sageconv.py:52-65), and the backward runs the reverse exchange.  The exchange itself is the
//     CALLER's (Exchange: a callback over torch.distributed's all_to_all_single on RCCL, gloo in the tests): this file has
//     no communicator.  The fused layer 0 is taken when this part has no boundary rows there, and still enters the
//     exchange (a collective every rank must enter) with the empty buffers;
//   - a layer without a slice by source scatters its input gradient with atomics, where the single-GPU step refuses;
//   - the gather by source reads g2 (gcat in out-row order, the peers' rows filled in by the reverse exchange), not gcat;
//   - gcat is kept for layer 0 too, more than 256 classes are refused (no separate column-sum pass), an empty layer
//     below defers a reduction over no blocks where the single-GPU step zero-fills, and nothing is timed;
//   - no dropout, no multi-label loss and no layer normalisation yet: its entry points pass none of them (DESIGN.md 4.8,
//     4.13: what adding them takes).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <mutex>
#include <type_traits>
#include <vector>

#include "cslicer_aggr.h"
#include "cslicer_dropout.h"
#include "cslicer_feat16.h"
#include "cslicer_hip.h"
#include "cslicer_layernorm.h"
#include "cslicer_loss.h"
#include "cslicer_multilabel.h"
#include "dev_common.h"
#include "feat_elem.h"
#include "table_readers.h"

namespace {

thread_local char s_err[200];

// every layer defers a bias sum and possibly a weight-gradient slab sum, the step one loss sum: one launch finishes them
static_assert(2 * CSL_MAX_LAYERS + 1 <= CSL_REDUCE_MULTI_MAX, "csl_reduce_multi_f32 takes the step's second stages in one call");

// GEMM row counts repeat from minibatch to minibatch (a plan per shape: gemm_lt.hip): multiples of row_pad for tall
// operands, of 256 below that (a rank of an N-GPU job sees a few hundred to a few thousand rows per layer)
inline int64_t pad_rows(int64_t m, int64_t row_pad) {
  if (row_pad <= 0) return m;
  const int64_t q = m >= row_pad ? row_pad : (row_pad < 256 ? row_pad : 256);
  return (m + q - 1) / q * q;
}

// one model layer's slice as both steps read it
struct Layer {
  const int32_t *indptr, *indices, *self_ids_in, *t_indptr, *t_indices;
  int64_t t_max_len, t_entries;
  int64_t rows;                      // the rows that are computed and padded: n_out on one GPU, n_owned on a rank
  int64_t n_in;
  const csl_sage_rank_slice* rank;   // what only a rank has (owned rows, boundary lists); null: the single-GPU step
  bool by_source() const { return t_indptr && t_indices; }
};
Layer view(const csl_sage_slice& s) {
  return {s.indptr, s.indices, s.self_ids_in, s.t_indptr, s.t_indices, s.t_max_len, s.t_entries, s.n_out, s.n_in, nullptr};
}
Layer view(const csl_sage_rank_slice& s) {
  return {s.indptr, s.indices, s.self_ids_in, s.t_indptr, s.t_indices, s.t_max_len, s.t_entries, s.n_owned, s.n_in, &s};
}
struct Layers {
  Layer v[CSL_MAX_LAYERS] = {};
  bool rank, ok;   // ok: slices given, 1..CSL_MAX_LAYERS of them
  template <typename Slice>
  Layers(int32_t L, const Slice* sl) : rank(std::is_same<Slice, csl_sage_rank_slice>::value), ok(sl && L >= 1 && L <= CSL_MAX_LAYERS) {
    for (int k = 0; ok && k < L; k++) v[k] = view(sl[k]);
  }
};

struct Layout {
  int64_t cat[CSL_MAX_LAYERS], y[CSL_MAX_LAYERS], gy[CSL_MAX_LAYERS], gcat[CSL_MAX_LAYERS], mp[CSL_MAX_LAYERS];
  // rank only.  send / recv: forward the partial sums of peer-owned rows and the partials received for owned rows,
  // backward their gradients the other way; agg: the merged sums of the owned rows, backward their gradient; gx: the input
  // gradient of a layer that scatters it; g2: gcat in out-row order of a layer that gathers it by source
  int64_t send[CSL_MAX_LAYERS], recv[CSL_MAX_LAYERS], agg[CSL_MAX_LAYERS], gx[CSL_MAX_LAYERS], g2[CSL_MAX_LAYERS];
  bool hub[CSL_MAX_LAYERS];
  // first stages of the step's reductions, each in a buffer of its own: they are all finished by ONE launch at the end
  int64_t slabs[CSL_MAX_LAYERS];    // [n_slabs][out][2 in] of a layer whose weight gradient is computed in row slabs
  int64_t bpart[CSL_MAX_LAYERS];    // [blocks][out]: per-block column sums behind gb_k (k < L-1: from layer k+1's backward)
  int64_t bblocks[CSL_MAX_LAYERS];  // (0 exactly when the layer has no rows: every *_scratch is ceil(mp / rows per block) wide)
  int64_t lpart;                    // [blocks of four rows]: the loss
  int64_t wpack;                    // W_0 in MFMA operand order (csl_sage_fwd_mfma_f32), -1: the deepest layer is not fused
  bool slabbed[CSL_MAX_LAYERS];
  bool top_cols;                    // the loss pass also leaves the top layer's bias column sums
  int64_t g, scratch, total;        // single GPU, more than 256 classes: the logits' gradient and the column-sum scratch
  // layer normalisation (csl_sage_fwd_bwd_norm), k < L-1: what the forward keeps for the backward, and the backward's two
  // first stages ([lnblocks][out] each: dgamma_k, and gb_k now that bpart is dbeta_k's)
  int64_t xhat[CSL_MAX_LAYERS], rstd[CSL_MAX_LAYERS], gpart[CSL_MAX_LAYERS], zpart[CSL_MAX_LAYERS], lnblocks[CSL_MAX_LAYERS];
};

// bump allocation of the step's buffers (floats); returns false for an unsupported model
bool lay_out(int32_t L, const int32_t* dims, const Layers& lv, int64_t row_pad, int32_t n_slabs, Layout& o, bool norm = false) {
  if (!dims || !lv.ok || n_slabs < 1) return false;
  const Layer* v = lv.v;
  int64_t at = 0;
  for (int k = 0; k < L; k++) {
    const int64_t in = dims[k], out = dims[k + 1];
    const Layer& s = v[k];
    const csl_sage_rank_slice* r = s.rank;
    if (in < 4 || in % 4 != 0 || out < 1 || s.rows < 0 || s.n_in < 0) return false;
    if (k + 1 < L && out % 4 != 0) return false;  // a hidden width feeds the next layer's float4 kernels
    if (r && (r->n_out < 0 || r->n_from < 0 || r->n_to < 0 || r->n_owned > r->n_out)) return false;
    // layer k's sources are layer k-1's rows: its outputs on one GPU, the nodes this part owns below on a rank
    if (k > 0 && s.n_in != v[k - 1].rows) return false;
    const int64_t mp = pad_rows(s.rows, row_pad);
    o.mp[k] = mp;
    o.send[k] = at, at += r ? up4(r->n_from * in) : 0;
    o.recv[k] = at, at += r ? up4(r->n_to * in) : 0;
    o.agg[k] = at, at += r ? up4(r->n_out * in) : 0;
    o.cat[k] = at, at += up4(mp * 2 * in);
    o.y[k] = at, at += up4(mp * out);
    o.gy[k] = at, at += up4(mp * out);
    o.gcat[k] = at, at += k > 0 || r ? up4(mp * 2 * in) : 0;   // (layer 0 has no input gradient; a rank keeps the buffer)
    const bool by_src = k > 0 && s.by_source();                // this layer's input gradient is gathered by source
    o.gx[k] = at, at += r && k > 0 && !by_src ? up4(s.n_in * in) : 0;
    o.g2[k] = at, at += r && by_src ? up4(r->n_out * 2 * in) : 0;
    o.hub[k] = k > 0 && s.t_max_len > CSL_T_SORTED_MAX;        // a hub list: its rows are gathered by many workgroups
    const int64_t wn = out * 2 * in;
    o.slabbed[k] = row_pad > 0 && mp >= row_pad && n_slabs > 1 && mp % n_slabs == 0 && wn % 4 == 0;
    o.slabs[k] = at, at += o.slabbed[k] ? up4(wn * n_slabs) : 0;
    // gb_k's first stage is written by layer k+1's backward (k < L-1): the gather by source (twice the blocks when that
    // layer has hub lists) or, on a rank without one, the mask pass behind the atomic scatter; k = L-1: see below
    int64_t part = 0;
    if (k + 1 < L)
      part = v[k + 1].rank && !v[k + 1].by_source()  ? csl_relu_bwd_colsum_scratch(mp, (int32_t)out)
             : v[k + 1].t_max_len > CSL_T_SORTED_MAX ? csl_sage_cat_bwd_t_hub_scratch(mp, (int32_t)out)
                                                     : csl_sage_cat_bwd_t_scratch(mp, (int32_t)out);
    o.bblocks[k] = part / out;
    o.bpart[k] = at, at += up4(part);
  }
  {
    const int k = L - 1;
    const int64_t C = dims[L], rows = o.mp[k], lblocks = (rows + 3) / 4;
    int64_t scratch = 0;
    o.top_cols = C <= 256;
    if (lv.rank && !o.top_cols) return false;   // (a rank has no separate column-sum pass)
    o.lpart = at, at += up4(lblocks);
    if (o.top_cols) {
      o.bblocks[k] = lblocks;
      o.bpart[k] = at, at += up4(lblocks * C);
    } else {
      scratch = csl_relu_bwd_colsum_scratch(rows, (int32_t)C);
    }
    // the gradient w.r.t. the logits IS the top layer's (padded) gy when the loss pass pads it; else a buffer of its own
    o.g = o.top_cols ? o.gy[k] : at;
    at += o.top_cols ? 0 : up4(v[k].rows * C);
    o.scratch = at, at += up4(scratch);
  }
  {
    // the deepest layer as ONE kernel (gather -> fp32 MFMA -> bias + ReLU) where its widths allow.  A rank: only WITHOUT
    // boundary rows on this part (every out row owned, nothing sent or received: a world of one, or a partition that keeps
    // a minibatch's neighbourhoods local), when its deepest layer is the single-GPU layer
    const csl_sage_rank_slice* r = v[0].rank;
    const bool local = !r || (r->n_from == 0 && r->n_to == 0 && r->n_owned == r->n_out);
    const int64_t wp = local && !getenv("CSLICER_NO_MFMA_FWD") ? csl_sage_fwd_mfma_scratch(dims[0], dims[1]) : -1;
    o.wpack = wp > 0 ? at : -1;
    if (wp > 0) at += up4(wp);
  }
  // (behind everything else: without norm every offset and the total are what they always were)
  for (int k = 0; norm && k + 1 < L; k++) {
    const int64_t out = dims[k + 1], part = csl_layernorm_bwd_scratch(o.mp[k], (int32_t)out);
    if (part < 0) return false;
    o.xhat[k] = at, at += up4(v[k].rows * out);
    o.rstd[k] = at, at += up4(v[k].rows);
    o.lnblocks[k] = part / out;
    o.gpart[k] = at, at += up4(part);
    o.zpart[k] = at, at += up4(part);
  }
  o.total = at;
  return true;
}

int64_t workspace_floats_of(int32_t L, const int32_t* dims, const Layers& lv, int64_t row_pad, int32_t n_slabs, bool norm = false) {
  Layout o;
  return lay_out(L, dims, lv, row_pad, n_slabs, o, norm) ? o.total : (int64_t)CSL_E_INVALID;
}

// ---- diagnostics: device time of the step's launches by group (csl_sage_step_timing / _read): HIP events around every
// launch on the step's own stream, read back (and the stream drained) by the caller.  Off by default: no cost.
struct TimedSpan {
  int group;
  hipEvent_t e0, e1;
};
bool g_timing = false;
std::vector<TimedSpan> g_spans;       // recorded, not yet read
std::vector<hipEvent_t> g_free;       // event pool
std::mutex g_tmu;
hipEvent_t take_event() {
  if (!g_free.empty()) {
    hipEvent_t e = g_free.back();
    g_free.pop_back();
    return e;
  }
  hipEvent_t e = nullptr;
  (void)hipEventCreate(&e);
  return e;
}
struct SpanGuard {   // records e0 now and e1 when it goes out of scope
  hipStream_t st;
  TimedSpan sp;
  bool on;
  SpanGuard(int group, void* stream) : st((hipStream_t)stream), on(g_timing && group >= 0) {   // (group < 0: untimed)
    if (!on) return;
    std::lock_guard<std::mutex> lk(g_tmu);
    sp.group = group, sp.e0 = take_event(), sp.e1 = take_event();
    (void)hipEventRecord(sp.e0, st);
  }
  ~SpanGuard() {
    if (!on) return;
    (void)hipEventRecord(sp.e1, st);
    std::lock_guard<std::mutex> lk(g_tmu);
    g_spans.push_back(sp);
  }
};

int failed(const char* what, int rc, int layer) {
  snprintf(s_err, sizeof(s_err), "%s failed (%d), layer %d", what, rc, layer);
  return rc;
}
// one launch of the step on `stream`, timed under `group` (< 0: untimed); a failure ends the step with its layer named
#define STEP(group, layer, x)                              \
  do {                                                     \
    SpanGuard sg_((group), stream);                        \
    const int rc_ = (x);                                   \
    if (rc_ < 0) return failed(#x, rc_, (layer));          \
  } while (0)

// ---- the resident feature table is float32 (kind 0: the _f32 entry points) or 16-bit (CSL_FEAT_F16 / CSL_FEAT_BF16: the
// _x16 twins, cslicer_feat16.h); only the deepest layer's forward reads it, through the readers of table_readers.h, and
// everything downstream of them is fp32 either way.

// the _x16 entry points refuse a table no reader takes before anything else
bool table16_refused(const void* feat, int32_t kind, int64_t ldf) {
  if (feat::table_ok(feat, kind, ldf)) return false;
  snprintf(s_err, sizeof(s_err), "16-bit feature table: kind %d (1 float16, 2 bfloat16), 8-byte aligned base, row stride a "
           "multiple of 4 elements expected", (int)kind);
  return true;
}

bool workspace_fits(int64_t total, const float* workspace, int64_t workspace_floats) {
  if (total <= workspace_floats && (total <= 0 || (workspace && aligned16(workspace)))) return true;
  snprintf(s_err, sizeof(s_err), "workspace: %lld floats needed, %lld given", (long long)total, (long long)workspace_floats);
  return false;
}

// where each parameter's gradient sits in the flat buffer: W_0, b_0, W_1, b_1, ..., then (a normalised model's)
// gamma_0, beta_0, gamma_1, beta_1, ... of every layer but the last
struct GradSlots {
  float *gW[CSL_MAX_LAYERS], *gb[CSL_MAX_LAYERS], *ggamma[CSL_MAX_LAYERS], *gbeta[CSL_MAX_LAYERS];
  GradSlots(float* grads, int L, const int32_t* dims) {
    int64_t at = 0;
    for (int j = 0; j < L; j++) {
      gW[j] = grads + at, at += (int64_t)dims[j + 1] * 2 * dims[j];
      gb[j] = grads + at, at += dims[j + 1];
    }
    for (int j = 0; j + 1 < L; j++) {
      ggamma[j] = grads + at, at += dims[j + 1];
      gbeta[j] = grads + at, at += dims[j + 1];
    }
  }
};

// the second stages of a step's reductions, collected as (source, blocks, width, destination) and finished by ONE launch
// (a step defers at most 2 L + 1 of them: see the static_assert above); a normalised model adds two per layer but the last,
// which at four layers is more than one launch takes: a second launch finishes what the first left
constexpr int DEFER_MAX = 4 * CSL_MAX_LAYERS - 1;
static_assert(DEFER_MAX <= 2 * CSL_REDUCE_MULTI_MAX, "two csl_reduce_multi_f32 launches take a normalised step's second stages");
struct Deferred {
  const float* src[DEFER_MAX];
  float* dst[DEFER_MAX];
  int64_t nblk[DEFER_MAX];
  int32_t h[DEFER_MAX];
  int n = 0;
  void add(const float* s, int64_t blocks, int32_t width, float* d) {
    if (n >= DEFER_MAX) return;   // (cannot happen: asserted at compile time)
    src[n] = s, nblk[n] = blocks, h[n] = width, dst[n] = d;
    n++;
  }
  int finish(void* stream) {
    const int first = n < CSL_REDUCE_MULTI_MAX ? n : CSL_REDUCE_MULTI_MAX;
    const int rc = csl_reduce_multi_f32(first, src, nblk, h, dst, stream);
    if (rc < 0 || first == n) return rc;
    return csl_reduce_multi_f32(n - first, src + first, nblk + first, h + first, dst + first, stream);
  }
};

// dropout between the layers (csl_sage_fwd_bwd_dropout, cslicer_dropout.h): layer k's out-node ids, the probability and the
// counter's seed and step
struct DropArgs {
  const int32_t* const* out_ids;
  float p;
  int64_t seed, step;
};

// the multi-label loss (csl_sage_fwd_bwd_multilabel, cslicer_multilabel.h): the packed label words in place of `labels`
struct MultiArgs {
  const int32_t* words;
  int64_t ldw;
};

// the options of the single-label loss (csl_sage_fwd_bwd_ce / csl_sage_rank_fwd_bwd_ce, cslicer_loss.h)
struct LossArgs {
  const float* class_weight;
  float label_smoothing;
};

// layer normalisation on the result of every layer but the last (csl_sage_fwd_bwd_norm, cslicer_layernorm.h)
struct NormArgs {
  const float* const* gammas;
  const float* const* betas;
  float eps;
};

// a rank's boundary exchange: the caller's callbacks.  `wait` given: `exchange` only STARTS the exchange (on a stream of
// the caller's) and `wait` makes `stream` wait for it -- called right before the received rows are first used, so the rows
// that never leave the GPU are aggregated while the boundary rows travel (dist_sageconv.py:57-64 on a side stream)
struct Exchange {
  csl_exchange_fn exchange;
  csl_exchange_wait_fn wait;
  void *user, *stream;
  int start(int layer, int backward, const float* src, float* dst, int32_t width) const {
    const int rc = exchange(user, layer, backward, src, dst, width, stream);
    if (rc >= 0) return CSL_OK;
    snprintf(s_err, sizeof(s_err), "the exchange callback failed (%d), layer %d, %s", rc, layer, backward ? "backward" : "forward");
    return rc;
  }
  int finish(int layer, int backward) const {
    const int rc = wait ? wait(user, layer, backward, stream) : 0;
    if (rc >= 0) return CSL_OK;
    snprintf(s_err, sizeof(s_err), "the exchange-wait callback failed (%d), layer %d", rc, layer);
    return rc;
  }
};

// gW_k = gy_k^T cat_k: nothing but a zero fill without rows, in row slabs whose sum is deferred, or one plain GEMM.
// group: the timing group of the GEMM (< 0: untimed)
int weight_grad(int group, const Layout& o, int k, const int32_t* dims, int32_t n_slabs, float* ws, float* gW, Deferred& later,
                void* stream) {
  const int64_t in = dims[k], out = dims[k + 1], mp = o.mp[k], wn = out * 2 * in;
  if (mp == 0) return hipMemsetAsync(gW, 0, sizeof(float) * wn, (hipStream_t)stream) == hipSuccess ? CSL_OK : CSL_E_HIP;
  SpanGuard sg(group, stream);
  if (!o.slabbed[k])
    return csl_gemm_f32(1, 0, out, 2 * in, mp, ws + o.gy[k], out, 0, ws + o.cat[k], 2 * in, 0, gW, 2 * in, 0, 1, nullptr, 0, stream);
  const int64_t rs = mp / n_slabs;
  later.add(ws + o.slabs[k], n_slabs, (int32_t)wn, gW);
  return csl_gemm_f32(1, 0, out, 2 * in, rs, ws + o.gy[k], out, rs * out, ws + o.cat[k], 2 * in, rs * 2 * in, ws + o.slabs[k],
                      2 * in, wn, n_slabs, nullptr, 0, stream);
}

// gy_below [mp_below, in] = the gather of g [., 2 in] over layer s's slice by source, under the ReLU mask of y_below and
// padded like its GEMM operand; its column sums stay as per-block partials in bpart.  indptr: the CSR whose row lengths
// divide the mean half, null where g carries it divided already (a rank's g2).
// A hub's list in the slice by source is thousands of entries, one wave's serial walk (1.3 ms instead of 30 us per launch
// on a Zipf graph: profiles/hub_probe.py): those rows are summed by a workgroup per segment of entries
int gather_by_source(const Layer& s, bool hub, const int32_t* indptr, const float* g, int32_t in, const float* y_below,
                     int64_t mp_below, float* gy_below, float* bpart, void* stream) {
  const int64_t ldg = 2 * (int64_t)in;
  if (hub)
    return csl_sage_cat_bwd_t_hub_f32(s.t_indptr, s.t_indices, s.t_entries, indptr, g, ldg, y_below, in, s.n_in, mp_below,
                                      gy_below, in, nullptr, bpart, in, stream);
  return csl_sage_cat_bwd_t_f32(s.t_indptr, s.t_indices, indptr, g, ldg, y_below, in, s.n_in, mp_below, gy_below, in, nullptr,
                                bpart, in, stream);
}

// The step behind all eight entry points.  lv: the slices (lv.rank: of a rank, with `xc` its exchange and `label_rows`);
// kind: the feature table's element kind (0: float32).  Single GPU only: `drop` (csl_sage_fwd_bwd_dropout) and `multi`
// (sigmoid-BCE on packed labels in place of the softmax cross-entropy: csl_sage_fwd_bwd_multilabel).  Both: `lossw` (the
// cross-entropy with class weights and label smoothing: the _ce entry points).
int sage_step(int32_t n_layers, const int32_t* dims, const Layers& lv, const float* const* weights, const float* const* biases,
              const void* feat, int32_t kind, int64_t ldf, const int32_t* feat_rows, const int32_t* seed_ids,
              const int32_t* label_rows, const int64_t* labels, float scale, int64_t row_pad, int32_t n_slabs,
              const Exchange* xc, float* grads, float* loss, float* workspace, int64_t workspace_floats, void* stream,
              const DropArgs* drop, const MultiArgs* multi, const LossArgs* lossw = nullptr, const NormArgs* norm = nullptr) {
  s_err[0] = 0;
  Layout o;
  if (!weights || !biases || !grads || !loss || (lv.rank && !xc->exchange) || !lay_out(n_layers, dims, lv, row_pad, n_slabs, o, norm != nullptr)) {
    if (lv.rank)
      snprintf(s_err, sizeof(s_err), "bad argument or unsupported model (widths multiples of 4, <= 256 classes, 1..%d layers, "
               "n_in of a layer = n_owned of the layer below)", CSL_MAX_LAYERS);
    else
      snprintf(s_err, sizeof(s_err), "bad argument or unsupported model (widths must be multiples of 4, 1..%d layers, "
               "n_in of a layer = n_out of the layer below)", CSL_MAX_LAYERS);
    return CSL_E_INVALID;
  }
  if (!workspace_fits(o.total, workspace, workspace_floats)) return CSL_E_INVALID;
  const int L = n_layers;
  float* ws = workspace;
  const GradSlots gs(grads, L, dims);
  // the timing groups of csl_sage_step_timing: the single-GPU step records them, a rank nothing
  const int t_fused = lv.rank ? -1 : CSL_STEP_FUSED_FWD, t_gemm = lv.rank ? -1 : CSL_STEP_GEMM;
  const int t_aggr = lv.rank ? -1 : CSL_STEP_AGGREGATION, t_other = lv.rank ? -1 : CSL_STEP_OTHER;
  // ---- forward
  for (int k = 0; k < L; k++) {
    const int32_t in = dims[k], out = dims[k + 1];
    const Layer& s = lv.v[k];
    const csl_sage_rank_slice* r = s.rank;
    const int64_t m = s.rows, mp = o.mp[k], ldc = 2 * (int64_t)in;
    // the deepest layer reads the resident feature rows through feat_rows (no gathered input matrix)
    const void* x = k == 0 ? feat : ws + o.y[k - 1];
    const int32_t xk = k == 0 ? kind : 0;   // (only the feature table may be 16-bit)
    const int64_t ldx = k == 0 ? ldf : (int64_t)in;
    const int32_t* map = k == 0 ? feat_rows : nullptr;
    if (k == 0 && o.wpack >= 0) {
      // rank: "no boundary rows" is a property of THIS part's slice: a peer may have some in the same minibatch, and the
      // exchange is a collective every rank must enter -- so it is issued here too, with the empty buffers (whether a
      // collective is entered depends only on L, which all ranks share)
      if (r) {
        if (const int rc = xc->start(0, 0, ws + o.send[0], ws + o.recv[0], in); rc < 0) return rc;
        if (const int rc = xc->finish(0, 0); rc < 0) return rc;
      }
      // gather [self | mean] into LDS, multiply on the fp32 matrix cores, bias + ReLU on the way out; the operand is
      // also written (the weight gradient reads it), but never read back by the forward
      STEP(t_fused, k, rd::sage_fwd_mfma(s.indptr, s.indices, s.self_ids_in, feat_rows, feat, kind, ldf, weights[0], ldc, biases[0],
                                         m, mp, in, out, 0, L > 1 && !norm ? 1 : 0, ws + o.cat[0], ldc, ws + o.y[0], out, ws + o.wpack,
                                         stream));
    } else {
      if (r) {
        // partial sums of the rows peers own, straight into the send buffer; then the rows this part owns
        STEP(-1, k, rd::spmm_sum_map(s.indptr, s.indices, r->from_all, r->n_from, x, xk, ldx, map, ws + o.send[k], in, in, 1, stream));
        if (const int rc = xc->start(k, 0, ws + o.send[k], ws + o.recv[k], in); rc < 0) return rc;
        STEP(-1, k, rd::spmm_sum_map(s.indptr, s.indices, r->owned_out_nodes, r->n_owned, x, xk, ldx, map, ws + o.agg[k], in, in, 0, stream));
        if (const int rc = xc->finish(k, 0); rc < 0) return rc;
        STEP(-1, k, csl_scatter_add_rows_atomic_f32(ws + o.agg[k], in, r->to_all, r->n_to, ws + o.recv[k], in, in, stream));
        STEP(-1, k, rd::sage_cat(nullptr, nullptr, s.self_ids_in, r->owned_out_nodes, r->owned_degree, map, x, xk, ldx, ws + o.agg[k],
                                 in, m, mp, ws + o.cat[k], ldc, in, 0, stream));
      } else {
        STEP(t_aggr, k, rd::sage_cat(s.indptr, s.indices, s.self_ids_in, nullptr, nullptr, map, x, xk, ldx, nullptr, 0, m, mp,
                                     ws + o.cat[k], ldc, in, 0, stream));
      }
      STEP(t_gemm, k, csl_gemm_f32(0, 1, mp, out, ldc, ws + o.cat[k], ldc, 0, weights[k], ldc, 0, ws + o.y[k], out, 0, 1, biases[k],
                                   k + 1 < L && !norm ? 1 : 0, stream));
    }
    // normalised: the layer ran with its ReLU off; y_k = relu(gamma * xhat + beta) in place, xhat_k and rstd_k kept
    if (norm && k + 1 < L)
      STEP(t_other, k, csl_layernorm_relu_fwd_f32(ws + o.y[k], out, norm->gammas[k], norm->betas[k], norm->eps, m, out, ws + o.y[k], out,
                                                  ws + o.xhat[k], out, ws + o.rstd[k], 1, stream));
    // y_k is stored after its ReLU and read as it is by the layer above and by the backward's mask (y_k > 0): dropped in
    // place it carries relu' * mask by itself
    if (drop && k + 1 < L)
      STEP(t_other, k, csl_dropout_f32(ws + o.y[k], out, ws + o.y[k], out, drop->out_ids[k], m, out, drop->p, drop->seed, k,
                                       drop->step, stream));
  }
  Deferred later;
  // ---- loss and its gradient w.r.t. the logits, bias column sums alongside (a rank: over the seeds this part owns, the
  // caller's `scale` = 1 / seeds of the WHOLE minibatch).  <= 256 classes: the pass pads the gradient into the top layer's
  // gy and leaves the column sums' first stage; more (single GPU): a column-sum pass of its own does both
  {
    const int k = L - 1;
    const int32_t C = dims[L];
    const int64_t m = lv.v[k].rows, rows = o.top_cols ? o.mp[k] : m;
    float* cols = o.top_cols ? ws + o.bpart[k] : nullptr;
    if (multi)
      STEP(t_other, k, csl_sigmoid_bce_partial_f32(ws + o.y[k], C, m, rows, C, seed_ids, label_rows, multi->words, multi->ldw, scale,
                                                   ws + o.g, C, ws + o.lpart, cols, stream));
    else if (lossw)
      STEP(t_other, k, csl_softmax_ce_w_partial_f32(ws + o.y[k], C, m, rows, C, seed_ids, label_rows, labels, lossw->class_weight,
                                                    lossw->label_smoothing, scale, ws + o.g, C, ws + o.lpart, cols, stream));
    else
      STEP(t_other, k, csl_softmax_ce_partial_f32(ws + o.y[k], C, m, rows, C, seed_ids, label_rows, labels, scale, ws + o.g, C,
                                                  ws + o.lpart, cols, stream));
    if (o.top_cols) later.add(cols, o.bblocks[k], C, gs.gb[k]);
    else STEP(t_aggr, k, csl_relu_bwd_colsum_f32(ws + o.g, C, nullptr, 0, m, o.mp[k], ws + o.gy[k], C, gs.gb[k], ws + o.scratch, C, stream));
    later.add(ws + o.lpart, (rows + 3) / 4, 1, loss);  // (blocks of four rows the loss pass covered)
  }
  // ---- backward
  for (int k = L - 1; k >= 0; k--) {
    const int32_t in = dims[k], out = dims[k + 1];
    const Layer& s = lv.v[k];
    const csl_sage_rank_slice* r = s.rank;
    const int64_t mp = o.mp[k], ldc = 2 * (int64_t)in;
    STEP(-1, k, weight_grad(t_gemm, o, k, dims, n_slabs, ws, gs.gW[k], later, stream));
    if (k == 0) break;   // (no gradient flows into the input features; the deepest layer's exchange has no backward)
    if (!r && !s.by_source()) {
      snprintf(s_err, sizeof(s_err), "layer %d has no slice by source (engine flag CSL_FLAG_TRANSPOSE)", k);
      return CSL_E_INVALID;
    }
    STEP(t_gemm, k, csl_gemm_f32(0, 0, mp, ldc, out, ws + o.gy[k], out, 0, weights[k], ldc, 0, ws + o.gcat[k], ldc, 0, 1, nullptr, 0,
                                 stream));
    // gradient w.r.t. layer k-1's pre-activation output (= this layer's input x), padded like its GEMM operand; its
    // column sums (gb_{k-1}) stay as per-block partials
    const int64_t mp_below = o.mp[k - 1];
    const float* y_below = ws + o.y[k - 1];
    float *gy_below = ws + o.gy[k - 1], *bpart = ws + o.bpart[k - 1];
    if (r && !s.by_source()) {
      // rank, no slice by source: operand gradient -> self rows of gx and owned rows of the merged sums' gradient (both
      // zeroed inside)
      STEP(-1, k, csl_sage_cat_rows_bwd_f32(s.self_ids_in, r->owned_out_nodes, r->owned_degree, r->n_owned, ws + o.gcat[k], ldc,
                                            ws + o.gx[k], s.n_in, ws + o.agg[k], r->n_out, in, stream));
      // what this part received forward gets its gradient back; the reverse exchange returns the gradients of the
      // partial sums this part sent
      STEP(-1, k, csl_gather_rows_f32(ws + o.agg[k], in, r->to_all, r->n_to, ws + o.recv[k], in, in, stream));
      if (const int rc = xc->start(k, 1, ws + o.recv[k], ws + o.send[k], in); rc < 0) return rc;
      STEP(-1, k, csl_spmm_sum_bwd_f32(s.indptr, s.indices, r->owned_out_nodes, r->n_owned, ws + o.agg[k], in, 0, ws + o.gx[k], in, in,
                                       stream));
      if (const int rc = xc->finish(k, 1); rc < 0) return rc;
      STEP(-1, k, csl_spmm_sum_bwd_f32(s.indptr, s.indices, r->from_all, r->n_from, ws + o.send[k], in, 1, ws + o.gx[k], in, in, stream));
      // ReLU mask of the layer below, padding of its GEMM operand, its bias column sums (first stage)
      if (mp_below > 0)
        STEP(-1, k, csl_relu_bwd_colsum_f32(ws + o.gx[k], in, y_below, in, s.n_in, mp_below, gy_below, in, nullptr, bpart, in, stream));
    } else if (r) {
      // rank, BY SOURCE: the operand gradient goes into out-row order (mean half / true degree), the rows peers own get
      // theirs from the reverse exchange, and ONE gather over the part's slice by source writes the input gradient with
      // the ReLU mask of the layer below, its padding and its bias sums -- no atomics, no zero fill
      float* g2 = ws + o.g2[k];
      STEP(-1, k, csl_sage_rank_g2_f32(r->owned_out_nodes, r->owned_degree, r->n_owned, ws + o.gcat[k], ldc, g2, ldc, in, stream));
      // what this part received forward gets its gradient back (the mean halves of the owned rows it was merged into)
      STEP(-1, k, csl_gather_rows_f32(g2 + in, ldc, r->to_all, r->n_to, ws + o.recv[k], in, in, stream));
      if (const int rc = xc->start(k, 1, ws + o.recv[k], ws + o.send[k], in); rc < 0) return rc;
      if (const int rc = xc->finish(k, 1); rc < 0) return rc;
      STEP(-1, k, csl_scatter_rows_f32(g2 + in, ldc, r->from_all, r->n_from, ws + o.send[k], in, in, stream));
      if (mp_below > 0) STEP(-1, k, gather_by_source(s, o.hub[k], nullptr, g2, in, y_below, mp_below, gy_below, bpart, stream));
    } else {
      STEP(t_aggr, k, gather_by_source(s, o.hub[k], s.indptr, ws + o.gcat[k], in, y_below, mp_below, gy_below, bpart, stream));
    }
    if (norm) {
      // normalised: gy_{k-1} holds mask * gradient w.r.t. the normalised row and its column sums are dbeta_{k-1}; the
      // backward of the norm turns it into dz in place and leaves the first stages of dgamma_{k-1} and gb_{k-1}
      if (o.bblocks[k - 1] > 0) {
        later.add(bpart, o.bblocks[k - 1], in, gs.gbeta[k - 1]);
        STEP(t_other, k, csl_layernorm_bwd_f32(gy_below, in, ws + o.xhat[k - 1], in, ws + o.rstd[k - 1], norm->gammas[k - 1], s.n_in,
                                               mp_below, in, ws + o.gpart[k - 1], ws + o.zpart[k - 1], stream));
        later.add(ws + o.gpart[k - 1], o.lnblocks[k - 1], in, gs.ggamma[k - 1]);
        later.add(ws + o.zpart[k - 1], o.lnblocks[k - 1], in, gs.gb[k - 1]);
      } else {
        for (float* g0 : {gs.gb[k - 1], gs.ggamma[k - 1], gs.gbeta[k - 1]})
          if (hipMemsetAsync(g0, 0, sizeof(float) * in, (hipStream_t)stream) != hipSuccess) return CSL_E_HIP;
      }
      continue;
    }
    // gb_{k-1}.  An empty layer below (no blocks): a rank defers a reduction over none, the single-GPU step zero-fills
    if (r || o.bblocks[k - 1] > 0) later.add(bpart, o.bblocks[k - 1], in, gs.gb[k - 1]);
    else if (hipMemsetAsync(gs.gb[k - 1], 0, sizeof(float) * in, (hipStream_t)stream) != hipSuccess) return CSL_E_HIP;
  }
  // ---- every deferred second stage (bias sums, weight-gradient slabs, the loss) in one launch
  STEP(t_other, -1, later.finish(stream));
  if (drop && L > 1) {
    // the backward crossed L-1-j dropped layers on its way to layer j with the mask alone: the factor s of each, which
    // commutes with everything downstream of it, goes onto the finished gradients
    // (gamma_j and beta_j take W_j's factor; with them four layers have more segments than one launch takes)
    float* seg[2 * CSL_SCALE_SEGMENTS_MAX];
    int64_t cnt[2 * CSL_SCALE_SEGMENTS_MAX];
    float fac[2 * CSL_SCALE_SEGMENTS_MAX];
    const double s1 = (double)(float)(1.0 / (1.0 - (double)drop->p));
    double f = 1.0;
    int ns = 0;
    for (int j = L - 2; j >= 0; j--) {
      f *= s1;
      seg[ns] = gs.gW[j], cnt[ns] = (int64_t)dims[j + 1] * 2 * dims[j], fac[ns] = (float)f, ns++;
      seg[ns] = gs.gb[j], cnt[ns] = dims[j + 1], fac[ns] = (float)f, ns++;
    }
    for (int j = L - 2; norm && j >= 0; j--) {
      seg[ns] = gs.ggamma[j], cnt[ns] = dims[j + 1], fac[ns] = fac[2 * (L - 2 - j)], ns++;
      seg[ns] = gs.gbeta[j], cnt[ns] = dims[j + 1], fac[ns] = fac[2 * (L - 2 - j)], ns++;
    }
    const int first = ns < CSL_SCALE_SEGMENTS_MAX ? ns : CSL_SCALE_SEGMENTS_MAX;
    STEP(t_other, -1, csl_scale_segments_f32(first, seg, cnt, fac, stream));
    if (ns > first) STEP(t_other, -1, csl_scale_segments_f32(ns - first, seg + first, cnt + first, fac + first, stream));
  }
  return CSL_OK;
}

}  // namespace

extern "C" {

const char* csl_sage_last_error(void) { return s_err; }

int csl_sage_step_timing(int32_t enable) {
  std::lock_guard<std::mutex> lk(g_tmu);
  g_timing = enable != 0;
  return CSL_OK;
}

int csl_sage_step_timing_read(double* ms, int64_t* launches) {
  if (!ms || !launches) return CSL_E_INVALID;
  std::lock_guard<std::mutex> lk(g_tmu);
  for (int g = 0; g < CSL_STEP_GROUPS; g++) ms[g] = 0.0, launches[g] = 0;
  int rc = CSL_OK;
  for (const TimedSpan& sp : g_spans) {
    float t = 0.f;
    if (hipEventSynchronize(sp.e1) != hipSuccess || hipEventElapsedTime(&t, sp.e0, sp.e1) != hipSuccess) rc = CSL_E_HIP;
    if (sp.group >= 0 && sp.group < CSL_STEP_GROUPS) ms[sp.group] += t, launches[sp.group]++;
    g_free.push_back(sp.e0), g_free.push_back(sp.e1);
  }
  g_spans.clear();
  return rc;
}

int64_t csl_sage_fwd_bwd_workspace(int32_t n_layers, const int32_t* dims, const csl_sage_slice* slices, int64_t row_pad,
                                   int32_t n_slabs) {
  return workspace_floats_of(n_layers, dims, Layers(n_layers, slices), row_pad, n_slabs);
}

int64_t csl_sage_rank_workspace(int32_t n_layers, const int32_t* dims, const csl_sage_rank_slice* slices, int64_t row_pad,
                                int32_t n_slabs) {
  return workspace_floats_of(n_layers, dims, Layers(n_layers, slices), row_pad, n_slabs);
}

int csl_sage_fwd_bwd_f32(int32_t n_layers, const int32_t* dims, const csl_sage_slice* sl, const float* const* weights,
                         const float* const* biases, const float* feat, int64_t ldf, const int32_t* feat_rows,
                         const int32_t* seed_ids, const int64_t* labels, float scale, int64_t row_pad, int32_t n_slabs,
                         float* grads, float* loss, float* workspace, int64_t workspace_floats, void* stream) {
  return sage_step(n_layers, dims, Layers(n_layers, sl), weights, biases, feat, 0, ldf, feat_rows, seed_ids, nullptr, labels, scale,
                   row_pad, n_slabs, nullptr, grads, loss, workspace, workspace_floats, stream, nullptr, nullptr);
}

int csl_sage_fwd_bwd_x16(int32_t n_layers, const int32_t* dims, const csl_sage_slice* sl, const float* const* weights,
                         const float* const* biases, const void* feat, int32_t kind, int64_t ldf, const int32_t* feat_rows,
                         const int32_t* seed_ids, const int64_t* labels, float scale, int64_t row_pad, int32_t n_slabs,
                         float* grads, float* loss, float* workspace, int64_t workspace_floats, void* stream) {
  if (table16_refused(feat, kind, ldf)) return CSL_E_INVALID;
  return sage_step(n_layers, dims, Layers(n_layers, sl), weights, biases, feat, kind, ldf, feat_rows, seed_ids, nullptr, labels,
                   scale, row_pad, n_slabs, nullptr, grads, loss, workspace, workspace_floats, stream, nullptr, nullptr);
}

int csl_sage_fwd_bwd_dropout(int32_t n_layers, const int32_t* dims, const csl_sage_slice* sl, const float* const* weights,
                             const float* const* biases, const void* feat, int32_t kind, int64_t ldf, const int32_t* feat_rows,
                             const int32_t* seed_ids, const int64_t* labels, float scale, int64_t row_pad, int32_t n_slabs,
                             float* grads, float* loss, float* workspace, int64_t workspace_floats,
                             const int32_t* const* out_ids, float p, int64_t seed, int64_t step, void* stream) {
  if (kind != 0 && table16_refused(feat, kind, ldf)) return CSL_E_INVALID;
  bool ok = p > 0.f && p < 1.f && n_layers >= 1 && n_layers <= CSL_MAX_LAYERS && sl && (n_layers == 1 || out_ids);
  for (int k = 0; ok && k + 1 < n_layers; k++) ok = sl[k].n_out <= 0 || out_ids[k];
  if (!ok) {
    snprintf(s_err, sizeof(s_err), "dropout: 0 < p < 1 and the out-node ids of every layer but the last expected (p = %g)",
             (double)p);
    return CSL_E_INVALID;
  }
  const DropArgs drop = {out_ids, p, seed, step};
  return sage_step(n_layers, dims, Layers(n_layers, sl), weights, biases, feat, kind, ldf, feat_rows, seed_ids, nullptr, labels,
                   scale, row_pad, n_slabs, nullptr, grads, loss, workspace, workspace_floats, stream, &drop, nullptr);
}

int csl_sage_fwd_bwd_multilabel(int32_t n_layers, const int32_t* dims, const csl_sage_slice* sl, const float* const* weights,
                                const float* const* biases, const void* feat, int32_t kind, int64_t ldf,
                                const int32_t* feat_rows, const int32_t* seed_ids, const int32_t* label_words, int64_t ldw,
                                float scale, int64_t row_pad, int32_t n_slabs, float* grads, float* loss, float* workspace,
                                int64_t workspace_floats, const int32_t* const* out_ids, float p, int64_t seed, int64_t step,
                                void* stream) {
  if (kind != 0 && table16_refused(feat, kind, ldf)) return CSL_E_INVALID;
  const bool plain = p == 0.f && !out_ids;
  bool ok = n_layers >= 1 && n_layers <= CSL_MAX_LAYERS && sl && dims && label_words && dims[n_layers] >= 1 &&
            dims[n_layers] <= 4096 && ldw >= (dims[n_layers] + 31) / 32 &&
            (plain || (p > 0.f && p < 1.f && (n_layers == 1 || out_ids)));
  for (int k = 0; ok && !plain && k + 1 < n_layers; k++) ok = sl[k].n_out <= 0 || out_ids[k];
  if (!ok) {
    snprintf(s_err, sizeof(s_err), "multilabel: packed label words of at least ceil(C / 32) per row, 1 <= C <= 4096, and "
             "either p == 0 without out-node ids or 0 < p < 1 with those of every layer but the last expected (p = %g)",
             (double)p);
    return CSL_E_INVALID;
  }
  const DropArgs drop = {out_ids, p, seed, step};
  const MultiArgs multi = {label_words, ldw};
  return sage_step(n_layers, dims, Layers(n_layers, sl), weights, biases, feat, kind, ldf, feat_rows, seed_ids, nullptr, nullptr,
                   scale, row_pad, n_slabs, nullptr, grads, loss, workspace, workspace_floats, stream, plain ? nullptr : &drop, &multi);
}

int csl_sage_rank_fwd_bwd_f32(int32_t n_layers, const int32_t* dims, const csl_sage_rank_slice* sl,
                              const float* const* weights, const float* const* biases, const float* feat, int64_t ldf,
                              const int32_t* feat_rows, const int32_t* seed_ids, const int32_t* label_rows,
                              const int64_t* labels, float scale, int64_t row_pad, int32_t n_slabs,
                              csl_exchange_fn exchange, csl_exchange_wait_fn wait, void* user, float* grads, float* loss,
                              float* workspace, int64_t workspace_floats, void* stream) {
  const Exchange xc = {exchange, wait, user, stream};
  return sage_step(n_layers, dims, Layers(n_layers, sl), weights, biases, feat, 0, ldf, feat_rows, seed_ids, label_rows, labels,
                   scale, row_pad, n_slabs, &xc, grads, loss, workspace, workspace_floats, stream, nullptr, nullptr);
}

int csl_sage_rank_fwd_bwd_x16(int32_t n_layers, const int32_t* dims, const csl_sage_rank_slice* sl,
                              const float* const* weights, const float* const* biases, const void* feat, int32_t kind,
                              int64_t ldf, const int32_t* feat_rows, const int32_t* seed_ids, const int32_t* label_rows,
                              const int64_t* labels, float scale, int64_t row_pad, int32_t n_slabs,
                              csl_exchange_fn exchange, csl_exchange_wait_fn wait, void* user, float* grads, float* loss,
                              float* workspace, int64_t workspace_floats, void* stream) {
  if (table16_refused(feat, kind, ldf)) return CSL_E_INVALID;
  const Exchange xc = {exchange, wait, user, stream};
  return sage_step(n_layers, dims, Layers(n_layers, sl), weights, biases, feat, kind, ldf, feat_rows, seed_ids, label_rows, labels,
                   scale, row_pad, n_slabs, &xc, grads, loss, workspace, workspace_floats, stream, nullptr, nullptr);
}

// what both _ce entry points refuse about the loss options (the other arguments: sage_step's own checks)
static bool loss_refused(int32_t n_layers, const int32_t* dims, const int64_t* labels, float label_smoothing) {
  if (!(label_smoothing >= 0.f && label_smoothing < 1.f)) {   // (a NaN compares false)
    snprintf(s_err, sizeof(s_err), "label_smoothing must be in [0, 1), not %g", (double)label_smoothing);
    return true;
  }
  if (!labels) {
    snprintf(s_err, sizeof(s_err), "labels: the int64 labels of the nodes expected, not NULL");
    return true;
  }
  if (dims && n_layers >= 1 && n_layers <= CSL_MAX_LAYERS && (dims[n_layers] < 1 || dims[n_layers] > 4096)) {
    snprintf(s_err, sizeof(s_err), "dims: 1 <= classes <= 4096 expected for the weighted loss, not %d", (int)dims[n_layers]);
    return true;
  }
  return false;
}

int csl_sage_fwd_bwd_ce(int32_t n_layers, const int32_t* dims, const csl_sage_slice* sl, const float* const* weights,
                        const float* const* biases, const void* feat, int32_t kind, int64_t ldf, const int32_t* feat_rows,
                        const int32_t* seed_ids, const int64_t* labels, const float* class_weight, float label_smoothing,
                        float scale, int64_t row_pad, int32_t n_slabs, float* grads, float* loss, float* workspace,
                        int64_t workspace_floats, const int32_t* const* out_ids, float p, int64_t seed, int64_t step,
                        void* stream) {
  if (kind != 0 && table16_refused(feat, kind, ldf)) return CSL_E_INVALID;
  if (loss_refused(n_layers, dims, labels, label_smoothing)) return CSL_E_INVALID;
  const bool plain = p == 0.f && !out_ids;
  bool ok = n_layers >= 1 && n_layers <= CSL_MAX_LAYERS && sl && (plain || (p > 0.f && p < 1.f && (n_layers == 1 || out_ids)));
  for (int k = 0; ok && !plain && k + 1 < n_layers; k++) ok = sl[k].n_out <= 0 || out_ids[k];
  if (!ok) {
    snprintf(s_err, sizeof(s_err), "dropout (p, out_ids): either p == 0 without out-node ids or 0 < p < 1 with those of every "
             "layer but the last expected (p = %g)", (double)p);
    return CSL_E_INVALID;
  }
  const DropArgs drop = {out_ids, p, seed, step};
  const LossArgs lossw = {class_weight, label_smoothing};
  return sage_step(n_layers, dims, Layers(n_layers, sl), weights, biases, feat, kind, ldf, feat_rows, seed_ids, nullptr, labels,
                   scale, row_pad, n_slabs, nullptr, grads, loss, workspace, workspace_floats, stream, plain ? nullptr : &drop,
                   nullptr, &lossw);
}

int csl_sage_rank_fwd_bwd_ce(int32_t n_layers, const int32_t* dims, const csl_sage_rank_slice* sl,
                             const float* const* weights, const float* const* biases, const void* feat, int32_t kind,
                             int64_t ldf, const int32_t* feat_rows, const int32_t* seed_ids, const int32_t* label_rows,
                             const int64_t* labels, const float* class_weight, float label_smoothing, float scale,
                             int64_t row_pad, int32_t n_slabs, csl_exchange_fn exchange, csl_exchange_wait_fn wait,
                             void* user, float* grads, float* loss, float* workspace, int64_t workspace_floats,
                             void* stream) {
  if (kind != 0 && table16_refused(feat, kind, ldf)) return CSL_E_INVALID;
  if (loss_refused(n_layers, dims, labels, label_smoothing)) return CSL_E_INVALID;
  const Exchange xc = {exchange, wait, user, stream};
  const LossArgs lossw = {class_weight, label_smoothing};
  return sage_step(n_layers, dims, Layers(n_layers, sl), weights, biases, feat, kind, ldf, feat_rows, seed_ids, label_rows, labels,
                   scale, row_pad, n_slabs, &xc, grads, loss, workspace, workspace_floats, stream, nullptr, nullptr, &lossw);
}

int64_t csl_sage_fwd_bwd_norm_workspace(int32_t n_layers, const int32_t* dims, const csl_sage_slice* slices, int64_t row_pad,
                                        int32_t n_slabs) {
  return workspace_floats_of(n_layers, dims, Layers(n_layers, slices), row_pad, n_slabs, true);
}

int csl_sage_fwd_bwd_norm(int32_t n_layers, const int32_t* dims, const csl_sage_slice* sl, const float* const* weights,
                          const float* const* biases, const void* feat, int32_t kind, int64_t ldf, const int32_t* feat_rows,
                          const int32_t* seed_ids, const int64_t* labels, const float* class_weight, float label_smoothing,
                          float scale, int64_t row_pad, int32_t n_slabs, float* grads, float* loss, float* workspace,
                          int64_t workspace_floats, const int32_t* const* out_ids, float p, int64_t seed, int64_t step,
                          const int32_t* label_words, int64_t ldw, const float* const* gammas, const float* const* betas,
                          float eps, void* stream) {
  if (kind != 0 && table16_refused(feat, kind, ldf)) return CSL_E_INVALID;
  if (!label_words && loss_refused(n_layers, dims, labels, label_smoothing)) return CSL_E_INVALID;
  const bool plain = p == 0.f && !out_ids;
  bool ok = n_layers >= 1 && n_layers <= CSL_MAX_LAYERS && sl && dims && (plain || (p > 0.f && p < 1.f && (n_layers == 1 || out_ids)));
  for (int k = 0; ok && !plain && k + 1 < n_layers; k++) ok = sl[k].n_out <= 0 || out_ids[k];
  if (ok && label_words) ok = dims[n_layers] >= 1 && dims[n_layers] <= 4096 && ldw >= (dims[n_layers] + 31) / 32;
  if (!ok) {
    snprintf(s_err, sizeof(s_err), "norm step: 1..%d layers; either p == 0 without out-node ids or 0 < p < 1 with those of every "
             "layer but the last; packed label words of at least ceil(C / 32) per row, 1 <= C <= 4096 (p = %g)",
             CSL_MAX_LAYERS, (double)p);
    return CSL_E_INVALID;
  }
  ok = eps > 0.f && (n_layers == 1 || (gammas && betas));
  for (int k = 0; ok && k + 1 < n_layers; k++) ok = gammas[k] && betas[k] && aligned16(gammas[k]) && aligned16(betas[k]);
  if (!ok) {
    snprintf(s_err, sizeof(s_err), "norm: eps > 0 and a 16-byte aligned gamma and beta for every layer but the last expected "
             "(eps = %g)", (double)eps);
    return CSL_E_INVALID;
  }
  const DropArgs drop = {out_ids, p, seed, step};
  const MultiArgs multi = {label_words, ldw};
  const LossArgs lossw = {class_weight, label_smoothing};
  const NormArgs norm = {gammas, betas, eps};
  return sage_step(n_layers, dims, Layers(n_layers, sl), weights, biases, feat, kind, ldf, feat_rows, seed_ids, nullptr,
                   label_words ? nullptr : labels, scale, row_pad, n_slabs, nullptr, grads, loss, workspace, workspace_floats, stream,
                   plain ? nullptr : &drop, label_words ? &multi : nullptr,
                   label_words || (!class_weight && label_smoothing == 0.f) ? nullptr : &lossw,   // (no option: the plain loss pass)
                   n_layers > 1 ? &norm : nullptr);
}

}  // extern "C"
