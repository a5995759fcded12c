// gat_dev.h -- the dropout policies of the attention kernels (private to csrc/; cslicer_gat_dropout.h).  Each
// attention kernel of aggregate.hip is a template over one of them, passed by value as its last argument: NoDrop is empty
// and the kernel is the undropped one, AttnDrop / FeatDrop carry what the mask needs and switch on the kernel's
// `if constexpr (DR::on)` statements.
//   Attention dropout: kappa_e in {0, s_a}, Philox of (source node id, destination node id, head quad | layer, step),
// multiplies the edge's weight p_e wherever it meets z or g_n -- the numerator, the z gradient, the dot product of the
// logit gradient -- and nowhere else: the denominator s, the stabiliser m and the g_s term see the undropped p_e.  A lane
// needs its own head's word only: one Philox call per edge and lane, computed where the edge is accumulated and never kept.
//   Feature dropout: cslicer_dropout.h's mask, keyed by the out node's id and the column quad over all H * D columns,
// written by the layer's epilogue beside its undropped output and applied to the gradient as the backward loads it.
#ifndef CSLICER_GAT_DEV_H
#define CSLICER_GAT_DEV_H

#include <hip/hip_runtime.h>

#include <cstdint>

#include "philox_dev.h"

namespace {

struct NoDrop {
  static constexpr bool on = false;
  bool ids_ok() const { return true; }
};

// what a dropped attention kernel takes on top of its parent's arguments (by value: 40 bytes of kernel arguments)
struct AttnDrop {
  static constexpr bool on = true;
  const int* src_ids;   // node id of source row u (the slice's in_nodes)
  const int* dst_ids;   // node id of destination row r (the slice's out_nodes)
  uint32_t thr;         // T = floor(p 2^32)
  float s;              // (float)(1 / (1 - p))
  uint32_t k0, k1;      // the key: the seed's two halves
  uint32_t w2;          // 0x80000000 | layer: the counter's third word without the head quad
  uint32_t step;        // t mod 2^32
  bool ids_ok() const { return src_ids && dst_ids; }
};

// kappa of edge (u -> v) for head h: s if the head's word keeps the edge, else 0
__device__ __forceinline__ float kappa(uint32_t u, uint32_t v, int h, const AttnDrop& d) {
  const uint4 w = philox4x32_10(make_uint4(u, v, d.w2 | ((uint32_t)(h >> 2) << 8), d.step), d.k0, d.k1);
  const int j = h & 3;
  const uint32_t x = j == 0 ? w.x : j == 1 ? w.y : j == 2 ? w.z : w.w;
  return x >= d.thr ? d.s : 0.f;
}

// the same for the epilogue pair
struct FeatDrop {
  static constexpr bool on = true;
  const int* ids;       // node id of output row r (the slice's out_nodes)
  uint32_t thr;
  float s;
  uint32_t k0, k1, layer, step;
  bool ids_ok() const { return ids != nullptr; }
};

// the quad at column c of the row of node v, masked
__device__ __forceinline__ float4 feat_mask(float4 a, int c, uint32_t v, const FeatDrop& d) {
  return drop4(a, philox4x32_10(make_uint4((uint32_t)(c >> 2), v, d.layer, d.step), d.k0, d.k1), d.thr, d.s);
}

// the policies packed from the entry points' arguments: false for what cslicer_gat_dropout.h refuses
bool feat_drop(const int32_t* ids, float p, int64_t seed, int32_t layer, int64_t step, FeatDrop* d) {
  if (!(p > 0.f && p < 1.f)) return false;
  const uint64_t sd = (uint64_t)seed;
  d->ids = ids;
  d->thr = (uint32_t)((double)p * 4294967296.0);
  d->s = (float)(1.0 / (1.0 - (double)p));
  d->k0 = (uint32_t)sd, d->k1 = (uint32_t)(sd >> 32);
  d->layer = (uint32_t)layer, d->step = (uint32_t)(uint64_t)step;
  return true;
}

bool attn_drop(const int32_t* src_ids, const int32_t* dst_ids, float p, int64_t seed, int32_t layer, int64_t step,
               AttnDrop* d) {
  if (!(p > 0.f && p < 1.f) || layer < 0 || layer >= 256) return false;
  const uint64_t sd = (uint64_t)seed;
  d->src_ids = src_ids, d->dst_ids = dst_ids;
  d->thr = (uint32_t)((double)p * 4294967296.0);   // (p < 1 in float32: below 2^32; the cast floors)
  d->s = (float)(1.0 / (1.0 - (double)p));
  d->k0 = (uint32_t)sd, d->k1 = (uint32_t)(sd >> 32);
  d->w2 = 0x80000000u | (uint32_t)layer;
  d->step = (uint32_t)(uint64_t)step;
  return true;
}

}  // namespace
#endif
