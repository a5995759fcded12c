// gat_dropout.hip -- attention dropout inside the fused edge-softmax aggregation (cslicer_gat_dropout.h): the
// dropped twins of aggregate.hip's k_gat_fwd / k_gat_bwd / k_gat_bwd_t / k_gat_bwd_t2, each with its parent's dispatch
// and register layouts.  A twin differs from its parent in ONE factor per edge and head: kappa_e in {0, s_a}, Philox of
// (source node id, destination node id, head quad | layer, step), multiplies the edge's weight p_e wherever it meets z or
// g_n -- the numerator, the z gradient, the dot product of the logit gradient -- and nowhere else: the denominator s, the
// stabiliser m and the g_s term see the undropped p_e.  A lane needs its own head's word only: one Philox call per edge
// and lane, computed where the edge is accumulated and never kept.  Below them the dropped epilogue pair: feature
// dropout written by the layer's epilogue beside its undropped output, and applied to the gradient as the backward loads it.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "cslicer_gat_dropout.h"
#include "dev_common.h"
#include "gat_dev.h"
#include "philox_dev.h"

namespace {

constexpr int BLK = 256;

__device__ __forceinline__ float leaky(float x, float slope) { return x > 0.f ? x : slope * x; }

// what every twin takes on top of its parent's arguments (by value: 40 bytes of kernel arguments)
struct AttnDrop {
  const int* src_ids;   // node id of source row u (the slice's in_nodes)
  const int* dst_ids;   // node id of destination row r (the slice's out_nodes)
  uint32_t thr;         // T = floor(p 2^32)
  float s;              // (float)(1 / (1 - p))
  uint32_t k0, k1;      // the key: the seed's two halves
  uint32_t w2;          // 0x80000000 | layer: the counter's third word without the head quad
  uint32_t step;        // t mod 2^32
};

// kappa of edge (u -> v) for head h: s if the head's word keeps the edge, else 0
__device__ __forceinline__ float kappa(uint32_t u, uint32_t v, int h, const AttnDrop& d) {
  const uint4 w = philox4x32_10(make_uint4(u, v, d.w2 | ((uint32_t)(h >> 2) << 8), d.step), d.k0, d.k1);
  const int j = h & 3;
  const uint32_t x = j == 0 ? w.x : j == 1 ? w.y : j == 2 ? w.z : w.w;
  return x >= d.thr ? d.s : 0.f;
}

// k_gat_fwd with the numerator dropped.  Both branches of the parent: the row of at most 16 edges and one chunk of columns
// with every load in flight before the first use (lane j also fetches the NODE id of edge j's source; it travels with the
// same shuffle as the row index), and the general chunked loop.  kappa is formed inside the accumulate loop, edge by edge:
// the 16 float4 and 16 logits of the first branch leave no room for 16 more live values.
__global__ __launch_bounds__(BLK) void k_gat_drop_fwd(const int* __restrict__ indptr, const int* __restrict__ indices,
                                                      long long n_rows, const float* __restrict__ el,
                                                      const float* __restrict__ er, const float* __restrict__ z, int H,
                                                      int D, float slope, float* __restrict__ m_out,
                                                      float* __restrict__ s_out, float* __restrict__ n_out, AttnDrop d) {
  const int lane = threadIdx.x & 63;
  const long long r = (long long)blockIdx.x * (BLK / 64) + (threadIdx.x >> 6);
  if (r >= n_rows) return;
  const int C = H * D;
  const int lpc = (64 / (D / 4)) * (D / 4);  // lanes per chunk: whole heads only
  const int e0 = indptr[r], e1 = indptr[r + 1];
  const uint32_t v = (uint32_t)d.dst_ids[r];
  constexpr int EK = 16;
  if (e1 - e0 <= EK && C <= lpc * 4) {
    const int deg = e1 - e0;
    const int c = lane * 4;
    const bool on = lane < lpc && c < C;
    const int h = on ? c / D : 0;
    if (deg == 0) {   // (no edge: nothing to read; the state of an empty softmax)
      if (on) {
        *reinterpret_cast<float4*>(n_out + r * C + c) = make_float4(0.f, 0.f, 0.f, 0.f);
        if (c % D == 0) {
          m_out[r * H + h] = -1e30f;
          s_out[r * H + h] = 0.f;
        }
      }
      return;
    }
    const int src_l = indices[e0 + (lane < deg ? lane : 0)];
    const int uid_l = d.src_ids[src_l];
    const float erv = er[r * H + h];
    float elv[EK];
    float4 zv[EK];
#pragma unroll
    for (int e = 0; e < EK; e++) {
      const long long src = __shfl(src_l, e < deg ? e : 0);
      elv[e] = el[src * H + h];
      zv[e] = *reinterpret_cast<const float4*>(z + src * C + (on ? c : 0));
    }
    float m = -1e30f;
#pragma unroll
    for (int e = 0; e < EK; e++)
      if (e < deg) m = fmaxf(m, leaky(elv[e] + erv, slope));
    float s = 0.f;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int e = 0; e < EK; e++) {
      if (e < deg) {
        const float p = expf(leaky(elv[e] + erv, slope) - m);
        s += p;
        const float kp = kappa((uint32_t)__shfl(uid_l, e), v, h, d) * p;
        acc.x += kp * zv[e].x, acc.y += kp * zv[e].y, acc.z += kp * zv[e].z, acc.w += kp * zv[e].w;
      }
    }
    if (on) {
      *reinterpret_cast<float4*>(n_out + r * C + c) = acc;
      if (c % D == 0) {
        m_out[r * H + h] = m;
        s_out[r * H + h] = s;
      }
    }
    return;
  }
  for (int c0 = 0; c0 < C; c0 += lpc * 4) {
    const int c = c0 + lane * 4;
    const bool on = lane < lpc && c < C;
    const int h = on ? c / D : 0;
    const float erv = er[r * H + h];
    float m = -1e30f;
    for (int e = e0; e < e1; e++) m = fmaxf(m, leaky(el[(long long)indices[e] * H + h] + erv, slope));
    float s = 0.f;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int e = e0; e < e1; e++) {
      const long long src = indices[e];
      const float p = expf(leaky(el[src * H + h] + erv, slope) - m);
      s += p;
      if (on) {
        const float4 zv = *reinterpret_cast<const float4*>(z + src * C + c);
        const float kp = kappa((uint32_t)d.src_ids[src], v, h, d) * p;
        acc.x += kp * zv.x;
        acc.y += kp * zv.y;
        acc.z += kp * zv.z;
        acc.w += kp * zv.w;
      }
    }
    if (on) {
      *reinterpret_cast<float4*>(n_out + r * C + c) = acc;
      if (c % D == 0) {
        m_out[r * H + h] = m;
        s_out[r * H + h] = s;
      }
    }
  }
}

// k_gat_bwd with the numerator dropped: g_z[u] += kappa p g_n and g_logit = (g_s + kappa <g_n, z_u>) p lrelu'.  The z
// gradient leaves in the parent's second register layout (64 consecutive floats per atomic instruction); the weight a
// column needs there is kappa p of its head, shuffled from a lane of the float4 layout that owns the head.
__global__ __launch_bounds__(BLK) void k_gat_drop_bwd(const int* __restrict__ indptr, const int* __restrict__ indices,
                                                      long long n_rows, const float* __restrict__ el,
                                                      const float* __restrict__ er, const float* __restrict__ z, int H,
                                                      int D, float slope, const float* __restrict__ m_in,
                                                      const float* __restrict__ g_s, const float* __restrict__ g_n,
                                                      float* g_el, float* __restrict__ g_er, float* g_z, AttnDrop d) {
  const int lane = threadIdx.x & 63;
  const long long r = (long long)blockIdx.x * (BLK / 64) + (threadIdx.x >> 6);
  if (r >= n_rows) return;
  const int C = H * D;
  const int gsz = D / 4;              // lanes of one head
  const int lpc = (64 / gsz) * gsz;   // lanes per chunk: whole heads only
  const int gl = lane % gsz;          // position inside the head's lane group
  const int e0 = indptr[r], e1 = indptr[r + 1];
  const uint32_t v = (uint32_t)d.dst_ids[r];
  for (int c0 = 0; c0 < C; c0 += lpc * 4) {
    const int c = c0 + lane * 4;
    const bool on = lane < lpc && c < C;
    const int h = on ? c / D : 0;
    const float erv = er[r * H + h], mh = m_in[r * H + h], gs = g_s[r * H + h];
    const float4 gn = on ? *reinterpret_cast<const float4*>(g_n + r * C + c) : make_float4(0.f, 0.f, 0.f, 0.f);
    const int chunk_end = c0 + lpc * 4 < C ? c0 + lpc * 4 : C;
    float gn2[4];
    int p_lane[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const int col = c0 + lane + 64 * k;
      gn2[k] = col < chunk_end ? g_n[r * C + col] : 0.f;
      p_lane[k] = col < chunk_end ? ((col / D) * D - c0) / 4 : 0;
    }
    float ger = 0.f;
    for (int e = e0; e < e1; e++) {
      const long long src = indices[e];
      const float raw = el[src * H + h] + erv;
      const float p = expf(leaky(raw, slope) - mh);
      const float kap = kappa((uint32_t)d.src_ids[src], v, h, d);
      float dot = 0.f;
      if (on) {
        const float4 zv = *reinterpret_cast<const float4*>(z + src * C + c);
        dot = gn.x * zv.x + gn.y * zv.y + gn.z * zv.z + gn.w * zv.w;
      }
      // sum over the head's lane group (any size): segmented tree, then the leader's value for all
      for (int o = 1; o < gsz; o <<= 1) {
        const float t = __shfl_down(dot, o);
        if (gl + o < gsz) dot += t;
      }
      dot = __shfl(dot, lane - gl);
      const float gsc = (gs + kap * dot) * p * (raw > 0.f ? 1.f : slope);
      const float kp = kap * p;
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const float pk = __shfl(kp, p_lane[k]);
        const int col = c0 + lane + 64 * k;
        if (col < chunk_end) atomicAdd(g_z + src * C + col, pk * gn2[k]);
      }
      if (on && c % D == 0) {
        atomicAdd(g_el + src * H + h, gsc);
        ger += gsc;
      }
    }
    if (on && c % D == 0) g_er[r * H + h] = ger;
  }
}

// k_gat_bwd_t (the backward by source) with the numerator dropped; the source's node id is read once per row
__global__ __launch_bounds__(BLK) void k_gat_drop_bwd_t(const int* __restrict__ tptr, const int* __restrict__ trow,
                                                        long long n_src, long long n_pad, const float* __restrict__ el,
                                                        const float* __restrict__ er, const float* __restrict__ z, int H,
                                                        int D, float slope, const float* __restrict__ m_in,
                                                        const float* __restrict__ g_s, const float* __restrict__ g_n,
                                                        float* __restrict__ g_el, float* g_er, float* __restrict__ g_z,
                                                        AttnDrop d) {
  const int lane = threadIdx.x & 63;
  const long long u = (long long)blockIdx.x * (BLK / 64) + (threadIdx.x >> 6);
  if (u >= n_pad) return;
  const int C = H * D, gsz = D / 4, lpc = (64 / gsz) * gsz, gl = lane % gsz;
  const int j0 = u < n_src ? tptr[u] : 0, j1 = u < n_src ? tptr[u + 1] : 0;
  const uint32_t uid = u < n_src ? (uint32_t)d.src_ids[u] : 0u;
  for (int c0 = 0; c0 < C; c0 += lpc * 4) {
    const int c = c0 + lane * 4;
    const bool on = lane < lpc && c < C;
    const int h = on ? c / D : 0;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f), zv = acc;
    float elu = 0.f, gel = 0.f;
    if (u < n_src) {
      elu = el[u * H + h];
      if (on) zv = *reinterpret_cast<const float4*>(z + u * C + c);
    }
    for (int j = j0; j < j1; j++) {
      const int r = trow[j];  // (wave-uniform)
      if (r < 0) continue;    // the node's self entry: attention runs over the sampled edges only
      const float raw = elu + er[(long long)r * H + h];
      const float p = expf(leaky(raw, slope) - m_in[(long long)r * H + h]);
      const float kap = kappa(uid, (uint32_t)d.dst_ids[r], h, d);
      float dot = 0.f;
      float4 gn = make_float4(0.f, 0.f, 0.f, 0.f);
      if (on) {
        gn = *reinterpret_cast<const float4*>(g_n + (long long)r * C + c);
        dot = gn.x * zv.x + gn.y * zv.y + gn.z * zv.z + gn.w * zv.w;
      }
      for (int o = 1; o < gsz; o <<= 1) {  // sum over the head's lane group
        const float t = __shfl_down(dot, o);
        if (gl + o < gsz) dot += t;
      }
      dot = __shfl(dot, lane - gl);
      const float gsc = (g_s[(long long)r * H + h] + kap * dot) * p * (raw > 0.f ? 1.f : slope);
      const float kp = kap * p;
      acc.x += kp * gn.x, acc.y += kp * gn.y, acc.z += kp * gn.z, acc.w += kp * gn.w;
      if (on && c % D == 0) {
        gel += gsc;
        atomicAdd(g_er + (long long)r * H + h, gsc);
      }
    }
    if (on) {
      *reinterpret_cast<float4*>(g_z + u * C + c) = acc;
      if (u < n_src && c % D == 0) g_el[u * H + h] = gel;
    }
  }
}

// k_gat_bwd_t2 (by source, the el half of the logits' backward folded in) with the numerator dropped.  Its second stage
// over the destinations, k_gat_logits_bwd_dst, knows nothing of dropout (g_er is complete when it runs) and is the parent's.
__global__ __launch_bounds__(BLK) void k_gat_drop_bwd_t2(const int* __restrict__ tptr, const int* __restrict__ trow,
                                                         long long n_src, long long n_pad, const float* __restrict__ el,
                                                         const float* __restrict__ er, const float* __restrict__ z, int H,
                                                         int D, float slope, const float* __restrict__ m_in,
                                                         const float* __restrict__ g_s, const float* __restrict__ g_n,
                                                         const float* __restrict__ al, float* g_er,
                                                         float* __restrict__ g_z, float* __restrict__ part_l,
                                                         long long rows_per_block, AttnDrop d) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int C = H * D, gsz = D / 4, lpc = (64 / gsz) * gsz, gl = lane % gsz;
  const long long r0 = (long long)blockIdx.x * rows_per_block;
  const long long r_end = r0 + rows_per_block < n_pad ? r0 + rows_per_block : n_pad;
  __shared__ float4 s_l[BLK];
  for (int c0 = 0; c0 < C; c0 += lpc * 4) {   // block-uniform
    const int c = c0 + lane * 4;
    const bool on = lane < lpc && c < C;
    const int h = on ? c / D : 0;
    float4 a4 = make_float4(0.f, 0.f, 0.f, 0.f), pl = a4;
    if (on) a4 = *reinterpret_cast<const float4*>(al + c);
    for (long long u = r0 + w; u < r_end; u += BLK / 64) {
      const int j0 = u < n_src ? tptr[u] : 0, j1 = u < n_src ? tptr[u + 1] : 0;
      const uint32_t uid = u < n_src ? (uint32_t)d.src_ids[u] : 0u;
      float4 acc = make_float4(0.f, 0.f, 0.f, 0.f), zv = acc;
      float elu = 0.f, gel = 0.f;
      if (u < n_src) {
        elu = el[u * H + h];
        if (on) zv = *reinterpret_cast<const float4*>(z + u * C + c);
      }
      for (int j = j0; j < j1; j++) {
        const int r = trow[j];  // (wave-uniform)
        if (r < 0) continue;    // the node's self entry: attention runs over the sampled edges only
        const float raw = elu + er[(long long)r * H + h];
        const float p = expf(leaky(raw, slope) - m_in[(long long)r * H + h]);
        const float kap = kappa(uid, (uint32_t)d.dst_ids[r], h, d);
        float dot = 0.f;
        float4 gn = make_float4(0.f, 0.f, 0.f, 0.f);
        if (on) {
          gn = *reinterpret_cast<const float4*>(g_n + (long long)r * C + c);
          dot = gn.x * zv.x + gn.y * zv.y + gn.z * zv.z + gn.w * zv.w;
        }
        for (int o = 1; o < gsz; o <<= 1) {  // sum over the head's lane group
          const float t = __shfl_down(dot, o);
          if (gl + o < gsz) dot += t;
        }
        dot = __shfl(dot, lane - gl);
        const float gsc = (g_s[(long long)r * H + h] + kap * dot) * p * (raw > 0.f ? 1.f : slope);
        const float kp = kap * p;
        acc.x += kp * gn.x, acc.y += kp * gn.y, acc.z += kp * gn.z, acc.w += kp * gn.w;
        gel += gsc;   // (every lane of the head's group carries the same value)
        if (on && c % D == 0) atomicAdd(g_er + (long long)r * H + h, gsc);
      }
      if (on) {
        acc.x += gel * a4.x, acc.y += gel * a4.y, acc.z += gel * a4.z, acc.w += gel * a4.w;   // + g_el a_l
        *reinterpret_cast<float4*>(g_z + u * C + c) = acc;
        pl.x += gel * zv.x, pl.y += gel * zv.y, pl.z += gel * zv.z, pl.w += gel * zv.w;       // g_attn_l's share
      }
    }
    __syncthreads();
    s_l[threadIdx.x] = pl;
    __syncthreads();
    if (w == 0 && on) {
      for (int k = 1; k < BLK / 64; k++) add4(pl, s_l[k * 64 + lane]);
      *reinterpret_cast<float4*>(part_l + (long long)blockIdx.x * C + c) = pl;
    }
  }
}

// ---- the dropped epilogue pair (feature dropout behind the layer's ELU): k_gat_finish_fwd / k_gat_finish_bwd of
// aggregate.hip with cslicer_dropout.h's mask, keyed by the out node's id and the column quad over all H * D columns.
struct FeatDrop {
  const int* ids;       // node id of output row r (the slice's out_nodes)
  uint32_t thr;
  float s;
  uint32_t k0, k1, layer, step;
};

__device__ __forceinline__ float4 feat_mask(float4 a, int c, uint32_t v, const FeatDrop& d) {
  const uint4 w = philox4x32_10(make_uint4((uint32_t)(c >> 2), v, d.layer, d.step), d.k0, d.k1);
  a.x = w.x >= d.thr ? a.x * d.s : 0.f;
  a.y = w.y >= d.thr ? a.y * d.s : 0.f;
  a.z = w.z >= d.thr ? a.z * d.s : 0.f;
  a.w = w.w >= d.thr ? a.w * d.s : 0.f;
  return a;
}

// out = act(n / s + bias) (kept for ELU') and y = the dropped out, in one pass: one more store, no more load
__global__ __launch_bounds__(BLK) void k_gat_finish_drop_fwd(const float* __restrict__ nsum, const float* __restrict__ ssum,
                                                             const float* __restrict__ bias, long long n, int H, int D,
                                                             int elu, float* __restrict__ out, float* __restrict__ y,
                                                             FeatDrop d) {
  const int lane = threadIdx.x & 63;
  const long long r = (long long)blockIdx.x * (BLK / 64) + (threadIdx.x >> 6);
  if (r >= n) return;
  const int C = H * D, gsz = D / 4, lpc = (64 / gsz) * gsz;
  const uint32_t v = (uint32_t)d.ids[r];
  for (int c0 = 0; c0 < C; c0 += lpc * 4) {
    const int c = c0 + lane * 4;
    if (lane >= lpc || c >= C) continue;
    const float inv = 1.f / fmaxf(ssum[r * H + c / D], 1e-30f);
    float4 o = *reinterpret_cast<const float4*>(nsum + r * C + c);
    const float4 b = *reinterpret_cast<const float4*>(bias + c);
    o.x = o.x * inv + b.x, o.y = o.y * inv + b.y, o.z = o.z * inv + b.z, o.w = o.w * inv + b.w;
    if (elu) o.x = o.x > 0.f ? o.x : expm1f(o.x), o.y = o.y > 0.f ? o.y : expm1f(o.y), o.z = o.z > 0.f ? o.z : expm1f(o.z), o.w = o.w > 0.f ? o.w : expm1f(o.w);
    *reinterpret_cast<float4*>(out + r * C + c) = o;
    *reinterpret_cast<float4*>(y + r * C + c) = feat_mask(o, c, v, d);
  }
}

// k_gat_finish_bwd with the mask applied to g as it is loaded; everything behind that is the parent's
__global__ __launch_bounds__(BLK) void k_gat_finish_drop_bwd(const float* __restrict__ g, long long ldg,
                                                             const float* __restrict__ out, const float* __restrict__ nsum,
                                                             const float* __restrict__ ssum, long long n, int H, int D,
                                                             int elu, float* __restrict__ g_n, float* __restrict__ g_s,
                                                             float* __restrict__ part, long long rows_per_block, FeatDrop d) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int C = H * D, gsz = D / 4, lpc = (64 / gsz) * gsz, gl = lane % gsz;
  const long long r0 = (long long)blockIdx.x * rows_per_block;
  const long long r_end = r0 + rows_per_block < n ? r0 + rows_per_block : n;
  __shared__ float s_p[BLK * 4];
  for (int c0 = 0; c0 < C; c0 += lpc * 4) {  // block-uniform
    const int c = c0 + lane * 4;
    const bool on = lane < lpc && c < C;
    const int h = on ? c / D : 0;
    float4 colacc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (long long r = r0 + w; r < r_end; r += BLK / 64) {  // wave-uniform
      float dot = 0.f;
      if (on) {
        float4 p = feat_mask(*reinterpret_cast<const float4*>(g + r * ldg + c), c, (uint32_t)d.ids[r], d);
        if (elu) {
          const float4 o = *reinterpret_cast<const float4*>(out + r * C + c);
          p.x *= o.x > 0.f ? 1.f : o.x + 1.f, p.y *= o.y > 0.f ? 1.f : o.y + 1.f;
          p.z *= o.z > 0.f ? 1.f : o.z + 1.f, p.w *= o.w > 0.f ? 1.f : o.w + 1.f;
        }
        add4(colacc, p);
        const float inv = 1.f / fmaxf(ssum[r * H + h], 1e-30f);
        const float4 nv = *reinterpret_cast<const float4*>(nsum + r * C + c);
        p.x *= inv, p.y *= inv, p.z *= inv, p.w *= inv;
        *reinterpret_cast<float4*>(g_n + r * C + c) = p;
        dot = -(p.x * nv.x + p.y * nv.y + p.z * nv.z + p.w * nv.w) * inv;
      }
      for (int o = 1; o < gsz; o <<= 1) {  // segmented tree over the head's lane group
        const float t = __shfl_down(dot, o);
        if (gl + o < gsz) dot += t;
      }
      if (on && gl == 0) g_s[r * H + h] = dot;
    }
    __syncthreads();
    reinterpret_cast<float4*>(s_p)[threadIdx.x] = colacc;
    __syncthreads();
    if (w == 0 && on) {
      for (int k = 1; k < BLK / 64; k++) add4(colacc, reinterpret_cast<float4*>(s_p)[k * 64 + lane]);
      *reinterpret_cast<float4*>(part + (long long)blockIdx.x * C + c) = colacc;
    }
  }
}

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

// the twins' common arguments, checked and packed: false for what cslicer_gat_dropout.h refuses
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

bool shape_ok(int32_t H, int32_t D) { return H >= 1 && H <= (1 << 24) && D >= 4 && D % 4 == 0 && D <= 256; }

dim3 wave_rows(long long rows) { return dim3((unsigned)((rows + BLK / 64 - 1) / (BLK / 64))); }

}  // namespace

extern "C" {

int csl_gat_drop_fwd_f32(const int32_t* indptr, const int32_t* indices, int64_t n_rows, const float* el, const float* er,
                         const float* z, int32_t H, int32_t D, float slope, float* m_out, float* s_out, float* n_out,
                         const int32_t* src_ids, const int32_t* dst_ids, float p_a, int64_t seed, int32_t layer,
                         int64_t step, void* stream) {
  AttnDrop d;
  if (!attn_drop(src_ids, dst_ids, p_a, seed, layer, step, &d) || n_rows < 0 || !shape_ok(H, D)) return CSL_E_INVALID;
  if (n_rows == 0) return CSL_OK;
  if (!indptr || !er || !m_out || !s_out || !n_out || !src_ids || !dst_ids || !aligned16(z) || !aligned16(n_out))
    return CSL_E_INVALID;
  hipLaunchKernelGGL(k_gat_drop_fwd, wave_rows(n_rows), dim3(BLK), 0, (hipStream_t)stream, indptr, indices,
                     (long long)n_rows, el, er, z, (int)H, (int)D, slope, m_out, s_out, n_out, d);
  return done();
}

int csl_gat_drop_bwd_f32(const int32_t* indptr, const int32_t* indices, int64_t n_rows, const float* el, const float* er,
                         const float* z, int32_t H, int32_t D, float slope, const float* m_in, const float* g_s,
                         const float* g_n, float* g_el, float* g_er, float* g_z, const int32_t* src_ids,
                         const int32_t* dst_ids, float p_a, int64_t seed, int32_t layer, int64_t step, void* stream) {
  AttnDrop d;
  if (!attn_drop(src_ids, dst_ids, p_a, seed, layer, step, &d) || n_rows < 0 || !shape_ok(H, D)) return CSL_E_INVALID;
  if (n_rows == 0) return CSL_OK;
  if (!indptr || !er || !m_in || !g_s || !g_n || !g_er || !src_ids || !dst_ids || !aligned16(z) || !aligned16(g_n) ||
      !aligned16(g_z))
    return CSL_E_INVALID;
  hipLaunchKernelGGL(k_gat_drop_bwd, wave_rows(n_rows), dim3(BLK), 0, (hipStream_t)stream, indptr, indices,
                     (long long)n_rows, el, er, z, (int)H, (int)D, slope, m_in, g_s, g_n, g_el, g_er, g_z, d);
  return done();
}

int csl_gat_drop_bwd_t_f32(const int32_t* t_indptr, const int32_t* t_indices, int64_t n_src, int64_t n_pad,
                           const float* el, const float* er, const float* z, int32_t H, int32_t D, float slope,
                           const float* m_in, const float* g_s, const float* g_n, float* g_el, float* g_er, float* g_z,
                           const int32_t* src_ids, const int32_t* dst_ids, float p_a, int64_t seed, int32_t layer,
                           int64_t step, void* stream) {
  AttnDrop d;
  if (!attn_drop(src_ids, dst_ids, p_a, seed, layer, step, &d) || n_src < 0 || n_pad < n_src || !shape_ok(H, D))
    return CSL_E_INVALID;
  if (n_pad == 0) return CSL_OK;
  if (!g_z || !aligned16(g_z) || (n_src > 0 && (!t_indptr || !el || !z || !g_el || !aligned16(z)))) return CSL_E_INVALID;
  if (n_src > 0 && (!er || !m_in || !g_s || !g_n || !g_er || !aligned16(g_n) || !src_ids || !dst_ids)) return CSL_E_INVALID;
  hipLaunchKernelGGL(k_gat_drop_bwd_t, wave_rows(n_pad), dim3(BLK), 0, (hipStream_t)stream, t_indptr, t_indices,
                     (long long)n_src, (long long)n_pad, el, er, z, (int)H, (int)D, slope, m_in, g_s, g_n, g_el, g_er, g_z, d);
  return done();
}

int csl_gat_drop_bwd_t_fused_f32(const int32_t* t_indptr, const int32_t* t_indices, int64_t n_src, int64_t n_pad,
                                 const float* el, const float* er_out, const float* z, int32_t H, int32_t D, float slope,
                                 const float* m_in, const float* g_s, const float* g_n, const float* attn_l,
                                 const float* attn_r, const int32_t* self_ids_in, int64_t n_out, float* g_er_out,
                                 float* g_z, float* g_attn_l, float* g_attn_r, float* scratch, const int32_t* src_ids,
                                 const int32_t* dst_ids, float p_a, int64_t seed, int32_t layer, int64_t step,
                                 void* stream) {
  AttnDrop d;
  if (!attn_drop(src_ids, dst_ids, p_a, seed, layer, step, &d) || n_src < 0 || n_pad < n_src || n_out < 0 ||
      !shape_ok(H, D) || !g_attn_l || !g_attn_r)
    return CSL_E_INVALID;
  hipStream_t st = (hipStream_t)stream;
  const int C = H * D;
  const long long r1 = gatx::t_rows(n_pad), r2 = gatx::t_rows(n_out);
  const long long b1 = (n_pad + r1 - 1) / r1, b2 = (n_out + r2 - 1) / r2;
  // every refusal before the first HIP call (the parent checks its second stage's arguments after its first launch)
  if (b1 > 0) {
    if (!g_z || !aligned16(g_z) || !scratch || !aligned16(scratch) || !attn_l || !aligned16(attn_l)) return CSL_E_INVALID;
    if (n_src > 0 && (!t_indptr || !el || !z || !aligned16(z) || !er_out || !m_in || !g_s || !g_n || !aligned16(g_n) ||
                      !g_er_out || !src_ids || !dst_ids))
      return CSL_E_INVALID;
  }
  if (b2 > 0 && (!attn_r || !aligned16(attn_r) || !self_ids_in || !scratch || !g_er_out || !z || !g_z)) return CSL_E_INVALID;
  if (b1 > 0) {
    if (n_out > 0 && hipMemsetAsync(g_er_out, 0, sizeof(float) * (size_t)n_out * H, st) != hipSuccess) return CSL_E_HIP;
    hipLaunchKernelGGL(k_gat_drop_bwd_t2, dim3((unsigned)b1), dim3(BLK), 0, st, t_indptr, t_indices, (long long)n_src,
                       (long long)n_pad, el, er_out, z, (int)H, (int)D, slope, m_in, g_s, g_n, attn_l, g_er_out, g_z, scratch,
                       r1, d);
  }
  if (b2 > 0) gatx::logits_bwd_dst(z, attn_r, self_ids_in, g_er_out, n_out, H, D, g_z, scratch + b1 * C, r2, stream);
  {
    // both second stages in one launch
    const float* src[2] = {scratch, scratch + b1 * C};
    const int64_t nb[2] = {b1, b2};
    const int32_t hh[2] = {C, C};
    float* dst[2] = {g_attn_l, g_attn_r};
    return csl_reduce_multi_f32(2, src, nb, hh, dst, stream);
  }
}

int csl_gat_finish_drop_fwd_f32(const float* n_in, const float* s_in, const float* bias, int64_t n, int32_t H, int32_t D,
                                int32_t elu, float* out, float* y, const int32_t* out_ids, float p_f, int64_t seed,
                                int32_t layer, int64_t step, void* stream) {
  FeatDrop d;
  if (!feat_drop(out_ids, p_f, seed, layer, step, &d) || n < 0 || !shape_ok(H, D)) return CSL_E_INVALID;
  if (n == 0) return CSL_OK;
  if (!n_in || !s_in || !bias || !out || !y || !out_ids || !aligned16(n_in) || !aligned16(bias) || !aligned16(out) ||
      !aligned16(y))
    return CSL_E_INVALID;
  hipLaunchKernelGGL(k_gat_finish_drop_fwd, wave_rows(n), dim3(BLK), 0, (hipStream_t)stream, n_in, s_in, bias, (long long)n,
                     (int)H, (int)D, (int)(elu != 0), out, y, d);
  return done();
}

int csl_gat_finish_drop_bwd_f32(const float* g, int64_t ldg, const float* out, const float* n_in, const float* s_in,
                                int64_t n, int32_t H, int32_t D, int32_t elu, float* g_n, float* g_s, float* g_bias,
                                float* scratch, const int32_t* out_ids, float p_f, int64_t seed, int32_t layer,
                                int64_t step, void* stream) {
  FeatDrop d;
  if (!feat_drop(out_ids, p_f, seed, layer, step, &d) || n < 0 || !shape_ok(H, D) || !g_bias) return CSL_E_INVALID;
  const int C = H * D;
  const long long rpb = gatx::finish_rows(n);
  const long long blocks = (n + rpb - 1) / rpb;
  if (blocks > 0) {
    if (!g || ldg < C || ldg % 4 != 0 || !n_in || !s_in || !g_n || !g_s || !scratch || !out_ids || (elu && !out) ||
        !aligned16(g) || !aligned16(n_in) || !aligned16(g_n) || !aligned16(scratch) || (out && !aligned16(out)))
      return CSL_E_INVALID;
    hipLaunchKernelGGL(k_gat_finish_drop_bwd, dim3((unsigned)blocks), dim3(BLK), 0, (hipStream_t)stream, g, (long long)ldg,
                       out, n_in, s_in, (long long)n, (int)H, (int)D, (int)(elu != 0), g_n, g_s, scratch, rpb, d);
  }
  gatx::colsum_finish(scratch, blocks, C, g_bias, stream);
  return done();
}

}  // extern "C"
