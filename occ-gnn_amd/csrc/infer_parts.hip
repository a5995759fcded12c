// infer_parts.hip -- full-neighbour inference split over the parts of the graph (include/cslicer_infer_parts.h), gfx950.
//
// A rank sums, per destination, the neighbours it owns (partial kernels), and merges the partials the other ranks sent
// for the destinations it owns (merge kernels).  The partial kernels keep the arithmetic of csrc/infer.hip exactly: a
// row's edges are split over the same G lane groups (edge j of an item to group j % G), each group adds its edges in
// ascending order (the attention kernel: in steps of T = min(G U, 64) edges with one rescale per step), and the groups
// are combined by the same xor butterfly; a row is then finished by csrc/infer.hip's own row ends (csrc/infer_dev.h,
// which both files include).  So with one part the results are bitwise those of csl_infer_*_f32.
//
// A wave may take `R` sub-CSR rows at once (the `pack` argument): slot s of the wave (64 / R lanes) holds one item, its
// G groups of 64 / (R G) lanes walk the row's column tiles.  Every lane loads the source index of its own edge, so a
// slot needs no cross-lane index broadcast.  The caller passes R = 1: packing was measured slower at every width
// (a slot's narrower tiles walk its edges once per tile).  No atomics anywhere.
//
// The GraphSAGE kernels that read the layer's input table (k_sage_part its rows, k_sage_merge the self row) are
// templated on its element type (csrc/feat_elem.h, include/cslicer_infer16.h), as csrc/infer.hip's are.
#include "cslicer_infer_parts.h"
#include "infer_dev.h"

namespace {

// the item of slot `slot` of this wave and its edge range [e0, e0 + n); n = 0 for a slot past the end of the list
struct Slot {
  bool live;
  int row, pos, e0, part, n;
};

template <int R>
__device__ __forceinline__ Slot slot_item(const int* __restrict__ indptr, const int4* __restrict__ items, long long n_items,
                                          int slot) {
  const long long it = ((long long)blockIdx.x * WPB + (threadIdx.x >> 6)) * R + slot;
  Slot s{it < n_items, 0, 0, 0, -1, 0};
  if (s.live) {
    const int4 item = items[it];
    const int rend = indptr[item.x + 1];
    s.row = item.x, s.pos = item.y, s.e0 = item.z, s.part = item.w;
    s.n = (item.w < 0 ? rend : (int)min((long long)item.z + SEG, (long long)rend)) - item.z;
  }
  return s;
}

// ---------------------------------------------------------------- GraphSAGE

template <int G, int R, typename E = float>
__global__ __launch_bounds__(BLK) void k_sage_part(const int* __restrict__ indptr, const int* __restrict__ indices,
                                                   const int4* __restrict__ items, long long n_items, long long pos0,
                                                   long long part0, const E* __restrict__ y, long long ldy, int W,
                                                   float* __restrict__ partial, float* __restrict__ send) {
  constexpr int SL = 64 / R, LG = SL / G, T = G * U < 64 ? G * U : 64;
  const int lane = threadIdx.x & 63, sl = lane % SL, g = sl / LG, q = sl % LG;
  const Slot it = slot_item<R>(indptr, items, n_items, lane / SL);   // (no early return: the butterfly needs every lane)
  const int W4 = W / 4;
  for (int t0 = 0; t0 < W4; t0 += LG) {
    const int c4 = t0 + q;
    const bool on = c4 < W4;
    float4 acc = f4zero();
    for (int j = 0; j < it.n; j += T) {
      typename feat::Elem<E>::Raw v[U];
#pragma unroll
      for (int u = 0; u < U; u++) {
        const int jj = j + u * G + g;
        const bool ok = on && u * G + g < T && jj < it.n;
        const int src = ok ? indices[it.e0 + jj] : 0;
        v[u] = ok ? feat::Elem<E>::ld(y + (long long)src * ldy + 4 * c4) : feat::Elem<E>::zero();
      }
#pragma unroll
      for (int u = 0; u < U; u++) add4(acc, feat::Elem<E>::up(v[u]));
    }
#pragma unroll
    for (int d = LG; d < SL; d <<= 1) add4(acc, shfl_xor4(acc, d));
    if (it.live && g == 0 && on) {
      float* dst = it.part >= 0 ? partial + (long long)(it.part - part0) * W : send + (long long)(it.pos - pos0) * W;
      st4(dst + 4 * c4, acc);
    }
  }
}

// one wave per hub row of the sub-CSR: its items' partials added in part order into the row's send row
__global__ __launch_bounds__(BLK) void k_sage_part_hubs(const int4* __restrict__ hubs, long long n_hubs, long long pos0,
                                                        long long part0, int W, const float* __restrict__ partial,
                                                        float* __restrict__ send) {
  const int lane = threadIdx.x & 63;
  const long long hi = (long long)blockIdx.x * WPB + (threadIdx.x >> 6);
  if (hi >= n_hubs) return;
  const int4 hub = hubs[hi];
  const int W4 = W / 4;
  const long long p0 = (long long)hub.z - part0;
  for (int c4 = lane; c4 < W4; c4 += 64) {
    float4 acc = f4zero();
    int p = 0;
    for (; p + U <= hub.w; p += U) {
      float4 v[U];
#pragma unroll
      for (int u = 0; u < U; u++) v[u] = ld4(partial + (p0 + p + u) * W + 4 * c4);
#pragma unroll
      for (int u = 0; u < U; u++) add4(acc, v[u]);
    }
    for (; p < hub.w; p++) add4(acc, ld4(partial + (p0 + p) * W + 4 * c4));
    st4(send + ((long long)hub.y - pos0) * W + 4 * c4, acc);
  }
}

// G destinations per wave, 64 / G lanes each: the received partials in list order, then the row's end
template <int G, typename E = float>
__global__ __launch_bounds__(BLK) void k_sage_merge(const int2* __restrict__ dst, const int* __restrict__ lists, long long n,
                                                    int P, const float* __restrict__ recv, const E* __restrict__ x,
                                                    long long ldx, int W, int proj, const float* __restrict__ bias, int relu,
                                                    float* __restrict__ out, long long ldo) {
  constexpr int LG = 64 / G;
  const int lane = threadIdx.x & 63, q = lane % LG;
  const long long i = ((long long)blockIdx.x * WPB + (threadIdx.x >> 6)) * G + lane / LG;
  if (i >= n) return;                                          // (no cross-lane traffic below)
  const int2 d = dst[i];
  const int* li = lists + i * P;
  const int W4 = W / 4;
  for (int c4 = q; c4 < W4; c4 += LG) {
    float4 acc = f4zero();
    for (int p = 0; p < P; p++) {
      const int r = li[p];
      if (r >= 0) add4(acc, ld4(recv + (long long)r * W + 4 * c4));
    }
    sage_finish(x, ldx, W, proj, bias, relu, out, ldo, i, d.x, d.y, c4, acc);
  }
}

// ---------------------------------------------------------------- GAT

template <int G, int R>
__global__ __launch_bounds__(BLK) void k_gat_part(const int* __restrict__ indptr, const int* __restrict__ indices,
                                                  const int4* __restrict__ items, long long n_items, long long pos0,
                                                  long long part0, const float* __restrict__ z, const float* __restrict__ el,
                                                  const float* __restrict__ er_rows, int H, int D, float slope,
                                                  float* __restrict__ partial, long long pld, float* __restrict__ send) {
  constexpr int SL = 64 / R, LG = SL / G, T = G * U < 64 ? G * U : 64;
  const int lane = threadIdx.x & 63, sl = lane % SL, g = sl / LG, q = sl % LG;
  const Slot it = slot_item<R>(indptr, items, n_items, lane / SL);
  const int C = H * D, C4 = C / 4, Dq = D / 4;
  for (int t0 = 0; t0 < C4; t0 += LG) {
    const int c4 = t0 + q;
    const bool on = c4 < C4;
    const int h = on ? c4 / Dq : 0;
    const float erv = it.live ? er_rows[(long long)(it.pos - pos0) * H + h] : 0.f;
    float m = -1e30f, s = 0.f;
    float4 n = f4zero();
    for (int j = 0; j < it.n; j += T) {
      float sc[U];
      float4 v[U];
#pragma unroll
      for (int u = 0; u < U; u++) {
        const int jj = j + u * G + g;
        const bool ok = on && u * G + g < T && jj < it.n;
        const int src = ok ? indices[it.e0 + jj] : 0;
        const float l = ok ? el[(long long)src * H + h] + erv : 0.f;
        sc[u] = ok ? (l > 0.f ? l : l * slope) : -INFINITY;
        v[u] = ok ? ld4(z + (long long)src * C + 4 * c4) : f4zero();
      }
      float mb = m;
#pragma unroll
      for (int u = 0; u < U; u++) mb = fmaxf(mb, sc[u]);
      const float a = expf(m - mb);
      s *= a;
      scale4(n, a);
#pragma unroll
      for (int u = 0; u < U; u++) {
        const float p = expf(sc[u] - mb);
        s += p;
        fma4(n, p, v[u]);
      }
      m = mb;
    }
#pragma unroll
    for (int d = LG; d < SL; d <<= 1) {
      const float m2 = __shfl_xor(m, d), s2 = __shfl_xor(s, d);
      lse_merge(m, s, n, m2, s2, shfl_xor4(n, d));
    }
    if (it.live && g == 0 && on) {
      float* pr = it.part >= 0 ? partial + (long long)(it.part - part0) * pld : send + (long long)(it.pos - pos0) * pld;
      st4(pr + 4 * c4, n);
      if (c4 % Dq == 0) pr[C + h] = m, pr[C + H + h] = s;
    }
  }
}

// one wave per hub row of the sub-CSR: its items' states merged in part order into the row's send row
__global__ __launch_bounds__(BLK) void k_gat_part_hubs(const int4* __restrict__ hubs, long long n_hubs, long long pos0,
                                                       long long part0, int H, int D, const float* __restrict__ partial,
                                                       long long pld, float* __restrict__ send) {
  const int lane = threadIdx.x & 63;
  const long long hi = (long long)blockIdx.x * WPB + (threadIdx.x >> 6);
  if (hi >= n_hubs) return;
  const int4 hub = hubs[hi];
  const int C = H * D, C4 = C / 4, Dq = D / 4;
  const long long p0 = (long long)hub.z - part0;
  float* out = send + ((long long)hub.y - pos0) * pld;
  for (int c4 = lane; c4 < C4; c4 += 64) {
    const int h = c4 / Dq;
    float m = -1e30f, s = 0.f;
    float4 n = f4zero();
    for (int p = 0; p < hub.w; p++) {
      const float* pr = partial + (p0 + p) * pld;
      lse_merge_hub(m, s, n, pr[C + h], pr[C + H + h], ld4(pr + 4 * c4));
    }
    st4(out + 4 * c4, n);
    if (c4 % Dq == 0) out[C + h] = m, out[C + H + h] = s;
  }
}

// one wave per destination: the received states merged in list order into the zero state, then the row's end
__global__ __launch_bounds__(BLK) void k_gat_merge(const int* __restrict__ lists, long long n, int P,
                                                   const float* __restrict__ recv, long long pld, int H, int D,
                                                   const float* __restrict__ bias, int last, int n_cls,
                                                   float* __restrict__ out, long long ldo) {
  extern __shared__ float lds[];
  const int lane = threadIdx.x & 63;
  const long long i = (long long)blockIdx.x * WPB + (threadIdx.x >> 6);
  if (i >= n) return;
  const int C = H * D, C4 = C / 4, Dq = D / 4;
  float* stage = lds + (threadIdx.x >> 6) * C;
  const int* li = lists + i * P;
  for (int c4 = lane; c4 < C4; c4 += 64) {
    const int h = c4 / Dq;
    float m = -1e30f, s = 0.f;
    float4 nn = f4zero();
    for (int p = 0; p < P; p++) {
      const int r = li[p];
      if (r < 0) continue;
      const float* pr = recv + (long long)r * pld;
      lse_merge(m, s, nn, pr[C + h], pr[C + H + h], ld4(pr + 4 * c4));
    }
    gat_finish(bias, last, out, ldo, stage, i, c4, s, nn);
  }
  if (last) gat_head_mean(stage, H, D, n_cls, out, ldo, i, lane);
}

// ---------------------------------------------------------------- host side (plan_ok, with_*: infer_dev.h, dev_common.h)

// rows per wave: as asked, but a group keeps at least 4 lanes
int pack_for(int G, int pack) {
  int R = pack >= 4 ? 4 : pack >= 2 ? 2 : 1;
  while (R > 1 && 64 / (R * G) < 4) R >>= 1;
  return R;
}

bool merge_ok(const int32_t* lists, int64_t n, int32_t P, const float* recv) {
  if (n < 0 || P < 1 || n >= (1ll << 31) * WPB) return false;
  if (n && (!lists || !recv || !aligned16(recv))) return false;
  return true;
}

// what the float32 and the 16-bit entry point of a GraphSAGE kernel check alike (everything but the table itself), and
// their launches over a table of element type E
bool sage_part_ok(const int32_t* indptr, const int32_t* indices, const int32_t* items, int64_t n_items,
                  const int32_t* hubs, int64_t n_hubs, int64_t pos0, int64_t part0, int64_t ldy, int32_t W, int32_t pack,
                  const void* partial) {
  if (!plan_ok(indptr, indices, items, n_items, hubs, n_hubs, pos0, part0, partial, false)) return false;
  return !(W < 4 || W % 4 != 0 || ldy % 4 != 0 || ldy < W || pack < 1);
}

template <typename E>
int sage_part_launch(const int32_t* indptr, const int32_t* indices, const int32_t* items, int64_t n_items,
                     const int32_t* hubs, int64_t n_hubs, int64_t pos0, int64_t part0, const E* y, int64_t ldy, int32_t W,
                     int32_t pack, float* partial, float* send, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  const int G = groups_for(W / 4), R = pack_for(G, pack);
  if (n_items)
    with_groups_rows(G, R, [&](auto g, auto r) {
      hipLaunchKernelGGL((k_sage_part<g(), r(), E>), dim3(blocks_of(n_items, R)), dim3(BLK), 0,
                         st, indptr, indices, reinterpret_cast<const int4*>(items), (long long)n_items, (long long)pos0,
                         (long long)part0, y, (long long)ldy, (int)W, partial, send);
    });
  if (n_hubs)
    hipLaunchKernelGGL(k_sage_part_hubs, dim3(blocks_of(n_hubs)), dim3(BLK), 0, st, reinterpret_cast<const int4*>(hubs),
                       (long long)n_hubs, (long long)pos0, (long long)part0, (int)W, partial, send);
  return done();
}

bool sage_merge_ok(const int32_t* lists, int64_t n, int32_t P, const float* recv, int64_t ldx, int32_t W, int32_t proj,
                   int64_t ldo) {
  if (!merge_ok(lists, n, P, recv)) return false;
  return !(W < 4 || W % 4 != 0 || ldx % 4 != 0 || ldo % 4 != 0 || ldx < W || ldo < (proj ? W : 2 * (int64_t)W));
}

template <typename E>
int sage_merge_launch(const int32_t* dst, const int32_t* lists, int64_t n, int32_t P, const float* recv, const E* x,
                      int64_t ldx, int32_t W, int32_t proj, const float* bias, int32_t relu, float* out, int64_t ldo,
                      void* stream) {
  hipStream_t st = (hipStream_t)stream;
  const int G = groups_for(W / 4);
  with_groups<1, 16>(G, [&](auto g) {
    hipLaunchKernelGGL((k_sage_merge<g(), E>), dim3(blocks_of(n, G)), dim3(BLK), 0, st,
                       reinterpret_cast<const int2*>(dst), lists, (long long)n, (int)P, recv, x, (long long)ldx, (int)W,
                       proj != 0, bias, relu != 0, out, (long long)ldo);
  });
  return done();
}

}  // namespace

extern "C" {

int csl_infer_sage_part_f32(const int32_t* indptr, const int32_t* indices, const int32_t* items, int64_t n_items,
                            const int32_t* hubs, int64_t n_hubs, int64_t pos0, int64_t part0, const float* y, int64_t ldy,
                            int32_t W, int32_t pack, float* partial, float* send, void* stream) {
  if (!sage_part_ok(indptr, indices, items, n_items, hubs, n_hubs, pos0, part0, ldy, W, pack, partial)) return CSL_E_INVALID;
  if (n_items == 0 && n_hubs == 0) return CSL_OK;
  if (!y || !send || !aligned16(y) || !aligned16(send)) return CSL_E_INVALID;
  return sage_part_launch<float>(indptr, indices, items, n_items, hubs, n_hubs, pos0, part0, y, ldy, W, pack, partial, send,
                                 stream);
}

int csl_infer_sage_part_x16(const int32_t* indptr, const int32_t* indices, const int32_t* items, int64_t n_items,
                            const int32_t* hubs, int64_t n_hubs, int64_t pos0, int64_t part0, const void* y, int32_t kind,
                            int64_t ldy, int32_t W, int32_t pack, float* partial, float* send, void* stream) {
  if (!feat::table_ok(y, kind, ldy)) return CSL_E_INVALID;
  if (!sage_part_ok(indptr, indices, items, n_items, hubs, n_hubs, pos0, part0, ldy, W, pack, partial)) return CSL_E_INVALID;
  if (n_items == 0 && n_hubs == 0) return CSL_OK;
  if (!send || !aligned16(send)) return CSL_E_INVALID;
  return with_elem(kind, [&](auto e) {
    typedef typename decltype(e)::type E;
    return sage_part_launch(indptr, indices, items, n_items, hubs, n_hubs, pos0, part0, static_cast<const E*>(y), ldy, W,
                            pack, partial, send, stream);
  });
}

int csl_infer_sage_merge_f32(const int32_t* dst, const int32_t* lists, int64_t n, int32_t P, const float* recv,
                             const float* x, int64_t ldx, int32_t W, int32_t proj, const float* bias, int32_t relu,
                             float* out, int64_t ldo, void* stream) {
  if (!sage_merge_ok(lists, n, P, recv, ldx, W, proj, ldo)) return CSL_E_INVALID;
  if (n == 0) return CSL_OK;
  if (!dst || (reinterpret_cast<uintptr_t>(dst) & 7u) || !x || !out || !aligned16(x) || !aligned16(out) || (bias && !aligned16(bias)))
    return CSL_E_INVALID;
  return sage_merge_launch<float>(dst, lists, n, P, recv, x, ldx, W, proj, bias, relu, out, ldo, stream);
}

int csl_infer_sage_merge_x16(const int32_t* dst, const int32_t* lists, int64_t n, int32_t P, const float* recv,
                             const void* x, int32_t kind, int64_t ldx, int32_t W, int32_t proj, const float* bias,
                             int32_t relu, float* out, int64_t ldo, void* stream) {
  if (!feat::table_ok(x, kind, ldx) || proj != 0) return CSL_E_INVALID;
  if (!sage_merge_ok(lists, n, P, recv, ldx, W, 0, ldo)) return CSL_E_INVALID;
  if (n == 0) return CSL_OK;
  if (!dst || (reinterpret_cast<uintptr_t>(dst) & 7u) || !out || !aligned16(out) || (bias && !aligned16(bias))) return CSL_E_INVALID;
  return with_elem(kind, [&](auto e) {
    typedef typename decltype(e)::type E;
    return sage_merge_launch(dst, lists, n, P, recv, static_cast<const E*>(x), ldx, W, 0, bias, relu, out, ldo, stream);
  });
}

int csl_infer_gat_part_f32(const int32_t* indptr, const int32_t* indices, const int32_t* items, int64_t n_items,
                           const int32_t* hubs, int64_t n_hubs, int64_t pos0, int64_t part0, const float* z,
                           const float* el, const float* er_rows, int32_t H, int32_t D, float slope, int32_t pack,
                           float* partial, float* send, void* stream) {
  if (!plan_ok(indptr, indices, items, n_items, hubs, n_hubs, pos0, part0, partial, false)) return CSL_E_INVALID;
  if (H < 1 || D < 4 || D % 4 != 0 || (int64_t)H * D > GAT_MAX_C || pack < 1) return CSL_E_INVALID;
  if (n_items == 0 && n_hubs == 0) return CSL_OK;
  if (!z || !el || !er_rows || !send || !aligned16(z) || !aligned16(send)) return CSL_E_INVALID;
  hipStream_t st = (hipStream_t)stream;
  const int G = groups_for(H * D / 4), R = pack_for(G, pack);
  const long long pld = csl_infer_gat_partial_ld(H, D);
  if (n_items)
    with_groups_rows(G, R, [&](auto g, auto r) {
      hipLaunchKernelGGL((k_gat_part<g(), r()>), dim3(blocks_of(n_items, R)), dim3(BLK), 0, st,
                         indptr, indices, reinterpret_cast<const int4*>(items), (long long)n_items, (long long)pos0,
                         (long long)part0, z, el, er_rows, (int)H, (int)D, slope, partial, pld, send);
    });
  if (n_hubs)
    hipLaunchKernelGGL(k_gat_part_hubs, dim3(blocks_of(n_hubs)), dim3(BLK), 0, st, reinterpret_cast<const int4*>(hubs),
                       (long long)n_hubs, (long long)pos0, (long long)part0, (int)H, (int)D, partial, pld, send);
  return done();
}

int csl_infer_gat_merge_f32(const int32_t* lists, int64_t n, int32_t P, const float* recv, int32_t H, int32_t D,
                            const float* bias, int32_t last, int32_t n_cls, float* out, int64_t ldo, void* stream) {
  if (!merge_ok(lists, n, P, recv)) return CSL_E_INVALID;
  if (H < 1 || D < 4 || D % 4 != 0 || (int64_t)H * D > (last ? GAT_LAST_MAX_C : GAT_MAX_C)) return CSL_E_INVALID;
  if (last ? (n_cls < 1 || n_cls > D || ldo < n_cls) : (ldo % 4 != 0 || ldo < (int64_t)H * D)) return CSL_E_INVALID;
  if (n == 0) return CSL_OK;
  if (!out || (!last && !aligned16(out)) || (bias && !aligned16(bias))) return CSL_E_INVALID;
  hipStream_t st = (hipStream_t)stream;
  const long long pld = csl_infer_gat_partial_ld(H, D);
  const size_t shmem = last ? (size_t)WPB * H * D * sizeof(float) : 0;
  hipLaunchKernelGGL(k_gat_merge, dim3(blocks_of(n)), dim3(BLK), shmem, st, lists, (long long)n, (int)P, recv, pld, (int)H,
                     (int)D, bias, last != 0, (int)n_cls, out, (long long)ldo);
  return done();
}

}  // extern "C"
