// infer.hip -- full-neighbour, layer-wise inference of the two models (include/cslicer_infer.h), gfx950.
//
// The training kernels are shaped for sampled rows (at most one fanout long); a full neighbourhood is power-law, so here a
// row is a list of work ITEMS of at most SEG edges (the split rule for skewed gathers: lists longer than a fixed share are
// summed in chunks by separate waves, and a second pass adds each destination's partials in chunk order).  One wave per
// item; the wave's 64 lanes form G groups of 64 / G lanes, a group covers one source row (lane q of a group holds float4
// column q of a 64 / G-float4 column tile), and each lane keeps U independent row loads in flight per step: G * U edges of
// the item are read at once.  The groups' sums are combined by a fixed xor butterfly, the hub partials in part order:
// no atomics, every result is bitwise reproducible.
//
// The GraphSAGE kernels are templated on the element type E of the table they gather (csrc/feat_elem.h): the first layer
// reads a float16 / bfloat16 feature table in place (include/cslicer_infer16.h), a lane loading four elements (8 bytes)
// and upcasting them in registers; everything after the load is the float32 code.
//
// The float4 helpers, the row ends (sage_finish, gat_finish, gat_head_mean, lse_merge) and the host helpers live in
// csrc/infer_dev.h, shared with csrc/infer_parts.hip.
#include "infer_dev.h"

namespace {

// ---------------------------------------------------------------- GraphSAGE

template <int G, typename E = float>
__global__ __launch_bounds__(BLK) void k_infer_sage(const int* __restrict__ indptr, const int* __restrict__ indices,
                                                    const int4* __restrict__ items, long long n_items, long long pos0,
                                                    long long part0, const E* __restrict__ x, long long ldx, int W,
                                                    int proj, const float* __restrict__ bias, int relu,
                                                    float* __restrict__ partial, float* __restrict__ out, long long ldo) {
  constexpr int LG = 64 / G;
  const int lane = threadIdx.x & 63, g = lane / LG, q = lane % LG;
  const long long it = (long long)blockIdx.x * WPB + (threadIdx.x >> 6);
  if (it >= n_items) return;                                   // (wave-uniform)
  const int4 item = items[it];
  const int row = item.x, e0 = item.z, part = item.w;
  const int rend = indptr[row + 1];
  const int e1 = part < 0 ? rend : (int)min((long long)e0 + SEG, (long long)rend);
  const int W4 = W / 4;
  const long long noff = proj ? W : 0;                         // the neighbour operand's first column in x
  for (int t0 = 0; t0 < W4; t0 += LG) {
    const int c4 = t0 + q;
    const bool on = c4 < W4;
    float4 acc = f4zero();
    for (int eb = e0; eb < e1; eb += 64) {
      const int nb = min(64, e1 - eb);
      const int mine = lane < nb ? indices[eb + lane] : 0;     // 64 edges' sources, one coalesced load
      for (int j = 0; j < nb; j += G * U) {
        typename feat::Elem<E>::Raw v[U];                      // (a 16-bit table: 8 bytes a load, upcast when added)
#pragma unroll
        for (int u = 0; u < U; u++) {
          const int jj = j + u * G + g;
          const int src = __shfl(mine, jj & 63);
          v[u] = (on && jj < nb) ? feat::Elem<E>::ld(x + (long long)src * ldx + noff + 4 * c4) : feat::Elem<E>::zero();
        }
#pragma unroll
        for (int u = 0; u < U; u++) add4(acc, feat::Elem<E>::up(v[u]));
      }
    }
#pragma unroll
    for (int d = LG; d < 64; d <<= 1) add4(acc, shfl_xor4(acc, d));
    if (g == 0 && on) {
      if (part >= 0)
        st4(partial + (long long)(part - part0) * W + 4 * c4, acc);
      else
        sage_finish(x, ldx, W, proj, bias, relu, out, ldo, (long long)item.y - pos0, row, rend - indptr[row], c4, acc);
    }
  }
}

// one wave per hub row: its partials added in part order, then the row's end
template <typename E = float>
__global__ __launch_bounds__(BLK) void k_infer_sage_hubs(const int* __restrict__ indptr, const int4* __restrict__ hubs,
                                                         long long n_hubs, long long pos0, long long part0,
                                                         const E* __restrict__ x, long long ldx, int W, int proj,
                                                         const float* __restrict__ bias, int relu,
                                                         const float* __restrict__ partial, float* __restrict__ out,
                                                         long long ldo) {
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
    sage_finish(x, ldx, W, proj, bias, relu, out, ldo, (long long)hub.y - pos0, hub.x, indptr[hub.x + 1] - indptr[hub.x],
                c4, acc);
  }
}

// ---------------------------------------------------------------- GAT

template <int G>
__global__ __launch_bounds__(BLK) void k_infer_gat(const int* __restrict__ indptr, const int* __restrict__ indices,
                                                   const int4* __restrict__ items, long long n_items, long long pos0,
                                                   long long part0, const float* __restrict__ z, const float* __restrict__ el,
                                                   const float* __restrict__ er, int H, int D, float slope,
                                                   const float* __restrict__ bias, int last, int n_cls,
                                                   float* __restrict__ partial, long long pld, float* __restrict__ out,
                                                   long long ldo) {
  extern __shared__ float lds[];
  constexpr int LG = 64 / G;
  const int lane = threadIdx.x & 63, g = lane / LG, q = lane % LG;
  const long long it = (long long)blockIdx.x * WPB + (threadIdx.x >> 6);
  if (it >= n_items) return;
  const int4 item = items[it];
  const int row = item.x, e0 = item.z, part = item.w;
  const int rend = indptr[row + 1];
  const int e1 = part < 0 ? rend : (int)min((long long)e0 + SEG, (long long)rend);
  const int C = H * D, C4 = C / 4, Dq = D / 4;
  float* stage = lds + (threadIdx.x >> 6) * C;
  for (int t0 = 0; t0 < C4; t0 += LG) {
    const int c4 = t0 + q;
    const bool on = c4 < C4;
    const int h = on ? c4 / Dq : 0;
    const float erv = er[(long long)row * H + h];
    float m = -1e30f, s = 0.f;
    float4 n = f4zero();
    for (int eb = e0; eb < e1; eb += 64) {
      const int nb = min(64, e1 - eb);
      const int mine = lane < nb ? indices[eb + lane] : 0;
      for (int j = 0; j < nb; j += G * U) {
        float sc[U];
        float4 v[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
          const int jj = j + u * G + g;
          const int src = __shfl(mine, jj & 63);
          const bool ok = on && jj < nb;
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
    }
#pragma unroll
    for (int d = LG; d < 64; d <<= 1) {
      const float m2 = __shfl_xor(m, d), s2 = __shfl_xor(s, d);
      lse_merge(m, s, n, m2, s2, shfl_xor4(n, d));
    }
    if (g == 0 && on) {
      if (part >= 0) {
        float* pr = partial + (long long)(part - part0) * pld;
        st4(pr + 4 * c4, n);
        if (c4 % Dq == 0) pr[C + h] = m, pr[C + H + h] = s;
      } else {
        gat_finish(bias, last, out, ldo, stage, (long long)item.y - pos0, c4, s, n);
      }
    }
  }
  if (last && part < 0) gat_head_mean(stage, H, D, n_cls, out, ldo, (long long)item.y - pos0, lane);
}

__global__ __launch_bounds__(BLK) void k_infer_gat_hubs(const int4* __restrict__ hubs, long long n_hubs, long long pos0,
                                                        long long part0, int H, int D, const float* __restrict__ bias,
                                                        int last, int n_cls, const float* __restrict__ partial, long long pld,
                                                        float* __restrict__ out, long long ldo) {
  extern __shared__ float lds[];
  const int lane = threadIdx.x & 63;
  const long long hi = (long long)blockIdx.x * WPB + (threadIdx.x >> 6);
  if (hi >= n_hubs) return;
  const int4 hub = hubs[hi];
  const int C = H * D, C4 = C / 4, Dq = D / 4;
  float* stage = lds + (threadIdx.x >> 6) * C;
  const long long p0 = (long long)hub.z - part0;
  for (int c4 = lane; c4 < C4; c4 += 64) {
    const int h = c4 / Dq;
    float m = -1e30f, s = 0.f;
    float4 n = f4zero();
    for (int p = 0; p < hub.w; p++) {
      const float* pr = partial + (p0 + p) * pld;
      lse_merge(m, s, n, pr[C + h], pr[C + H + h], ld4(pr + 4 * c4));
    }
    gat_finish(bias, last, out, ldo, stage, (long long)hub.y - pos0, c4, s, n);
  }
  if (last) gat_head_mean(stage, H, D, n_cls, out, ldo, (long long)hub.y - pos0, lane);
}

// ---------------------------------------------------------------- a 16-bit table's rows as a float32 GEMM operand

// dst[k, 0:H) = float32(src[k, 0:H)) for n consecutive rows: 1 << lg lanes per row (lane q the quads q, q + 2^lg, ...),
// an 8-byte load and a 16-byte store per quad
template <typename E>
__global__ __launch_bounds__(BLK) void k_upcast_rows(const E* __restrict__ src, long long lds, long long n,
                                                     float* __restrict__ dst, long long ldd, int H4, int lg) {
  const long long k = ((long long)blockIdx.x * BLK + threadIdx.x) >> lg;
  if (k >= n) return;
  for (int c4 = threadIdx.x & ((1 << lg) - 1); c4 < H4; c4 += 1 << lg)
    st4(dst + k * ldd + 4 * c4, feat::Elem<E>::up(feat::Elem<E>::ld(src + k * lds + 4 * c4)));
}

// ---------------------------------------------------------------- evaluation head

__global__ __launch_bounds__(BLK) void k_infer_eval_rows(const float* __restrict__ L, long long ld, long long n, int C,
                                                         const long long* __restrict__ labels, long long* __restrict__ pred,
                                                         float* __restrict__ loss_row) {
  const int lane = threadIdx.x & 63;
  const long long k = (long long)blockIdx.x * WPB + (threadIdx.x >> 6);
  if (k >= n) return;
  const float* r = L + k * ld;
  float v = -INFINITY;
  int bj = C;
  for (int j = lane; j < C; j += 64) {
    const float x = r[j];
    if (bj == C || x > v) v = x, bj = j;               // a lane's columns ascend: the first maximum is kept
  }
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const float v2 = __shfl_xor(v, d);
    const int j2 = __shfl_xor(bj, d);
    if (j2 < C && (bj == C || v2 > v || (v2 == v && j2 < bj))) v = v2, bj = j2;
  }
  float t = 0.f;
  for (int j = lane; j < C; j += 64) t += expf(r[j] - v);
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) t += __shfl_xor(t, d);
  if (lane == 0) {
    const long long y = labels[k];
    pred[k] = bj;
    // (v - r[y] first: a difference of two logits is exact up to the result's own rounding, so the loss keeps its
    // relative accuracy at any offset of the row; v + logf(t) first rounds at the size of the logits: 2.6e-5 of a row's
    // loss was seen at two classes and logits of about 80)
    loss_row[k] = (y >= 0 && y < C) ? (v - r[y]) + logf(t) : NAN;
  }
}

__global__ __launch_bounds__(BLK) void k_infer_eval_sum(const long long* __restrict__ pred,
                                                        const long long* __restrict__ labels,
                                                        const float* __restrict__ loss_row, long long n,
                                                        double* __restrict__ loss_sum, long long* __restrict__ correct) {
  __shared__ double sl[BLK];
  __shared__ long long sc[BLK];
  double l = 0.0;
  long long c = 0;
  for (long long k = threadIdx.x; k < n; k += BLK) {
    l += (double)loss_row[k];
    c += pred[k] == labels[k];
  }
  sl[threadIdx.x] = l;
  sc[threadIdx.x] = c;
  __syncthreads();
  for (int w = BLK / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) sl[threadIdx.x] += sl[threadIdx.x + w], sc[threadIdx.x] += sc[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) *loss_sum = sl[0], *correct = sc[0];
}

// ---------------------------------------------------------------- host side

// what csl_infer_sage_f32 and csl_infer_sage_x16 check alike (everything but the table itself)
bool sage_args_ok(const int32_t* indptr, const int32_t* indices, const int32_t* items, int64_t n_items,
                  const int32_t* hubs, int64_t n_hubs, int64_t pos0, int64_t part0, int64_t ldx, int32_t W, int32_t proj,
                  const void* partial, int64_t ldo) {
  if (!plan_ok(indptr, indices, items, n_items, hubs, n_hubs, pos0, part0, partial, true)) return false;
  return !(W < 4 || W % 4 != 0 || ldx % 4 != 0 || ldo % 4 != 0 || ldx < (proj ? 2 * (int64_t)W : W) ||
           ldo < (proj ? W : 2 * (int64_t)W));
}

// the two launches of a GraphSAGE layer call over a table of element type E (arguments checked by the caller)
template <typename E>
int sage_launch(const int32_t* indptr, const int32_t* indices, const int32_t* items, int64_t n_items, const int32_t* hubs,
                int64_t n_hubs, int64_t pos0, int64_t part0, const E* x, int64_t ldx, int32_t W, int32_t proj,
                const float* bias, int32_t relu, float* partial, float* out, int64_t ldo, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  const int G = groups_for(W / 4);
  const int rl = relu != 0, pj = proj != 0;
  if (n_items)
    with_groups<1, 16>(G, [&](auto g) {
      hipLaunchKernelGGL((k_infer_sage<g(), E>), dim3(blocks_of(n_items)), dim3(BLK), 0, st, indptr, indices,
                         reinterpret_cast<const int4*>(items), (long long)n_items, (long long)pos0, (long long)part0, x,
                         (long long)ldx, (int)W, pj, bias, rl, partial, out, (long long)ldo);
    });
  if (n_hubs)
    hipLaunchKernelGGL(k_infer_sage_hubs<E>, dim3(blocks_of(n_hubs)), dim3(BLK), 0, st, indptr,
                       reinterpret_cast<const int4*>(hubs), (long long)n_hubs, (long long)pos0, (long long)part0, x,
                       (long long)ldx, (int)W, pj, bias, rl, partial, out, (long long)ldo);
  return done();
}

template <typename E>
void upcast_launch(const void* src, int64_t lds, int64_t n, float* dst, int64_t ldd, int32_t H, hipStream_t st) {
  int lg = 2;                                                  // 4 .. 64 lanes per row: the quads of a row, rounded up
  while (lg < 6 && (1 << lg) < H / 4) lg++;
  const long long rpb = BLK >> lg;
  hipLaunchKernelGGL(k_upcast_rows<E>, dim3((unsigned)((n + rpb - 1) / rpb)), dim3(BLK), 0, st, static_cast<const E*>(src),
                     (long long)lds, (long long)n, dst, (long long)ldd, (int)(H / 4), lg);
}

}  // namespace

extern "C" {

int32_t csl_infer_seg(void) { return SEG; }

int csl_infer_sage_f32(const int32_t* indptr, const int32_t* indices, const int32_t* items, int64_t n_items,
                       const int32_t* hubs, int64_t n_hubs, int64_t pos0, int64_t part0, const float* x, int64_t ldx,
                       int32_t W, int32_t proj, const float* bias, int32_t relu, float* partial, float* out, int64_t ldo,
                       void* stream) {
  if (!sage_args_ok(indptr, indices, items, n_items, hubs, n_hubs, pos0, part0, ldx, W, proj, partial, ldo))
    return CSL_E_INVALID;
  if (n_items == 0 && n_hubs == 0) return CSL_OK;
  if (!x || !out || !aligned16(x) || !aligned16(out) || (bias && !aligned16(bias))) return CSL_E_INVALID;
  return sage_launch<float>(indptr, indices, items, n_items, hubs, n_hubs, pos0, part0, x, ldx, W, proj, bias, relu, partial,
                            out, ldo, stream);
}

int csl_infer_sage_x16(const int32_t* indptr, const int32_t* indices, const int32_t* items, int64_t n_items,
                       const int32_t* hubs, int64_t n_hubs, int64_t pos0, int64_t part0, const void* x, int32_t kind,
                       int64_t ldx, int32_t W, int32_t proj, const float* bias, int32_t relu, float* partial, float* out,
                       int64_t ldo, void* stream) {
  if (!feat::table_ok(x, kind, ldx) || proj != 0) return CSL_E_INVALID;
  if (!sage_args_ok(indptr, indices, items, n_items, hubs, n_hubs, pos0, part0, ldx, W, 0, partial, ldo))
    return CSL_E_INVALID;
  if (n_items == 0 && n_hubs == 0) return CSL_OK;
  if (!out || !aligned16(out) || (bias && !aligned16(bias))) return CSL_E_INVALID;
  return with_elem(kind, [&](auto e) {
    typedef typename decltype(e)::type E;
    return sage_launch(indptr, indices, items, n_items, hubs, n_hubs, pos0, part0, static_cast<const E*>(x), ldx, W, 0, bias,
                       relu, partial, out, ldo, stream);
  });
}

int csl_upcast_rows_x16(const void* src, int32_t kind, int64_t lds, int64_t n, float* dst, int64_t ldd, int32_t H,
                        void* stream) {
  if (!feat::table_ok(src, kind, lds) || H < 4 || H % 4 != 0 || lds < H || ldd < H || ldd % 4 != 0 || n < 0 ||
      n >= (1ll << 31))
    return CSL_E_INVALID;
  if (n == 0) return CSL_OK;
  if (!dst || !aligned16(dst)) return CSL_E_INVALID;
  with_elem(kind, [&](auto e) { upcast_launch<typename decltype(e)::type>(src, lds, n, dst, ldd, H, (hipStream_t)stream); });
  return done();
}

int64_t csl_infer_gat_partial_ld(int32_t H, int32_t D) {
  if (H < 1 || D < 4) return CSL_E_INVALID;
  return (int64_t)H * D + (2 * (int64_t)H + 3) / 4 * 4;
}

int csl_infer_gat_f32(const int32_t* indptr, const int32_t* indices, const int32_t* items, int64_t n_items,
                      const int32_t* hubs, int64_t n_hubs, int64_t pos0, int64_t part0, const float* z, const float* el,
                      const float* er, int32_t H, int32_t D, float slope, const float* bias, int32_t last, int32_t n_cls,
                      float* partial, float* out, int64_t ldo, void* stream) {
  if (!plan_ok(indptr, indices, items, n_items, hubs, n_hubs, pos0, part0, partial, true)) return CSL_E_INVALID;
  if (H < 1 || D < 4 || D % 4 != 0 || (int64_t)H * D > (last ? GAT_LAST_MAX_C : GAT_MAX_C)) return CSL_E_INVALID;
  if (last ? (n_cls < 1 || n_cls > D || ldo < n_cls) : (ldo % 4 != 0 || ldo < (int64_t)H * D)) return CSL_E_INVALID;
  if (n_items == 0 && n_hubs == 0) return CSL_OK;
  if (!z || !el || !er || !out || !aligned16(z) || (!last && !aligned16(out)) || (bias && !aligned16(bias))) return CSL_E_INVALID;
  hipStream_t st = (hipStream_t)stream;
  const int C = H * D;
  const int G = groups_for(C / 4);
  const long long pld = csl_infer_gat_partial_ld(H, D);
  const size_t shmem = last ? (size_t)WPB * C * sizeof(float) : 0;
  const int ls = last != 0;
  if (n_items)
    with_groups<1, 16>(G, [&](auto g) {
      hipLaunchKernelGGL(k_infer_gat<g()>, dim3(blocks_of(n_items)), dim3(BLK), shmem, st, indptr, indices,
                         reinterpret_cast<const int4*>(items), (long long)n_items, (long long)pos0, (long long)part0, z, el,
                         er, (int)H, (int)D, slope, bias, ls, (int)n_cls, partial, pld, out, (long long)ldo);
    });
  if (n_hubs)
    hipLaunchKernelGGL(k_infer_gat_hubs, dim3(blocks_of(n_hubs)), dim3(BLK), shmem, st,
                       reinterpret_cast<const int4*>(hubs), (long long)n_hubs, (long long)pos0, (long long)part0, (int)H,
                       (int)D, bias, ls, (int)n_cls, partial, pld, out, (long long)ldo);
  return done();
}

int csl_infer_eval_f32(const float* logits, int64_t ld, int64_t n, int32_t C, const int64_t* labels, int64_t* pred,
                       float* loss_row, double* loss_sum, int64_t* correct, void* stream) {
  if (n < 0 || C < 1 || ld < C || !loss_sum || !correct) return CSL_E_INVALID;
  if (n > 0 && (!logits || !labels || !pred || !loss_row)) return CSL_E_INVALID;
  if (n >= (1ll << 31) * WPB) return CSL_E_INVALID;
  hipStream_t st = (hipStream_t)stream;
  if (n > 0)
    hipLaunchKernelGGL(k_infer_eval_rows, dim3(blocks_of(n)), dim3(BLK), 0, st, logits, (long long)ld, (long long)n,
                       (int)C, reinterpret_cast<const long long*>(labels), reinterpret_cast<long long*>(pred), loss_row);
  hipLaunchKernelGGL(k_infer_eval_sum, dim3(1), dim3(BLK), 0, st, reinterpret_cast<const long long*>(pred),
                     reinterpret_cast<const long long*>(labels), loss_row, (long long)n, loss_sum,
                     reinterpret_cast<long long*>(correct));
  return done();
}

}  // extern "C"
