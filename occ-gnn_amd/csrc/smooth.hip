// smooth.hip -- one label-propagation step over full rows (include/cslicer_smooth.h), gfx950: the hot path of Correct and
// Smooth (cslicer/smooth.py), run once per iteration and chunk.
//
// A sibling of k_infer_sage (csrc/infer.hip) on the same work list: one wave per item, G = groups_for(W / 4) groups of
// 64 / G lanes, a group covers one source row (lane q of a group holds float4 column q of a column tile), U independent
// row loads in flight per lane, the groups' sums combined by the fixed xor butterfly, a hub row's partials added in part
// order by a second pass.  The gathered matrix is the PRE-SCALED iterate dinv (.) X, so the inner loop is the plain row
// sum of that kernel; only the row end differs: it scales by alpha dinv[v], adds the base term, clamps, and writes the
// iterate and / or the next step's pre-scaled operand.  No atomics.
#include "cslicer_smooth.h"
#include "infer_dev.h"

namespace {

struct PropEnd {
  const float* __restrict__ dinv;
  const float* __restrict__ base;
  float* __restrict__ out;
  float* __restrict__ out_s;
  long long ldb, ldo, ldos;
  float alpha, beta, lo, hi;
};

__device__ __forceinline__ float clampf(const float y, const float lo, const float hi) {
  return y < lo ? lo : (y > hi ? hi : y);                      // (both comparisons are false for a NaN: it stays)
}

// the end of a row: position k, graph row `row`, float4 column c4 of its sum.  The roundings are those the header
// states (and tests/smooth_ref.py bounds): nothing here may be contracted differently from kernel to kernel.
__device__ __forceinline__ void prop_finish(const PropEnd& p, long long k, int row, int c4, const float4 acc) {
#pragma clang fp contract(off)
  const float dv = p.dinv[row];
  const float a = p.alpha * dv;
  float4 y = make_float4(a * acc.x, a * acc.y, a * acc.z, a * acc.w);
  if (p.base) {
    const float4 b = ld4(p.base + k * p.ldb + 4 * c4);
    y.x = __builtin_fmaf(p.beta, b.x, y.x), y.y = __builtin_fmaf(p.beta, b.y, y.y);
    y.z = __builtin_fmaf(p.beta, b.z, y.z), y.w = __builtin_fmaf(p.beta, b.w, y.w);
  }
  y.x = clampf(y.x, p.lo, p.hi), y.y = clampf(y.y, p.lo, p.hi), y.z = clampf(y.z, p.lo, p.hi), y.w = clampf(y.w, p.lo, p.hi);
  if (p.out) st4(p.out + k * p.ldo + 4 * c4, y);
  if (p.out_s) st4(p.out_s + k * p.ldos + 4 * c4, make_float4(dv * y.x, dv * y.y, dv * y.z, dv * y.w));
}

template <int G>
__global__ __launch_bounds__(BLK) void k_prop(const int* __restrict__ indptr, const int* __restrict__ indices,
                                              const int4* __restrict__ items, long long n_items, long long pos0,
                                              long long part0, const float* __restrict__ xs, long long ldx, int W,
                                              float* __restrict__ partial, const PropEnd end) {
  constexpr int LG = 64 / G;
  const int lane = threadIdx.x & 63, g = lane / LG, q = lane % LG;
  const long long it = (long long)blockIdx.x * WPB + (threadIdx.x >> 6);
  if (it >= n_items) return;                                   // (wave-uniform)
  const int4 item = items[it];
  const int row = item.x, e0 = item.z, part = item.w;
  const int rend = indptr[row + 1];
  const int e1 = part < 0 ? rend : (int)min((long long)e0 + SEG, (long long)rend);
  const int W4 = W / 4;
  for (int t0 = 0; t0 < W4; t0 += LG) {
    const int c4 = t0 + q;
    const bool on = c4 < W4;
    float4 acc = f4zero();
    for (int eb = e0; eb < e1; eb += 64) {
      const int nb = min(64, e1 - eb);
      const int mine = lane < nb ? indices[eb + lane] : 0;     // 64 edges' sources, one coalesced load
      for (int j = 0; j < nb; j += G * U) {
        float4 v[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
          const int jj = j + u * G + g;
          const int src = __shfl(mine, jj & 63);
          v[u] = (on && jj < nb) ? ld4(xs + (long long)src * ldx + 4 * c4) : f4zero();
        }
#pragma unroll
        for (int u = 0; u < U; u++) add4(acc, v[u]);
      }
    }
#pragma unroll
    for (int d = LG; d < 64; d <<= 1) add4(acc, shfl_xor4(acc, d));
    if (g == 0 && on) {
      if (part >= 0)
        st4(partial + (long long)(part - part0) * W + 4 * c4, acc);
      else
        prop_finish(end, (long long)item.y - pos0, row, c4, acc);
    }
  }
}

// one wave per hub row: its partials added in part order, then the row's end
__global__ __launch_bounds__(BLK) void k_prop_hubs(const int4* __restrict__ hubs, long long n_hubs, long long pos0,
                                                   long long part0, int W, const float* __restrict__ partial,
                                                   const PropEnd end) {
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
    prop_finish(end, (long long)hub.y - pos0, hub.x, c4, acc);
  }
}

bool ld_ok(int64_t ld, int32_t W) { return ld % 4 == 0 && ld >= W; }

}  // namespace

extern "C" int csl_prop_f32(const int32_t* indptr, const int32_t* indices, const int32_t* items, int64_t n_items,
                            const int32_t* hubs, int64_t n_hubs, int64_t pos0, int64_t part0, const float* xs, int64_t ldx,
                            int32_t W, const float* dinv, float alpha, const float* base, int64_t ldb, float beta, float lo,
                            float hi, float* partial, float* out, int64_t ldo, float* out_s, int64_t ldos, void* stream) {
  if (!plan_ok(indptr, indices, items, n_items, hubs, n_hubs, pos0, part0, partial, false)) return CSL_E_INVALID;
  if (W < 4 || W % 4 != 0 || !ld_ok(ldx, W) || (base && !ld_ok(ldb, W)) || (out && !ld_ok(ldo, W)) ||
      (out_s && !ld_ok(ldos, W)))
    return CSL_E_INVALID;
  if (!aligned16(xs) || !aligned16(base) || !aligned16(out) || !aligned16(out_s)) return CSL_E_INVALID;
  if (!(lo <= hi) || !std::isfinite(alpha) || !std::isfinite(beta)) return CSL_E_INVALID;   // (a NaN bound fails lo <= hi)
  if ((xs && (out_s == xs || out == xs))) return CSL_E_INVALID;
  if (n_items == 0 && n_hubs == 0) return CSL_OK;
  if (!dinv || (n_items && !xs) || (!out && !out_s)) return CSL_E_INVALID;
  hipStream_t st = (hipStream_t)stream;
  const PropEnd end = {dinv, base, out, out_s, (long long)ldb, (long long)ldo, (long long)ldos, alpha, beta, lo, hi};
  if (n_items)
    with_groups<1, 16>(groups_for(W / 4), [&](auto g) {
      hipLaunchKernelGGL(k_prop<g()>, dim3(blocks_of(n_items)), dim3(BLK), 0, st, indptr, indices,
                         reinterpret_cast<const int4*>(items), (long long)n_items, (long long)pos0, (long long)part0, xs,
                         (long long)ldx, (int)W, partial, end);
    });
  if (n_hubs)
    hipLaunchKernelGGL(k_prop_hubs, dim3(blocks_of(n_hubs)), dim3(BLK), 0, st, reinterpret_cast<const int4*>(hubs),
                       (long long)n_hubs, (long long)pos0, (long long)part0, (int)W, partial, end);
  return done();
}
