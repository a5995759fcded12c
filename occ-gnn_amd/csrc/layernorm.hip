// layernorm.hip -- layer normalisation between the GraphSAGE layers behind the C ABI (cslicer_layernorm.h):
// a forward that normalises a row, applies gamma / beta and the ReLU, and a backward that turns the gradient w.r.t. the
// normalised row into the gradient w.r.t. the row, in place, with the first stage of the column sums behind dgamma and the
// bias gradient.  Both are shaped the way k_dropout is: a row is walked by the power-of-two group of lanes that covers its
// H / 4 quads (a wave at the most), 256 >> lg rows per pass of a workgroup, 16-byte accesses, and the row reductions stay
// inside the lane group (butterfly shuffles: every lane ends with the same bits, in a fixed order).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "cslicer_layernorm.h"
#include "dev_common.h"

namespace {

constexpr int LBLK = 256;
constexpr int LN_REG_HQ = 256;   // a row of up to 256 quads (H = 1024) stays in registers between the passes

__device__ __forceinline__ float group_sum(float v, int lg) {
  for (int o = 1; o < (1 << lg); o <<= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ float sum4(const float4 a) { return (a.x + a.y) + (a.z + a.w); }
__device__ __forceinline__ float4 sub4(const float4 a, const float m) { return make_float4(a.x - m, a.y - m, a.z - m, a.w - m); }
__device__ __forceinline__ float4 mul4(const float4 a, const float4 b) { return make_float4(a.x * b.x, a.y * b.y, a.z * b.z, a.w * b.w); }
__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void st4(float* p, const float4 v) { *reinterpret_cast<float4*>(p) = v; }

// xhat and y of one quad: xhat = c * rstd (c the centred quad), y = gamma * xhat + beta, ReLU on request
__device__ __forceinline__ void ln_out(const float4 c, const float r, const float4 g, const float4 b, const int relu, float* yq,
                                       float* hq_) {
  const float4 h = make_float4(c.x * r, c.y * r, c.z * r, c.w * r);
  float4 o = make_float4(fmaf(g.x, h.x, b.x), fmaf(g.y, h.y, b.y), fmaf(g.z, h.z, b.z), fmaf(g.w, h.w, b.w));
  if (relu) o = make_float4(fmaxf(o.x, 0.f), fmaxf(o.y, 0.f), fmaxf(o.z, 0.f), fmaxf(o.w, 0.f));
  if (hq_) st4(hq_, h);
  st4(yq, o);
}

// NQ quads a lane holds (1: H / 4 <= 64, one quad per lane of the group; 4: a wave over up to 256 quads).  z and y may be
// the same matrix (a lane reads its quads before it writes them; no quad is touched by two lanes), hence no __restrict__ on
// them.  A lane past the last row loads nothing and stores nothing but runs the shuffles with its group.
template <int NQ>
__global__ __launch_bounds__(LBLK) void k_layernorm_fwd(const float* z, long long ldz, const float* __restrict__ gamma,
                                                        const float* __restrict__ beta, float eps, long long n, int hq, int lg,
                                                        float* y, long long ldy, float* __restrict__ xhat, long long ldh,
                                                        float* __restrict__ rstd, int relu) {
  const long long row = (long long)blockIdx.x * (LBLK >> lg) + (threadIdx.x >> lg);
  const int lane = threadIdx.x & ((1 << lg) - 1);
  const bool on = row < n;
  const float* zr = z + row * ldz;
  const float fh = (float)(4 * hq);
  float4 v[NQ];
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < NQ; i++) {
    const int q = lane + (i << lg);
    v[i] = on && q < hq ? ld4(zr + 4 * q) : make_float4(0.f, 0.f, 0.f, 0.f);
    s += sum4(v[i]);
  }
  const float mean = group_sum(s, lg) / fh;
  float ss = 0.f;
#pragma unroll
  for (int i = 0; i < NQ; i++) {
    const int q = lane + (i << lg);
    v[i] = sub4(v[i], mean);
    if (q < hq) ss += sum4(mul4(v[i], v[i]));
  }
  const float r = 1.0f / sqrtf(group_sum(ss, lg) / fh + eps);
  if (!on) return;
#pragma unroll
  for (int i = 0; i < NQ; i++) {
    const int q = lane + (i << lg);
    if (q < hq) ln_out(v[i], r, ld4(gamma + 4 * q), ld4(beta + 4 * q), relu, y + row * ldy + 4 * q, xhat ? xhat + row * ldh + 4 * q : nullptr);
  }
  if (rstd && lane == 0) rstd[row] = r;
}

// a row wider than the registers hold: one wave a row, the row read three times (mean, centred squares, output)
__global__ __launch_bounds__(LBLK) void k_layernorm_fwd_wide(const float* z, long long ldz, const float* __restrict__ gamma,
                                                             const float* __restrict__ beta, float eps, long long n, int hq,
                                                             float* y, long long ldy, float* __restrict__ xhat, long long ldh,
                                                             float* __restrict__ rstd, int relu) {
  const long long row = (long long)blockIdx.x * (LBLK >> 6) + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= n) return;   // (a whole wave: its shuffles have no partner left behind)
  const float* zr = z + row * ldz;
  const float fh = (float)(4 * hq);
  float s = 0.f;
  for (int q = lane; q < hq; q += 64) s += sum4(ld4(zr + 4 * q));
  const float mean = group_sum(s, 6) / fh;
  float ss = 0.f;
  for (int q = lane; q < hq; q += 64) {
    const float4 c = sub4(ld4(zr + 4 * q), mean);
    ss += sum4(mul4(c, c));
  }
  const float r = 1.0f / sqrtf(group_sum(ss, 6) / fh + eps);
  for (int q = lane; q < hq; q += 64)
    ln_out(sub4(ld4(zr + 4 * q), mean), r, ld4(gamma + 4 * q), ld4(beta + 4 * q), relu, y + row * ldy + 4 * q,
           xhat ? xhat + row * ldh + 4 * q : nullptr);
  if (rstd && lane == 0) rstd[row] = r;
}

// ---- backward.  A workgroup owns `rpb` rows (ln_rows) and leaves their column sums of dn * xhat and of dz in
// gpart[block][H] / bpart[block][H]: the first stage of csl_relu_bwd_colsum_f32's two-stage form (no atomics, nothing to
// pre-zero, a fixed order), finished by csl_reduce_multi_f32.
__host__ __device__ inline long long ln_rows(long long n_pad, int hq) {
  if (hq > LN_REG_HQ) return 128;   // (the wide kernel keeps a wave's 32 rows' means in its lanes)
  int lg = 0;
  while (lg < 6 && (1 << lg) < hq) lg++;
  // 32 rows (one pass of the workgroup where that is more): a hidden layer of ten thousand rows is then a few hundred
  // workgroups, not 84 walking 32 dependent passes each; more only beyond 2048 blocks
  long long r = (LBLK >> lg) > 32 ? (LBLK >> lg) : 32;
  while ((n_pad + r - 1) / r > 2048) r *= 2;
  return r;
}

// the row groups of the workgroup hold sums of the same columns: a tree over the groups in LDS, group 0 ends with the total
__device__ __forceinline__ float4 groups_sum(float4 acc, float4* s, int lg) {
  const int sub = threadIdx.x >> lg;
  __syncthreads();
  s[threadIdx.x] = acc;
  __syncthreads();
  for (int o = (LBLK >> lg) / 2; o > 0; o >>= 1) {
    if (sub < o) add4(s[threadIdx.x], s[threadIdx.x + (o << lg)]);
    __syncthreads();
  }
  return s[threadIdx.x];
}

// dz of one quad from a = gamma * dn, xhat, the two row means and rstd
__device__ __forceinline__ float4 ln_dz(const float4 a, const float4 x, const float m1, const float m2, const float r) {
  return make_float4(r * (a.x - m1 - x.x * m2), r * (a.y - m1 - x.y * m2), r * (a.z - m1 - x.z * m2), r * (a.w - m1 - x.w * m2));
}

template <int NQ>
__global__ __launch_bounds__(LBLK) void k_layernorm_bwd(float* __restrict__ dn, long long ldd, const float* __restrict__ xhat,
                                                        long long ldh, const float* __restrict__ rstd,
                                                        const float* __restrict__ gamma, long long n, int hq, int lg,
                                                        long long rpb, float* __restrict__ gpart, float* __restrict__ bpart) {
  __shared__ float4 s_sum[LBLK];
  const int lane = threadIdx.x & ((1 << lg) - 1), sub = threadIdx.x >> lg, rg = LBLK >> lg;
  const long long r0 = (long long)blockIdx.x * rpb;
  const long long r_end = r0 + rpb < n ? r0 + rpb : n;
  const float fh = (float)(4 * hq);
  float4 gm[NQ], ag[NQ], ab[NQ];
#pragma unroll
  for (int i = 0; i < NQ; i++) {
    const int q = lane + (i << lg);
    gm[i] = q < hq ? ld4(gamma + 4 * q) : make_float4(0.f, 0.f, 0.f, 0.f);
    ag[i] = ab[i] = make_float4(0.f, 0.f, 0.f, 0.f);
  }
  // (the row loop is block-uniform: a group past the last row runs the shuffles on zeros)
  for (long long rb = r0; rb < r_end; rb += rg) {
    const long long row = rb + sub;
    const bool on = row < r_end;
    float4 d[NQ], x[NQ], a[NQ];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int i = 0; i < NQ; i++) {
      const int q = lane + (i << lg);
      const bool in = on && q < hq;
      d[i] = in ? ld4(dn + row * ldd + 4 * q) : make_float4(0.f, 0.f, 0.f, 0.f);
      x[i] = in ? ld4(xhat + row * ldh + 4 * q) : make_float4(0.f, 0.f, 0.f, 0.f);
      a[i] = mul4(gm[i], d[i]);
      s1 += sum4(a[i]);
      s2 += sum4(mul4(a[i], x[i]));
    }
    const float m1 = group_sum(s1, lg) / fh, m2 = group_sum(s2, lg) / fh;
    if (!on) continue;
    const float r = rstd[row];
#pragma unroll
    for (int i = 0; i < NQ; i++) {
      const int q = lane + (i << lg);
      if (q >= hq) continue;
      const float4 dz = ln_dz(a[i], x[i], m1, m2, r);
      st4(dn + row * ldd + 4 * q, dz);
      add4(ag[i], mul4(d[i], x[i]));
      add4(ab[i], dz);
    }
  }
#pragma unroll
  for (int i = 0; i < NQ; i++) {
    const int q = lane + (i << lg);
    const float4 tg = groups_sum(ag[i], s_sum, lg), tb = groups_sum(ab[i], s_sum, lg);
    if (sub == 0 && q < hq) {
      st4(gpart + (long long)blockIdx.x * 4 * hq + 4 * q, tg);
      st4(bpart + (long long)blockIdx.x * 4 * hq + 4 * q, tb);
    }
  }
}

// a row wider than the registers hold: a wave a row, 128 rows a workgroup (32 a wave).  The rows' two means are taken first
// (the pass after them overwrites dn) and kept one row a lane; then the columns go by in chunks of 256 quads whose column
// sums fit the registers.
__global__ __launch_bounds__(LBLK) void k_layernorm_bwd_wide(float* __restrict__ dn, long long ldd, const float* __restrict__ xhat,
                                                             long long ldh, const float* __restrict__ rstd,
                                                             const float* __restrict__ gamma, long long n, int hq,
                                                             float* __restrict__ gpart, float* __restrict__ bpart) {
  __shared__ float4 s_sum[LBLK];
  constexpr int WAVES = LBLK / 64, RPW = 128 / WAVES;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long r0 = (long long)blockIdx.x * 128;
  const long long r_end = r0 + 128 < n ? r0 + 128 : n;
  const float fh = (float)(4 * hq);
  float k1 = 0.f, k2 = 0.f;
  for (int j = 0; j < RPW; j++) {
    const long long row = r0 + (long long)j * WAVES + wave;
    if (row >= r_end) break;   // (wave-uniform)
    float s1 = 0.f, s2 = 0.f;
    for (int q = lane; q < hq; q += 64) {
      const float4 a = mul4(ld4(gamma + 4 * q), ld4(dn + row * ldd + 4 * q));
      s1 += sum4(a);
      s2 += sum4(mul4(a, ld4(xhat + row * ldh + 4 * q)));
    }
    s1 = group_sum(s1, 6) / fh, s2 = group_sum(s2, 6) / fh;
    if (lane == j) k1 = s1, k2 = s2;
  }
  // (the chunk loop is block-uniform: every thread reaches the barriers)
  for (int c0 = 0; c0 < hq; c0 += 256) {
    float4 gm[4], ag[4], ab[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const int q = c0 + lane + 64 * i;
      gm[i] = q < hq ? ld4(gamma + 4 * q) : make_float4(0.f, 0.f, 0.f, 0.f);
      ag[i] = ab[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    for (int j = 0; j < RPW; j++) {
      const long long row = r0 + (long long)j * WAVES + wave;
      if (row >= r_end) break;
      const float m1 = __shfl(k1, j), m2 = __shfl(k2, j), r = rstd[row];
#pragma unroll
      for (int i = 0; i < 4; i++) {
        const int q = c0 + lane + 64 * i;
        if (q >= hq) continue;
        const float4 d = ld4(dn + row * ldd + 4 * q), x = ld4(xhat + row * ldh + 4 * q);
        const float4 dz = ln_dz(mul4(gm[i], d), x, m1, m2, r);
        st4(dn + row * ldd + 4 * q, dz);
        add4(ag[i], mul4(d, x));
        add4(ab[i], dz);
      }
    }
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const int q = c0 + lane + 64 * i;
      const float4 tg = groups_sum(ag[i], s_sum, 6), tb = groups_sum(ab[i], s_sum, 6);
      if (wave == 0 && q < hq) {
        st4(gpart + (long long)blockIdx.x * 4 * hq + 4 * q, tg);
        st4(bpart + (long long)blockIdx.x * 4 * hq + 4 * q, tb);
      }
    }
  }
}

bool ld_ok(int64_t ld, int32_t H) { return ld >= H && ld % 4 == 0; }
int lanes_lg(int hq) {
  int lg = 0;
  while (lg < 6 && (1 << lg) < hq) lg++;
  return lg;
}

}  // namespace

extern "C" {

int csl_layernorm_relu_fwd_f32(const float* z, int64_t ldz, const float* gamma, const float* beta, float eps, int64_t n,
                               int32_t H, float* y, int64_t ldy, float* xhat, int64_t ldh, float* rstd, int32_t relu,
                               void* stream) {
  if (!(eps > 0.f) || n < 0 || H < 4 || H % 4 != 0 || !ld_ok(ldz, H) || !ld_ok(ldy, H) || (xhat == nullptr) != (rstd == nullptr) ||
      (xhat && (!ld_ok(ldh, H) || !aligned16(xhat))))
    return CSL_E_INVALID;
  if (n == 0) return CSL_OK;
  if (!z || !y || !gamma || !beta || !aligned16(z) || !aligned16(y) || !aligned16(gamma) || !aligned16(beta)) return CSL_E_INVALID;
  const int hq = H / 4, lg = lanes_lg(hq);
  const long long rows = LBLK >> lg, blocks = (n + rows - 1) / rows;
  if (blocks > 0x7fffffffLL) return CSL_E_INVALID;
  hipStream_t st = (hipStream_t)stream;
  if (hq <= 64)
    hipLaunchKernelGGL(k_layernorm_fwd<1>, dim3((unsigned)blocks), dim3(LBLK), 0, st, z, (long long)ldz, gamma, beta, eps,
                       (long long)n, hq, lg, y, (long long)ldy, xhat, (long long)ldh, rstd, (int)relu);
  else if (hq <= LN_REG_HQ)
    hipLaunchKernelGGL(k_layernorm_fwd<4>, dim3((unsigned)blocks), dim3(LBLK), 0, st, z, (long long)ldz, gamma, beta, eps,
                       (long long)n, hq, lg, y, (long long)ldy, xhat, (long long)ldh, rstd, (int)relu);
  else
    hipLaunchKernelGGL(k_layernorm_fwd_wide, dim3((unsigned)blocks), dim3(LBLK), 0, st, z, (long long)ldz, gamma, beta, eps,
                       (long long)n, hq, y, (long long)ldy, xhat, (long long)ldh, rstd, (int)relu);
  return done();
}

int64_t csl_layernorm_bwd_scratch(int64_t n_pad, int32_t H) {
  if (n_pad < 0 || H < 4 || H % 4 != 0) return CSL_E_INVALID;
  const long long rpb = ln_rows(n_pad, H / 4);
  return ((n_pad + rpb - 1) / rpb) * (int64_t)H;
}

int csl_layernorm_bwd_f32(float* dn, int64_t ldd, const float* xhat, int64_t ldh, const float* rstd, const float* gamma,
                          int64_t n, int64_t n_pad, int32_t H, float* gpart, float* bpart, void* stream) {
  if (n < 0 || n_pad < n || H < 4 || H % 4 != 0 || !ld_ok(ldd, H) || !ld_ok(ldh, H)) return CSL_E_INVALID;
  if (n_pad == 0) return CSL_OK;
  if (!gpart || !bpart || !aligned16(gpart) || !aligned16(bpart) || !gamma || !aligned16(gamma)) return CSL_E_INVALID;
  if (n > 0 && (!dn || !xhat || !rstd || !aligned16(dn) || !aligned16(xhat))) return CSL_E_INVALID;
  const int hq = H / 4, lg = lanes_lg(hq);
  const long long rpb = ln_rows(n_pad, hq), blocks = (n_pad + rpb - 1) / rpb;
  if (blocks > 0x7fffffffLL) return CSL_E_INVALID;
  hipStream_t st = (hipStream_t)stream;
  if (hq <= 64)
    hipLaunchKernelGGL(k_layernorm_bwd<1>, dim3((unsigned)blocks), dim3(LBLK), 0, st, dn, (long long)ldd, xhat, (long long)ldh, rstd,
                       gamma, (long long)n, hq, lg, rpb, gpart, bpart);
  else if (hq <= LN_REG_HQ)
    hipLaunchKernelGGL(k_layernorm_bwd<4>, dim3((unsigned)blocks), dim3(LBLK), 0, st, dn, (long long)ldd, xhat, (long long)ldh, rstd,
                       gamma, (long long)n, hq, lg, rpb, gpart, bpart);
  else
    hipLaunchKernelGGL(k_layernorm_bwd_wide, dim3((unsigned)blocks), dim3(LBLK), 0, st, dn, (long long)ldd, xhat, (long long)ldh,
                       rstd, gamma, (long long)n, hq, gpart, bpart);
  return done();
}

}  // extern "C"
