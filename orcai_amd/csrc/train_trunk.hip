// train_trunk.hip -- training-mode BatchNorm and the backward kernels of the convolutional trunk of ResNetLSTM for
// gfx950, on the padded channel-quad planes of model_fwd.hip ([snippet][CQ][HP][WP][4], zero pads never written).
// Reference: architectures.py:162-206 (layers), train.py:201-219 (model.fit computes these gradients inside Keras).
//
// Because the pads of every activation / gradient tensor are zero, reductions run over whole planes with no masks.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "lds_optin.h"
#include "orcai_hip.h"
#include "zero_fill.h"

namespace {

// Sum of v over the 64 lanes, delivered in lane 63: four row_shr steps inside each row of 16 lanes, then row_bcast:15 / row_bcast:31 carry the row totals
// across rows -- DPP operands instead of six ds_bpermute per value (a marching wave reduces dozens of accumulators when it ends).
__device__ __forceinline__ float wave_sum_lane63(float v) {
  v += __uint_as_float(__builtin_amdgcn_update_dpp(0u, __float_as_uint(v), 0x111 /*row_shr:1*/, 0xf, 0xf, true));
  v += __uint_as_float(__builtin_amdgcn_update_dpp(0u, __float_as_uint(v), 0x112 /*row_shr:2*/, 0xf, 0xf, true));
  v += __uint_as_float(__builtin_amdgcn_update_dpp(0u, __float_as_uint(v), 0x114 /*row_shr:4*/, 0xf, 0xf, true));
  v += __uint_as_float(__builtin_amdgcn_update_dpp(0u, __float_as_uint(v), 0x118 /*row_shr:8*/, 0xf, 0xf, true));  // lane 15 of every row: the row's sum
  v += __uint_as_float(__builtin_amdgcn_update_dpp(0u, __float_as_uint(v), 0x142 /*row_bcast:15*/, 0xa, 0xf, false));  // rows 1, 3 += lane 15 of rows 0, 2
  v += __uint_as_float(__builtin_amdgcn_update_dpp(0u, __float_as_uint(v), 0x143 /*row_bcast:31*/, 0xc, 0xf, false));  // rows 2, 3 += lane 31
  return v;
}

// The same for a double (the two halves travel as 32-bit DPP moves): the float64 block reductions of the pooling backward were LDS trees of
// eight barrier-separated levels over a [256][8 .. 12] double image (16 .. 24 KB of LDS per workgroup, nine barriers per reduction).
template <int CTRL, int ROW_MASK, bool BOUND>
__device__ __forceinline__ double dpp_f64(double v) {
  const uint32_t lo = (uint32_t)__double2loint(v), hi = (uint32_t)__double2hiint(v);
  return __hiloint2double((int)__builtin_amdgcn_update_dpp(0u, hi, CTRL, ROW_MASK, 0xf, BOUND), (int)__builtin_amdgcn_update_dpp(0u, lo, CTRL, ROW_MASK, 0xf, BOUND));
}
__device__ __forceinline__ double wave_sum_lane63(double v) {
  v += dpp_f64<0x111, 0xf, true>(v);
  v += dpp_f64<0x112, 0xf, true>(v);
  v += dpp_f64<0x114, 0xf, true>(v);
  v += dpp_f64<0x118, 0xf, true>(v);
  v += dpp_f64<0x142, 0xa, false>(v);
  v += dpp_f64<0x143, 0xc, false>(v);
  return v;
}



typedef float f32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ f32x4 mfma16(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
inline uint32_t magic_for(uint32_t d) { return (uint32_t)((0x100000000ull + d - 1) / d); }
inline unsigned blocks_for(int64_t n) { return (unsigned)((n + 255) / 256); }

// ---------------------------------------------------------------- per-channel sums over planes
// sums[c] += sum x, sumsq[c] += sum x^2 (sumsq may be NULL) over all snippets and pixels; float64 accumulation.
__global__ __launch_bounds__(256) void planes_sums_kernel(const float* __restrict__ x, int CQ, int64_t plane, int B, double* __restrict__ sums,
                                                           double* __restrict__ sumsq) {
  __shared__ double red[256][4];
  const int cq = blockIdx.y;
  double s[4] = {0, 0, 0, 0}, q[4] = {0, 0, 0, 0};
  // snippet-outer / pixel-inner: no 64-bit division per element (it cost more than the rest of the loop body)
  const int p0 = blockIdx.x * 256 + threadIdx.x, pstep = gridDim.x * 256;
  // last snippet first: the pass follows the kernel that wrote x in ascending snippet order, and whatever of x is still in the
  // Infinity Cache is its tail
  for (int b = B - 1; b >= 0; --b) {
    const float4* xp = reinterpret_cast<const float4*>(x) + ((int64_t)b * CQ + cq) * plane;
    for (int p = p0; p < (int)plane; p += pstep) {
      const float4 v = xp[p];
      s[0] += v.x; s[1] += v.y; s[2] += v.z; s[3] += v.w;
      q[0] += (double)v.x * v.x; q[1] += (double)v.y * v.y; q[2] += (double)v.z * v.z; q[3] += (double)v.w * v.w;
    }
  }
  for (int pass = 0; pass < (sumsq ? 2 : 1); ++pass) {
    const double* src = pass ? q : s;
    for (int k = 0; k < 4; ++k) red[threadIdx.x][k] = src[k];
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
      if (threadIdx.x < o)
        for (int k = 0; k < 4; ++k) red[threadIdx.x][k] += red[threadIdx.x + o][k];
      __syncthreads();
    }
    if (threadIdx.x < 4) atomicAdd(&(pass ? sumsq : sums)[cq * 4 + threadIdx.x], red[0][threadIdx.x]);
    __syncthreads();
  }
}

// The same sums for SMALL planes (blocks 3-4: a few thousand pixels): there planes_sums_kernel's 128 grid-striding workgroups per
// quad, each ending in a block reduction and same-line double atomics, cost more than the data (48 us for 30 MB).  One workgroup per
// 4096 consecutive pixels of a (snippet, quad) plane, 16 loads per thread four at a time, totals added to one of SUM_SHARDS copies of
// the accumulators (copy = workgroup index mod SUM_SHARDS) so that same-line atomics stay few; the finish kernel adds the copies:
// 13 us.  On block 1 this shape is SLOWER than the striding kernel (284 vs 239 us), so the launcher picks by plane size.
constexpr int SUM_SHARDS = 32;
__global__ __launch_bounds__(256) void planes_sums_sharded_kernel(const float* __restrict__ x, int CQ, int plane, int nchunk, double* __restrict__ shards /*[SUM_SHARDS][CQ][8]*/) {
  __shared__ double red[4][8];
  const int cq = blockIdx.y, b = blockIdx.x / nchunk, chunk = blockIdx.x - b * nchunk;
  const float4* xp = reinterpret_cast<const float4*>(x) + ((int64_t)b * CQ + cq) * plane;
  double t[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  const int p0 = chunk * 4096 + threadIdx.x;
#pragma unroll
  for (int it = 0; it < 4; ++it) {
    float4 v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int p = p0 + (it * 4 + u) * 256;
      v[u] = p < plane ? xp[p] : make_float4(0.f, 0.f, 0.f, 0.f);  // the tail adds zeros, like the pads
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      t[0] += v[u].x; t[1] += v[u].y; t[2] += v[u].z; t[3] += v[u].w;
      t[4] += (double)v[u].x * v[u].x; t[5] += (double)v[u].y * v[u].y; t[6] += (double)v[u].z * v[u].z; t[7] += (double)v[u].w * v[u].w;
    }
  }
#pragma unroll
  for (int k = 0; k < 8; ++k)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) t[k] += __shfl_xor(t[k], o, 64);
  if ((threadIdx.x & 63) == 0)
#pragma unroll
    for (int k = 0; k < 8; ++k) red[threadIdx.x >> 6][k] = t[k];
  __syncthreads();
  if (threadIdx.x < 8)
    atomicAdd(&shards[((int64_t)(blockIdx.x % SUM_SHARDS) * CQ + cq) * 8 + threadIdx.x],
              red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x]);
}

__global__ void bn_finish_stats_sharded_kernel(const double* __restrict__ shards, int C, int CQ, double count, float* __restrict__ mean, float* __restrict__ var) {
  const int c = blockIdx.x * 64 + threadIdx.x;
  if (c >= C) return;
  double su = 0.0, sq = 0.0;
  for (int sh = 0; sh < SUM_SHARDS; ++sh) {
    su += shards[((int64_t)sh * CQ + (c >> 2)) * 8 + (c & 3)];
    sq += shards[((int64_t)sh * CQ + (c >> 2)) * 8 + 4 + (c & 3)];
  }
  const double mu = su / count;
  const double v = sq / count - mu * mu;
  mean[c] = (float)mu;
  var[c] = (float)(v < 0.0 ? 0.0 : v);
}

__global__ void bn_finish_stats_kernel(const double* __restrict__ sums, const double* __restrict__ sumsq, int C, double count, float* __restrict__ mean,
                                       float* __restrict__ var) {
  const int c = blockIdx.x * 64 + threadIdx.x;
  if (c >= C) return;
  const double mu = sums[c] / count;
  double v = sumsq[c] / count - mu * mu;
  mean[c] = (float)mu;
  var[c] = (float)(v < 0.0 ? 0.0 : v);
}

// y = [relu](v * s + t) at interior pixels (s = gamma*rsqrt(var+eps), t = beta - mean*s); pads of y are left untouched (zero).
__global__ __launch_bounds__(256) void bn_planes_apply_kernel(const float* __restrict__ v, int C, int H, int W, int WP, int R, const float* __restrict__ mean,
                                                               const float* __restrict__ var, const float* __restrict__ gamma,
                                                               const float* __restrict__ beta, float eps, int relu, float* __restrict__ y, int B) {
  const int CQ = (C + 3) >> 2;
  const int pix = blockIdx.x * 256 + threadIdx.x;  // grid.y = (snippet, quad): 32-bit index math only
  if (pix >= H * W) return;
  const int bq = blockIdx.y, cq = bq % CQ;
  const int yy = pix / W, xx = pix - yy * W;
  const int64_t off = (int64_t)bq * ((int64_t)(H + 2 * R) * WP) + (int64_t)(yy + R) * WP + xx;
  const float4 a = reinterpret_cast<const float4*>(v)[off];
  float in[4] = {a.x, a.y, a.z, a.w}, o[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int c = cq * 4 + k;
    if (c < C) {
      const float s = gamma[c] * rsqrtf(var[c] + eps);
      float r = fmaf(in[k], s, beta[c] - mean[c] * s);
      o[k] = relu ? fmaxf(r, 0.0f) : r;
    } else {
      o[k] = 0.0f;
    }
  }
  reinterpret_cast<float4*>(y)[off] = make_float4(o[0], o[1], o[2], o[3]);
}

// BN backward, reduction part over planes: dy_eff = relu ? dy*(y>0) : dy;  dbeta[c] += sum dy_eff, dgamma[c] += sum dy_eff*xhat
__global__ __launch_bounds__(256) void bn_planes_bwd_sums_kernel(const float* __restrict__ dy, const float* __restrict__ v, int C, int64_t plane, int B,
                                                                  const float* __restrict__ mean, const float* __restrict__ var,
                                                                  const float* __restrict__ gamma, const float* __restrict__ beta, float eps, int relu,
                                                                  double* __restrict__ dbeta, double* __restrict__ dgamma) {
  __shared__ double red[256][4];
  const int cq = blockIdx.y, CQ = (C + 3) >> 2;
  float mu[4], inv[4], g[4], bt[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int c = cq * 4 + k, cc = c < C ? c : 0;
    mu[k] = mean[cc]; inv[k] = rsqrtf(var[cc] + eps); g[k] = gamma[cc]; bt[k] = beta[cc];
  }
  double s[4] = {0, 0, 0, 0}, q[4] = {0, 0, 0, 0};
  const int p0 = blockIdx.x * 256 + threadIdx.x, pstep = gridDim.x * 256;
  for (int b = B - 1; b >= 0; --b) {  // snippet-outer / pixel-inner: no 64-bit division per element
    const int64_t base = ((int64_t)b * CQ + cq) * plane;
    const float4* dp = reinterpret_cast<const float4*>(dy) + base;
    const float4* vp = reinterpret_cast<const float4*>(v) + base;
    for (int p = p0; p < (int)plane; p += pstep) {
      const float4 d4 = dp[p];
      const float4 v4 = vp[p];
      const float d[4] = {d4.x, d4.y, d4.z, d4.w}, vv[4] = {v4.x, v4.y, v4.z, v4.w};
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float xh = (vv[k] - mu[k]) * inv[k];
        float de = d[k];
        if (relu && !(fmaf(xh, g[k], bt[k]) > 0.0f)) de = 0.0f;
        s[k] += (double)de;
        q[k] += (double)de * (double)xh;
      }
    }
  }
  for (int pass = 0; pass < 2; ++pass) {
    const double* src = pass ? q : s;
    for (int k = 0; k < 4; ++k) red[threadIdx.x][k] = src[k];
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
      if (threadIdx.x < o)
        for (int k = 0; k < 4; ++k) red[threadIdx.x][k] += red[threadIdx.x + o][k];
      __syncthreads();
    }
    if (threadIdx.x < 4 && cq * 4 + threadIdx.x < C) atomicAdd(&(pass ? dgamma : dbeta)[cq * 4 + threadIdx.x], red[0][threadIdx.x]);
    __syncthreads();
  }
}

// dv = gamma*inv*(dy_eff - dbeta/N - xhat*dgamma/N) at interior pixels (pads of dv stay zero)
__global__ __launch_bounds__(256) void bn_planes_bwd_apply_kernel(const float* __restrict__ dy, const float* __restrict__ v, int C, int H, int W, int WP, int R,
                                                                   const float* __restrict__ mean, const float* __restrict__ var,
                                                                   const float* __restrict__ gamma, const float* __restrict__ beta, float eps, int relu,
                                                                   const double* __restrict__ dbeta, const double* __restrict__ dgamma, double count,
                                                                   float* __restrict__ dv, int B) {
  const int CQ = (C + 3) >> 2;
  const int64_t interior = (int64_t)H * W;
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (int64_t)B * CQ * interior) return;
  const int64_t bq = idx / interior, pix = idx - bq * interior;
  const int cq = (int)(bq % CQ);
  const int yy = (int)(pix / W), xx = (int)(pix - (int64_t)yy * W);
  const int64_t off = bq * ((int64_t)(H + 2 * R) * WP) + (int64_t)(yy + R) * WP + xx;
  const float4 d4 = reinterpret_cast<const float4*>(dy)[off];
  const float4 v4 = reinterpret_cast<const float4*>(v)[off];
  const float d[4] = {d4.x, d4.y, d4.z, d4.w}, vv[4] = {v4.x, v4.y, v4.z, v4.w};
  float o[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int c = cq * 4 + k;
    if (c < C) {
      const float inv = rsqrtf(var[c] + eps);
      const float xh = (vv[k] - mean[c]) * inv;
      float de = d[k];
      if (relu && !(fmaf(xh, gamma[c], beta[c]) > 0.0f)) de = 0.0f;
      o[k] = gamma[c] * inv * (de - (float)(dbeta[c] / count) - xh * (float)(dgamma[c] / count));
    } else {
      o[k] = 0.0f;
    }
  }
  reinterpret_cast<float4*>(dv)[off] = make_float4(o[0], o[1], o[2], o[3]);
}

// ---------------------------------------------------------------- BN backward apply fused with the transposed pointwise conv
// dv = gamma*inv*(dy_eff - dbeta/N - xhat*dgamma/N)  (as bn_planes_bwd_apply_kernel)  AND  du = Wpw dv  in one pass:
// one wave = 64 consecutive flat pixels (1 KiB-aligned windows, no halo: both ops are per pixel), lane = pixel.  Per channel
// quad of the conv OUTPUT side the lane loads dy and v (dwordx4 each), forms dv on the VALU with wave-uniform per-channel
// constants, stores it (the pointwise weight gradient reads it next), transposes the 4 VGPRs into MFMA B fragments
// (permlane swaps, as in sepconv_kernel) and multiplies by the transposed pointwise weights (A operand, row = conv INPUT
// channel).  Replaces bn_planes_bwd_apply_kernel + the ktap = 1 sepconv pass: dv is no longer re-read for du.
__device__ __forceinline__ void swap32t(float& a, float& b) {
  auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(a), __float_as_uint(b), false, false);
  a = __uint_as_float(r[0]);
  b = __uint_as_float(r[1]);
}
__device__ __forceinline__ void swap16t(float& a, float& b) {
  auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(a), __float_as_uint(b), false, false);
  a = __uint_as_float(r[0]);
  b = __uint_as_float(r[1]);
}

template <int MT>
__global__ __launch_bounds__(256) void bn_bwd_pw_kernel(const float* dy, const float* __restrict__ v, int C, int H, int W, int WP, int R,
                                                         const float* __restrict__ mean, const float* __restrict__ var, const float* __restrict__ gamma,
                                                         const float* __restrict__ beta, float eps, int relu, const double* __restrict__ dbeta,
                                                         const double* __restrict__ dgamma, float inv_count, const float* __restrict__ wt /*[C][Cin]*/, int Cin,
                                                         float* dv /*may alias dy*/, float* __restrict__ du /*[B][CQin][HP][WP][4]*/, int tasks,
                                                         uint32_t magic_WP) {
  const int lane = threadIdx.x & 63;
  const int task = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (task >= tasks) return;
  const int b = blockIdx.y;
  const int lk = lane >> 4, lj = lane & 15;
  const int CQ = (C + 3) >> 2, CQi = (Cin + 3) >> 2;
  const int plane = (H + 2 * R) * WP;
  const int qbase = R * WP + task * 64;  // interior rows only; windows are 1 KiB aligned (plane and row pitch are multiples of 4 pixels... of 64 B)
  const int q = qbase + lane;
  const int row = (int)__umulhi((uint32_t)q, magic_WP);
  const bool live = (q - row * WP) < W && row < R + H;
  const int qc = q < plane ? q : plane - 1;
  const float4* dyp = reinterpret_cast<const float4*>(dy) + (int64_t)b * CQ * plane + qc;
  const float4* vp = reinterpret_cast<const float4*>(v) + (int64_t)b * CQ * plane + qc;
  float4* dvp = reinterpret_cast<float4*>(dv) + (int64_t)b * CQ * plane + qc;
  f32x4 acc[MT][4];
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[m][t] = (f32x4){0.f, 0.f, 0.f, 0.f};
  float4 nd = dyp[0], nv = vp[0];
  for (int cq = 0; cq < CQ; ++cq) {
    const float4 d4 = nd, v4 = nv;
    if (cq + 1 < CQ) {
      nd = dyp[(int64_t)(cq + 1) * plane];
      nv = vp[(int64_t)(cq + 1) * plane];
    }
    float afrag[MT];
#pragma unroll
    for (int m = 0; m < MT; ++m) {
      const int co = cq * 4 + lk, ci = m * 16 + lj;  // k = conv-output channel, row = conv-input channel
      const bool ok = co < C && ci < Cin;
      const float av = wt[ok ? co * Cin + ci : 0];
      afrag[m] = ok ? av : 0.0f;
    }
    const float dd[4] = {d4.x, d4.y, d4.z, d4.w}, vv[4] = {v4.x, v4.y, v4.z, v4.w};
    float o[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int c = cq * 4 + k;  // wave-uniform: the per-channel constants are scalar loads
      if (c < C) {
        const float inv = rsqrtf(var[c] + eps);
        const float xh = (vv[k] - mean[c]) * inv;
        float de = dd[k];
        if (relu && !(fmaf(xh, gamma[c], beta[c]) > 0.0f)) de = 0.0f;
        o[k] = live ? gamma[c] * inv * (de - (float)dbeta[c] * inv_count - xh * ((float)dgamma[c] * inv_count)) : 0.0f;
      } else {
        o[k] = 0.0f;
      }
    }
    if (live) dvp[(int64_t)cq * plane] = make_float4(o[0], o[1], o[2], o[3]);
    swap32t(o[0], o[2]);
    swap32t(o[1], o[3]);
    swap16t(o[0], o[1]);
    swap16t(o[2], o[3]);
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int m = 0; m < MT; ++m) acc[m][t] = mfma16(afrag[m], o[t], acc[m][t]);
  }
  float4* dup = reinterpret_cast<float4*>(du) + (int64_t)b * CQi * plane;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int flat = qbase + 16 * t + lj;
    const int r2 = (int)__umulhi((uint32_t)flat, magic_WP);
    if (!((flat - r2 * WP) < W && r2 < R + H)) continue;
#pragma unroll
    for (int m = 0; m < MT; ++m) {
      const int oq = m * 4 + lk;
      if (oq < CQi) dup[(int64_t)oq * plane + flat] = make_float4(acc[m][t][0], acc[m][t][1], acc[m][t][2], acc[m][t][3]);
    }
  }
}


// ---------------------------------------------------------------- BN backward apply + du = Wpw dv + pointwise weight gradient, one pass
// bn_bwd_pw_kernel forms dv per pixel, stores it, and orcai_outer_reduce reads it back (with the depthwise output u) for
// dWpw[ci][co] = sum_pixels u[ci][p] dv[co][p]: dv is written and read once for nothing else.  Here the wave that forms dv also contracts it
// with u: dv and u of its 64-pixel window go through a WAVE-PRIVATE LDS image [channel][pixel] (pitch 66: the 16 channel rows x 2 pixels of a
// half-wave hit 32 distinct banks), read back as MFMA operands with k = pixel (k-step s takes pixels {4 s + lk}).  No workgroup barrier:
// a wave reads only what it wrote.  Waves walk the windows of one snippet (grid.y) with a stride, accumulate the MT x NT weight-gradient
// tiles in registers and write one partial product each; add_partials_kernel sums them into dWpw.  dv never reaches HBM (one write and one
// read of the widest gradient tensor of every separable conv less per step).  Channels: Cin <= 16 MT, C <= 16 NT, (MT + NT) * 16.5 KiB of
// LDS per four-wave workgroup; beyond MT + NT = 4 workgroups of two waves (three per compute unit at 5 tiles, ~21 KiB per wave) -- used up to
// MT + NT = 6; measured (profiles/r03_ab_pw_wgrad_tiles.log): a win of 0.42 ms per step at MT + NT <= 4 (block 1 of orcai-V1), a LOSS of 0.28 + 0.10 ms with block 2 on the two-wave
// workgroups (1.5 waves per SIMD), so the launcher accepts MT + NT <= 4 by default and wider layers keep the two kernels.
template <int MT, int NT, int NW /*waves per workgroup: 4, or 2 where four wave images would leave one workgroup per compute unit*/>
__global__ __launch_bounds__(64 * NW) void bn_bwd_pw_wgrad_kernel(const float* __restrict__ dy, const float* __restrict__ v, const float* __restrict__ u /*[B][CQi][HP][WP][4]*/, int C,
                                                               int H, int W, int WP, int R, const float* __restrict__ mean, const float* __restrict__ var,
                                                               const float* __restrict__ gamma, const float* __restrict__ beta, float eps, int relu,
                                                               const double* __restrict__ dbeta, const double* __restrict__ dgamma, float inv_count,
                                                               const float* __restrict__ wt /*[C][Cin]*/, int Cin, float* __restrict__ du /*[B][CQi][HP][WP][4]*/,
                                                               int tasks, uint32_t magic_WP, float* __restrict__ part /*[gridDim.y][gridDim.x][NW][Cin*C]*/) {
  constexpr int P = 66, MAXQ = 4 * (MT > NT ? MT : NT);
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lk = lane >> 4, lj = lane & 15;
  float* As = smem + wave * (MT + NT) * 16 * P;  // [MT*16][P]: u, rows past Cin stay zero
  float* Bs = As + MT * 16 * P;                  // [NT*16][P]: dv
  for (int i = lane; i < (MT + NT) * 16 * P; i += 64) As[i] = 0.0f;
  const int b = blockIdx.y;
  const int CQ = (C + 3) >> 2, CQi = (Cin + 3) >> 2;
  const int plane = (H + 2 * R) * WP;
  f32x4 wacc[MT * NT];
#pragma unroll
  for (int i = 0; i < MT * NT; ++i) wacc[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
  const float4* dyb = reinterpret_cast<const float4*>(dy) + (int64_t)b * CQ * plane;
  const float4* vb = reinterpret_cast<const float4*>(v) + (int64_t)b * CQ * plane;
  const float4* ub = reinterpret_cast<const float4*>(u) + (int64_t)b * CQi * plane;
  float4* dub = reinterpret_cast<float4*>(du) + (int64_t)b * CQi * plane;

  // All loads of a window (dy, v of every output quad, u of every input quad: 16 B per lane each) are requested while the PREVIOUS window's
  // weight-gradient MFMAs run -- with the LDS images two workgroups (8 waves) fit a compute unit, so a wave has to cover its own memory
  // latency; requests past the last window are clamped to it (unconditional, never used).
  constexpr int MAXQO = 4 * NT;
  float4 ru[MAXQ], rd[MAXQO], rv[MAXQO];
  auto request = [&](int task) {
    const int tc = task < tasks ? task : tasks - 1;
    const int q = R * WP + tc * 64 + lane;
    const int qc = q < plane ? q : plane - 1;
#pragma unroll
    for (int i = 0; i < MAXQ; ++i)
      if (i < CQi) ru[i] = ub[(int64_t)i * plane + qc];
#pragma unroll
    for (int i = 0; i < MAXQO; ++i)
      if (i < CQ) {
        rd[i] = dyb[(int64_t)i * plane + qc];
        rv[i] = vb[(int64_t)i * plane + qc];
      }
  };
  request(blockIdx.x * NW + wave);
  for (int task = blockIdx.x * NW + wave; task < tasks; task += gridDim.x * NW) {
    const int qbase = R * WP + task * 64;  // interior rows only; 1 KiB-aligned windows
    const int q = qbase + lane;
    const int row = (int)__umulhi((uint32_t)q, magic_WP);
    const bool live = (q - row * WP) < W && row < R + H;
    f32x4 acc[MT][4];
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
      for (int t = 0; t < 4; ++t) acc[m][t] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int cq = 0; cq < MAXQO; ++cq) {
      if (cq < CQ) {  // wave-uniform
        const float4 d4 = rd[cq], v4 = rv[cq];
        float afrag[MT];
#pragma unroll
        for (int m = 0; m < MT; ++m) {
          const int co = cq * 4 + lk, ci = m * 16 + lj;  // k = conv-output channel, row = conv-input channel
          const bool ok = co < C && ci < Cin;
          const float av = wt[ok ? co * Cin + ci : 0];
          afrag[m] = ok ? av : 0.0f;
        }
        const float dd[4] = {d4.x, d4.y, d4.z, d4.w}, vv[4] = {v4.x, v4.y, v4.z, v4.w};
        float o[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int c = cq * 4 + k;  // wave-uniform: the per-channel constants are scalar loads
          if (c < C) {
            const float inv = rsqrtf(var[c] + eps);
            const float xh = (vv[k] - mean[c]) * inv;
            float de = dd[k];
            if (relu && !(fmaf(xh, gamma[c], beta[c]) > 0.0f)) de = 0.0f;
            o[k] = live ? gamma[c] * inv * (de - (float)dbeta[c] * inv_count - xh * ((float)dgamma[c] * inv_count)) : 0.0f;
          } else {
            o[k] = 0.0f;
          }
          Bs[(4 * cq + k) * P + lane] = o[k];
        }
        swap32t(o[0], o[2]);
        swap32t(o[1], o[3]);
        swap16t(o[0], o[1]);
        swap16t(o[2], o[3]);
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
          for (int m = 0; m < MT; ++m) acc[m][t] = mfma16(afrag[m], o[t], acc[m][t]);
      }
    }
#pragma unroll
    for (int i = 0; i < MAXQ; ++i)
      if (i < CQi) {
        As[(4 * i + 0) * P + lane] = ru[i].x; As[(4 * i + 1) * P + lane] = ru[i].y; As[(4 * i + 2) * P + lane] = ru[i].z; As[(4 * i + 3) * P + lane] = ru[i].w;
      }
    request(task + gridDim.x * NW);  // in flight during the stores and the weight-gradient MFMAs below
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int flat = qbase + 16 * t + lj;
      const int r2 = (int)__umulhi((uint32_t)flat, magic_WP);
      if (!((flat - r2 * WP) < W && r2 < R + H)) continue;
#pragma unroll
      for (int m = 0; m < MT; ++m) {
        const int oq = m * 4 + lk;
        if (oq < CQi) dub[(int64_t)oq * plane + flat] = make_float4(acc[m][t][0], acc[m][t][1], acc[m][t][2], acc[m][t][3]);
      }
    }
    // dWpw tile (mt, nt) += sum over this window's 64 pixels: A[i = ci][k = pixel] B[k = pixel][j = co]; the image was written by this
    // wave alone (LDS operations of one wave complete in order)
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        const float* ar = As + (mt * 16 + lj) * P + lk;
        const float* br = Bs + (nt * 16 + lj) * P + lk;
        f32x4 c0 = wacc[mt * NT + nt], c1 = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < 16; s += 2) {
          c0 = mfma16(ar[4 * s], br[4 * s], c0);
          c1 = mfma16(ar[4 * s + 4], br[4 * s + 4], c1);
        }
        wacc[mt * NT + nt] = c0 + c1;
      }
  }
  float* mine = part + ((int64_t)(blockIdx.y * gridDim.x + blockIdx.x) * NW + wave) * Cin * C;
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int ca = mt * 16 + lk * 4 + r, cb = nt * 16 + lj;
        if (ca < Cin && cb < C) mine[ca * C + cb] = wacc[mt * NT + nt][r];
      }
}

__global__ void f64_to_f32_kernel(const double* __restrict__ a, float* __restrict__ b, int n, int accumulate) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i < n) b[i] = accumulate ? b[i] + (float)a[i] : (float)a[i];
}
// the two BatchNorm parameter gradients (d beta, d gamma) in one launch
__global__ void f64_to_f32_pair_kernel(const double* __restrict__ a0, float* __restrict__ b0, const double* __restrict__ a1, float* __restrict__ b1, int n) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i < n) {
    b0[i] = (float)a0[i];
    b1[i] = (float)a1[i];
  }
}

// ---------------------------------------------------------------- max-pool backward
// dy[y][x] = sum over the pooling windows (i, j) containing (y, x) of dout[i][j] * [ybn[y][x] == max of that window]
// MaxPooling2D((3,2), strides 2, "same"): windows overlap only in rows (row 2i+2-pt closes window i and opens window i+1).
// One thread owns pooled column j of one (snippet, quad) and walks PB_ROWS pooled rows downwards, carrying the shared
// row's values and its partial gradient in registers, so every input value is loaded once and every gradient written once
// (plus a one-window halo at the top of the chunk that recomputes the carry).  Lanes run along j: 32 contiguous bytes per lane.
constexpr int PB_ROWS = 8;

__global__ __launch_bounds__(256) void pool_bwd_kernel(const float* __restrict__ dout /*[B][CQ][Ho+2R][WPo][4]*/, const float* __restrict__ ybn /*[B][CQ][HP][WP][4]*/,
                                                        int C, int H, int W, int WP, int R, int Ho, int Wo, int WPo, int pad_top, int pad_left,
                                                        float* __restrict__ dy /*[B][CQ][HP][WP][4]*/, int B, const float* __restrict__ bn_gamma,
                                                        const float* __restrict__ bn_mean, const float* __restrict__ bn_var, float bn_eps,
                                                        double* __restrict__ bn_sums /*[2][4*CQ]: sum dy, sum dy*xhat*/,
                                                        double* __restrict__ dout_sums = nullptr /*[4*CQ]: sum of dout per channel (the residual conv's bias gradient)*/) {
  // bn_gamma != NULL: ybn holds the PRE-BatchNorm tensor v; BN(v) = fma(v, gamma*inv, ..) is monotone, increasing for gamma >= 0
  // and decreasing for gamma < 0, so the arg-max of BN(v) is the arg-max of sign(gamma) * v.
  // bn_sums != NULL: the reductions of that BatchNorm's backward (sum of dy and of dy * xhat per channel) are accumulated here,
  // where every gradient value and the v it belongs to are in registers anyway (one workgroup = one (snippet, quad): blockIdx.y).
  const int CQ = (C + 3) >> 2;
  const int nchunk = (Ho + PB_ROWS - 1) / PB_ROWS;
  const int idx = blockIdx.x * 256 + threadIdx.x;
  const bool in_range = idx < nchunk * Wo;
  const int j = in_range ? idx % Wo : 0;
  const int chunk = in_range ? idx / Wo : 0;
  const int64_t bq = blockIdx.y;
  float bs[4] = {0.f, 0.f, 0.f, 0.f}, bqs[4] = {0.f, 0.f, 0.f, 0.f}, bmu[4] = {0.f, 0.f, 0.f, 0.f}, binv[4] = {0.f, 0.f, 0.f, 0.f};
  float ds[4] = {0.f, 0.f, 0.f, 0.f};  // dout_sums: every pooled pixel belongs to exactly one thread's OWN windows (i0 <= i < i1)
  if (bn_sums) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int c = (int)(bq % CQ) * 4 + k, cc = c < C ? c : 0;
      bmu[k] = bn_mean[cc];
      binv[k] = rsqrtf(bn_var[cc] + bn_eps);
    }
  }
  const float4* yp = reinterpret_cast<const float4*>(ybn) + bq * ((int64_t)(H + 2 * R) * WP);
  const float4* dp = reinterpret_cast<const float4*>(dout) + bq * ((int64_t)(Ho + 2 * R) * WPo);
  float4* gp = reinterpret_cast<float4*>(dy) + bq * ((int64_t)(H + 2 * R) * WP);
  const int x0 = 2 * j - pad_left, x1 = x0 + 1;
  const bool cx0 = x0 >= 0 && x0 < W, cx1 = x1 < W;  // x1 >= 0 always
  const float4 ninf = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY), zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
  float4 sgn = make_float4(1.f, 1.f, 1.f, 1.f);
  if (bn_gamma) {
    const int c0 = (int)(bq % CQ) * 4;
    sgn = make_float4(bn_gamma[c0 < C ? c0 : 0] < 0.f ? -1.f : 1.f, bn_gamma[c0 + 1 < C ? c0 + 1 : 0] < 0.f ? -1.f : 1.f,
                      bn_gamma[c0 + 2 < C ? c0 + 2 : 0] < 0.f ? -1.f : 1.f, bn_gamma[c0 + 3 < C ? c0 + 3 : 0] < 0.f ? -1.f : 1.f);
  }
  auto ld = [&](int y, int x, bool cx) -> float4 {
    if (!(cx && y >= 0 && y < H)) return ninf;
    const float4 t = yp[(int64_t)(y + R) * WP + x];
    return make_float4(t.x * sgn.x, t.y * sgn.y, t.z * sgn.z, t.w * sgn.w);
  };
  auto mx4 = [](float4 a, float4 b) { return make_float4(fmaxf(a.x, b.x), fmaxf(a.y, b.y), fmaxf(a.z, b.z), fmaxf(a.w, b.w)); };
  auto route_first = [](float4 v0, float4 v1, float4 v2, float4 v3, float4 v4, float4 v5, float4 m, float4 d, float4 (&g)[6]) {
    const float4 v[6] = {v0, v1, v2, v3, v4, v5};
    const float mm[4] = {m.x, m.y, m.z, m.w}, dd[4] = {d.x, d.y, d.z, d.w};
    float o[6][4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      bool taken = false;
#pragma unroll
      for (int p = 0; p < 6; ++p) {
        const float vv = k == 0 ? v[p].x : (k == 1 ? v[p].y : (k == 2 ? v[p].z : v[p].w));
        const bool hit = vv == mm[k];
        o[p][k] = (hit && !taken) ? dd[k] : 0.f;
        taken = taken || hit;
      }
    }
#pragma unroll
    for (int p = 0; p < 6; ++p) g[p] = make_float4(o[p][0], o[p][1], o[p][2], o[p][3]);
  };
  auto add4 = [](float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); };
  auto emit = [&](int64_t pos, float4 g, float4 tv) {  // store one gradient pixel-quad; tv = sign(gamma) * v at that position
    gp[pos] = g;
    if (bn_sums) {
      const float gg[4] = {g.x, g.y, g.z, g.w}, vv[4] = {tv.x * sgn.x, tv.y * sgn.y, tv.z * sgn.z, tv.w * sgn.w};
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        bs[k] += gg[k];
        bqs[k] = fmaf(gg[k], (vv[k] - bmu[k]) * binv[k], bqs[k]);
      }
    }
  };
  const int i0 = chunk * PB_ROWS, i1 = in_range ? ((i0 + PB_ROWS < Ho) ? i0 + PB_ROWS : Ho) : i0;
  const int istart = i0 > 0 ? i0 - 1 : 0;  // halo window: only its contribution to the shared row is kept
  float4 t0 = ld(2 * istart - pad_top, x0, cx0), t1 = ld(2 * istart - pad_top, x1, cx1);  // first row of the current window
  float4 c0 = zero4, c1 = zero4;                                                            // gradient carried into that row
  // the five loads of a window (two rows x two columns of v, one gradient) are unconditional (clamped coordinates, masked after
  // arrival) and requested one window ahead
  const int xc0 = x0 < 0 ? 0 : (x0 >= W ? W - 1 : x0), xc1 = x1 >= W ? W - 1 : x1;
  float4 raw[4], dn;
  auto request = [&](int i) {
    const int r0 = 2 * i - pad_top;
#pragma unroll
    for (int a = 0; a < 2; ++a) {
      int y = r0 + 1 + a;
      y = y < 0 ? 0 : (y >= H ? H - 1 : y);
      raw[2 * a] = yp[(int64_t)(y + R) * WP + xc0];
      raw[2 * a + 1] = yp[(int64_t)(y + R) * WP + xc1];
    }
    dn = dp[(int64_t)((i < Ho ? i : Ho - 1) + R) * WPo + j];
  };
  auto masked = [&](float4 t, int y, bool cx) {
    return (cx && y >= 0 && y < H) ? make_float4(t.x * sgn.x, t.y * sgn.y, t.z * sgn.z, t.w * sgn.w) : ninf;
  };
  if (istart < i1) request(istart);
  for (int i = istart; i < i1; ++i) {
    const int r0 = 2 * i - pad_top;
    const float4 m0 = masked(raw[0], r0 + 1, cx0), m1 = masked(raw[1], r0 + 1, cx1);
    const float4 b0 = masked(raw[2], r0 + 2, cx0), b1 = masked(raw[3], r0 + 2, cx1);
    const float4 d = dn;
    if (i + 1 < i1) request(i + 1);
    const float4 m = mx4(mx4(mx4(t0, t1), mx4(m0, m1)), mx4(b0, b1));
    // the gradient of a window goes to its FIRST maximal position in scan order (rows, then columns) -- what TensorFlow's MaxPoolGrad (argmax)
    // and torch's max_pool2d backward do; with ties (frequent once activations are stored in f16) "every maximal position" would count the
    // window's gradient more than once
    float4 g6[6];
    route_first(t0, t1, m0, m1, b0, b1, m, d, g6);
    if (i >= i0) {
      ds[0] += d.x; ds[1] += d.y; ds[2] += d.z; ds[3] += d.w;
      if (r0 >= 0) {
        if (cx0) emit((int64_t)(r0 + R) * WP + x0, add4(c0, g6[0]), t0);
        if (cx1) emit((int64_t)(r0 + R) * WP + x1, add4(c1, g6[1]), t1);
      }
      if (r0 + 1 < H) {  // r0 + 1 >= 0 always
        if (cx0) emit((int64_t)(r0 + 1 + R) * WP + x0, g6[2], m0);
        if (cx1) emit((int64_t)(r0 + 1 + R) * WP + x1, g6[3], m1);
      }
    }
    c0 = g6[4];
    c1 = g6[5];
    t0 = b0;
    t1 = b1;
  }
  const int rl = 2 * i1 - pad_top;  // first row of window i1: written here only when there is no window i1 (else the next chunk owns it)
  if (in_range && i1 == Ho && rl < H) {
    if (cx0) emit((int64_t)(rl + R) * WP + x0, c0, t0);
    if (cx1) emit((int64_t)(rl + R) * WP + x1, c1, t1);
  }
  if (bn_sums) {  // workgroup reduction (float64): DPP sums inside each wave, the four waves through 384 bytes of LDS, 8 (+ 4) atomics per workgroup
    __shared__ double red[4][12];
#pragma unroll
    for (int k = 0; k < 12; ++k) {
      const double v = wave_sum_lane63((double)(k < 4 ? bs[k & 3] : (k < 8 ? bqs[k & 3] : ds[k & 3])));
      if ((threadIdx.x & 63) == 63) red[threadIdx.x >> 6][k] = v;
    }
    __syncthreads();
    if (threadIdx.x < 12) {
      const int k = threadIdx.x & 3, c = (int)(bq % CQ) * 4 + k;
      const double tot = (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
      if (c < C) {
        if (threadIdx.x < 8) atomicAdd(&bn_sums[(threadIdx.x >> 2) * 4 * CQ + c], tot);
        else if (dout_sums) atomicAdd(&dout_sums[c], tot);
      }
    }
  }
}

// ---------------------------------------------------------------- D[ca][cb] += sum_pixels A[ca][p] * Bq[cb][p]
// (pointwise / residual weight gradients).  256 pixels per pass go through LDS as [channel][pixel] (pitch 258: the
// 16 channel rows x 2 pixels of a half-wave hit 32 distinct banks), then MFMA with k = pixel.  The next pass's global
// loads are issued into registers before the MFMA phase.  Every block writes its partial product to a workspace and a
// second kernel adds the partials into D: same-line float atomics serialise at ~12 ns each, which with 512 blocks cost
// more than the whole reduction.
// a_mode 1: A is sampled at pixel (2i, 2j) of planes (Ha, Wa) for each pixel (i, j) of the Bq planes (stride-2 1x1 conv).
constexpr int OR_MAXQ = 16;  // up to 64 channels per operand

// PP pixels per pass (the LDS image is [channel][PP + 2]).  256: a thread stages one pixel of BOTH operands; 128: the first 128 threads
// stage A, the other 128 stage B -- half the LDS per workgroup, which is what decides the occupancy of this kernel
// ((MT + NT) * 16.5 KiB at 256 pixels: one workgroup per compute unit from 40 channels per operand on).
template <int PP>
__global__ __launch_bounds__(256) void outer_reduce_kernel(const float* __restrict__ A, int Ca, const float* __restrict__ Bq, int Cb, int H, int W, int WP, int R,
                                                            int B, int a_mode, int Ha, int WPa, float* __restrict__ part /*[gridDim.x][Ca*Cb]*/, uint32_t magic_WP) {
  constexpr int OR_P = PP + 2, PARTS = 256 / PP;
  static_assert(PP == 256 || PP == 128, "pixels per pass");
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int CQa = (Ca + 3) >> 2, CQb = (Cb + 3) >> 2;
  const int MT = (Ca + 15) >> 4, NT = (Cb + 15) >> 4, ntile = MT * NT;
  float* As = smem;                    // [MT*16][OR_P]  (rows past CQa*4 stay zero)
  float* Bs = smem + MT * 16 * OR_P;   // [NT*16][OR_P]
  for (int i = threadIdx.x; i < (MT + NT) * 16 * OR_P; i += 256) smem[i] = 0.0f;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lk = lane >> 4, lj = lane & 15;
  const int pix = tid & (PP - 1);
  const bool do_a = PARTS == 1 || tid < PP, do_b = PARTS == 1 || tid >= PP;  // wave-uniform
  const int plane = (H + 2 * R) * WP;
  const int64_t plane_a = a_mode ? (int64_t)(Ha + 2 * R) * WPa : plane;
  f32x4 acc[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) acc[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
  const int chunks_per_plane = (plane + PP - 1) / PP;
  const int64_t nchunks = (int64_t)B * chunks_per_plane;
  float4 rq[OR_MAXQ];  // this thread's pixel of its operand(s): PARTS == 1 keeps A here and B in rb
  float4 rb[PARTS == 1 ? OR_MAXQ : 1];
  auto fetch = [&](int64_t ch) {
    const int64_t b = ch / chunks_per_plane;
    const int p = (int)(ch - b * chunks_per_plane) * PP + pix;  // this thread's pixel
    const bool pin = ch < nchunks && p < plane;
    int pa = p;
    bool ain = pin;
    if (a_mode) {
      const int row = (int)__umulhi((uint32_t)(pin ? p : 0), magic_WP);
      const int x = p - row * WP, i = row - R;
      ain = pin && i >= 0 && i < H && x < W;
      pa = ain ? (2 * i + R) * WPa + 2 * x : 0;
    }
#pragma unroll
    for (int q = 0; q < OR_MAXQ; ++q) {
      if (PARTS == 1) {
        rq[q] = (q < CQa && ain) ? reinterpret_cast<const float4*>(A)[((int64_t)b * CQa + q) * plane_a + pa] : make_float4(0.f, 0.f, 0.f, 0.f);
        rb[q] = (q < CQb && pin) ? reinterpret_cast<const float4*>(Bq)[((int64_t)b * CQb + q) * plane + p] : make_float4(0.f, 0.f, 0.f, 0.f);
      } else if (do_a) {
        rq[q] = (q < CQa && ain) ? reinterpret_cast<const float4*>(A)[((int64_t)b * CQa + q) * plane_a + pa] : make_float4(0.f, 0.f, 0.f, 0.f);
      } else {
        rq[q] = (q < CQb && pin) ? reinterpret_cast<const float4*>(Bq)[((int64_t)b * CQb + q) * plane + p] : make_float4(0.f, 0.f, 0.f, 0.f);
      }
    }
  };
  fetch(blockIdx.x);
  for (int64_t ch = blockIdx.x; ch < nchunks; ch += gridDim.x) {
    __syncthreads();  // previous pass's MFMA reads are done (also orders the initial zero fill)
#pragma unroll
    for (int q = 0; q < OR_MAXQ; ++q) {
      if (PARTS == 1) {
        if (q < CQa) {
          As[(4 * q + 0) * OR_P + pix] = rq[q].x; As[(4 * q + 1) * OR_P + pix] = rq[q].y; As[(4 * q + 2) * OR_P + pix] = rq[q].z; As[(4 * q + 3) * OR_P + pix] = rq[q].w;
        }
        if (q < CQb) {
          Bs[(4 * q + 0) * OR_P + pix] = rb[q].x; Bs[(4 * q + 1) * OR_P + pix] = rb[q].y; Bs[(4 * q + 2) * OR_P + pix] = rb[q].z; Bs[(4 * q + 3) * OR_P + pix] = rb[q].w;
        }
      } else {
        float* dst = do_a ? As : Bs;
        if (q < (do_a ? CQa : CQb)) {
          dst[(4 * q + 0) * OR_P + pix] = rq[q].x; dst[(4 * q + 1) * OR_P + pix] = rq[q].y; dst[(4 * q + 2) * OR_P + pix] = rq[q].z; dst[(4 * q + 3) * OR_P + pix] = rq[q].w;
        }
      }
    }
    __syncthreads();
    fetch(ch + gridDim.x);  // in flight during the MFMA phase
#pragma unroll
    for (int ti = 0; ti < 4; ++ti) {
      const int tile = wave + 4 * ti;
      if (tile < ntile) {  // wave-uniform
        const int mt = tile / NT, nt = tile - mt * NT;
        const float* ar = As + (mt * 16 + lj) * OR_P + lk;
        const float* br = Bs + (nt * 16 + lj) * OR_P + lk;
        f32x4 c0 = acc[ti], c1 = (f32x4){0.f, 0.f, 0.f, 0.f};
        for (int s = 0; s < PP / 4; s += 2) {  // A[i = ca][k = pixel], B[k = pixel][j = cb]; two interleaved accumulator chains
          c0 = mfma16(ar[4 * s], br[4 * s], c0);
          c1 = mfma16(ar[4 * s + 4], br[4 * s + 4], c1);
        }
        acc[ti] = c0 + c1;
      }
    }
  }
  float* mine = part + (int64_t)blockIdx.x * Ca * Cb;
#pragma unroll
  for (int ti = 0; ti < 4; ++ti) {
    const int tile = wave + 4 * ti;
    if (tile < ntile) {
      const int mt = tile / NT, nt = tile - mt * NT;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int ca = mt * 16 + lk * 4 + r, cb = nt * 16 + lj;
        if (ca < Ca && cb < Cb) mine[ca * Cb + cb] = acc[ti][r];
      }
    }
  }
}

// D[i] += sum over the partial products: lanes run along i (coalesced), blockIdx.y takes one eighth of the partials and adds its
// share with one atomic (8 adds per address).
__global__ __launch_bounds__(256) void add_partials_kernel(const float* __restrict__ part, int nparts, int n, float* __restrict__ D) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int per = (nparts + gridDim.y - 1) / gridDim.y;
  const int k0 = blockIdx.y * per, k1 = (k0 + per < nparts) ? k0 + per : nparts;
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
  int k = k0;
  for (; k + 3 < k1; k += 4) {
    s0 += part[(int64_t)k * n + i]; s1 += part[(int64_t)(k + 1) * n + i]; s2 += part[(int64_t)(k + 2) * n + i]; s3 += part[(int64_t)(k + 3) * n + i];
  }
  for (; k < k1; ++k) s0 += part[(int64_t)k * n + i];
  if (k1 > k0) atomicAdd(&D[i], (s0 + s1) + (s2 + s3));
}

// ---------------------------------------------------------------- depthwise weight gradient
// dW[c][tap] += sum_p r[c][p + off(tap)] * du[c][p]   with r = relu_in ? relu(x) : x.  One wave = 64-pixel windows of one
// (snippet, quad); lanes R..63-R contribute; 4 x k x k accumulators per lane, wave-reduced once at the end.
template <int KS, int SH>
__device__ __forceinline__ float lsh(float v) {  // value of lane (l + SH): one DPP wave shift per lane of distance
  if constexpr (SH == 0) return v;
  else if constexpr (SH < 0)
    return lsh<KS, SH + 1>(__uint_as_float(__builtin_amdgcn_update_dpp(0u, __float_as_uint(v), 0x138 /*wave_shr:1*/, 0xf, 0xf, true)));
  else
    return lsh<KS, SH - 1>(__uint_as_float(__builtin_amdgcn_update_dpp(0u, __float_as_uint(v), 0x130 /*wave_shl:1*/, 0xf, 0xf, true)));
}

// BNIN: x holds the pre-normalisation tensor v of the BatchNorm + ReLU in front of the conv; r = max(fma(v, gamma * inv, beta - mean * gamma * inv), 0)
// inside the image, 0 in the pads (the arithmetic of bn_planes_apply_kernel: the tensor that pass would have materialised, bit for bit).
struct InBnW {
  const float *mean = nullptr, *var = nullptr, *gamma = nullptr, *beta = nullptr;
  float eps = 0.0f;
  uint32_t magic_WP = 0;
};

template <int KS, bool BNIN = false>
__global__ __launch_bounds__(256) void dw_wgrad_kernel(const float* __restrict__ x, const float* __restrict__ du, int C, int H, int W, int WP, int RP, int relu_in,
                                                        float* __restrict__ dW /*[KS*KS][C], Keras (k,k,C,1)*/, int tasks, int tasks_per_wave, InBnW ib = InBnW{}) {
  constexpr int R = KS / 2, VAL = 64 - 2 * R, KK = KS * KS;
  const int lane = threadIdx.x & 63;
  const int wv = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int cq = blockIdx.y, b = blockIdx.z;
  const int CQ = (C + 3) >> 2;
  const int plane = (H + 2 * RP) * WP;
  const float4* xp = reinterpret_cast<const float4*>(x) + ((int64_t)b * CQ + cq) * plane;
  const float4* dp = reinterpret_cast<const float4*>(du) + ((int64_t)b * CQ + cq) * plane;
  float acc[4][KK];
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int t = 0; t < KK; ++t) acc[j][t] = 0.0f;
  const bool contributes = lane >= R && lane < 64 - R;
  float bsc[4] = {0.f, 0.f, 0.f, 0.f}, bsh[4] = {0.f, 0.f, 0.f, 0.f};
  if (BNIN) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int c = cq * 4 + j;
      if (c < C) {
        bsc[j] = ib.gamma[c] * rsqrtf(ib.var[c] + ib.eps);
        bsh[j] = ib.beta[c] - ib.mean[c] * bsc[j];
      }
    }
  }
  // the next window's KS + 1 loads are requested before the current window's products (unconditional, clamped; the gradient of a
  // non-contributing lane is zeroed afterwards): two windows in flight per wave
  const int task0 = wv * tasks_per_wave, task_end = min((wv + 1) * tasks_per_wave, tasks);
  float4 gn = make_float4(0.f, 0.f, 0.f, 0.f), an[KS];
  auto request = [&](int task) {
    const int q = RP * WP + task * VAL - R + lane;
    gn = dp[q < plane ? q : plane - 1];
#pragma unroll
    for (int dy = 0; dy < KS; ++dy) {
      int i = q + (dy - R) * WP;
      i = i < 0 ? 0 : (i >= plane ? plane - 1 : i);
      an[dy] = xp[i];
    }
  };
  constexpr bool AHEAD = KS == 3;  // k = 5, 7 hold 100 / 196 accumulators: no room for a second set of rows
  if (AHEAD && task0 < task_end) request(task0);
  for (int task = task0; task < task_end; ++task) {
    const int q = RP * WP + task * VAL - R + lane;
    const bool live = contributes && q < plane;
    if (!AHEAD) request(task);
    const float g[4] = {live ? gn.x : 0.f, live ? gn.y : 0.f, live ? gn.z : 0.f, live ? gn.w : 0.f};
    float4 ac[KS];
#pragma unroll
    for (int dy = 0; dy < KS; ++dy) ac[dy] = an[dy];
    if (AHEAD && task + 1 < task_end) request(task + 1);
    int brow = 0;
    bool bcol = false;
    if (BNIN) {  // this lane's pixel of the flat padded plane (the rows above / below share its column)
      const int qq = q < 0 ? 0 : q;
      brow = (int)__umulhi((uint32_t)qq, ib.magic_WP);
      bcol = q >= 0 && (qq - brow * WP) < W;
    }
#pragma unroll
    for (int dy = 0; dy < KS; ++dy) {
      const float4 a4 = ac[dy];
      float a[4] = {a4.x, a4.y, a4.z, a4.w};
      const bool inside = BNIN && bcol && (brow + dy - R) >= RP && (brow + dy - R) < RP + H;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (BNIN) a[j] = inside ? fmaxf(fmaf(a[j], bsc[j], bsh[j]), 0.0f) : 0.0f;
        if (relu_in) a[j] = fmaxf(a[j], 0.0f);
        if constexpr (KS == 3) {
          acc[j][dy * 3 + 0] = fmaf(lsh<KS, -1>(a[j]), g[j], acc[j][dy * 3 + 0]);
          acc[j][dy * 3 + 1] = fmaf(a[j], g[j], acc[j][dy * 3 + 1]);
          acc[j][dy * 3 + 2] = fmaf(lsh<KS, 1>(a[j]), g[j], acc[j][dy * 3 + 2]);
        } else if constexpr (KS == 5) {
          acc[j][dy * 5 + 0] = fmaf(lsh<KS, -2>(a[j]), g[j], acc[j][dy * 5 + 0]);
          acc[j][dy * 5 + 1] = fmaf(lsh<KS, -1>(a[j]), g[j], acc[j][dy * 5 + 1]);
          acc[j][dy * 5 + 2] = fmaf(a[j], g[j], acc[j][dy * 5 + 2]);
          acc[j][dy * 5 + 3] = fmaf(lsh<KS, 1>(a[j]), g[j], acc[j][dy * 5 + 3]);
          acc[j][dy * 5 + 4] = fmaf(lsh<KS, 2>(a[j]), g[j], acc[j][dy * 5 + 4]);
        } else {
          acc[j][dy * 7 + 0] = fmaf(lsh<KS, -3>(a[j]), g[j], acc[j][dy * 7 + 0]);
          acc[j][dy * 7 + 1] = fmaf(lsh<KS, -2>(a[j]), g[j], acc[j][dy * 7 + 1]);
          acc[j][dy * 7 + 2] = fmaf(lsh<KS, -1>(a[j]), g[j], acc[j][dy * 7 + 2]);
          acc[j][dy * 7 + 3] = fmaf(a[j], g[j], acc[j][dy * 7 + 3]);
          acc[j][dy * 7 + 4] = fmaf(lsh<KS, 1>(a[j]), g[j], acc[j][dy * 7 + 4]);
          acc[j][dy * 7 + 5] = fmaf(lsh<KS, 2>(a[j]), g[j], acc[j][dy * 7 + 5]);
          acc[j][dy * 7 + 6] = fmaf(lsh<KS, 3>(a[j]), g[j], acc[j][dy * 7 + 6]);
        }
      }
    }
  }
  // one wave reduction per accumulator, one LDS reduction per block, then 4*k*k atomics per block (same-line device atomics
  // serialise at ~12 ns each, so they are kept to a few thousand per line)
  __shared__ float red[4][4 * KK];
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int t = 0; t < KK; ++t) {
      const float v = wave_sum_lane63(acc[j][t]);
      if (lane == 63) red[threadIdx.x >> 6][j * KK + t] = v;
    }
  __syncthreads();
  if (threadIdx.x < 4 * KK) {
    const int j = threadIdx.x / KK;
    const int t = threadIdx.x - j * KK;  // Keras depthwise kernel layout (k, k, C, 1): element (tap, channel) at tap*C + channel
    if (cq * 4 + j < C) atomicAdd(&dW[t * C + cq * 4 + j], red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x]);
  }
}

// ---------------------------------------------------------------- depthwise weight gradient, k = 3, marching down a column strip
// dw_wgrad_kernel requests every x row three times through L1 (as the row above, the row of, and the row below three different windows) and
// runs at 3.2-3.7 TB/s on block-1 planes.  Here a wave owns a strip of 64 columns (62 of them outputs) of ONE channel quad and walks down a
// segment of image rows: the x rows r - 1 and r stay in registers from the previous steps (with their two horizontally shifted copies), row
// r + 1 and the gradient row r are the only loads of a step -- every byte is requested once -- and they are in flight two steps ahead.  The
// loop is unrolled by three so that the roles (above, same, below) rotate through register sets without moves.  BNIN: BatchNorm + ReLU of
// the pre-normalisation tensor applied once per arriving row (dw_wgrad_kernel does it three times per value).
template <bool BNIN>
__global__ __launch_bounds__(256) void dw_wgrad_march_kernel(const float* __restrict__ x, const float* __restrict__ du, int C, int H, int W, int WP, int relu_in,
                                                              float* __restrict__ dW /*[9][C]*/, int nstrip, int nseg, int rows_per_seg, InBnW ib) {
  constexpr int KK = 9;
  const int lane = threadIdx.x & 63;
  const int task = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int cq = blockIdx.y, b = blockIdx.z;
  const int CQ = (C + 3) >> 2;
  const int plane = (H + 2) * WP;
  const float4* xp = reinterpret_cast<const float4*>(x) + ((int64_t)b * CQ + cq) * plane;
  const float4* dp = reinterpret_cast<const float4*>(du) + ((int64_t)b * CQ + cq) * plane;
  float acc[4][KK];
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int t = 0; t < KK; ++t) acc[j][t] = 0.0f;
  const bool has_task = task < nstrip * nseg;  // wave-uniform
  const int strip = has_task ? task % nstrip : 0, seg = has_task ? task / nstrip : 0;
  const int xcol = strip * 62 - 1 + lane;                   // image column of this lane (lane 0 and 63: halo only)
  const bool out_lane = has_task && lane >= 1 && lane <= 62 && xcol < W;
  const bool col_in = xcol >= 0 && xcol < W;
  const int r_begin = seg * rows_per_seg, r_end = has_task ? min(r_begin + rows_per_seg, H) : r_begin;
  float bsc[4] = {0.f, 0.f, 0.f, 0.f}, bsh[4] = {0.f, 0.f, 0.f, 0.f};
  if (BNIN) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int c = cq * 4 + j;
      if (c < C) {
        bsc[j] = ib.gamma[c] * rsqrtf(ib.var[c] + ib.eps);
        bsh[j] = ib.beta[c] - ib.mean[c] * bsc[j];
      }
    }
  }
  struct Row { float c[4], l[4], r[4]; };  // the row's values at this lane's column, at the column to its left, to its right
  auto xload = [&](int row) -> float4 {    // image row `row` (-1 .. H): padded-plane row row + 1; clamped, masked on arrival
    int i = (row + 1) * WP + xcol;
    i = i < 0 ? 0 : (i >= plane ? plane - 1 : i);
    return xp[i];
  };
  auto dload = [&](int row) -> float4 {
    int i = (row + 1) * WP + xcol;
    i = i < 0 ? 0 : (i >= plane ? plane - 1 : i);
    return dp[i];
  };
  auto arrive = [&](const float4& raw, int row, Row& o) {
    const float v[4] = {raw.x, raw.y, raw.z, raw.w};
    const bool inside = col_in && row >= 0 && row < H;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float a = v[j];
      if (BNIN) a = inside ? fmaxf(fmaf(a, bsc[j], bsh[j]), 0.0f) : 0.0f;
      else if (relu_in) a = fmaxf(a, 0.0f);  // the planes' pads hold zeros already
      o.c[j] = a;
      o.l[j] = lsh<3, -1>(a);
      o.r[j] = lsh<3, 1>(a);
    }
  };
  auto step = [&](const Row& up, const Row& mid, const Row& dn, const float4& g4, int row) {
    const bool live = out_lane && row < r_end;
    const float g[4] = {live ? g4.x : 0.f, live ? g4.y : 0.f, live ? g4.z : 0.f, live ? g4.w : 0.f};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      acc[j][0] = fmaf(up.l[j], g[j], acc[j][0]); acc[j][1] = fmaf(up.c[j], g[j], acc[j][1]); acc[j][2] = fmaf(up.r[j], g[j], acc[j][2]);
      acc[j][3] = fmaf(mid.l[j], g[j], acc[j][3]); acc[j][4] = fmaf(mid.c[j], g[j], acc[j][4]); acc[j][5] = fmaf(mid.r[j], g[j], acc[j][5]);
      acc[j][6] = fmaf(dn.l[j], g[j], acc[j][6]); acc[j][7] = fmaf(dn.c[j], g[j], acc[j][7]); acc[j][8] = fmaf(dn.r[j], g[j], acc[j][8]);
    }
  };
  if (r_begin < r_end) {
    Row A, Bq, Cq;
    arrive(xload(r_begin - 1), r_begin - 1, A);
    arrive(xload(r_begin), r_begin, Bq);
    // in flight: (x row r + 1, gradient row r) of the next THREE steps, one slot per step of the unrolled loop, each refilled right after it is
    // consumed -- three steps of distance, and no register set with a load in flight is ever moved
    float4 px0 = xload(r_begin + 1), pg0 = dload(r_begin), px1 = xload(r_begin + 2), pg1 = dload(r_begin + 1), px2 = xload(r_begin + 3), pg2 = dload(r_begin + 2);
    for (int r = r_begin; r < r_end; r += 3) {  // rows past r_end contribute nothing (live is false); loads stay in the plane (clamped)
      { const float4 xr = px0, gr = pg0; px0 = xload(r + 4); pg0 = dload(r + 3); arrive(xr, r + 1, Cq); step(A, Bq, Cq, gr, r); }       // up A, mid Bq, down Cq
      { const float4 xr = px1, gr = pg1; px1 = xload(r + 5); pg1 = dload(r + 4); arrive(xr, r + 2, A); step(Bq, Cq, A, gr, r + 1); }    // up Bq, mid Cq, down A
      { const float4 xr = px2, gr = pg2; px2 = xload(r + 6); pg2 = dload(r + 5); arrive(xr, r + 3, Bq); step(Cq, A, Bq, gr, r + 2); }   // up Cq, mid A, down Bq
    }
  }
  __shared__ float red[4][4 * KK];
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int t = 0; t < KK; ++t) {
      const float v = wave_sum_lane63(acc[j][t]);
      if (lane == 63) red[threadIdx.x >> 6][j * KK + t] = v;
    }
  __syncthreads();
  if (threadIdx.x < 4 * KK) {
    const int j = threadIdx.x / KK;
    const int t = threadIdx.x - j * KK;  // Keras depthwise kernel layout (k, k, C, 1): element (tap, channel) at tap*C + channel
    if (cq * 4 + j < C) atomicAdd(&dW[t * C + cq * 4 + j], red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x]);
  }
}

// ---------------------------------------------------------------- depthwise backward in ONE marching pass (k = 3)
// The two passes of a separable conv's backward that read the depthwise-output gradient du -- the input gradient dr = du (*) flipped taps
// (orcai_sepconv_planes_epi: du and the reference tensor in, dr out) and the depthwise weight gradient (orcai_dw_wgrad[_bn]: x and du in) --
// use the SAME operands at every pixel: with q = p + tap offset,
//   dr[p]    = sum_tap wrev[tap] * du[p + off(tap)]            dWrev[tap] = sum_p x[p] * du[p + off(tap)]        (dW[tap] = dWrev[8 - tap])
// and the epilogue extras of the input-gradient pass (EPI 2: backward sums of the BatchNorm whose pre-normalisation tensor is x; EPI 3: ReLU mask
// x > 0) read x at p as well.  So one wave marches down a column strip of one channel quad with the three du rows (and their two shifted
// copies) in registers; a step loads ONE du row and ONE x row (in flight three steps ahead, as in dw_wgrad_march_kernel), and writes one dr row:
// du, x read once, dr written once -- 3 plane passes where the two launches moved 2 + 3 (EPI 2) or 2 + 2.
// SW lanes per strip (64, 32 or 16: SW - 2 output columns): a wave carries 64 / SW strips of the same (snippet, quad), so planes narrower than
// 62 columns do not idle most lanes (W = 86: three 30-column strips = 96 lanes).  Strips beside each other in a wave exchange garbage through the
// DPP shifts only into their halo lanes, which produce nothing.
// C0 (block 1's first separable conv): its input y0 = relu(bn0(conv0(snippet))) is not read but REBUILT per pixel from the nine taps of the
// 1-channel snippet -- conv0_kernel's fma chain in its order, fma(acc, 1, bias), then the BNIN stage -- so `x` is the entry conv's
// pre-normalisation value v0 formed in registers: the pass reads du and 4 bytes per pixel of input instead of du and y0, and the EPI 2 sums it
// leaves are bn0's backward sums (orcai_conv0_bn_bwd_x's first pass over dr1 and the input disappears).  The three input rows rotate with the du
// rows; a strip's halo lanes hold the neighbouring input columns.
struct Conv0In {
  const float* in = nullptr;       // [B] snippets of H x W at snippet_stride
  int64_t snippet_stride = 0;
  const float* w0 = nullptr;       // [9][16]
  const float* bias = nullptr;     // [16]
  const float* resq = nullptr;     // optional [B][4][Ho + 2][WPo][4]: the residual branch's gradient w.r.t. y0 at the even pixels (2i, 2j), as planes of the
  int Ho = 0, WPo = 0;             // pooled resolution; added to dr (and so part of bn0's sums) instead of a scatter-add pass over dr afterwards
};

template <int SW, int EPI, bool BNIN, bool C0 = false>
__global__ __launch_bounds__(256) void dw_bwd_march_kernel(const float* __restrict__ x, const float* __restrict__ du, int C, int H, int W, int WP, int relu_in,
                                                            const float* __restrict__ wrev /*[CQ][9][4] reversed taps*/, float* __restrict__ dr,
                                                            float* __restrict__ dW /*[9][C]*/, double* __restrict__ shards /*EPI 2: [32][CQ][8]*/, int nstrip,
                                                            int nseg, int rps, InBnW ib, int epi_relu, Conv0In c0 = Conv0In{}) {
  static_assert(SW == 64 || SW == 32 || SW == 16, "strip lanes");
  static_assert(EPI == 0 || EPI == 2 || EPI == 3, "epilogue extras");
  static_assert(EPI != 2 || BNIN, "EPI 2: x is the pre-normalisation tensor of the BatchNorm whose backward sums are taken");
  static_assert(!C0 || (BNIN && EPI == 2), "C0: the entry conv's pre-normalisation tensor rebuilt on the fly, bn0's sums in the epilogue");
  constexpr int KK = 9, NSUB = 64 / SW;
  const int lane = threadIdx.x & 63, sl = lane % SW, sub = lane / SW;
  const int cq = blockIdx.y, b = blockIdx.z;
  const int CQ = (C + 3) >> 2;
  const int plane = (H + 2) * WP;
  const int64_t pbase = ((int64_t)b * CQ + cq) * plane;
  const float4* xp = reinterpret_cast<const float4*>(C0 ? du : x) + pbase;  // C0: x is not read
  const float4* dp = reinterpret_cast<const float4*>(du) + pbase;
  float4* op = reinterpret_cast<float4*>(dr) + pbase;
  const int task = (blockIdx.x * 4 + (threadIdx.x >> 6)) * NSUB + sub;
  const bool has_task = task < nstrip * nseg;
  const int strip = has_task ? task % nstrip : 0, seg = has_task ? task / nstrip : 0;
  const int xcol = strip * (SW - 2) - 1 + sl;  // image column of this lane (first and last lane of a strip: halo only)
  const bool out_lane = has_task && sl >= 1 && sl <= SW - 2 && xcol < W;
  const int r_begin = seg * rps, r_end = min(r_begin + rps, H);  // per strip; every strip of the wave walks rps rows
  float acc[4][KK];
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int t = 0; t < KK; ++t) acc[j][t] = 0.0f;
  float s1[4] = {0.f, 0.f, 0.f, 0.f}, s2[4] = {0.f, 0.f, 0.f, 0.f};  // EPI 2: sum g, sum g * xhat over this lane's pixels
  float wt[4][KK];  // wave-uniform: scalar loads
#pragma unroll
  for (int t = 0; t < KK; ++t)
#pragma unroll
    for (int j = 0; j < 4; ++j) wt[j][t] = wrev[(cq * KK + t) * 4 + j];
  float bsc[4] = {0.f, 0.f, 0.f, 0.f}, bsh[4] = {0.f, 0.f, 0.f, 0.f}, bmu[4] = {0.f, 0.f, 0.f, 0.f}, binv[4] = {0.f, 0.f, 0.f, 0.f}, bgm[4] = {0.f, 0.f, 0.f, 0.f},
        bbt[4] = {0.f, 0.f, 0.f, 0.f};
  if (BNIN) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int c = cq * 4 + j;
      if (c < C) {  // wave-uniform values computed on the vector unit: back to scalar registers (24 VGPRs otherwise)
        auto uni = [](float v) { return __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(v))); };
        binv[j] = uni(rsqrtf(ib.var[c] + ib.eps));
        bmu[j] = ib.mean[c]; bgm[j] = ib.gamma[c]; bbt[j] = ib.beta[c];
        bsc[j] = uni(bgm[j] * binv[j]);  // bn_planes_apply_kernel's folded form: the tensor the forward conv saw, bit for bit
        bsh[j] = uni(bbt[j] - bmu[j] * bsc[j]);
      }
    }
  }
  // C0: the entry conv's taps and bias of this quad.  Wave-uniform, but deliberately in VECTOR registers: with the 36 depthwise taps and the
  // BatchNorm constants already scalar, 40 more scalars spilled 134 SGPRs into v_readlane traffic inside the row loop (the kernel has the VGPRs to
  // spare at its two waves per SIMD).  The opaque zero keeps the compiler from proving the addresses uniform.
  float w0q[KK][4], b0q[4] = {0.f, 0.f, 0.f, 0.f};
  if (C0) {
    int vz;
    asm volatile("v_mov_b32 %0, 0" : "=v"(vz));
#pragma unroll
    for (int t = 0; t < KK; ++t)
#pragma unroll
      for (int j = 0; j < 4; ++j) w0q[t][j] = c0.w0[t * 16 + cq * 4 + j + vz];
#pragma unroll
    for (int j = 0; j < 4; ++j) b0q[j] = c0.bias[cq * 4 + j + vz];
  }
  const float* inb = C0 ? c0.in + (int64_t)b * c0.snippet_stride : nullptr;
  struct InRow { float c, l, r; };
  auto iload = [&](int row) -> float {  // snippet pixel (row, xcol), zero outside the image ("same" padding); unconditional, clamped
    const int rr = row < 0 ? 0 : (row >= H ? H - 1 : row), cc = xcol < 0 ? 0 : (xcol >= W ? W - 1 : xcol);
    const float v = inb[(int64_t)rr * W + cc];
    // multiplied, not selected: a select lets the compiler predicate the LOAD (a branch in the steady state, and with it vmcnt(0) at every step)
    return v * ((row >= 0 && row < H && xcol >= 0 && xcol < W) ? 1.0f : 0.0f);
  };
  auto iarrive = [&](float v, InRow& o) {
    o.c = v;
    o.l = lsh<3, -1>(v);
    o.r = lsh<3, 1>(v);
  };
  auto conv0_at = [&](const InRow& up, const InRow& mid, const InRow& dn) -> float4 {
    const float a[KK] = {up.l, up.c, up.r, mid.l, mid.c, mid.r, dn.l, dn.c, dn.r};
    float v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float cv = 0.0f;
#pragma unroll
      for (int t = 0; t < KK; ++t) cv = fmaf(a[t], w0q[t][j], cv);  // conv0_kernel's chain, taps in (dy, dx) order
      v[j] = fmaf(cv, 1.0f, b0q[j]);                                   // ... and its fma(acc, scale = 1, shift = bias)
    }
    return make_float4(v[0], v[1], v[2], v[3]);
  };
  struct Row { float c[4], l[4], r[4]; };
  auto pix = [&](int row) -> int {  // image row `row` (-1 .. H): padded-plane row row + 1; clamped (rows past the segment feed dead steps only)
    const int i = (row + 1) * WP + xcol;
    return i < 0 ? 0 : (i >= plane ? plane - 1 : i);
  };
  auto arrive = [&](const float4& raw, Row& o) {
    const float v[4] = {raw.x, raw.y, raw.z, raw.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      o.c[j] = v[j];
      o.l[j] = lsh<3, -1>(v[j]);
      o.r[j] = lsh<3, 1>(v[j]);
    }
  };
  float4 radd = make_float4(0.f, 0.f, 0.f, 0.f);  // C0 with a residual gradient: its value at this lane's pixel for the current step (0 off the even pixels)
  auto step = [&](const Row& up, const Row& mid, const Row& dn, const float4& x4, int row) {
    const bool live = out_lane && row < r_end;
    const float xv[4] = {x4.x, x4.y, x4.z, x4.w};
    const float ra[4] = {radd.x, radd.y, radd.z, radd.w};
    float d[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float y = xv[j];
      if (BNIN) y = fmaxf(fmaf(y, bsc[j], bsh[j]), 0.0f);  // a live lane is inside the image
      else if (relu_in) y = fmaxf(y, 0.0f);
      y = live ? y : 0.0f;
      float a = up.l[j] * wt[j][0];
      a = fmaf(up.c[j], wt[j][1], a); a = fmaf(up.r[j], wt[j][2], a);
      a = fmaf(mid.l[j], wt[j][3], a); a = fmaf(mid.c[j], wt[j][4], a); a = fmaf(mid.r[j], wt[j][5], a);
      a = fmaf(dn.l[j], wt[j][6], a); a = fmaf(dn.c[j], wt[j][7], a); a = fmaf(dn.r[j], wt[j][8], a);
      if (C0) a += ra[j];  // the residual branch's gradient joins before the sums and the store
      acc[j][0] = fmaf(up.l[j], y, acc[j][0]); acc[j][1] = fmaf(up.c[j], y, acc[j][1]); acc[j][2] = fmaf(up.r[j], y, acc[j][2]);
      acc[j][3] = fmaf(mid.l[j], y, acc[j][3]); acc[j][4] = fmaf(mid.c[j], y, acc[j][4]); acc[j][5] = fmaf(mid.r[j], y, acc[j][5]);
      acc[j][6] = fmaf(dn.l[j], y, acc[j][6]); acc[j][7] = fmaf(dn.c[j], y, acc[j][7]); acc[j][8] = fmaf(dn.r[j], y, acc[j][8]);
      if (EPI == 2) {  // the arithmetic of bn_planes_bwd_sums_kernel / the EPI 2 epilogue of the tile kernels
        const float xh = (xv[j] - bmu[j]) * binv[j];
        const bool gate = !epi_relu || fmaf(xh, bgm[j], bbt[j]) > 0.0f;
        const float gg = (live && gate) ? a : 0.0f;
        s1[j] += gg;
        s2[j] = fmaf(gg, xh, s2[j]);
      }
      if (EPI == 3) a = xv[j] > 0.0f ? a : 0.0f;
      d[j] = a;
    }
    if (C0) {  // unconditional store: a dead lane writes zeros to its pixel of the top pad row (zeros, never anything else), so the steady state has no branch
      const int pc = xcol < 0 ? 0 : (xcol >= WP ? WP - 1 : xcol);
      op[live ? (row + 1) * WP + xcol : pc] = make_float4(live ? d[0] : 0.f, live ? d[1] : 0.f, live ? d[2] : 0.f, live ? d[3] : 0.f);
    } else if (live) {
      op[(row + 1) * WP + xcol] = make_float4(d[0], d[1], d[2], d[3]);
    }
  };
  if (C0) {
    if (__builtin_amdgcn_ballot_w64(has_task) != 0) {  // wave-uniform
      Row A, Bq, Cq;
      InRow IA, IB, IC;
      arrive(dp[pix(r_begin - 1)], A);
      arrive(dp[pix(r_begin)], Bq);
      iarrive(iload(r_begin - 1), IA);
      iarrive(iload(r_begin), IB);
      // in flight: (du row r + 1, snippet row r + 1) of the next three steps
      float4 pg0 = dp[pix(r_begin + 1)], pg1 = dp[pix(r_begin + 2)], pg2 = dp[pix(r_begin + 3)];
      float pi0 = iload(r_begin + 1), pi1 = iload(r_begin + 2), pi2 = iload(r_begin + 3);
      // residual gradient of row r (compact planes at the pooled resolution): requested three steps ahead as well; every lane loads (its pixel's
      // pair partner the same 16 bytes), only even (row, column) keep the value
      // (no branch anywhere in the steady state: without a residual gradient the loads read the du plane at the same small indices and are discarded --
      // a wave-uniform branch around them makes the wait-count pass drain every request of the step at its join)
      const bool has_res = c0.resq != nullptr;
      const float4* rqp = has_res ? reinterpret_cast<const float4*>(c0.resq) + ((int64_t)b * CQ + cq) * ((int64_t)(c0.Ho + 2) * c0.WPo) : dp;
      const bool col_even = has_res && xcol >= 0 && (xcol & 1) == 0;
      const int jq = xcol < 0 ? 0 : (xcol >> 1);
      const int jc = jq >= c0.WPo ? c0.WPo - 1 : jq;
      auto rload = [&](int row) -> float4 {
        int iq = row >> 1;
        iq = iq < 0 ? 0 : (iq >= c0.Ho ? c0.Ho - 1 : iq);
        return rqp[(iq + 1) * c0.WPo + jc];
      };
      auto rkeep = [&](const float4& v, int row) { radd = (col_even && (row & 1) == 0) ? v : make_float4(0.f, 0.f, 0.f, 0.f); };
      float4 pr0 = rload(r_begin), pr1 = rload(r_begin + 1), pr2 = rload(r_begin + 2);
      for (int i = 0; i < rps; i += 3) {
        const int r = r_begin + i;
        { const float4 gr = pg0, rr = pr0; const float ir = pi0; pg0 = dp[pix(r + 4)]; pi0 = iload(r + 4); pr0 = rload(r + 3); arrive(gr, Cq); iarrive(ir, IC); rkeep(rr, r); step(A, Bq, Cq, conv0_at(IA, IB, IC), r); }
        { const float4 gr = pg1, rr = pr1; const float ir = pi1; pg1 = dp[pix(r + 5)]; pi1 = iload(r + 5); pr1 = rload(r + 4); arrive(gr, A); iarrive(ir, IA); rkeep(rr, r + 1); step(Bq, Cq, A, conv0_at(IB, IC, IA), r + 1); }
        { const float4 gr = pg2, rr = pr2; const float ir = pi2; pg2 = dp[pix(r + 6)]; pi2 = iload(r + 6); pr2 = rload(r + 5); arrive(gr, Bq); iarrive(ir, IB); rkeep(rr, r + 2); step(Cq, A, Bq, conv0_at(IC, IA, IB), r + 2); }
      }
    }
  } else if (__builtin_amdgcn_ballot_w64(has_task) != 0) {  // wave-uniform
    Row A, Bq, Cq;
    arrive(dp[pix(r_begin - 1)], A);
    arrive(dp[pix(r_begin)], Bq);
    // in flight: (du row r + 1, x row r) of the next THREE steps, one slot per step of the unrolled loop, refilled right after it is consumed
    float4 pg0 = dp[pix(r_begin + 1)], px0 = xp[pix(r_begin)], pg1 = dp[pix(r_begin + 2)], px1 = xp[pix(r_begin + 1)], pg2 = dp[pix(r_begin + 3)], px2 = xp[pix(r_begin + 2)];
    for (int i = 0; i < rps; i += 3) {  // rps is a multiple of three; rows past r_end contribute nothing
      const int r = r_begin + i;
      { const float4 gr = pg0, xr = px0; pg0 = dp[pix(r + 4)]; px0 = xp[pix(r + 3)]; arrive(gr, Cq); step(A, Bq, Cq, xr, r); }      // up A, mid Bq, down Cq
      { const float4 gr = pg1, xr = px1; pg1 = dp[pix(r + 5)]; px1 = xp[pix(r + 4)]; arrive(gr, A); step(Bq, Cq, A, xr, r + 1); }   // up Bq, mid Cq, down A
      { const float4 gr = pg2, xr = px2; pg2 = dp[pix(r + 6)]; px2 = xp[pix(r + 5)]; arrive(gr, Bq); step(Cq, A, Bq, xr, r + 2); }  // up Cq, mid A, down Bq
    }
  }
  constexpr int NRED = 4 * KK + (EPI == 2 ? 8 : 0);
  __shared__ float red[4][NRED];
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int t = 0; t < KK; ++t) {
      const float v = wave_sum_lane63(acc[j][t]);
      if (lane == 63) red[threadIdx.x >> 6][j * KK + t] = v;
    }
  if (EPI == 2) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float v = wave_sum_lane63(j < 4 ? s1[j & 3] : s2[j & 3]);
      if (lane == 63) red[threadIdx.x >> 6][4 * KK + j] = v;
    }
  }
  __syncthreads();
  if (threadIdx.x < 4 * KK) {
    const int j = threadIdx.x / KK;
    const int t = threadIdx.x - j * KK;  // accumulator t belongs to the REVERSED tap: Keras layout (k, k, C, 1), element (tap, channel) at tap * C + channel
    if (cq * 4 + j < C) atomicAdd(&dW[(KK - 1 - t) * C + cq * 4 + j], red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x]);
  } else if (EPI == 2 && threadIdx.x < NRED) {
    const int j = threadIdx.x - 4 * KK;  // 0..3 sum g, 4..7 sum g * xhat: one f64 atomic per value and workgroup into one of 32 accumulator copies
    const float tot = red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
    atomicAdd(&shards[((int64_t)((blockIdx.x + 7 * b + 3 * cq) & 31) * CQ + cq) * 8 + j], (double)tot);
  }
}

// ---------------------------------------------------------------- the entry conv's two reduction passes, marching (k = 3)
// conv0_stats_kernel / conv0_bn_bwd_x_kernel<.., true> work on 8 x 32-pixel tiles with the input halo staged in LDS: two barriers, ~40
// instructions of tile arithmetic and an LDS round trip per 256 pixels, for a conv of 144 multiply-adds per pixel -- they run at 4 x the time their
// arithmetic needs (0.17 and 0.23 ms per step).  The marching form of dw_bwd_march_kernel<.., C0> has neither: a wave owns a 62-column strip of
// one channel quad, the three snippet rows rotate through registers (each value loaded once, 4 bytes per lane), the taps are scalars, partial sums
// live in registers over a segment of rows and are reduced once per workgroup.
//   MODE 0: batch statistics of v0 = fma(conv, scale, shift) -> shards [32][4][8] (sum | sum of squares per quad), as conv0_stats_kernel
//   MODE 1: entry conv weight gradient with bn0's backward applied on the fly (conv0_bn_bwd_x_kernel<3, true>): dW0[tap][c] += in_tap * dv0[c]
template <int MODE>
__global__ __launch_bounds__(256) void conv0_march_kernel(const float* __restrict__ in, int64_t snippet_stride, int H, int W, int WP, const float* __restrict__ w0 /*[9][16]*/,
                                                           const float* __restrict__ scale, const float* __restrict__ shift, double* __restrict__ shards,
                                                           const float* __restrict__ dy /*MODE 1: [B][4][H + 2][WP][4]*/, const float* __restrict__ mean,
                                                           const float* __restrict__ var, const float* __restrict__ gamma, const float* __restrict__ beta, float eps,
                                                           const double* __restrict__ dbeta, const double* __restrict__ dgamma, float inv_count,
                                                           float* __restrict__ dW /*MODE 1: [9][16]*/, int nstrip, int nseg, int rps) {
  constexpr int KK = 9;
  const int lane = threadIdx.x & 63;
  const int cq = blockIdx.y, b = blockIdx.z;
  const int plane = (H + 2) * WP;
  const int task = blockIdx.x * 4 + (threadIdx.x >> 6);
  const bool has_task = task < nstrip * nseg;
  const int strip = has_task ? task % nstrip : 0, seg = has_task ? task / nstrip : 0;
  const int xcol = strip * 62 - 1 + lane;
  const bool out_lane = has_task && lane >= 1 && lane <= 62 && xcol < W;
  const int r_begin = seg * rps, r_end = min(r_begin + rps, H);
  const float* inb = in + (int64_t)b * snippet_stride;
  const float4* dp = MODE == 1 ? reinterpret_cast<const float4*>(dy) + ((int64_t)b * 4 + cq) * plane : nullptr;
  float wq[KK][4], sc[4], sh[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int c = cq * 4 + j;
    sc[j] = MODE == 1 ? 1.0f : scale[c];  // MODE 1: conv0_bn_bwd_x_kernel's fma(cv, 1, bias)
    sh[j] = shift[c];
#pragma unroll
    for (int t = 0; t < KK; ++t) wq[t][j] = w0[t * 16 + c];
  }
  float mu[4] = {0.f, 0.f, 0.f, 0.f}, inv[4] = {0.f, 0.f, 0.f, 0.f}, g[4] = {0.f, 0.f, 0.f, 0.f}, bt[4] = {0.f, 0.f, 0.f, 0.f}, c1[4] = {0.f, 0.f, 0.f, 0.f},
        c2[4] = {0.f, 0.f, 0.f, 0.f};
  if (MODE == 1) {
    auto uni = [](float v) { return __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(v))); };
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int c = cq * 4 + j;
      mu[j] = mean[c]; inv[j] = uni(rsqrtf(var[c] + eps)); g[j] = gamma[c]; bt[j] = beta[c];
      c1[j] = uni((float)dbeta[c] * inv_count);
      c2[j] = uni((float)dgamma[c] * inv_count);
    }
  }
  constexpr int NACC = MODE == 1 ? 4 * KK : 8;
  float acc[NACC];
#pragma unroll
  for (int i = 0; i < NACC; ++i) acc[i] = 0.0f;
  struct InRow { float c, l, r; };
  auto iload = [&](int row) -> float {  // zero outside the image; multiplied, not selected, so that the load itself stays unconditional
    const int rr = row < 0 ? 0 : (row >= H ? H - 1 : row), cc = xcol < 0 ? 0 : (xcol >= W ? W - 1 : xcol);
    return inb[(int64_t)rr * W + cc] * ((row >= 0 && row < H && xcol >= 0 && xcol < W) ? 1.0f : 0.0f);
  };
  auto dload = [&](int row) -> float4 {
    if (MODE != 1) return make_float4(0.f, 0.f, 0.f, 0.f);
    int i = (row + 1) * WP + xcol;
    i = i < 0 ? 0 : (i >= plane ? plane - 1 : i);
    return dp[i];
  };
  auto iarrive = [&](float v, InRow& o) {
    o.c = v;
    o.l = lsh<3, -1>(v);
    o.r = lsh<3, 1>(v);
  };
  auto step = [&](const InRow& up, const InRow& mid, const InRow& dn, const float4& d4, int row) {
    const bool live = out_lane && row < r_end;
    const float a[KK] = {up.l, up.c, up.r, mid.l, mid.c, mid.r, dn.l, dn.c, dn.r};
    const float dd[4] = {d4.x, d4.y, d4.z, d4.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float cv = 0.0f;
#pragma unroll
      for (int t = 0; t < KK; ++t) cv = fmaf(a[t], wq[t][j], cv);  // conv0_kernel's chain, taps in (dy, dx) order
      const float v = fmaf(cv, sc[j], sh[j]);
      if (MODE == 0) {
        const float lv = live ? v : 0.0f;
        acc[j] += lv;
        acc[4 + j] = fmaf(lv, lv, acc[4 + j]);
      } else {
        const float xh = (v - mu[j]) * inv[j];
        const float de = (live && fmaf(xh, g[j], bt[j]) > 0.0f) ? dd[j] : 0.0f;  // bn0 is followed by a ReLU
        const float gq = live ? g[j] * inv[j] * (de - c1[j] - xh * c2[j]) : 0.0f;
#pragma unroll
        for (int t = 0; t < KK; ++t) acc[j * KK + t] = fmaf(a[t], gq, acc[j * KK + t]);
      }
    }
  };
  if (__builtin_amdgcn_ballot_w64(has_task) != 0) {  // wave-uniform
    InRow IA, IB, IC;
    iarrive(iload(r_begin - 1), IA);
    iarrive(iload(r_begin), IB);
    float pi0 = iload(r_begin + 1), pi1 = iload(r_begin + 2), pi2 = iload(r_begin + 3);
    float4 pd0 = dload(r_begin), pd1 = dload(r_begin + 1), pd2 = dload(r_begin + 2);
    for (int i = 0; i < rps; i += 3) {
      const int r = r_begin + i;
      { const float ir = pi0; const float4 dr_ = pd0; pi0 = iload(r + 4); pd0 = dload(r + 3); iarrive(ir, IC); step(IA, IB, IC, dr_, r); }
      { const float ir = pi1; const float4 dr_ = pd1; pi1 = iload(r + 5); pd1 = dload(r + 4); iarrive(ir, IA); step(IB, IC, IA, dr_, r + 1); }
      { const float ir = pi2; const float4 dr_ = pd2; pi2 = iload(r + 6); pd2 = dload(r + 5); iarrive(ir, IB); step(IC, IA, IB, dr_, r + 2); }
    }
  }
  __shared__ float red[4][NACC];
#pragma unroll
  for (int i = 0; i < NACC; ++i) {
    const float v = wave_sum_lane63(acc[i]);
    if (lane == 63) red[threadIdx.x >> 6][i] = v;
  }
  __syncthreads();
  if (threadIdx.x < NACC) {
    const float tot = red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
    if (MODE == 0) {
      atomicAdd(&shards[((int64_t)((blockIdx.x + 7 * b + 3 * cq) & 31) * 4 + cq) * 8 + threadIdx.x], (double)tot);  // [sum 4 | sum of squares 4]
    } else {
      const int j = threadIdx.x / KK, t = threadIdx.x - j * KK;
      atomicAdd(&dW[t * 16 + cq * 4 + j], tot);
    }
  }
}

// the 32 accumulator copies [32][CQ][8] -> scratch2C = dbeta[4 CQ] | dgamma[4 CQ] (doubles), in place by one workgroup (all reads before the first write)
__global__ __launch_bounds__(256) void bwd_sums_compact_kernel(double* __restrict__ shards, int CQ) {
  const int t = threadIdx.x;
  double tot = 0.0;
  if (t < 8 * CQ) {
    const int which = t >= 4 * CQ, c = which ? t - 4 * CQ : t;
    for (int sh = 0; sh < 32; ++sh) tot += shards[((int64_t)sh * CQ + (c >> 2)) * 8 + which * 4 + (c & 3)];
  }
  __syncthreads();
  if (t < 8 * CQ) shards[t] = tot;
}

// ---------------------------------------------------------------- conv0 weight gradient
// dW0[tap][c] += sum_p in[p + off(tap)] * dv0[c][p]; the single-channel input is the UNPADDED snippet image.
template <int KS>
__global__ __launch_bounds__(256) void conv0_wgrad_kernel(const float* __restrict__ in, int64_t snippet_stride, const float* __restrict__ dv /*[B][4][HP][WP][4]*/,
                                                           int H, int W, int WP, int B, float* __restrict__ dW /*[KS*KS][16]*/) {
  // block (bx, cq) walks every snippet; one wave reduction + one LDS reduction + 4*k*k atomics per block at the very end
  // (device-scope float atomics on a handful of addresses serialise at the memory side, so they are kept to gridDim.x per address)
  constexpr int R = KS / 2, KK = KS * KS;
  __shared__ float red[4][4 * KK];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int cq = blockIdx.y;
  const int plane = (H + 2 * R) * WP;
  float acc[4][KK];
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int t = 0; t < KK; ++t) acc[j][t] = 0.0f;
  const int total = H * W;
  for (int b = 0; b < B; ++b) {
    const float* src = in + (int64_t)b * snippet_stride;
    const float4* dp = reinterpret_cast<const float4*>(dv) + ((int64_t)b * 4 + cq) * plane;
    for (int p = blockIdx.x * 256 + threadIdx.x; p < total; p += gridDim.x * 256) {
      const int y = p / W, x = p - y * W;
      const float4 g4 = dp[(y + R) * WP + x];
      const float g[4] = {g4.x, g4.y, g4.z, g4.w};
#pragma unroll
      for (int dy = 0; dy < KS; ++dy)
#pragma unroll
        for (int dx = 0; dx < KS; ++dx) {
          const int yy = y + dy - R, xx = x + dx - R;
          const float a = (yy >= 0 && yy < H && xx >= 0 && xx < W) ? src[yy * W + xx] : 0.0f;
#pragma unroll
          for (int j = 0; j < 4; ++j) acc[j][dy * KS + dx] = fmaf(a, g[j], acc[j][dy * KS + dx]);
        }
    }
  }
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int t = 0; t < KK; ++t) {
      const float v = wave_sum_lane63(acc[j][t]);
      if (lane == 63) red[wave][j * KK + t] = v;
    }
  __syncthreads();
  if (threadIdx.x < 4 * KK) {
    const int j = threadIdx.x / KK, t = threadIdx.x - j * KK;
    atomicAdd(&dW[t * 16 + cq * 4 + j], red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x]);
  }
}

// Entry conv weight gradient with the BatchNorm (+ReLU) backward of bn0 applied on the fly: dv = gamma*inv*(dy_eff - dbeta/N -
// xhat*dgamma/N) is formed per pixel from (dy, v, sums) and consumed at once -- the entry conv has no input gradient, so dv is
// never written.  Same work distribution and block-level reduction as conv0_wgrad_kernel.
template <int KS>
__global__ __launch_bounds__(256) void conv0_bn_wgrad_kernel(const float* __restrict__ in, int64_t snippet_stride, const float* __restrict__ dy,
                                                              const float* __restrict__ v /*[B][4][HP][WP][4]*/, int H, int W, int WP, int B,
                                                              const float* __restrict__ mean, const float* __restrict__ var, const float* __restrict__ gamma,
                                                              const float* __restrict__ beta, float eps, const double* __restrict__ dbeta,
                                                              const double* __restrict__ dgamma, float inv_count, float* __restrict__ dW /*[KS*KS][16]*/) {
  constexpr int R = KS / 2, KK = KS * KS;
  __shared__ float red[4][4 * KK];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int cq = blockIdx.y;
  const int plane = (H + 2 * R) * WP;
  float mu[4], inv[4], g[4], bt[4], c1[4], c2[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int c = cq * 4 + k;  // the entry conv has exactly 16 filters: 4 full quads
    mu[k] = mean[c]; inv[k] = rsqrtf(var[c] + eps); g[k] = gamma[c]; bt[k] = beta[c];
    c1[k] = (float)dbeta[c] * inv_count; c2[k] = (float)dgamma[c] * inv_count;
  }
  float acc[4][KK];
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int t = 0; t < KK; ++t) acc[j][t] = 0.0f;
  const int total = H * W;
  for (int b = 0; b < B; ++b) {
    const float* src = in + (int64_t)b * snippet_stride;
    const float4* dp = reinterpret_cast<const float4*>(dy) + ((int64_t)b * 4 + cq) * plane;
    const float4* vp = reinterpret_cast<const float4*>(v) + ((int64_t)b * 4 + cq) * plane;
    for (int p = blockIdx.x * 256 + threadIdx.x; p < total; p += gridDim.x * 256) {
      const int y = p / W, x = p - y * W;
      const float4 d4 = dp[(y + R) * WP + x], v4 = vp[(y + R) * WP + x];
      const float dd[4] = {d4.x, d4.y, d4.z, d4.w}, vv[4] = {v4.x, v4.y, v4.z, v4.w};
      float gq[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float xh = (vv[k] - mu[k]) * inv[k];
        const float de = (fmaf(xh, g[k], bt[k]) > 0.0f) ? dd[k] : 0.0f;  // bn0 is followed by a ReLU (architectures.py:167-168)
        gq[k] = g[k] * inv[k] * (de - c1[k] - xh * c2[k]);
      }
#pragma unroll
      for (int dyy = 0; dyy < KS; ++dyy)
#pragma unroll
        for (int dx = 0; dx < KS; ++dx) {
          const int yy = y + dyy - R, xx = x + dx - R;
          const float a = (yy >= 0 && yy < H && xx >= 0 && xx < W) ? src[yy * W + xx] : 0.0f;
#pragma unroll
          for (int j = 0; j < 4; ++j) acc[j][dyy * KS + dx] = fmaf(a, gq[j], acc[j][dyy * KS + dx]);
        }
    }
  }
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int t = 0; t < KK; ++t) {
      const float s2 = wave_sum_lane63(acc[j][t]);
      if (lane == 63) red[wave][j * KK + t] = s2;
    }
  __syncthreads();
  if (threadIdx.x < 4 * KK) {
    const int j = threadIdx.x / KK, t = threadIdx.x - j * KK;
    atomicAdd(&dW[t * 16 + cq * 4 + j], red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x]);
  }
}

// ---------------------------------------------------------------- bn0 backward with v0 RECOMPUTED from the 1-channel input
// The training forward no longer stores v0 = conv0(x) + bias (model_fwd.hip: conv0_stats_kernel + conv0_kernel's BatchNorm stage): the two
// kernels of bn0's backward rebuild it per pixel from the k x k input taps they load anyway -- the fma chain of conv0_kernel in its order,
// then fma(acc, 1, bias): bit for bit the value the forward pass normalised -- instead of reading 0.52 GB of v0 each.
// Work distribution of conv0_kernel (8 x 32-pixel tiles, the input halo staged once per tile in LDS, thread = pixel), one channel quad per
// blockIdx.y, persistent over the tiles: per-thread partial sums live in registers across ~70 tiles and are reduced once per workgroup.
template <int KS, bool WGRAD>
__global__ __launch_bounds__(256) void conv0_bn_bwd_x_kernel(const float* __restrict__ in, int64_t snippet_stride, const float* __restrict__ dy, int H, int W, int WP, int B,
                                                              const float* __restrict__ w0 /*[KS*KS][16]*/, const float* __restrict__ bias,
                                                              const float* __restrict__ mean, const float* __restrict__ var, const float* __restrict__ gamma,
                                                              const float* __restrict__ beta, float eps, double* __restrict__ shards /*!WGRAD: [32][4][8] sum g | sum g xhat*/,
                                                              const double* __restrict__ dbeta, const double* __restrict__ dgamma, float inv_count,
                                                              float* __restrict__ part /*WGRAD: [gridDim.x][KS*KS*16] partial weight gradients*/) {
  constexpr int TH = 8, TW = 32, R = KS / 2, KK = KS * KS, HH = TH + KS - 1, HW = TW + KS - 1, HP_ = HW + 1, NACC = WGRAD ? 4 * KK : 8;
  __shared__ float halo[HH][HP_];
  __shared__ float red[4][NACC];
  const int cq = blockIdx.y;
  const int plane = (H + 2 * R) * WP;
  float mu[4], inv[4], g[4], bt[4], c1[4], c2[4], wq[KK][4], bs[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int c = cq * 4 + k;
    mu[k] = mean[c]; inv[k] = rsqrtf(var[c] + eps); g[k] = gamma[c]; bt[k] = beta[c]; bs[k] = bias[c];
    c1[k] = WGRAD ? (float)dbeta[c] * inv_count : 0.0f;
    c2[k] = WGRAD ? (float)dgamma[c] * inv_count : 0.0f;
#pragma unroll
    for (int t = 0; t < KK; ++t) wq[t][k] = w0[t * 16 + c];
  }
  float acc[NACC];
#pragma unroll
  for (int i = 0; i < NACC; ++i) acc[i] = 0.0f;
  const int tx = (W + TW - 1) / TW, ty = (H + TH - 1) / TH;
  const int ntiles = tx * ty * B;
  const int py = threadIdx.x / TW, px = threadIdx.x % TW;
  // The NEXT tile's input halo (<= 2 values per thread at k = 3) and gradient quad are requested before the current tile is worked on and
  // handed over through registers: a tile does not start by waiting for a round trip to memory.
  constexpr int HN = (HH * HW + 255) / 256;
  float hreg[HN];
  float4 dnext = make_float4(0.f, 0.f, 0.f, 0.f);
  auto request = [&](int tile) {
    const bool any = tile < ntiles;
    const int tl = any ? tile : 0;
    const int b = tl / (tx * ty), rem = tl - b * (tx * ty);
    const int y0 = (rem / tx) * TH, x0 = (rem - (rem / tx) * tx) * TW;
    const float* src = in + (int64_t)b * snippet_stride;
#pragma unroll
    for (int k = 0; k < HN; ++k) {
      const int i = threadIdx.x + 256 * k;
      const int r = i / HW, c = i % HW;
      const int yy = y0 + r - R, xx = x0 + c - R;
      hreg[k] = (any && i < HH * HW && yy >= 0 && yy < H && xx >= 0 && xx < W) ? src[(int64_t)yy * W + xx] : 0.0f;
    }
    const int y = y0 + py, x = x0 + px;
    dnext = (any && y < H && x < W) ? (reinterpret_cast<const float4*>(dy) + ((int64_t)b * 4 + cq) * plane)[(y + R) * WP + x] : make_float4(0.f, 0.f, 0.f, 0.f);
  };
  request(blockIdx.x);
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int b = tile / (tx * ty), rem = tile - b * (tx * ty);
    const int y0 = (rem / tx) * TH, x0 = (rem - (rem / tx) * tx) * TW;
    const int y = y0 + py, x = x0 + px;
    const bool live = y < H && x < W;
    (void)b;
    __syncthreads();  // the previous tile's halo reads are done
#pragma unroll
    for (int k = 0; k < HN; ++k) {
      const int i = threadIdx.x + 256 * k;
      if (i < HH * HW) halo[i / HW][i % HW] = hreg[k];
    }
    const float4 d4 = dnext;
    __syncthreads();
    request(tile + gridDim.x);
    float a[KK];
#pragma unroll
    for (int dyy = 0; dyy < KS; ++dyy)
#pragma unroll
      for (int dx = 0; dx < KS; ++dx) a[dyy * KS + dx] = halo[py + dyy][px + dx];
    const float dd[4] = {d4.x, d4.y, d4.z, d4.w};
    float gq[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      float cv = 0.0f;
#pragma unroll
      for (int t = 0; t < KK; ++t) cv = fmaf(a[t], wq[t][k], cv);  // conv0_kernel's chain, taps in (dy, dx) order
      const float v = fmaf(cv, 1.0f, bs[k]);                        // ... and its fma(acc, scale = 1, shift = bias)
      const float xh = (v - mu[k]) * inv[k];
      const float de = (live && fmaf(xh, g[k], bt[k]) > 0.0f) ? dd[k] : 0.0f;  // bn0 is followed by a ReLU (architectures.py:167-168)
      if (WGRAD) {
        gq[k] = live ? g[k] * inv[k] * (de - c1[k] - xh * c2[k]) : 0.0f;
      } else {
        acc[k] += de;
        acc[4 + k] = fmaf(de, xh, acc[4 + k]);
      }
    }
    if (WGRAD) {
#pragma unroll
      for (int t = 0; t < KK; ++t)
#pragma unroll
        for (int k = 0; k < 4; ++k) acc[k * KK + t] = fmaf(a[t], gq[k], acc[k * KK + t]);
    }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < NACC; ++i) {
    const float v = wave_sum_lane63(acc[i]);
    if (lane == 63) red[wave][i] = v;
  }
  __syncthreads();
  if (threadIdx.x < NACC) {
    const float tot = (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
    if (WGRAD) {
      const int k = threadIdx.x / KK, t = threadIdx.x - k * KK;
      part[(int64_t)blockIdx.x * (KK * 16) + t * 16 + cq * 4 + k] = tot;  // Keras layout [tap][filter]; every (workgroup, quad) owns its slots
    } else {
      atomicAdd(&shards[((int64_t)(blockIdx.x & 31) * 4 + cq) * 8 + threadIdx.x], (double)tot);  // [sum g (4) | sum g xhat (4)] of this quad
    }
  }
}

// [32][4][8] accumulator copies -> scratch2C = dbeta[16] | dgamma[16] (doubles), in place (all reads before the first write)
__global__ void conv0_sums_compact_kernel(double* __restrict__ shards) {
  const int t = threadIdx.x;  // 0..31: dbeta[t] for t < 16, dgamma[t - 16] beyond
  const int which = t >> 4, c = t & 15;
  double tot = 0.0;
  for (int sh = 0; sh < 32; ++sh) tot += shards[((int64_t)sh * 4 + (c >> 2)) * 8 + which * 4 + (c & 3)];
  __syncthreads();
  shards[t] = tot;
}

// ---------------------------------------------------------------- the entry conv's input gradient
// dx[b][p] = sum over taps t, channels c of w0[t][c] * dv[c][p - off(t)], dv = bn0's (+ReLU) input gradient -- the value conv0_march_kernel<1> /
// conv0_bn_bwd_x_kernel<.., true> contract with the input taps for dW0, formed here with their expressions in their order (the fma chain of
// conv0_kernel, fma(cv, 1, bias), (float)dbeta * inv_count) from the snippet, dy and the sums those passes left in scratch2C.  Every dx element has
// one owner: no atomics, no reduction across lanes or workgroups, so dx is the same from run to run.
//
// k = 3, marching: a wave owns a 62-column strip over a segment of rows; lane l works on column strip * 62 - 1 + l and forms dv for ALL 16 channels of
// its pixel (four float4 loads from the four quad planes, each dy quad loaded once per strip).  dv at the two halo lanes needs one snippet column
// beyond the wave: lanes 0 and 63 load it themselves (4 bytes per row).  Per pixel the nine scalars s[t] = sum_c w0[t][c] * dv[c] are formed (the
// taps and the per-channel constants are wave-uniform), the six off-centre ones move one lane left / right (DPP) and all nine are added into three
// rotating output-row accumulators: row y - 1 is complete, and stored, when dv row y has passed.  No LDS, no barriers.
__global__ __launch_bounds__(256) void conv0_dx_march_kernel(const float* __restrict__ in, int64_t snippet_stride, const float* __restrict__ dy /*[B][4][H + 2][WP][4]*/, int H,
                                                              int W, int WP, const float* __restrict__ w0 /*[9][16]*/, const float* __restrict__ bias,
                                                              const float* __restrict__ mean, const float* __restrict__ var, const float* __restrict__ gamma,
                                                              const float* __restrict__ beta, float eps, const double* __restrict__ sums /*dbeta[16] | dgamma[16]*/,
                                                              float inv_count, float* __restrict__ dx /*[B][H][W]*/, int nstrip, int nseg, int rps) {
  constexpr int KK = 9;
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.z;
  const int task = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (task >= nstrip * nseg) return;  // wave-uniform; the kernel has no barrier
  const int strip = task % nstrip, seg = task / nstrip;
  const int xcol = strip * 62 - 1 + lane;
  const bool col_ok = xcol >= 0 && xcol < W;
  const bool out_lane = lane >= 1 && lane <= 62 && xcol < W;
  const bool edge_lane = lane == 0 || lane == 63;
  const int ecol = lane == 0 ? xcol - 1 : xcol + 1;  // the snippet column beyond the wave that a halo lane's own conv needs
  const bool ecol_ok = ecol >= 0 && ecol < W;
  const int cc = xcol < 0 ? 0 : (xcol >= W ? W - 1 : xcol), ec = ecol < 0 ? 0 : (ecol >= W ? W - 1 : ecol);
  const int r_begin = seg * rps, r_end = min(r_begin + rps, H);
  const int plane = (H + 2) * WP;
  const float* inb = in + (int64_t)b * snippet_stride;
  const float4* dp = reinterpret_cast<const float4*>(dy) + (int64_t)b * 4 * plane;
  float* dxb = dx + (int64_t)b * H * W;
  struct InRow { float c, l, r; };
  struct Raw { float v, e; };
  struct DyRow { float4 q[4]; };
  auto iload = [&](int row) -> Raw {  // zero outside the image (the conv's "same" padding); the addresses are clamped into the snippet
    const int rr = row < 0 ? 0 : (row >= H ? H - 1 : row);
    const bool row_ok = row >= 0 && row < H;
    Raw o;
    const float v = inb[(int64_t)rr * W + cc];
    o.v = (row_ok && col_ok) ? v : 0.0f;
    o.e = 0.0f;
    if (edge_lane) {
      const float e = inb[(int64_t)rr * W + ec];
      o.e = (row_ok && ecol_ok) ? e : 0.0f;
    }
    return o;
  };
  auto dload = [&](int row) -> DyRow {  // interior addresses only (clamped); what a clamped load delivers is masked where dv is formed
    const int rr = row < 0 ? 0 : (row >= H ? H - 1 : row);
    DyRow o;
#pragma unroll
    for (int cq = 0; cq < 4; ++cq) o.q[cq] = dp[(int64_t)cq * plane + (rr + 1) * WP + cc];
    return o;
  };
  auto iarrive = [&](const Raw& raw, InRow& o) {
    o.c = raw.v;
    const float l = lsh<3, -1>(raw.v), r = lsh<3, 1>(raw.v);
    o.l = lane == 0 ? raw.e : l;
    o.r = lane == 63 ? raw.e : r;
  };
  // The pass needs 272 wave-uniform values per pixel row (144 taps, 8 constants for each of 16 channels): more than a wave has scalar registers.
  // The channels are therefore worked on quad by quad in a loop that is NOT unrolled: a quad's taps and raw constants are scalar loads inside
  // it (68 values, the budget conv0_march_kernel lives in), and the four derived constants of every channel (values no load can deliver) sit in
  // one vector register, lane kind * 16 + c, formed once per wave by the lane that holds them and read with v_readlane.
  float ctab;
  {
    const int c = lane & 15, kind = lane >> 4;
    const float inv = rsqrtf(var[c] + eps);
    ctab = kind == 0 ? inv : kind == 1 ? (float)sums[c] * inv_count : kind == 2 ? (float)sums[16 + c] * inv_count : gamma[c] * inv;
  }
  auto tab = [&](int i) { return __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(ctab), i)); };
  InRow up, mid, dn;
  iarrive(iload(r_begin - 2), up);
  iarrive(iload(r_begin - 1), mid);
  Raw pin = iload(r_begin);
  DyRow pd = dload(r_begin - 1);
  float accA = 0.0f, accB = 0.0f;  // dx rows y - 1 and y while dv row y is worked on
  for (int y = r_begin - 1; y <= r_end; ++y) {
    iarrive(pin, dn);
    float4 q0 = pd.q[0], q1 = pd.q[1], q2 = pd.q[2], q3 = pd.q[3];
    pin = iload(y + 2);
    pd = dload(y + 1);
    const bool valid = col_ok && y >= 0 && y < H;  // dv is zero outside the image
    const float a[KK] = {up.l, up.c, up.r, mid.l, mid.c, mid.r, dn.l, dn.c, dn.r};
    float s[KK];
#pragma unroll
    for (int t = 0; t < KK; ++t) s[t] = 0.0f;
#pragma clang loop unroll(disable)
    for (int cq = 0; cq < 4; ++cq) {
      const float dd[4] = {q0.x, q0.y, q0.z, q0.w};
      q0 = q1; q1 = q2; q2 = q3;  // the quads take turns in q0: no register array is indexed by the loop counter
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int c = cq * 4 + j;
        const float mu = mean[c], g = gamma[c], bt = beta[c];
        const float inv = tab(c), c1 = tab(16 + c), c2 = tab(32 + c), gi = tab(48 + c);  // gi = g * inv, the first product of conv0_march_kernel's dv
        float cv = 0.0f;
#pragma unroll
        for (int t = 0; t < KK; ++t) cv = fmaf(a[t], w0[t * 16 + c], cv);  // conv0_kernel's chain, taps in (dy, dx) order
        const float v = fmaf(cv, 1.0f, bias[c]);
        const float xh = (v - mu) * inv;
        const float de = (valid && fmaf(xh, g, bt) > 0.0f) ? dd[j] : 0.0f;  // bn0 is followed by a ReLU
        const float gq = valid ? gi * (de - c1 - xh * c2) : 0.0f;
#pragma unroll
        for (int t = 0; t < KK; ++t) s[t] = fmaf(w0[t * 16 + c], gq, s[t]);
      }
    }
    // dv at (y, x) reaches dx at (y + ty - 1, x + tx - 1) through tap (ty, tx): lane l takes tx = 0 from lane l + 1 and tx = 2 from lane l - 1
    accA += lsh<3, 1>(s[0]) + s[1] + lsh<3, -1>(s[2]);
    accB += lsh<3, 1>(s[3]) + s[4] + lsh<3, -1>(s[5]);
    const float accC = lsh<3, 1>(s[6]) + s[7] + lsh<3, -1>(s[8]);
    if (out_lane && y - 1 >= r_begin) dxb[(int64_t)(y - 1) * W + xcol] = accA;  // y <= r_end: row y - 1 is inside the segment
    accA = accB;
    accB = accC;
    up = mid;
    mid = dn;
  }
}

// k = 5 / 7 (and k = 3 beyond the marching kernel's limits): the plain tile form.  8 x 32 output pixels per workgroup; the snippet halo (2R around the
// tile) is staged in LDS, dv of all 16 channels is formed once per pixel of the tile + R and kept in LDS, a thread then gathers its k x k x 16 products.
template <int KS>
__global__ __launch_bounds__(256) void conv0_dx_tile_kernel(const float* __restrict__ in, int64_t snippet_stride, const float* __restrict__ dy, int H, int W, int WP,
                                                             const float* __restrict__ w0 /*[KS*KS][16]*/, const float* __restrict__ bias, const float* __restrict__ mean,
                                                             const float* __restrict__ var, const float* __restrict__ gamma, const float* __restrict__ beta, float eps,
                                                             const double* __restrict__ sums, float inv_count, float* __restrict__ dx, int tx, int ty) {
  constexpr int R = KS / 2, KK = KS * KS, TH = 8, TW = 32, DH = TH + 2 * R, DW = TW + 2 * R, IH = TH + 4 * R, IW = TW + 4 * R;
  __shared__ float tin[IH][IW + 1];
  __shared__ float tdv[16][DH][DW + 1];
  __shared__ float wl[KK][16];
  __shared__ float cst[8][16];  // bias | mean | inv | gamma | beta | dbeta / N | dgamma / N | gamma * inv
  const int tile = blockIdx.x;
  const int b = tile / (tx * ty), rem = tile - b * (tx * ty);
  const int y0 = (rem / tx) * TH, x0 = (rem - (rem / tx) * tx) * TW;
  const int plane = (H + 2 * R) * WP;
  const float* src = in + (int64_t)b * snippet_stride;
  const float4* dp = reinterpret_cast<const float4*>(dy) + (int64_t)b * 4 * plane;
  if (threadIdx.x < 16) {
    const int c = threadIdx.x;
    const float inv = rsqrtf(var[c] + eps), g = gamma[c];
    cst[0][c] = bias[c]; cst[1][c] = mean[c]; cst[2][c] = inv; cst[3][c] = g; cst[4][c] = beta[c];
    cst[5][c] = (float)sums[c] * inv_count; cst[6][c] = (float)sums[16 + c] * inv_count; cst[7][c] = g * inv;
  }
  for (int i = threadIdx.x; i < KK * 16; i += 256) wl[i / 16][i % 16] = w0[i];
  for (int i = threadIdx.x; i < IH * IW; i += 256) {
    const int r = i / IW, c = i - r * IW;
    const int yy = y0 + r - 2 * R, xx = x0 + c - 2 * R;
    tin[r][c] = (yy >= 0 && yy < H && xx >= 0 && xx < W) ? src[(int64_t)yy * W + xx] : 0.0f;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < DH * DW; i += 256) {
    const int r = i / DW, cl = i - r * DW;
    const int yy = y0 + r - R, xx = x0 + cl - R;
    const bool valid = yy >= 0 && yy < H && xx >= 0 && xx < W;  // dv is zero outside the image
    float a[KK];
#pragma unroll
    for (int dyy = 0; dyy < KS; ++dyy)
#pragma unroll
      for (int dxx = 0; dxx < KS; ++dxx) a[dyy * KS + dxx] = tin[r + dyy][cl + dxx];
    for (int cq = 0; cq < 4; ++cq) {
      const float4 d4 = valid ? dp[(int64_t)cq * plane + (yy + R) * WP + xx] : make_float4(0.f, 0.f, 0.f, 0.f);
      const float dd[4] = {d4.x, d4.y, d4.z, d4.w};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int c = cq * 4 + j;
        float cv = 0.0f;
#pragma unroll
        for (int t = 0; t < KK; ++t) cv = fmaf(a[t], wl[t][c], cv);  // conv0_kernel's chain, taps in (dy, dx) order
        const float v = fmaf(cv, 1.0f, cst[0][c]);
        const float xh = (v - cst[1][c]) * cst[2][c];
        const float de = (valid && fmaf(xh, cst[3][c], cst[4][c]) > 0.0f) ? dd[j] : 0.0f;
        tdv[c][r][cl] = valid ? cst[7][c] * (de - cst[5][c] - xh * cst[6][c]) : 0.0f;
      }
    }
  }
  __syncthreads();
  const int py = threadIdx.x / TW, px = threadIdx.x % TW;
  const int y = y0 + py, x = x0 + px;
  if (y < H && x < W) {
    float acc = 0.0f;
    for (int dyy = 0; dyy < KS; ++dyy)
      for (int dxx = 0; dxx < KS; ++dxx)
#pragma unroll
        for (int c = 0; c < 16; ++c) acc = fmaf(wl[dyy * KS + dxx][c], tdv[c][py + 2 * R - dyy][px + 2 * R - dxx], acc);
    dx[(int64_t)b * H * W + (int64_t)y * W + x] = acc;
  }
}

// ---------------------------------------------------------------- kernel-layout copies of the trunk weights, one launch per step
// desc[i] = {type, src offset, dst offset, C, aux}: type 0 = Keras depthwise (k,k,C,1) -> [ceil(C/4)][k*k][4] (aux = k*k; zero taps for
// the padding channels), type 1 = the same with the taps reversed (input-gradient conv), type 2 = pointwise (1,1,Cin,Cout) ->
// transposed [Cout][Cin] (C = Cin, aux = Cout).  One workgroup per descriptor; replaces ~80 tiny framework kernels per step.
__global__ __launch_bounds__(256) void pack_weights_kernel(const float* __restrict__ w, const int* __restrict__ desc, float* __restrict__ out) {
  const int* d = desc + blockIdx.x * 5;
  const int type = d[0], C = d[3], aux = d[4];
  const float* src = w + d[1];
  float* dst = out + d[2];
  if (type <= 1) {
    const int KK = aux, CQ = (C + 3) >> 2;
    for (int i = threadIdx.x; i < CQ * KK * 4; i += 256) {
      const int j = i & 3, tap = (i >> 2) % KK, cq = (i >> 2) / KK;
      const int c = cq * 4 + j, ts = type ? KK - 1 - tap : tap;
      dst[i] = c < C ? src[ts * C + c] : 0.0f;
    }
  } else {
    const int Cin = C, Cout = aux;
    for (int i = threadIdx.x; i < Cin * Cout; i += 256) {
      const int co = i / Cin, ci = i - co * Cin;
      dst[i] = src[ci * Cout + co];
    }
  }
}

// ---------------------------------------------------------------- Keras Reshape layout [B][H][W*C] -> planes (gradient of the final conv)
__global__ __launch_bounds__(256) void feat_to_planes_kernel(const float* __restrict__ f, int C, int H, int W, int WP, int R, float* __restrict__ out, int B) {
  const int CQ = (C + 3) >> 2;
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t interior = (int64_t)H * W;
  if (idx >= (int64_t)B * CQ * interior) return;
  const int64_t bq = idx / interior, pix = idx - bq * interior;
  const int cq = (int)(bq % CQ);
  const int64_t b = bq / CQ;
  const int yy = (int)(pix / W), xx = (int)(pix - (int64_t)yy * W);
  const float* src = f + ((b * H + yy) * (int64_t)W + xx) * C + cq * 4;
  float o[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) o[k] = (cq * 4 + k < C) ? src[k] : 0.0f;
  reinterpret_cast<float4*>(out)[bq * ((int64_t)(H + 2 * R) * WP) + (int64_t)(yy + R) * WP + xx] = make_float4(o[0], o[1], o[2], o[3]);
}

// elementwise on whole plane buffers: dx = (y > 0) ? dy : 0   /  x += y
__global__ __launch_bounds__(256) void relu_bwd4_kernel(const float4* __restrict__ dy, const float4* __restrict__ y, int64_t n4, float4* __restrict__ dx) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n4) return;
  const float4 d = dy[i], v = y[i];
  dx[i] = make_float4(v.x > 0.f ? d.x : 0.f, v.y > 0.f ? d.y : 0.f, v.z > 0.f ? d.z : 0.f, v.w > 0.f ? d.w : 0.f);
}

template <int SW>
static int launch_dw_bwd(hipStream_t st, const float* x, const float* du, int B, int C, int H, int W, int WP, int relu_in, const float* wrev, float* dr, float* dW, int epi,
                         const InBnW& ib, int epi_relu, double* shards, int nstrip, const Conv0In* c0 = nullptr) {
  constexpr int NSUB = 64 / SW;
  const int CQ = (C + 3) / 4;
  const int64_t per_seg = (int64_t)B * CQ * nstrip;
  int nseg = (int)((16384ll * NSUB + per_seg - 1) / per_seg);  // ~16 waves per SIMD over the chip in total (8 192 ... 24 576 measured: flat, profiles/r04_ab_march_waves.log)
  if (nseg < 1) nseg = 1;
  if (nseg > (H + 23) / 24) nseg = (H + 23) / 24;  // at least 24 rows per segment: two halo rows of du are re-read per segment
  int rps = (H + nseg - 1) / nseg;
  rps = (rps + 2) / 3 * 3;  // whole iterations of the loop unrolled by three
  nseg = (H + rps - 1) / rps;
  const int waves = (nstrip * nseg + NSUB - 1) / NSUB;
  dim3 grid((waves + 3) / 4, CQ, B);
  if (c0) hipLaunchKernelGGL((dw_bwd_march_kernel<SW, 2, true, true>), grid, dim3(256), 0, st, x, du, C, H, W, WP, 0, wrev, dr, dW, shards, nstrip, nseg, rps, ib, 1, *c0);
  else if (epi == 2) hipLaunchKernelGGL((dw_bwd_march_kernel<SW, 2, true>), grid, dim3(256), 0, st, x, du, C, H, W, WP, 0, wrev, dr, dW, shards, nstrip, nseg, rps, ib, epi_relu, Conv0In{});
  else if (epi == 3) hipLaunchKernelGGL((dw_bwd_march_kernel<SW, 3, false>), grid, dim3(256), 0, st, x, du, C, H, W, WP, relu_in, wrev, dr, dW, shards, nstrip, nseg, rps, ib, 0, Conv0In{});
  else if (ib.mean) hipLaunchKernelGGL((dw_bwd_march_kernel<SW, 0, true>), grid, dim3(256), 0, st, x, du, C, H, W, WP, 0, wrev, dr, dW, shards, nstrip, nseg, rps, ib, 0, Conv0In{});
  else hipLaunchKernelGGL((dw_bwd_march_kernel<SW, 0, false>), grid, dim3(256), 0, st, x, du, C, H, W, WP, relu_in, wrev, dr, dW, shards, nstrip, nseg, rps, ib, 0, Conv0In{});
  return (int)hipGetLastError();
}

}  // namespace

extern "C" {

int orcai_bn_planes_stats(const float* v, int B, int C, int H, int W, int ksize, double* scratch2C, float* mean, float* var, void* stream) {
  if (!v || !scratch2C || !mean || !var || B <= 0 || C <= 0 || H <= 0 || W <= 0) return ORCAI_E_BADARG;
  if (C > 64) return ORCAI_E_BADARG;  // scratch2C holds 8 doubles per channel quad of at most 64 channels (the caller cannot pass its size)
  hipStream_t st = (hipStream_t)stream;
  const int CQ = (C + 3) / 4, R = ksize / 2, WP = orcai_padded_width(W, ksize);
  const int64_t plane = (int64_t)(H + 2 * R) * WP;
  if (plane >= (1ll << 31)) return ORCAI_E_UNSUPPORTED;
  if (plane < 16384) {  // small planes: the full-occupancy pass with sharded accumulators (scratch: f64[8 * ceil(C/4) * 32])
    const int nchunk = (int)((plane + 4095) / 4096);
    hipError_t e = orcai_zero::zero_async(scratch2C, sizeof(double) * 8 * CQ * SUM_SHARDS, st);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(planes_sums_sharded_kernel, dim3((unsigned)(B * nchunk), CQ), dim3(256), 0, st, v, CQ, (int)plane, nchunk, scratch2C);
    hipLaunchKernelGGL(bn_finish_stats_sharded_kernel, dim3((C + 63) / 64), dim3(64), 0, st, scratch2C, C, CQ, (double)B * H * W, mean, var);
    return (int)hipGetLastError();
  }
  hipError_t e = orcai_zero::zero_async(scratch2C, sizeof(double) * 8 * CQ, st);
  if (e != hipSuccess) return (int)e;
  int gx = (int)((B * plane + 255) / 256);
  if (gx > 128) gx = 128;  // few blocks per quad: each ends with same-line double atomics
  hipLaunchKernelGGL(planes_sums_kernel, dim3(gx, CQ), dim3(256), 0, st, v, CQ, plane, B, scratch2C, scratch2C + 4 * CQ);
  hipLaunchKernelGGL(bn_finish_stats_kernel, dim3((C + 63) / 64), dim3(64), 0, st, scratch2C, scratch2C + 4 * CQ, C, (double)B * H * W, mean, var);
  return (int)hipGetLastError();
}

int orcai_bn_finish_sharded(const double* shards, int B, int C, int H, int W, float* mean, float* var, void* stream) {
  if (!shards || !mean || !var || B <= 0 || C <= 0 || C > 64 || H <= 0 || W <= 0) return ORCAI_E_BADARG;
  hipLaunchKernelGGL(bn_finish_stats_sharded_kernel, dim3((C + 63) / 64), dim3(64), 0, (hipStream_t)stream, shards, C, (C + 3) / 4, (double)B * H * W, mean, var);
  return (int)hipGetLastError();
}

int orcai_planes_sum(const float* x, int B, int C, int H, int W, int ksize, double* scratchC, float* out, int accumulate, void* stream) {
  if (!x || !scratchC || !out || B <= 0 || C <= 0 || C > 64 || H <= 0 || W <= 0) return ORCAI_E_BADARG;
  hipStream_t st = (hipStream_t)stream;
  const int CQ = (C + 3) / 4, R = ksize / 2, WP = orcai_padded_width(W, ksize);
  const int64_t plane = (int64_t)(H + 2 * R) * WP;
  if (plane >= (1ll << 31)) return ORCAI_E_UNSUPPORTED;
  hipError_t e = orcai_zero::zero_async(scratchC, sizeof(double) * 4 * CQ, st);
  if (e != hipSuccess) return (int)e;
  int gx = (int)((B * plane + 255) / 256);
  if (gx > 128) gx = 128;  // few blocks per quad: each ends with same-line double atomics
  hipLaunchKernelGGL(planes_sums_kernel, dim3(gx, CQ), dim3(256), 0, st, x, CQ, plane, B, scratchC, (double*)nullptr);
  hipLaunchKernelGGL(f64_to_f32_kernel, dim3((C + 63) / 64), dim3(64), 0, st, scratchC, out, C, accumulate);
  return (int)hipGetLastError();
}

int orcai_bn_planes_apply(const float* v, int B, int C, int H, int W, int ksize, const float* mean, const float* var, const float* gamma, const float* beta,
                          float eps, int relu, float* y, void* stream) {
  if (!v || !y || !mean || !var || !gamma || !beta || B <= 0 || C <= 0) return ORCAI_E_BADARG;
  const int64_t bq = (int64_t)B * ((C + 3) / 4);
  if (bq > 65535 || (int64_t)H * W >= (1ll << 31)) return ORCAI_E_UNSUPPORTED;
  hipLaunchKernelGGL(bn_planes_apply_kernel, dim3(blocks_for((int64_t)H * W), (unsigned)bq), dim3(256), 0, (hipStream_t)stream, v, C, H, W,
                     orcai_padded_width(W, ksize), ksize / 2, mean, var, gamma, beta, eps, relu, y, B);
  return (int)hipGetLastError();
}

int orcai_bn_planes_bwd(const float* dy, const float* v, int B, int C, int H, int W, int ksize, const float* mean, const float* var, const float* gamma,
                        const float* beta, float eps, int relu, double* scratch2C, float* dbeta, float* dgamma, float* dv, void* stream) {
  if (!dy || !v || !dv || !scratch2C || !dbeta || !dgamma || B <= 0 || C <= 0 || C > 64 || H <= 0 || W <= 0) return ORCAI_E_BADARG;
  hipStream_t st = (hipStream_t)stream;
  const int CQ = (C + 3) / 4, R = ksize / 2, WP = orcai_padded_width(W, ksize);
  const int64_t plane = (int64_t)(H + 2 * R) * WP;
  if (plane >= (1ll << 31)) return ORCAI_E_UNSUPPORTED;
  hipError_t e = orcai_zero::zero_async(scratch2C, sizeof(double) * 8 * CQ, st);
  if (e != hipSuccess) return (int)e;
  int gx = (int)((B * plane + 255) / 256);
  if (gx > 128) gx = 128;  // few blocks per quad: each ends with same-line double atomics
  double* db = scratch2C;
  double* dg = scratch2C + 4 * CQ;
  hipLaunchKernelGGL(bn_planes_bwd_sums_kernel, dim3(gx, CQ), dim3(256), 0, st, dy, v, C, plane, B, mean, var, gamma, beta, eps, relu, db, dg);
  const int64_t n = (int64_t)B * CQ * H * W;
  hipLaunchKernelGGL(bn_planes_bwd_apply_kernel, dim3(blocks_for(n)), dim3(256), 0, st, dy, v, C, H, W, WP, R, mean, var, gamma, beta, eps, relu, db, dg,
                     (double)B * H * W, dv, B);
  hipLaunchKernelGGL(f64_to_f32_pair_kernel, dim3((C + 63) / 64), dim3(64), 0, st, db, dbeta, dg, dgamma, C);
  return (int)hipGetLastError();
}

int orcai_bn_bwd_pointwise(const float* dy, const float* v, int B, int C, int H, int W, int ksize, const float* mean, const float* var, const float* gamma,
                           const float* beta, float eps, int relu, double* scratch2C, int sums_ready, float* dbeta, float* dgamma, const float* wt, int Cin,
                           float* dv, float* du, void* stream) {
  if (!dy || !v || !dv || !du || !wt || !scratch2C || !dbeta || !dgamma || B <= 0 || C <= 0 || Cin <= 0 || C > 64 || Cin > 64) return ORCAI_E_BADARG;
  hipStream_t st = (hipStream_t)stream;
  const int CQ = (C + 3) / 4, R = ksize / 2, WP = orcai_padded_width(W, ksize);
  const int64_t plane = (int64_t)(H + 2 * R) * WP;
  if (plane >= (1ll << 29)) return ORCAI_E_UNSUPPORTED;
  double* db = scratch2C;
  double* dg = scratch2C + 4 * CQ;
  if (!sums_ready) {  // sums_ready: the producer of dy (orcai_pool_bwd_bn) already accumulated sum dy / sum dy*xhat into scratch
    hipError_t e = orcai_zero::zero_async(scratch2C, sizeof(double) * 8 * CQ, st);
    if (e != hipSuccess) return (int)e;
    int gx = (int)((B * plane + 255) / 256);
    if (gx > 128) gx = 128;
    hipLaunchKernelGGL(bn_planes_bwd_sums_kernel, dim3(gx, CQ), dim3(256), 0, st, dy, v, C, plane, B, mean, var, gamma, beta, eps, relu, db, dg);
  }
  const int tasks = (H * WP + 63) / 64;
  dim3 grid((tasks + 3) / 4, B);
  const float inv_count = (float)(1.0 / ((double)B * H * W));
#define ORCAI_BBP(MT_)                                                                                                                                 \
  hipLaunchKernelGGL((bn_bwd_pw_kernel<MT_>), grid, dim3(256), 0, st, dy, v, C, H, W, WP, R, mean, var, gamma, beta, eps, relu, db, dg, inv_count, wt, Cin, \
                     dv, du, tasks, magic_for(WP))
  switch ((Cin + 15) / 16) {
    case 1: ORCAI_BBP(1); break;
    case 2: ORCAI_BBP(2); break;
    case 3: ORCAI_BBP(3); break;
    case 4: ORCAI_BBP(4); break;
    default: return ORCAI_E_UNSUPPORTED;
  }
#undef ORCAI_BBP
  hipLaunchKernelGGL(f64_to_f32_pair_kernel, dim3((C + 63) / 64), dim3(64), 0, st, db, dbeta, dg, dgamma, C);
  return (int)hipGetLastError();
}

static int g_pw_wgrad_tiles = 4;  // widest layer (ceil(Cin/16) + ceil(C/16)) orcai_bn_bwd_pointwise_wgrad accepts (orcai_pw_wgrad_tiles: experiments)

int orcai_pw_wgrad_tiles(int tiles) {
  const int prev = g_pw_wgrad_tiles;
  if (tiles >= 0) g_pw_wgrad_tiles = tiles > 6 ? 6 : tiles;
  return prev;
}

int orcai_bn_bwd_pointwise_wgrad(const float* dy, const float* v, const float* u, int B, int C, int H, int W, int ksize, const float* mean, const float* var,
                                 const float* gamma, const float* beta, float eps, int relu, double* scratch2C, int sums_ready, float* dbeta, float* dgamma,
                                 const float* wt, int Cin, float* du, float* dWpw, float* workspace, int64_t workspace_floats, void* stream) {
  if (!dy || !v || !u || !du || !wt || !scratch2C || !dbeta || !dgamma || !dWpw || !workspace || B <= 0 || C <= 0 || Cin <= 0 || C > 64 || Cin > 64) return ORCAI_E_BADARG;
  const int MTv = (Cin + 15) / 16, NTv = (C + 15) / 16;
  if (MTv + NTv > g_pw_wgrad_tiles || B > 65535) return ORCAI_E_UNSUPPORTED;  // checked before anything is touched: the caller runs orcai_bn_bwd_pointwise + orcai_outer_reduce
  const int NWv = MTv + NTv <= 4 ? 4 : 2;
  hipStream_t st = (hipStream_t)stream;
  const int CQ = (C + 3) / 4, R = ksize / 2, WP = orcai_padded_width(W, ksize);
  const int64_t plane = (int64_t)(H + 2 * R) * WP;
  if (plane >= (1ll << 29)) return ORCAI_E_UNSUPPORTED;
  const int tasks = (H * WP + 63) / 64;
  // workgroups per snippet: two (four-wave) / three-four (two-wave) workgroups per compute unit over the whole grid, at least ~16 windows per wave
  int gx = ((NWv == 4 ? 512 : 1024) + B - 1) / B;
  if (gx < 1) gx = 1;
  if (gx * NWv * 16 > tasks) gx = (tasks + NWv * 16 - 1) / (NWv * 16);
  while ((int64_t)gx * B * NWv * Cin * C > workspace_floats && gx > 1) --gx;
  if ((int64_t)gx * B * NWv * Cin * C > workspace_floats) return ORCAI_E_UNSUPPORTED;
  double* db = scratch2C;
  double* dg = scratch2C + 4 * CQ;
  if (!sums_ready) {
    hipError_t e = orcai_zero::zero_async(scratch2C, sizeof(double) * 8 * CQ, st);
    if (e != hipSuccess) return (int)e;
    int gs = (int)((B * plane + 255) / 256);
    if (gs > 128) gs = 128;
    hipLaunchKernelGGL(bn_planes_bwd_sums_kernel, dim3(gs, CQ), dim3(256), 0, st, dy, v, C, plane, B, mean, var, gamma, beta, eps, relu, db, dg);
  }
  const size_t lds = (size_t)NWv * (MTv + NTv) * 16 * 66 * sizeof(float);
  const float inv_count = (float)(1.0 / ((double)B * H * W));
  dim3 grid(gx, B);
  void *prof0 = nullptr, *prof1 = nullptr;
  orcai_profile_take(&prof0, &prof1);  // measurement hook (orcai_profile_bracket): events around the main kernel only
#define ORCAI_BBW(MT_, NT_, NW_)                                                                                                                       \
  {                                                                                                                                                    \
    if (const hipError_t e = orcai_lds::ensure_dynamic_lds<bn_bwd_pw_wgrad_kernel<MT_, NT_, NW_>>(lds); e != hipSuccess) return (int)e;                \
    if (prof0) (void)hipEventRecord((hipEvent_t)prof0, st);                                                                                                \
    hipLaunchKernelGGL((bn_bwd_pw_wgrad_kernel<MT_, NT_, NW_>), grid, dim3(64 * NW_), lds, st, dy, v, u, C, H, W, WP, R, mean, var, gamma, beta, eps, relu, db, \
                       dg, inv_count, wt, Cin, du, tasks, magic_for(WP), workspace);                                                                    \
    if (prof1) (void)hipEventRecord((hipEvent_t)prof1, st);                                                                                                \
  }
  const int key = MTv * 10 + NTv;
  switch (key) {
    case 11: ORCAI_BBW(1, 1, 4) break;
    case 12: ORCAI_BBW(1, 2, 4) break;
    case 21: ORCAI_BBW(2, 1, 4) break;
    case 22: ORCAI_BBW(2, 2, 4) break;
    case 13: ORCAI_BBW(1, 3, 4) break;
    case 31: ORCAI_BBW(3, 1, 4) break;
    case 23: ORCAI_BBW(2, 3, 2) break;
    case 32: ORCAI_BBW(3, 2, 2) break;
    case 33: ORCAI_BBW(3, 3, 2) break;
    case 14: ORCAI_BBW(1, 4, 2) break;
    case 24: ORCAI_BBW(2, 4, 2) break;
    default: return ORCAI_E_UNSUPPORTED;
  }
#undef ORCAI_BBW
  hipLaunchKernelGGL(add_partials_kernel, dim3(blocks_for((int64_t)Cin * C), 8), dim3(256), 0, st, workspace, gx * B * NWv, Cin * C, dWpw);
  hipLaunchKernelGGL(f64_to_f32_pair_kernel, dim3((C + 63) / 64), dim3(64), 0, st, db, dbeta, dg, dgamma, C);
  return (int)hipGetLastError();
}

static int pool_bwd_bn_impl(const float* dout, const float* ybn, int B, int C, int H, int W, int ksize, float* dy, const float* bn_gamma, const float* bn_mean,
                            const float* bn_var, float bn_eps, double* bn_sums, double* dout_sums, float* dbias, void* stream) {
  if (!dout || !ybn || !dy || B <= 0 || C <= 0 || C > 64 || H <= 0 || W <= 0) return ORCAI_E_BADARG;
  if (bn_sums && (!bn_gamma || !bn_mean || !bn_var)) return ORCAI_E_BADARG;
  if (dout_sums && (!bn_sums || !dbias)) return ORCAI_E_BADARG;
  if ((int64_t)B * ((C + 3) / 4) > 65535) return ORCAI_E_UNSUPPORTED;  // grid.y = (snippet, quad)
  const int Ho = (H + 1) / 2, Wo = (W + 1) / 2;
  int tot_h = (Ho - 1) * 2 + 3 - H, tot_w = (Wo - 1) * 2 + 2 - W;
  if (tot_h < 0) tot_h = 0;
  if (tot_w < 0) tot_w = 0;
  const int CQ = (C + 3) / 4;
  hipStream_t st = (hipStream_t)stream;
  if (bn_sums) {
    hipError_t e = orcai_zero::zero_async(bn_sums, sizeof(double) * 8 * CQ, st);
    if (e != hipSuccess) return (int)e;
  }
  if (dout_sums) {
    hipError_t e = orcai_zero::zero_async(dout_sums, sizeof(double) * 4 * CQ, st);
    if (e != hipSuccess) return (int)e;
  }
  const int per_bq = ((Ho + PB_ROWS - 1) / PB_ROWS) * Wo;
  dim3 grid((per_bq + 255) / 256, (unsigned)(B * CQ));
  hipLaunchKernelGGL(pool_bwd_kernel, grid, dim3(256), 0, st, dout, ybn, C, H, W, orcai_padded_width(W, ksize), ksize / 2, Ho, Wo,
                     orcai_padded_width(Wo, ksize), tot_h / 2, tot_w / 2, dy, B, bn_gamma, bn_mean, bn_var, bn_eps, bn_sums, dout_sums);
  if (dout_sums) hipLaunchKernelGGL(f64_to_f32_kernel, dim3((C + 63) / 64), dim3(64), 0, st, dout_sums, dbias, C, 0);
  return (int)hipGetLastError();
}

int orcai_pool_bwd_bn(const float* dout, const float* ybn, int B, int C, int H, int W, int ksize, float* dy, const float* bn_gamma, const float* bn_mean,
                      const float* bn_var, float bn_eps, double* bn_sums, void* stream) {
  return pool_bwd_bn_impl(dout, ybn, B, C, H, W, ksize, dy, bn_gamma, bn_mean, bn_var, bn_eps, bn_sums, nullptr, nullptr, stream);
}

int orcai_pool_bwd_bn_bias(const float* dout, const float* ybn, int B, int C, int H, int W, int ksize, float* dy, const float* bn_gamma, const float* bn_mean,
                           const float* bn_var, float bn_eps, double* bn_sums, double* dout_sums, float* dbias, void* stream) {
  if (!dout_sums || !dbias) return ORCAI_E_BADARG;
  return pool_bwd_bn_impl(dout, ybn, B, C, H, W, ksize, dy, bn_gamma, bn_mean, bn_var, bn_eps, bn_sums, dout_sums, dbias, stream);
}

int orcai_pool_bwd(const float* dout, const float* ybn, int B, int C, int H, int W, int ksize, float* dy, void* stream) {
  return orcai_pool_bwd_bn(dout, ybn, B, C, H, W, ksize, dy, nullptr, nullptr, nullptr, 0.0f, nullptr, stream);
}

int orcai_outer_reduce(const float* A, int Ca, const float* Bq, int Cb, int B, int H, int W, int ksize, int a_stride2, int Ha, int Wa, float* D,
                       float* workspace, int64_t workspace_floats, void* stream) {
  if (!A || !Bq || !D || !workspace || Ca <= 0 || Cb <= 0 || Ca > 64 || Cb > 64 || B <= 0 || H <= 0 || W <= 0) return ORCAI_E_BADARG;
  if (workspace_floats < (int64_t)Ca * Cb) return ORCAI_E_BADARG;
  if (a_stride2 && (Ha < 2 * H - 1 || Wa < 2 * W - 1)) return ORCAI_E_BADARG;  // A is sampled at (2i, 2j)
  const int WP = orcai_padded_width(W, ksize), R = ksize / 2;
  // dynamic LDS beyond the 64 KiB default (any operand wider than 32 channels) needs the opt-in below: a launch without it was the one
  // difference between the test shapes that ran and the one that aborted in round 1
  const int MTN = (Ca + 15) / 16 + (Cb + 15) / 16;
  // 256 pixels per pass while two workgroups fit a compute unit (<= 32 channels per operand: 66 KiB), 128 beyond (50-66 KiB instead
  // of 99-132)
  const int PP = MTN <= 4 ? 256 : 128;
  const size_t lds = (size_t)(MTN * 16) * (PP + 2) * sizeof(float);
  if (const hipError_t e = PP == 256 ? orcai_lds::ensure_dynamic_lds<outer_reduce_kernel<256>>(lds) : orcai_lds::ensure_dynamic_lds<outer_reduce_kernel<128>>(lds); e != hipSuccess)
    return (int)e;
  const int plane = (H + 2 * R) * WP;
  const int64_t nchunks = (int64_t)B * ((plane + PP - 1) / PP);
  const int64_t cap = PP == 256 ? 512 : 768;  // two / three workgroups per compute unit
  int64_t grid = nchunks < cap ? nchunks : cap;
  if (grid * Ca * Cb > workspace_floats) grid = workspace_floats / ((int64_t)Ca * Cb);
  if (grid < 1) return ORCAI_E_BADARG;
  hipStream_t st = (hipStream_t)stream;
  if (PP == 256)
    hipLaunchKernelGGL(outer_reduce_kernel<256>, dim3((unsigned)grid), dim3(256), lds, st, A, Ca, Bq, Cb, H, W, WP, R, B, a_stride2, Ha,
                       a_stride2 ? orcai_padded_width(Wa, ksize) : 0, workspace, magic_for(WP));
  else
    hipLaunchKernelGGL(outer_reduce_kernel<128>, dim3((unsigned)grid), dim3(256), lds, st, A, Ca, Bq, Cb, H, W, WP, R, B, a_stride2, Ha,
                       a_stride2 ? orcai_padded_width(Wa, ksize) : 0, workspace, magic_for(WP));
  hipLaunchKernelGGL(add_partials_kernel, dim3(blocks_for((int64_t)Ca * Cb), 8), dim3(256), 0, st, workspace, (int)grid, Ca * Cb, D);
  return (int)hipGetLastError();
}

static int g_dw_wgrad_march = 1;  // k = 3, planes at least 100 pixels wide: dw_wgrad_march_kernel (orcai_dw_wgrad_march: A/B)

int orcai_dw_wgrad_march(int on) {
  const int prev = g_dw_wgrad_march;
  if (on >= 0) g_dw_wgrad_march = on ? 1 : 0;
  return prev;
}

static int dw_wgrad_impl(const float* x, const float* du, int B, int C, int H, int W, int ksize_planes, int ktap, int relu_in, float* dW, const InBnW* bn, void* stream) {
  if (!x || !du || !dW || B <= 0 || B > 65535 || C <= 0 || H <= 0 || W <= 0 || ktap > ksize_planes) return ORCAI_E_BADARG;
  const int WP = orcai_padded_width(W, ksize_planes), RP = ksize_planes / 2;
  const int VAL = 64 - 2 * (ktap / 2);
  const int tasks = (H * WP + VAL - 1) / VAL;
  int tpw = (tasks + 7) / 8;  // 8 waves = 2 blocks per (snippet, quad): the wave / block reductions + atomics are paid once per block
  if (tpw < 8) tpw = 8;
  dim3 grid(((tasks + tpw - 1) / tpw + 3) / 4, (C + 3) / 4, B);
  hipStream_t st = (hipStream_t)stream;
  if (ktap == 3 && ksize_planes == 3 && g_dw_wgrad_march && W >= 100 && (int64_t)(H + 2) * WP < (1ll << 27)) {
    // wide planes (block 1 of orcai-V1): the marching kernel requests every byte once.  Strips of 62 columns; segments of rows so that the
    // grid has >= ~4 waves per SIMD over the chip
    const int nstrip = (W + 61) / 62;
    int nseg = (int)((16384 + (int64_t)B * ((C + 3) / 4) * nstrip - 1) / ((int64_t)B * ((C + 3) / 4) * nstrip));
    if (nseg < 1) nseg = 1;
    if (nseg > (H + 23) / 24) nseg = (H + 23) / 24;  // at least 24 rows per segment: two halo rows are re-read per segment
    int rps = (H + nseg - 1) / nseg;
    rps = (rps + 2) / 3 * 3;  // whole iterations of the loop unrolled by three
    nseg = (H + rps - 1) / rps;
    dim3 gridm((nstrip * nseg + 3) / 4, (C + 3) / 4, B);
    InBnW ib;
    if (bn) ib = *bn;
    if (bn) hipLaunchKernelGGL((dw_wgrad_march_kernel<true>), gridm, dim3(256), 0, st, x, du, C, H, W, WP, 0, dW, nstrip, nseg, rps, ib);
    else hipLaunchKernelGGL((dw_wgrad_march_kernel<false>), gridm, dim3(256), 0, st, x, du, C, H, W, WP, relu_in, dW, nstrip, nseg, rps, ib);
    return (int)hipGetLastError();
  }
  if (bn) {
    if (ktap != 3 || (int64_t)(H + 2 * RP) * WP >= (1ll << 29)) return ORCAI_E_UNSUPPORTED;
    InBnW ib = *bn;
    ib.magic_WP = magic_for(WP);
    hipLaunchKernelGGL((dw_wgrad_kernel<3, true>), grid, dim3(256), 0, st, x, du, C, H, W, WP, RP, 0, dW, tasks, tpw, ib);
    return (int)hipGetLastError();
  }
  switch (ktap) {
    case 3: hipLaunchKernelGGL(dw_wgrad_kernel<3>, grid, dim3(256), 0, st, x, du, C, H, W, WP, RP, relu_in, dW, tasks, tpw, InBnW{}); break;
    case 5: hipLaunchKernelGGL(dw_wgrad_kernel<5>, grid, dim3(256), 0, st, x, du, C, H, W, WP, RP, relu_in, dW, tasks, tpw, InBnW{}); break;
    case 7: hipLaunchKernelGGL(dw_wgrad_kernel<7>, grid, dim3(256), 0, st, x, du, C, H, W, WP, RP, relu_in, dW, tasks, tpw, InBnW{}); break;
    default: return ORCAI_E_UNSUPPORTED;
  }
  return (int)hipGetLastError();
}

int orcai_dw_wgrad(const float* x, const float* du, int B, int C, int H, int W, int ksize_planes, int ktap, int relu_in, float* dW, void* stream) {
  return dw_wgrad_impl(x, du, B, C, H, W, ksize_planes, ktap, relu_in, dW, nullptr, stream);
}

int orcai_dw_wgrad_bn(const float* v, const float* du, int B, int C, int H, int W, const float* in_mean, const float* in_var, const float* in_gamma, const float* in_beta,
                      float in_eps, float* dW, void* stream) {
  if (!in_mean || !in_var || !in_gamma || !in_beta) return ORCAI_E_BADARG;
  InBnW ib;
  ib.mean = in_mean; ib.var = in_var; ib.gamma = in_gamma; ib.beta = in_beta; ib.eps = in_eps;
  return dw_wgrad_impl(v, du, B, C, H, W, 3, 3, 0, dW, &ib, stream);
}

int orcai_dw_bwd_fused(const float* x, const float* du, int B, int C, int H, int W, int relu_in, const float* dw_rev, float* dr, float* dW, int epi, const float* bn_mean,
                       const float* bn_var, const float* bn_gamma, const float* bn_beta, float bn_eps, int bn_relu, double* shards, void* stream) {
  if (!x || !du || !dw_rev || !dr || !dW || B <= 0 || C <= 0 || H <= 0 || W <= 0 || (epi != 0 && epi != 2 && epi != 3)) return ORCAI_E_BADARG;
  const bool bn = bn_mean != nullptr;
  if (bn && (!bn_var || !bn_gamma || !bn_beta)) return ORCAI_E_BADARG;
  if (epi == 2 && (!bn || !shards)) return ORCAI_E_BADARG;
  if (epi == 3 && (bn || !relu_in)) return ORCAI_E_BADARG;  // the mask x > 0 is the ReLU in front of the conv
  const int WP = orcai_padded_width(W, 3), CQ = (C + 3) / 4;
  if (B > 65535 || CQ > 65535 || C > 64 || (int64_t)(H + 2) * WP >= (1ll << 27) || ((uintptr_t)x & 15) || ((uintptr_t)du & 15) || ((uintptr_t)dr & 15)) return ORCAI_E_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  InBnW ib;
  if (bn) { ib.mean = bn_mean; ib.var = bn_var; ib.gamma = bn_gamma; ib.beta = bn_beta; ib.eps = bn_eps; }
  if (epi == 2) {
    hipError_t e = orcai_zero::zero_async(shards, sizeof(double) * 8 * CQ * 32, st);
    if (e != hipSuccess) return (int)e;
  }
  // strip width: the one that idles the fewest lanes (ties: the widest -- fewer halo columns)
  int best = 64, best_lanes = ((W + 61) / 62) * 64;
  if (((W + 29) / 30) * 32 < best_lanes) { best = 32; best_lanes = ((W + 29) / 30) * 32; }
  if (((W + 13) / 14) * 16 < best_lanes) { best = 16; best_lanes = ((W + 13) / 14) * 16; }
  int rc;
  if (best == 64) rc = launch_dw_bwd<64>(st, x, du, B, C, H, W, WP, relu_in, dw_rev, dr, dW, epi, ib, bn_relu, shards, (W + 61) / 62);
  else if (best == 32) rc = launch_dw_bwd<32>(st, x, du, B, C, H, W, WP, relu_in, dw_rev, dr, dW, epi, ib, bn_relu, shards, (W + 29) / 30);
  else rc = launch_dw_bwd<16>(st, x, du, B, C, H, W, WP, relu_in, dw_rev, dr, dW, epi, ib, bn_relu, shards, (W + 13) / 14);
  if (rc != 0) return rc;
  if (epi == 2) hipLaunchKernelGGL(bwd_sums_compact_kernel, dim3(1), dim3(256), 0, st, shards, CQ);
  return (int)hipGetLastError();
}

static int g_conv0_march = 1;  // k = 3: the entry conv's statistics pass and the second pass of its backward on conv0_march_kernel (orcai_conv0_march: A/B)

int orcai_conv0_march(int on) {
  const int prev = g_conv0_march;
  if (on >= 0) g_conv0_march = on ? 1 : 0;
  return prev;
}

static void conv0_march_geometry(int B, int H, int W, int& nstrip, int& nseg, int& rps) {
  nstrip = (W + 61) / 62;
  const int64_t per_seg = (int64_t)B * 4 * nstrip;
  nseg = (int)((16384 + per_seg - 1) / per_seg);
  if (nseg < 1) nseg = 1;
  if (nseg > (H + 23) / 24) nseg = (H + 23) / 24;
  rps = (H + nseg - 1) / nseg;
  rps = (rps + 2) / 3 * 3;
  nseg = (H + rps - 1) / rps;
}

int orcai_conv0_stats_march(const float* in, int64_t snippet_stride, int B, int H, int W, const float* w, const float* scale, const float* shift, double* shards, void* stream) {
  if (!in || !w || !scale || !shift || !shards || B <= 0 || H <= 0 || W <= 0) return ORCAI_E_BADARG;
  if (B > 65535 || (int64_t)H * W >= (1ll << 30)) return ORCAI_E_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  hipError_t e = orcai_zero::zero_async(shards, sizeof(double) * 8 * 4 * 32, st);
  if (e != hipSuccess) return (int)e;
  int nstrip, nseg, rps;
  conv0_march_geometry(B, H, W, nstrip, nseg, rps);
  dim3 grid((nstrip * nseg + 3) / 4, 4, B);
  hipLaunchKernelGGL((conv0_march_kernel<0>), grid, dim3(256), 0, st, in, snippet_stride, H, W, orcai_padded_width(W, 3), w, scale, shift, shards, (const float*)nullptr,
                     (const float*)nullptr, (const float*)nullptr, (const float*)nullptr, (const float*)nullptr, 0.0f, (const double*)nullptr, (const double*)nullptr, 0.0f,
                     (float*)nullptr, nstrip, nseg, rps);
  return (int)hipGetLastError();
}

int orcai_dw_bwd_fused_conv0(const float* in, int64_t snippet_stride, const float* du, int B, int H, int W, const float* w0, const float* bias0, const float* dw_rev, float* dr,
                             float* dW, const float* bn_mean, const float* bn_var, const float* bn_gamma, const float* bn_beta, float bn_eps, double* shards, const float* resq,
                             void* stream) {
  if (!in || !du || !w0 || !bias0 || !dw_rev || !dr || !dW || !bn_mean || !bn_var || !bn_gamma || !bn_beta || !shards || B <= 0 || H <= 0 || W <= 0) return ORCAI_E_BADARG;
  const int C = 16, CQ = 4, WP = orcai_padded_width(W, 3);
  if (B > 65535 || (int64_t)(H + 2) * WP >= (1ll << 27) || (int64_t)H * W >= (1ll << 30) || ((uintptr_t)du & 15) || ((uintptr_t)dr & 15) || ((uintptr_t)resq & 15))
    return ORCAI_E_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  InBnW ib;
  ib.mean = bn_mean; ib.var = bn_var; ib.gamma = bn_gamma; ib.beta = bn_beta; ib.eps = bn_eps;
  Conv0In c0;
  c0.in = in; c0.snippet_stride = snippet_stride; c0.w0 = w0; c0.bias = bias0;
  c0.resq = resq; c0.Ho = (H + 1) / 2; c0.WPo = orcai_padded_width((W + 1) / 2, 3);
  hipError_t e = orcai_zero::zero_async(shards, sizeof(double) * 8 * CQ * 32, st);
  if (e != hipSuccess) return (int)e;
  int best = 64, best_lanes = ((W + 61) / 62) * 64;
  if (((W + 29) / 30) * 32 < best_lanes) { best = 32; best_lanes = ((W + 29) / 30) * 32; }
  if (((W + 13) / 14) * 16 < best_lanes) { best = 16; best_lanes = ((W + 13) / 14) * 16; }
  int rc;
  if (best == 64) rc = launch_dw_bwd<64>(st, nullptr, du, B, C, H, W, WP, 0, dw_rev, dr, dW, 2, ib, 1, shards, (W + 61) / 62, &c0);
  else if (best == 32) rc = launch_dw_bwd<32>(st, nullptr, du, B, C, H, W, WP, 0, dw_rev, dr, dW, 2, ib, 1, shards, (W + 29) / 30, &c0);
  else rc = launch_dw_bwd<16>(st, nullptr, du, B, C, H, W, WP, 0, dw_rev, dr, dW, 2, ib, 1, shards, (W + 13) / 14, &c0);
  if (rc != 0) return rc;
  hipLaunchKernelGGL(bwd_sums_compact_kernel, dim3(1), dim3(256), 0, st, shards, CQ);
  return (int)hipGetLastError();
}

int orcai_conv0_bn_bwd_x_ready(const float* in, int64_t snippet_stride, const float* dy, int B, int H, int W, int ksize, const float* w0, const float* bias, const float* mean,
                               const float* var, const float* gamma, const float* beta, float eps, double* scratch2C, float* dbeta, float* dgamma, float* dW, float* workspace,
                               int64_t workspace_floats, void* stream) {
  // orcai_conv0_bn_bwd_x whose first pass already happened: scratch2C holds bn0's backward sums dbeta[16] | dgamma[16] (orcai_dw_bwd_fused_conv0)
  if (!in || !dy || !w0 || !bias || !dW || !scratch2C || !dbeta || !dgamma || !workspace || B <= 0) return ORCAI_E_BADARG;
  if ((int64_t)H * W >= (1ll << 30)) return ORCAI_E_BADARG;
  hipStream_t st = (hipStream_t)stream;
  const int C = 16, R = ksize / 2, WP = orcai_padded_width(W, ksize), KK = ksize * ksize;
  const int64_t plane = (int64_t)(H + 2 * R) * WP;
  const int64_t ntiles = (int64_t)((W + 31) / 32) * ((H + 7) / 8) * B;
  if (plane >= (1ll << 31) || ntiles >= (1ll << 31)) return ORCAI_E_UNSUPPORTED;
  int gx = (int)(ntiles < 512 ? ntiles : 512);
  if ((int64_t)gx * KK * 16 > workspace_floats) gx = (int)(workspace_floats / (KK * 16));
  if (gx < 1) return ORCAI_E_BADARG;
  double* db = scratch2C;
  double* dg = scratch2C + 16;
  const float inv_count = (float)(1.0 / ((double)B * H * W));
  if (ksize == 3 && g_conv0_march && B <= 65535) {  // marching second pass: no tiles, no LDS, weight gradient straight into dW (36 atomics per workgroup)
    int nstrip, nseg, rps;
    conv0_march_geometry(B, H, W, nstrip, nseg, rps);
    dim3 gm((nstrip * nseg + 3) / 4, 4, B);
    hipLaunchKernelGGL((conv0_march_kernel<1>), gm, dim3(256), 0, st, in, snippet_stride, H, W, WP, w0, (const float*)nullptr, bias, (double*)nullptr, dy, mean, var, gamma, beta, eps,
                       (const double*)db, (const double*)dg, inv_count, dW, nstrip, nseg, rps);
    hipLaunchKernelGGL(f64_to_f32_pair_kernel, dim3(1), dim3(64), 0, st, db, dbeta, dg, dgamma, C);
    return (int)hipGetLastError();
  }
  dim3 grid(gx, 4);
#define ORCAI_C0XR(KS_)                                                                                                                                    \
  hipLaunchKernelGGL((conv0_bn_bwd_x_kernel<KS_, true>), grid, dim3(256), 0, st, in, snippet_stride, dy, H, W, WP, B, w0, bias, mean, var, gamma, beta, eps,  \
                     (double*)nullptr, db, dg, inv_count, workspace)
  switch (ksize) {
    case 3: ORCAI_C0XR(3); break;
    case 5: ORCAI_C0XR(5); break;
    case 7: ORCAI_C0XR(7); break;
    default: return ORCAI_E_UNSUPPORTED;
  }
#undef ORCAI_C0XR
  hipLaunchKernelGGL(add_partials_kernel, dim3(blocks_for(KK * 16), 8), dim3(256), 0, st, workspace, gx, KK * 16, dW);
  hipLaunchKernelGGL(f64_to_f32_pair_kernel, dim3(1), dim3(64), 0, st, db, dbeta, dg, dgamma, C);
  return (int)hipGetLastError();
}

int orcai_conv0_wgrad(const float* in, int64_t snippet_stride, const float* dv, int B, int H, int W, int ksize, float* dW, void* stream) {
  if (!in || !dv || !dW || B <= 0) return ORCAI_E_BADARG;
  const int WP = orcai_padded_width(W, ksize);
  if ((int64_t)H * W >= (1ll << 30)) return ORCAI_E_BADARG;
  dim3 grid(256, 4);
  hipStream_t st = (hipStream_t)stream;
  switch (ksize) {
    case 3: hipLaunchKernelGGL(conv0_wgrad_kernel<3>, grid, dim3(256), 0, st, in, snippet_stride, dv, H, W, WP, B, dW); break;
    case 5: hipLaunchKernelGGL(conv0_wgrad_kernel<5>, grid, dim3(256), 0, st, in, snippet_stride, dv, H, W, WP, B, dW); break;
    case 7: hipLaunchKernelGGL(conv0_wgrad_kernel<7>, grid, dim3(256), 0, st, in, snippet_stride, dv, H, W, WP, B, dW); break;
    default: return ORCAI_E_UNSUPPORTED;
  }
  return (int)hipGetLastError();
}

int orcai_conv0_bn_bwd(const float* in, int64_t snippet_stride, const float* dy, const float* v, int B, int H, int W, int ksize, const float* mean,
                       const float* var, const float* gamma, const float* beta, float eps, double* scratch2C, float* dbeta, float* dgamma, float* dW,
                       void* stream) {
  if (!in || !dy || !v || !dW || !scratch2C || !dbeta || !dgamma || B <= 0) return ORCAI_E_BADARG;
  if ((int64_t)H * W >= (1ll << 30)) return ORCAI_E_BADARG;
  hipStream_t st = (hipStream_t)stream;
  const int C = 16, CQ = 4, R = ksize / 2, WP = orcai_padded_width(W, ksize);
  const int64_t plane = (int64_t)(H + 2 * R) * WP;
  if (plane >= (1ll << 31)) return ORCAI_E_UNSUPPORTED;
  hipError_t e = orcai_zero::zero_async(scratch2C, sizeof(double) * 8 * CQ, st);
  if (e != hipSuccess) return (int)e;
  int gx = (int)((B * plane + 255) / 256);
  if (gx > 128) gx = 128;
  double* db = scratch2C;
  double* dg = scratch2C + 4 * CQ;
  hipLaunchKernelGGL(bn_planes_bwd_sums_kernel, dim3(gx, CQ), dim3(256), 0, st, dy, v, C, plane, B, mean, var, gamma, beta, eps, 1, db, dg);
  const float inv_count = (float)(1.0 / ((double)B * H * W));
  dim3 grid(256, 4);
  switch (ksize) {
    case 3: hipLaunchKernelGGL(conv0_bn_wgrad_kernel<3>, grid, dim3(256), 0, st, in, snippet_stride, dy, v, H, W, WP, B, mean, var, gamma, beta, eps, db, dg, inv_count, dW); break;
    case 5: hipLaunchKernelGGL(conv0_bn_wgrad_kernel<5>, grid, dim3(256), 0, st, in, snippet_stride, dy, v, H, W, WP, B, mean, var, gamma, beta, eps, db, dg, inv_count, dW); break;
    case 7: hipLaunchKernelGGL(conv0_bn_wgrad_kernel<7>, grid, dim3(256), 0, st, in, snippet_stride, dy, v, H, W, WP, B, mean, var, gamma, beta, eps, db, dg, inv_count, dW); break;
    default: return ORCAI_E_UNSUPPORTED;
  }
  hipLaunchKernelGGL(f64_to_f32_pair_kernel, dim3(1), dim3(64), 0, st, db, dbeta, dg, dgamma, C);
  return (int)hipGetLastError();
}

int orcai_conv0_bn_bwd_x(const float* in, int64_t snippet_stride, const float* dy, int B, int H, int W, int ksize, const float* w0, const float* bias, const float* mean,
                         const float* var, const float* gamma, const float* beta, float eps, double* scratch2C, float* dbeta, float* dgamma, float* dW, float* workspace,
                         int64_t workspace_floats, void* stream) {
  if (!in || !dy || !w0 || !bias || !dW || !scratch2C || !dbeta || !dgamma || !workspace || B <= 0) return ORCAI_E_BADARG;
  if ((int64_t)H * W >= (1ll << 30)) return ORCAI_E_BADARG;
  hipStream_t st = (hipStream_t)stream;
  const int C = 16, R = ksize / 2, WP = orcai_padded_width(W, ksize), KK = ksize * ksize;
  const int64_t plane = (int64_t)(H + 2 * R) * WP;
  const int64_t ntiles = (int64_t)((W + 31) / 32) * ((H + 7) / 8) * B;
  if (plane >= (1ll << 31) || ntiles >= (1ll << 31)) return ORCAI_E_UNSUPPORTED;
  int gx = (int)(ntiles < 512 ? ntiles : 512);  // x 4 quads: eight workgroups per compute unit
  if ((int64_t)gx * KK * 16 > workspace_floats) gx = (int)(workspace_floats / (KK * 16));
  if (gx < 1) return ORCAI_E_BADARG;
  hipError_t e = orcai_zero::zero_async(scratch2C, sizeof(double) * 8 * 4 * 32, st);  // 32 accumulator copies
  if (e != hipSuccess) return (int)e;
  double* db = scratch2C;
  double* dg = scratch2C + 16;
  const float inv_count = (float)(1.0 / ((double)B * H * W));
  dim3 grid(gx, 4);
#define ORCAI_C0X(KS_)                                                                                                                                     \
  hipLaunchKernelGGL((conv0_bn_bwd_x_kernel<KS_, false>), grid, dim3(256), 0, st, in, snippet_stride, dy, H, W, WP, B, w0, bias, mean, var, gamma, beta, eps, scratch2C, \
                     (const double*)nullptr, (const double*)nullptr, inv_count, (float*)nullptr);                                                           \
  hipLaunchKernelGGL(conv0_sums_compact_kernel, dim3(1), dim3(32), 0, st, scratch2C);                                                                       \
  hipLaunchKernelGGL((conv0_bn_bwd_x_kernel<KS_, true>), grid, dim3(256), 0, st, in, snippet_stride, dy, H, W, WP, B, w0, bias, mean, var, gamma, beta, eps,  \
                     (double*)nullptr, db, dg, inv_count, workspace)
  switch (ksize) {
    case 3: ORCAI_C0X(3); break;
    case 5: ORCAI_C0X(5); break;
    case 7: ORCAI_C0X(7); break;
    default: return ORCAI_E_UNSUPPORTED;
  }
#undef ORCAI_C0X
  hipLaunchKernelGGL(add_partials_kernel, dim3(blocks_for(KK * 16), 8), dim3(256), 0, st, workspace, gx, KK * 16, dW);
  hipLaunchKernelGGL(f64_to_f32_pair_kernel, dim3(1), dim3(64), 0, st, db, dbeta, dg, dgamma, C);
  return (int)hipGetLastError();
}

int orcai_conv0_bn_bwd_dx(const float* in, int64_t snippet_stride, const float* dy, int B, int H, int W, int ksize, const float* w0, const float* bias, const float* mean,
                          const float* var, const float* gamma, const float* beta, float eps, const double* sums2C, float* dx, void* stream) {
  if (!in || !dy || !w0 || !bias || !mean || !var || !gamma || !beta || !sums2C || !dx || B <= 0 || H <= 0 || W <= 0) return ORCAI_E_BADARG;
  if (ksize != 3 && ksize != 5 && ksize != 7) return ORCAI_E_BADARG;
  if ((uintptr_t)dy & 15) return ORCAI_E_BADARG;
  const int R = ksize / 2, WP = orcai_padded_width(W, ksize);
  const int64_t plane = (int64_t)(H + 2 * R) * WP;
  const int64_t ntiles = (int64_t)((W + 31) / 32) * ((H + 7) / 8) * B;
  if ((int64_t)H * W >= (1ll << 30) || plane >= (1ll << 27) || ntiles >= (1ll << 31)) return ORCAI_E_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  const float inv_count = (float)(1.0 / ((double)B * H * W));
  if (ksize == 3 && B <= 65535) {
    // segments of rows: enough waves to fill the device (each segment forms two dv rows beyond its own, so not shorter than 16 rows)
    const int nstrip = (W + 61) / 62;
    const int64_t cols = (int64_t)B * nstrip;
    int nseg = (int)((8192 + cols - 1) / cols);
    if (nseg > (H + 15) / 16) nseg = (H + 15) / 16;
    if (nseg < 1) nseg = 1;
    const int rps = (H + nseg - 1) / nseg;
    nseg = (H + rps - 1) / rps;
    dim3 grid((nstrip * nseg + 3) / 4, 1, B);
    hipLaunchKernelGGL(conv0_dx_march_kernel, grid, dim3(256), 0, st, in, snippet_stride, dy, H, W, WP, w0, bias, mean, var, gamma, beta, eps, sums2C, inv_count, dx, nstrip, nseg,
                       rps);
    return (int)hipGetLastError();
  }
  const int tx = (W + 31) / 32, ty = (H + 7) / 8;
#define ORCAI_C0DX(KS_)                                                                                                                                          \
  hipLaunchKernelGGL(conv0_dx_tile_kernel<KS_>, dim3((unsigned)ntiles), dim3(256), 0, st, in, snippet_stride, dy, H, W, WP, w0, bias, mean, var, gamma, beta, eps, sums2C, \
                     inv_count, dx, tx, ty)
  switch (ksize) {
    case 3: ORCAI_C0DX(3); break;
    case 5: ORCAI_C0DX(5); break;
    default: ORCAI_C0DX(7); break;
  }
#undef ORCAI_C0DX
  return (int)hipGetLastError();
}

int orcai_pack_weights(const float* w, const int* desc, int n_desc, float* out, void* stream) {
  if (!w || !desc || !out || n_desc <= 0) return ORCAI_E_BADARG;
  hipLaunchKernelGGL(pack_weights_kernel, dim3(n_desc), dim3(256), 0, (hipStream_t)stream, w, desc, out);
  return (int)hipGetLastError();
}

int orcai_feat_to_planes(const float* f, int B, int C, int H, int W, int ksize, float* out, void* stream) {
  if (!f || !out || B <= 0 || C <= 0) return ORCAI_E_BADARG;
  const int64_t n = (int64_t)B * ((C + 3) / 4) * H * W;
  hipLaunchKernelGGL(feat_to_planes_kernel, dim3(blocks_for(n)), dim3(256), 0, (hipStream_t)stream, f, C, H, W, orcai_padded_width(W, ksize), ksize / 2, out, B);
  return (int)hipGetLastError();
}

int orcai_planes_relu_bwd(const float* dy, const float* y, int64_t n_floats, float* dx, void* stream) {
  if (!dy || !y || !dx || n_floats <= 0 || (n_floats & 3)) return ORCAI_E_BADARG;
  hipLaunchKernelGGL(relu_bwd4_kernel, dim3(blocks_for(n_floats / 4)), dim3(256), 0, (hipStream_t)stream, (const float4*)dy, (const float4*)y, n_floats / 4,
                     (float4*)dx);
  return (int)hipGetLastError();
}

}  // extern "C"
