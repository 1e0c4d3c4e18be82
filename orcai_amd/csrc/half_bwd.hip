// half_bwd.hip -- training on the f16 path (BASELINE configs[4]): batch-statistics BatchNorm and the backward kernels of the
// convolutional trunk on f16 channel-octet planes (half_planes.h).  Activations AND activation gradients are stored in f16 (the
// gradients carry a static loss scale, orcai_masked_bce_w / orcai_adam_step's gscale); every reduction -- BatchNorm sums, weight
// gradients -- accumulates in f32 / f64 and lands in the f32 gradient buffer of the f32 master weights.
// Same decomposition as train_trunk.hip (reference: architectures.py:162-206; train.py:201-219 computes these inside Keras).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "half_planes.h"
#include "lds_optin.h"
#include "orcai_hip.h"
#include "zero_fill.h"

namespace {

// Sum of v over the 64 lanes, delivered in lane 63: four row_shr steps inside each row of 16 lanes, then row_bcast:15 / row_bcast:31 carry the row totals
// across rows -- six v_add_f32 with a DPP operand instead of six ds_bpermute + six adds per value (a marching wave reduces 88 accumulators when it ends).
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



using namespace orcai_half;

inline unsigned blocks_for(int64_t n) { return (unsigned)((n + 255) / 256); }

struct O8 {
  float v[8];
};
__device__ __forceinline__ O8 ld8(const h16* base, int64_t idx) {
  O8 o;
  unpack8(reinterpret_cast<const h16x8*>(base)[idx], o.v);
  return o;
}
__device__ __forceinline__ void st8(h16* base, int64_t idx, const O8& o) { reinterpret_cast<h16x8*>(base)[idx] = pack8(o.v); }

// block reduction of 8 doubles per thread (256 threads) -> thread 0..7 hold the totals in red[0][k]
__device__ __forceinline__ void block_reduce8(double (&red)[256][8], const double (&val)[8]) {
#pragma unroll
  for (int k = 0; k < 8; ++k) red[threadIdx.x][k] = val[k];
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o)
#pragma unroll
      for (int k = 0; k < 8; ++k) red[threadIdx.x][k] += red[threadIdx.x + o][k];
    __syncthreads();
  }
}

// ---------------------------------------------------------------- per-channel sums over planes (pads are zero: no masks)
__global__ __launch_bounds__(256) void planes_sums_h_kernel(const h16* __restrict__ x, int CO, int64_t plane, int B, double* __restrict__ sums,
                                                             double* __restrict__ sumsq) {
  __shared__ double red[256][8];
  const int co = blockIdx.y;
  double s[8] = {0, 0, 0, 0, 0, 0, 0, 0}, q[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  const int p0 = blockIdx.x * 256 + threadIdx.x, pstep = gridDim.x * 256;
  for (int b = B - 1; b >= 0; --b) {  // last snippet first: the tail of what the preceding kernel wrote may still be in the Infinity Cache
    const int64_t base = ((int64_t)b * CO + co) * plane;
    for (int p = p0; p < (int)plane; p += pstep) {
      const O8 v = ld8(x, base + p);
#pragma unroll
      for (int k = 0; k < 8; ++k) { s[k] += v.v[k]; q[k] += (double)v.v[k] * v.v[k]; }
    }
  }
  block_reduce8(red, s);
  if (threadIdx.x < 8) atomicAdd(&sums[co * 8 + threadIdx.x], red[0][threadIdx.x]);
  __syncthreads();
  if (sumsq) {
    block_reduce8(red, q);
    if (threadIdx.x < 8) atomicAdd(&sumsq[co * 8 + threadIdx.x], red[0][threadIdx.x]);
  }
}

// small planes: one workgroup per 4096 consecutive pixels of a (snippet, octet) plane, totals to one of SUM_SHARDS accumulator copies
// (see planes_sums_sharded_kernel of train_trunk.hip)
constexpr int SUM_SHARDS = 32;
__global__ __launch_bounds__(256) void planes_sums_sharded_h_kernel(const h16* __restrict__ x, int CO, int plane, int nchunk, double* __restrict__ shards /*[SUM_SHARDS][CO][16]*/) {
  __shared__ double red[4][16];
  const int co = blockIdx.y, b = blockIdx.x / nchunk, chunk = blockIdx.x - b * nchunk;
  const int64_t base = ((int64_t)b * CO + co) * plane;
  double t[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) t[k] = 0.0;
  const int p0 = chunk * 4096 + threadIdx.x;
#pragma unroll
  for (int it = 0; it < 4; ++it) {
    h16x8 v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int p = p0 + (it * 4 + u) * 256;
      v[u] = reinterpret_cast<const h16x8*>(x)[base + (p < plane ? p : plane - 1)];
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (p0 + (it * 4 + u) * 256 < plane) {
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const float f = (float)v[u][k];
          t[k] += f;
          t[8 + k] += (double)f * f;
        }
      }
  }
#pragma unroll
  for (int k = 0; k < 16; ++k)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) t[k] += __shfl_xor(t[k], o, 64);
  if ((threadIdx.x & 63) == 0)
#pragma unroll
    for (int k = 0; k < 16; ++k) red[threadIdx.x >> 6][k] = t[k];
  __syncthreads();
  if (threadIdx.x < 16)
    atomicAdd(&shards[((int64_t)(blockIdx.x % SUM_SHARDS) * CO + co) * 16 + threadIdx.x],
              red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x]);
}

__global__ void bn_finish_stats_sharded_h_kernel(const double* __restrict__ shards, int C, int CO, double count, float* __restrict__ mean, float* __restrict__ var) {
  const int c = blockIdx.x * 64 + threadIdx.x;
  if (c >= C) return;
  double su = 0.0, sq = 0.0;
  for (int sh = 0; sh < SUM_SHARDS; ++sh) {
    su += shards[((int64_t)sh * CO + (c >> 3)) * 16 + (c & 7)];
    sq += shards[((int64_t)sh * CO + (c >> 3)) * 16 + 8 + (c & 7)];
  }
  const double mu = su / count;
  const double v = sq / count - mu * mu;
  mean[c] = (float)mu;
  var[c] = (float)(v < 0.0 ? 0.0 : v);
}

__global__ void bn_finish_stats_h_kernel(const double* __restrict__ sums, const double* __restrict__ sumsq, int C, double count, float* __restrict__ mean,
                                         float* __restrict__ var) {
  const int c = blockIdx.x * 64 + threadIdx.x;
  if (c >= C) return;
  const double mu = sums[c] / count;
  const double v = sumsq[c] / count - mu * mu;
  mean[c] = (float)mu;
  var[c] = (float)(v < 0.0 ? 0.0 : v);
}

__global__ void f64_to_f32_h_kernel(const double* __restrict__ a, float* __restrict__ b, int n, int accumulate) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i < n) b[i] = accumulate ? b[i] + (float)a[i] : (float)a[i];
}
// the two BatchNorm parameter gradients (d beta, d gamma) in one launch
__global__ void f64_to_f32_pair_h_kernel(const double* __restrict__ a0, float* __restrict__ b0, const double* __restrict__ a1, float* __restrict__ b1, int n) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i < n) {
    b0[i] = (float)a0[i];
    b1[i] = (float)a1[i];
  }
}

// y = [relu](v * s + t) at interior pixels; pads of y stay zero
__global__ __launch_bounds__(256) void bn_planes_apply_h_kernel(const h16* __restrict__ v, int C, int H, int W, int WP, int R, const float* __restrict__ mean,
                                                                 const float* __restrict__ var, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                 float eps, int relu, h16* __restrict__ y) {
  const int CO = (C + 7) >> 3;
  const int pix = blockIdx.x * 256 + threadIdx.x;
  if (pix >= H * W) return;
  const int bq = blockIdx.y, co = bq % CO;
  const int yy = pix / W, xx = pix - yy * W;
  const int64_t off = (int64_t)bq * ((int64_t)(H + 2 * R) * WP) + (int64_t)(yy + R) * WP + xx;
  const O8 a = ld8(v, off);
  O8 o;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int c = co * 8 + k;
    if (c < C) {
      const float s = gamma[c] * rsqrtf(var[c] + eps);
      const float r = fmaf(a.v[k], s, beta[c] - mean[c] * s);
      o.v[k] = relu ? fmaxf(r, 0.0f) : r;
    } else {
      o.v[k] = 0.0f;
    }
  }
  st8(y, off, o);
}

// BN backward sums over planes: dbeta[c] += sum dy_eff, dgamma[c] += sum dy_eff * xhat   (dy_eff = relu ? dy * (BN(v) > 0) : dy)
__global__ __launch_bounds__(256) void bn_planes_bwd_sums_h_kernel(const h16* __restrict__ dy, const h16* __restrict__ v, int C, int64_t plane, int B,
                                                                    const float* __restrict__ mean, const float* __restrict__ var, const float* __restrict__ gamma,
                                                                    const float* __restrict__ beta, float eps, int relu, double* __restrict__ dbeta,
                                                                    double* __restrict__ dgamma) {
  __shared__ double red[256][8];
  const int co = blockIdx.y, CO = (C + 7) >> 3;
  float mu[8], inv[8], g[8], bt[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int c = co * 8 + k, cc = c < C ? c : 0;
    mu[k] = mean[cc]; inv[k] = rsqrtf(var[cc] + eps); g[k] = gamma[cc]; bt[k] = beta[cc];
  }
  double s[8] = {0, 0, 0, 0, 0, 0, 0, 0}, q[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  const int p0 = blockIdx.x * 256 + threadIdx.x, pstep = gridDim.x * 256;
  for (int b = B - 1; b >= 0; --b) {  // last snippet first: the tail of what the preceding kernel wrote may still be in the Infinity Cache
    const int64_t base = ((int64_t)b * CO + co) * plane;
    for (int p = p0; p < (int)plane; p += pstep) {
      const O8 d = ld8(dy, base + p), vv = ld8(v, base + p);
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const float xh = (vv.v[k] - mu[k]) * inv[k];
        float de = d.v[k];
        if (relu && !(fmaf(xh, g[k], bt[k]) > 0.0f)) de = 0.0f;
        s[k] += (double)de;
        q[k] += (double)de * (double)xh;
      }
    }
  }
  block_reduce8(red, s);
  if (threadIdx.x < 8 && co * 8 + threadIdx.x < C) atomicAdd(&dbeta[co * 8 + threadIdx.x], red[0][threadIdx.x]);
  __syncthreads();
  block_reduce8(red, q);
  if (threadIdx.x < 8 && co * 8 + threadIdx.x < C) atomicAdd(&dgamma[co * 8 + threadIdx.x], red[0][threadIdx.x]);
}

// ---------------------------------------------------------------- BN backward apply fused with the transposed pointwise conv
// The per-channel constants of a BatchNorm backward, once per workgroup in LDS: tab[c] = {mean, inv = rsqrt(var + eps), gamma, beta | A = gamma inv,
// c1 = dbeta / N, c2 = dgamma / N, 0} (zeros for c >= C: dv = 0 there).  Formed inside the pixel loop they are wave-uniform arithmetic the compiler
// spreads over scalar loads, double -> float conversions and v_rsq on the vector ALU: a quarter of the fused weight-gradient kernel's 1 000 vector
// instructions per 256-pixel pass (profiles/r04_pmc_issue_hps.json: VALU issuing on 81 % of SIMD cycles).  Two broadcast 16-byte LDS reads per channel instead.
template <class Row0, class Row1>
__device__ __forceinline__ void fill_bn_bwd_table(Row0 row0, Row1 row1, int Cpad, int C, const float* __restrict__ mean, const float* __restrict__ var,
                                                  const float* __restrict__ gamma, const float* __restrict__ beta, float eps, const double* __restrict__ dbeta,
                                                  const double* __restrict__ dgamma, float inv_count, int tid, int nthreads) {
  for (int c = tid; c < Cpad; c += nthreads) {
    float4 k0 = make_float4(0.f, 0.f, 0.f, 0.f), k1 = k0;
    if (c < C) {
      const float inv = rsqrtf(var[c] + eps);
      k0 = make_float4(mean[c], inv, gamma[c], beta[c]);
      k1 = make_float4(gamma[c] * inv, (float)dbeta[c] * inv_count, (float)dgamma[c] * inv_count, 0.0f);
    }
    *row0(c) = k0;
    *row1(c) = k1;
  }
}
// dv of one channel value from the table row (the arithmetic of the original in-loop form, operation for operation)
__device__ __forceinline__ float bn_bwd_value(const float4* __restrict__ r0, const float4* __restrict__ r1, float vv, float dd, int relu, bool live) {
  const float4 k0 = *r0, k1 = *r1;
  const float xh = (vv - k0.x) * k0.y;
  float de = dd;
  if (relu && !(fmaf(xh, k0.z, k0.w) > 0.0f)) de = 0.0f;
  return live ? k1.x * (de - k1.y - xh * k1.z) : 0.0f;
}

// dv = gamma*inv*(dy_eff - dbeta/N - xhat*dgamma/N) (stored, f16) AND du = Wpw dv in one pass: one wave = 64 consecutive flat pixels.
// wtf: A fragments of the TRANSPOSED pointwise weights, [KG of the conv-OUTPUT channels][MT of the conv-INPUT channels][64][8].
template <int MT>
__global__ __launch_bounds__(256) void bn_bwd_pw_h_kernel(const h16* dy, const h16* __restrict__ v, int C, int H, int W, int WP, int R,
                                                           const float* __restrict__ mean, const float* __restrict__ var, const float* __restrict__ gamma,
                                                           const float* __restrict__ beta, float eps, int relu, const double* __restrict__ dbeta,
                                                           const double* __restrict__ dgamma, float inv_count, const h16* __restrict__ wtf, int Cin,
                                                           h16* dv /*may alias dy*/, h16* __restrict__ du, int tasks, uint32_t magic_WP) {
  __shared__ __attribute__((aligned(16))) float bnk[64 * 8];  // BatchNorm backward constants of the <= 64 channels (fill_bn_bwd_table)
  const int lane = threadIdx.x & 63;
  const int task = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int CO = (C + 7) >> 3, COi = (Cin + 7) >> 3, KG = (CO + 3) >> 2;
  auto bn0 = [&](int c) { return reinterpret_cast<float4*>(bnk + c * 8); };
  auto bn1 = [&](int c) { return reinterpret_cast<float4*>(bnk + c * 8 + 4); };
  fill_bn_bwd_table(bn0, bn1, CO * 8, C, mean, var, gamma, beta, eps, dbeta, dgamma, inv_count, threadIdx.x, 256);
  __syncthreads();
  if (task >= tasks) return;
  const int b = blockIdx.y;
  const int lk = lane >> 4, lj = lane & 15;
  const int plane = (H + 2 * R) * WP;
  const int qbase = R * WP + task * 64;
  const int q = qbase + lane;
  const int row = (int)__umulhi((uint32_t)q, magic_WP);
  const bool live = (q - row * WP) < W && row < R + H;
  const int qc = q < plane ? q : plane - 1;
  const int64_t base = (int64_t)b * CO * plane + qc;
  f32x4 acc[MT][4];
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[m][t] = (f32x4){0.f, 0.f, 0.f, 0.f};
  for (int kg = 0; kg < KG; ++kg) {
    u32x4 d[4];
#pragma unroll
    for (int oo = 0; oo < 4; ++oo) {
      const int o = kg * 4 + oo;
      if (o < CO) {  // wave-uniform
        const O8 dd = ld8(dy, base + (int64_t)o * plane), vv = ld8(v, base + (int64_t)o * plane);
        O8 r;
#pragma unroll
        for (int k = 0; k < 8; ++k) r.v[k] = bn_bwd_value(bn0(o * 8 + k), bn1(o * 8 + k), vv.v[k], dd.v[k], relu, live);
        const h16x8 packed = pack8(r.v);
        if (live) reinterpret_cast<h16x8*>(dv)[base + (int64_t)o * plane] = packed;
        d[oo] = as_u(packed);
      } else {
        d[oo] = (u32x4){0u, 0u, 0u, 0u};
      }
    }
    octets_to_fragments(d);
#pragma unroll
    for (int m = 0; m < MT; ++m) {
      const h16x8 a = reinterpret_cast<const h16x8*>(wtf)[(kg * MT + m) * 64 + lane];
#pragma unroll
      for (int t = 0; t < 4; ++t) acc[m][t] = mfma_h(a, as_h(d[t]), acc[m][t]);
    }
  }
#pragma unroll
  for (int tp = 0; tp < 4; tp += 2) {
    const int flat = qbase + 16 * (tp + (lk & 1)) + lj;
    const int r2 = (int)__umulhi((uint32_t)flat, magic_WP);
    const bool ok = (flat - r2 * WP) < W && r2 < R + H;
#pragma unroll
    for (int m = 0; m < MT; ++m) {
      float a[4], bq[4], o8[8];
#pragma unroll
      for (int r = 0; r < 4; ++r) { a[r] = acc[m][tp][r]; bq[r] = acc[m][tp + 1][r]; }
      tiles_to_octet(a, bq, o8);
      const int oq = 2 * m + (lk >> 1);
      if (ok && oq < COi) reinterpret_cast<h16x8*>(du)[((int64_t)b * COi + oq) * plane + flat] = pack8(o8);
    }
  }
}

// ---------------------------------------------------------------- max-pool backward (row-marching; see pool_bwd_kernel of train_trunk.hip)
constexpr int PB_ROWS = 8;

__device__ __forceinline__ O8 o8_fill(float x) {
  O8 o;
#pragma unroll
  for (int k = 0; k < 8; ++k) o.v[k] = x;
  return o;
}

__global__ __launch_bounds__(256) void pool_bwd_h_kernel(const h16* __restrict__ dout, const h16* __restrict__ ybn, int C, int H, int W, int WP, int R, int Ho, int Wo,
                                                          int WPo, int pad_top, int pad_left, h16* __restrict__ dy, const float* __restrict__ bn_gamma,
                                                          const float* __restrict__ bn_mean, const float* __restrict__ bn_var, float bn_eps,
                                                          double* __restrict__ bn_sums /*[2][8*CO]*/,
                                                          double* __restrict__ dout_sums = nullptr /*[8*CO]: sum of dout per channel (the residual conv's bias gradient)*/) {
  const int CO = (C + 7) >> 3;
  const int nchunk = (Ho + PB_ROWS - 1) / PB_ROWS;
  const int idx = blockIdx.x * 256 + threadIdx.x;
  const bool in_range = idx < nchunk * Wo;
  const int j = in_range ? idx % Wo : 0;
  const int chunk = in_range ? idx / Wo : 0;
  const int64_t bq = blockIdx.y;
  const int co = (int)(bq % CO);
  float bs[8], bqs[8], bmu[8], binv[8], sgn[8];
  float ds[8];  // dout_sums: every pooled pixel belongs to exactly one thread's OWN windows (i0 <= i < i1)
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int c = co * 8 + k, cc = c < C ? c : 0;
    bs[k] = 0.f; bqs[k] = 0.f; ds[k] = 0.f;
    bmu[k] = bn_sums ? bn_mean[cc] : 0.f;
    binv[k] = bn_sums ? rsqrtf(bn_var[cc] + bn_eps) : 0.f;
    sgn[k] = (bn_gamma && bn_gamma[cc] < 0.f) ? -1.f : 1.f;
  }
  const int64_t pin = bq * ((int64_t)(H + 2 * R) * WP), pout = bq * ((int64_t)(Ho + 2 * R) * WPo);
  const int x0 = 2 * j - pad_left, x1 = x0 + 1;
  const bool cx0 = x0 >= 0 && x0 < W, cx1 = x1 < W;
  auto ld = [&](int y, int x, bool cx) -> O8 {
    if (!(cx && y >= 0 && y < H)) return o8_fill(-INFINITY);
    O8 t = ld8(ybn, pin + (int64_t)(y + R) * WP + x);
#pragma unroll
    for (int k = 0; k < 8; ++k) t.v[k] *= sgn[k];
    return t;
  };
  auto mx8 = [](const O8& a, const O8& b) { O8 o;
#pragma unroll
    for (int k = 0; k < 8; ++k) o.v[k] = fmaxf(a.v[k], b.v[k]);
    return o; };
  auto add8 = [](const O8& a, const O8& b) { O8 o;
#pragma unroll
    for (int k = 0; k < 8; ++k) o.v[k] = a.v[k] + b.v[k];
    return o; };
  auto emit = [&](int64_t pos, const O8& g, const O8& tv) {
    // the gradient is STORED in f16: the BatchNorm sums must see the same rounded values the consumer will read
    const h16x8 gh = pack8(g.v);
    reinterpret_cast<h16x8*>(dy)[pin + pos] = gh;
    if (bn_sums) {
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const float gg = (float)gh[k];
        bs[k] += gg;
        bqs[k] = fmaf(gg, (tv.v[k] * sgn[k] - bmu[k]) * binv[k], bqs[k]);
      }
    }
  };
  const int i0 = chunk * PB_ROWS, i1 = in_range ? ((i0 + PB_ROWS < Ho) ? i0 + PB_ROWS : Ho) : i0;
  const int istart = i0 > 0 ? i0 - 1 : 0;
  O8 t0 = ld(2 * istart - pad_top, x0, cx0), t1 = ld(2 * istart - pad_top, x1, cx1);
  O8 c0 = o8_fill(0.f), c1 = o8_fill(0.f);
  // the five loads of a window are unconditional (clamped coordinates, masked after arrival) and requested one window ahead, kept
  // packed (4 registers each) until they are used -- as in the f32 kernel
  const int xc0 = x0 < 0 ? 0 : (x0 >= W ? W - 1 : x0), xc1 = x1 >= W ? W - 1 : x1;
  h16x8 raw[4], dn;
  auto request = [&](int i) {
    const int r0 = 2 * i - pad_top;
#pragma unroll
    for (int a = 0; a < 2; ++a) {
      int y = r0 + 1 + a;
      y = y < 0 ? 0 : (y >= H ? H - 1 : y);
      raw[2 * a] = reinterpret_cast<const h16x8*>(ybn)[pin + (int64_t)(y + R) * WP + xc0];
      raw[2 * a + 1] = reinterpret_cast<const h16x8*>(ybn)[pin + (int64_t)(y + R) * WP + xc1];
    }
    dn = reinterpret_cast<const h16x8*>(dout)[pout + (int64_t)((i < Ho ? i : Ho - 1) + R) * WPo + j];
  };
  auto masked = [&](h16x8 t, int y, bool cx) -> O8 {
    O8 o;
    unpack8(t, o.v);
    const bool ok = cx && y >= 0 && y < H;
#pragma unroll
    for (int k = 0; k < 8; ++k) o.v[k] = ok ? o.v[k] * sgn[k] : -INFINITY;
    return o;
  };
  if (istart < i1) request(istart);
  for (int i = istart; i < i1; ++i) {
    const int r0 = 2 * i - pad_top;
    const O8 m0 = masked(raw[0], r0 + 1, cx0), m1 = masked(raw[1], r0 + 1, cx1);
    const O8 b0 = masked(raw[2], r0 + 2, cx0), b1 = masked(raw[3], r0 + 2, cx1);
    O8 d;
    unpack8(dn, d.v);
    if (i + 1 < i1) request(i + 1);
    const O8 m = mx8(mx8(mx8(t0, t1), mx8(m0, m1)), mx8(b0, b1));
    // first maximal position in scan order takes the window's gradient (pool_bwd_kernel of train_trunk.hip): f16 values tie often
    O8 g6[6];
    {
      const O8* v[6] = {&t0, &t1, &m0, &m1, &b0, &b1};
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        bool taken = false;
#pragma unroll
        for (int p = 0; p < 6; ++p) {
          const bool hit = v[p]->v[k] == m.v[k];
          g6[p].v[k] = (hit && !taken) ? d.v[k] : 0.f;
          taken = taken || hit;
        }
      }
    }
    if (i >= i0) {
      if (dout_sums) {
#pragma unroll
        for (int k = 0; k < 8; ++k) ds[k] += d.v[k];
      }
      if (r0 >= 0) {
        if (cx0) emit((int64_t)(r0 + R) * WP + x0, add8(c0, g6[0]), t0);
        if (cx1) emit((int64_t)(r0 + R) * WP + x1, add8(c1, g6[1]), t1);
      }
      if (r0 + 1 < H) {
        if (cx0) emit((int64_t)(r0 + 1 + R) * WP + x0, g6[2], m0);
        if (cx1) emit((int64_t)(r0 + 1 + R) * WP + x1, g6[3], m1);
      }
    }
    c0 = g6[4];
    c1 = g6[5];
    t0 = b0;
    t1 = b1;
  }
  const int rl = 2 * i1 - pad_top;
  if (in_range && i1 == Ho && rl < H) {
    if (cx0) emit((int64_t)(rl + R) * WP + x0, c0, t0);
    if (cx1) emit((int64_t)(rl + R) * WP + x1, c1, t1);
  }
  if (bn_sums) {  // workgroup reduction (float64): DPP sums inside each wave, the four waves through 768 bytes of LDS, 16 (+ 8) atomics per workgroup
    __shared__ double red[4][24];
#pragma unroll
    for (int k = 0; k < 24; ++k) {
      const double v = wave_sum_lane63((double)(k < 8 ? bs[k & 7] : (k < 16 ? bqs[k & 7] : ds[k & 7])));
      if ((threadIdx.x & 63) == 63) red[threadIdx.x >> 6][k] = v;
    }
    __syncthreads();
    if (threadIdx.x < 24) {
      const int k = threadIdx.x & 7;
      const double tot = (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
      if (co * 8 + k < C) {
        if (threadIdx.x < 16) atomicAdd(&bn_sums[(threadIdx.x >> 3) * 8 * CO + co * 8 + k], tot);
        else if (dout_sums) atomicAdd(&dout_sums[co * 8 + k], tot);
      }
    }
  }
}

// ---------------------------------------------------------------- D[ca][cb] += sum_pixels A[ca][p] * Bq[cb][p]   (pointwise / residual weight gradients)
// The contraction index is the PIXEL, but a 16-byte vector of the planes holds 8 channels of one pixel.  256 pixels per pass are staged
// in LDS exactly as they arrive -- image [pixel][channel], one ds_write_b128 per octet -- and the MFMA operands are fetched with the
// hardware transposing read ds_read_b64_tr_b16: a 16-lane group reads a block of 4 pixels x 16 channels and lane i receives channel
// i's four pixels, so two reads give a lane the 8 consecutive pixels of one channel that v_mfma_f32_16x16x32_f16 wants with k = pixel
// (the first version wrote the image transposed with eight 2-byte stores per octet: 1.15 ms per step for the 13 launches).
// Row pitch = 16-byte multiple (16 channels per tile row + one 16-byte pad).  Per-workgroup partial products + an add kernel.
typedef short v4s __attribute__((__vector_size__(4 * sizeof(short))));

__device__ __forceinline__ h16x8 tr_fragment(const h16* img, int pitch_h, int pix0, int col0, int lj) {
  // block rows = pixels pix0 + {0..3} and pix0 + 4 + {0..3}, columns col0 .. col0 + 15; lane 4q + p of the group addresses row q, columns 4p..4p+3
  const h16* a = img + (pix0 + (lj >> 2)) * pitch_h + col0 + 4 * (lj & 3);
  const v4s lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) v4s*)a);
  const v4s hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) v4s*)(a + 4 * pitch_h));
  typedef short v8s __attribute__((__vector_size__(8 * sizeof(short))));
  const v8s both = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
  return __builtin_bit_cast(h16x8, both);
}

__global__ __launch_bounds__(256) void outer_reduce_h_kernel(const h16* __restrict__ A, int Ca, const h16* __restrict__ Bq, int Cb, int H, int W, int WP, int R, int B,
                                                              int a_mode, int Ha, int WPa, float* __restrict__ part, uint32_t magic_WP) {
  extern __shared__ __attribute__((aligned(16))) h16 smem_h[];
  const int COa = (Ca + 7) >> 3, COb = (Cb + 7) >> 3;
  const int MT = (Ca + 15) >> 4, NT = (Cb + 15) >> 4, ntile = MT * NT;
  const int pa_h = MT * 16 + 8, pb_h = NT * 16 + 8;  // row pitches in halves (16-byte multiples)
  h16* As = smem_h;                 // [256 pixels][pa_h]
  h16* Bs = smem_h + 256 * pa_h;    // [256 pixels][pb_h]
  for (int i = threadIdx.x; i < 256 * (pa_h + pb_h) / 2; i += 256) reinterpret_cast<uint32_t*>(smem_h)[i] = 0u;  // channel columns past C stay zero
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lk = lane >> 4, lj = lane & 15;
  const int plane = (H + 2 * R) * WP;
  const int64_t plane_a = a_mode ? (int64_t)(Ha + 2 * R) * WPa : plane;
  f32x4 acc[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) acc[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
  const int chunks_per_plane = (plane + 255) >> 8;
  const int64_t nchunks = (int64_t)B * chunks_per_plane;
  // the next pass's octets are requested into registers before this pass's MFMA phase (as the f32 kernel does): without it every
  // pass exposed one full memory latency between its two barriers
  constexpr int MAXO = 8;  // up to 64 channels per operand
  h16x8 ra[MAXO], rb[MAXO];
  auto fetch = [&](int64_t ch) {
    const int64_t b = ch / chunks_per_plane;
    const int p = (int)(ch - b * chunks_per_plane) * 256 + tid;
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
    for (int q = 0; q < MAXO; ++q) {
      ra[q] = (q < COa && ain) ? reinterpret_cast<const h16x8*>(A)[((int64_t)b * COa + q) * plane_a + pa] : zero_h();
      rb[q] = (q < COb && pin) ? reinterpret_cast<const h16x8*>(Bq)[((int64_t)b * COb + q) * plane + p] : zero_h();
    }
  };
  fetch(blockIdx.x);
  for (int64_t ch = blockIdx.x; ch < nchunks; ch += gridDim.x) {
    __syncthreads();  // the previous pass's MFMA reads are done (and the zero fill is visible)
#pragma unroll
    for (int q = 0; q < MAXO; ++q) {
      if (q < COa) *reinterpret_cast<h16x8*>(As + tid * pa_h + 8 * q) = ra[q];
      if (q < COb) *reinterpret_cast<h16x8*>(Bs + tid * pb_h + 8 * q) = rb[q];
    }
    __syncthreads();
    fetch(ch + gridDim.x);  // in flight during the MFMA phase
#pragma unroll
    for (int ti = 0; ti < 4; ++ti) {
      const int tile = wave + 4 * ti;
      if (tile < ntile) {  // wave-uniform: EXEC stays all ones inside, as the transposing read requires
        const int mt = tile / NT, nt = tile - mt * NT;
        f32x4 c0 = acc[ti];
#pragma unroll
        for (int s = 0; s < 8; ++s)  // A[row = ca][k = pixel 32 s + 8 lk + e], B[k = the same pixel][col = cb]
          c0 = mfma_h(tr_fragment(As, pa_h, 32 * s + 8 * lk, 16 * mt, lj), tr_fragment(Bs, pb_h, 32 * s + 8 * lk, 16 * nt, lj), c0);
        acc[ti] = c0;
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

// ---------------------------------------------------------------- BN backward apply + du = Wpw dv + POINTWISE WEIGHT GRADIENT u (x) dv in one pass
// The f16 twin of bn_bwd_pw_wgrad_kernel (train_trunk.hip): bn_bwd_pw_h_kernel's arithmetic for dv and du, and outer_reduce_h_kernel's contraction
// over pixels for dW[ci][co] += sum_p u[ci][p] dv[co][p] -- dv is formed per pixel, rounded to f16 exactly as the two-launch path stores it, used for
// both products and NEVER written: one write and one read of the widest gradient tensor of the conv are gone, and the separate orcai_h_outer_reduce
// launch with them.  A workgroup of 4 waves owns 256 consecutive flat pixels per pass (lane = pixel for the BatchNorm arithmetic and the du MFMAs, as
// bn_bwd_pw_h_kernel); the pass's u and dv octets go through one LDS image [pixel][channel] and come back through the transposing read
// ds_read_b64_tr_b16 as MFMA operands with k = pixel, wave w taking output tile w (<= 2 x 2 tiles of 16 channels: orcai-V1's block 1 in all three
// hyper-parameter-search widths); the next pass's 16-byte loads are in flight in registers during the MFMA phase.  Per-workgroup partial products +
// add_partials_h_kernel.
template <int MT /*conv-INPUT tiles: rows of du and of dW*/, int NT /*conv-OUTPUT tiles: columns of dW*/>
// (256, 4): at most 128 registers -- without the hint the compiler took 152 of the 256 a 256-thread workgroup may have, which is three waves per SIMD where the
// 40 KB of LDS allow four: 0.46 -> 0.40 ms on block 1 (30 -> 30); same-box A/B of the same hint on ten other kernels of the step: none moved by more than its noise
// (tools/ab_so.sh; the marching depthwise backward and the f16 pooling backward would spill)
__global__ __launch_bounds__(256, 4) void bn_bwd_pw_wgrad_h_kernel(const h16* __restrict__ dy, const h16* __restrict__ v, const h16* __restrict__ u, int C, int H, int W, int WP, int R,
                                                                 int B, const float* __restrict__ mean, const float* __restrict__ var, const float* __restrict__ gamma,
                                                                 const float* __restrict__ beta, float eps, int relu, const double* __restrict__ dbeta,
                                                                 const double* __restrict__ dgamma, float inv_count, const h16* __restrict__ wtf, int Cin,
                                                                 h16* __restrict__ du, float* __restrict__ part, uint32_t magic_WP) {
  static_assert(MT <= 2 && NT <= 2, "one output tile per wave");
  constexpr int pa_h = MT * 16 + 8, pb_h = NT * 16 + 8;  // row pitches in halves (16-byte multiples; the extra 16 bytes spread the rows over the banks)
  constexpr int COA = MT * 2, COB = NT * 2;             // octets per operand (channels past Cin / C are zero)
  __shared__ __attribute__((aligned(16))) h16 As[256 * pa_h];  // u  [pixel][conv-input channel]
  __shared__ __attribute__((aligned(16))) h16 Bs[256 * pb_h];  // dv [pixel][conv-output channel]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lk = lane >> 4, lj = lane & 15;
  const int CO = (C + 7) >> 3, COi = (Cin + 7) >> 3;
  const int plane = (H + 2 * R) * WP;
  for (int i = tid; i < 256 * pa_h / 2; i += 256) reinterpret_cast<uint32_t*>(As)[i] = 0u;
  for (int i = tid; i < 256 * pb_h / 2; i += 256) reinterpret_cast<uint32_t*>(Bs)[i] = 0u;
  // BatchNorm backward constants of conv-output channel c live in the 16 padding bytes of row c of the two images (the passes write halves [0, 16 MT) and
  // [0, 16 NT) of a row only): a table of its own would be the 33rd LDS granule of a workgroup that fits a compute unit exactly four times at 32
  static_assert(NT * 16 <= 256, "one image row per channel");
  auto bn0 = [&](int c) { return reinterpret_cast<float4*>(As + c * pa_h + MT * 16); };
  auto bn1 = [&](int c) { return reinterpret_cast<float4*>(Bs + c * pb_h + NT * 16); };
  __syncthreads();  // the zero fill is done
  fill_bn_bwd_table(bn0, bn1, NT * 16, C, mean, var, gamma, beta, eps, dbeta, dgamma, inv_count, tid, 256);
  __syncthreads();
  const int chunks_per_plane = (H * WP + 255) >> 8;  // 256-pixel chunks covering the H image rows of a plane (start at row R)
  const int64_t nchunks = (int64_t)B * chunks_per_plane;
  f32x4 wacc = (f32x4){0.f, 0.f, 0.f, 0.f};  // this wave's tile of dW: tile index = wave (< MT * NT)
  h16x8 rdy[COB], rv[COB], ru[COA];
  auto fetch = [&](int64_t ch) {
    const int64_t b = ch / chunks_per_plane;
    const int q = R * WP + (int)(ch - b * chunks_per_plane) * 256 + tid;
    const bool pin = ch < nchunks && q < plane;
    const int qc = pin ? q : 0;
#pragma unroll
    for (int o = 0; o < COB; ++o) {
      rdy[o] = (o < CO && pin) ? reinterpret_cast<const h16x8*>(dy)[((int64_t)b * CO + o) * plane + qc] : zero_h();
      rv[o] = (o < CO && pin) ? reinterpret_cast<const h16x8*>(v)[((int64_t)b * CO + o) * plane + qc] : zero_h();
    }
#pragma unroll
    for (int o = 0; o < COA; ++o) ru[o] = (o < COi && pin) ? reinterpret_cast<const h16x8*>(u)[((int64_t)b * COi + o) * plane + qc] : zero_h();
  };
  fetch(blockIdx.x);
  for (int64_t ch = blockIdx.x; ch < nchunks; ch += gridDim.x) {
    const int64_t b = ch / chunks_per_plane;
    const int qbase = R * WP + (int)(ch - b * chunks_per_plane) * 256 + wave * 64;  // this wave's 64-pixel window
    const int q = qbase + lane;
    const int row = (int)__umulhi((uint32_t)q, magic_WP);
    const bool live = q < plane && (q - row * WP) < W && row < R + H;
    // ---- dv per pixel (bn_bwd_pw_h_kernel's arithmetic, rounded to f16 as the two-launch path stores it)
    u32x4 d[4];
    h16x8 dvo[COB];
#pragma unroll
    for (int o = 0; o < 4; ++o) {
      if (o < COB && o < CO) {
        float dd[8], vv[8], r[8];
        unpack8(rdy[o], dd);
        unpack8(rv[o], vv);
#pragma unroll
        for (int k = 0; k < 8; ++k) r[k] = bn_bwd_value(bn0(o * 8 + k), bn1(o * 8 + k), vv[k], dd[k], relu, live);
        dvo[o < COB ? o : 0] = pack8(r);
        d[o] = as_u(dvo[o < COB ? o : 0]);
      } else {
        if (o < COB) dvo[o] = zero_h();
        d[o] = (u32x4){0u, 0u, 0u, 0u};
      }
    }
    __syncthreads();  // the previous pass's transposing reads are done (and, first pass, the zero fill is visible)
#pragma unroll
    for (int o = 0; o < COB; ++o) *reinterpret_cast<h16x8*>(Bs + tid * pb_h + 8 * o) = dvo[o];
#pragma unroll
    for (int o = 0; o < COA; ++o) *reinterpret_cast<h16x8*>(As + tid * pa_h + 8 * o) = ru[o];
    __syncthreads();
    fetch(ch + gridDim.x);  // the next pass's loads: in flight during both MFMA phases
    // ---- du = Wpw dv: one K group of 4 octets (C <= 32)
    {
      f32x4 acc[MT][4];
#pragma unroll
      for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[m][t] = (f32x4){0.f, 0.f, 0.f, 0.f};
      octets_to_fragments(d);
#pragma unroll
      for (int m = 0; m < MT; ++m) {
        const h16x8 a = reinterpret_cast<const h16x8*>(wtf)[m * 64 + lane];
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[m][t] = mfma_h(a, as_h(d[t]), acc[m][t]);
      }
#pragma unroll
      for (int tp = 0; tp < 4; tp += 2) {
        const int flat = qbase + 16 * (tp + (lk & 1)) + lj;
        const int r2 = (int)__umulhi((uint32_t)flat, magic_WP);
        const bool ok = flat < plane && (flat - r2 * WP) < W && r2 < R + H;
#pragma unroll
        for (int m = 0; m < MT; ++m) {
          float a[4], bq[4], o8[8];
#pragma unroll
          for (int r = 0; r < 4; ++r) { a[r] = acc[m][tp][r]; bq[r] = acc[m][tp + 1][r]; }
          tiles_to_octet(a, bq, o8);
          const int oq = 2 * m + (lk >> 1);
          if (ok && oq < COi) reinterpret_cast<h16x8*>(du)[((int64_t)b * COi + oq) * plane + flat] = pack8(o8);
        }
      }
    }
    // ---- dW tile of this wave over the pass's 256 pixels: A[row = ci][k = pixel], B[k = pixel][col = co]
    if (wave < MT * NT) {  // wave-uniform: EXEC stays all ones inside, as the transposing read requires
      const int mt = wave / NT, nt = wave - mt * NT;
#pragma unroll
      for (int s8 = 0; s8 < 8; ++s8)
        wacc = mfma_h(tr_fragment(As, pa_h, 32 * s8 + 8 * lk, 16 * mt, lj), tr_fragment(Bs, pb_h, 32 * s8 + 8 * lk, 16 * nt, lj), wacc);
    }
  }
  if (wave < MT * NT) {
    float* mine = part + (int64_t)blockIdx.x * Cin * C;
    const int mt = wave / NT, nt = wave - mt * NT;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int ca = mt * 16 + lk * 4 + r, cb = nt * 16 + lj;
      if (ca < Cin && cb < C) mine[ca * C + cb] = wacc[r];
    }
  }
}

__global__ __launch_bounds__(256) void add_partials_h_kernel(const float* __restrict__ part, int nparts, int n, float* __restrict__ D) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int per = (nparts + gridDim.y - 1) / gridDim.y;
  const int k0 = blockIdx.y * per, k1 = (k0 + per < nparts) ? k0 + per : nparts;
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;  // four loads in flight per thread (as add_partials_kernel of the f32 path)
  int k = k0;
  for (; k + 3 < k1; k += 4) {
    s0 += part[(int64_t)k * n + i]; s1 += part[(int64_t)(k + 1) * n + i]; s2 += part[(int64_t)(k + 2) * n + i]; s3 += part[(int64_t)(k + 3) * n + i];
  }
  for (; k < k1; ++k) s0 += part[(int64_t)k * n + i];
  if (k1 > k0) atomicAdd(&D[i], (s0 + s1) + (s2 + s3));
}

// ---------------------------------------------------------------- depthwise weight gradient
// dW[tap][c] += sum_p r[c][p + off(tap)] * du[c][p], r = relu_in ? relu(x) : x.  One block handles ONE HALF of an octet (4 channels:
// 4 x k x k f32 accumulators per lane), one wave = 64-pixel windows, lanes R..63-R contribute; wave + block reduction, then atomics.
template <int SH>
__device__ __forceinline__ float lshf(float v) {
  return __uint_as_float(lane_shift_u<SH>(__float_as_uint(v)));
}

// NCH channels of the octet per block: 8 for k = 3 (72 accumulators per lane), 4 for k = 5, 7 (one block per half octet: 100 / 196).
template <int KS, int NCH>
__global__ __launch_bounds__(256) void dw_wgrad_h_kernel(const h16* __restrict__ x, const h16* __restrict__ du, int C, int H, int W, int WP, int RP, int relu_in,
                                                          float* __restrict__ dW /*[KS*KS][C]*/, int tasks, int tasks_per_wave) {
  constexpr int R = KS / 2, VAL = 64 - 2 * R, KK = KS * KS, PARTS = 8 / NCH;
  const int lane = threadIdx.x & 63;
  const int wv = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int co = blockIdx.y / PARTS, c0 = (blockIdx.y % PARTS) * NCH, b = blockIdx.z;
  const int CO = (C + 7) >> 3;
  const int plane = (H + 2 * RP) * WP;
  const int64_t base = ((int64_t)b * CO + co) * plane;
  float acc[NCH][KK];
#pragma unroll
  for (int j = 0; j < NCH; ++j)
#pragma unroll
    for (int t = 0; t < KK; ++t) acc[j][t] = 0.0f;
  const bool contributes = lane >= R && lane < 64 - R;
  // k = 3: the next window's four loads are requested before the current window's products (unconditional, clamped; the gradient of
  // a non-contributing lane is zeroed afterwards): two windows in flight per wave, as in the f32 kernel
  constexpr bool AHEAD = KS == 3;
  const int task0 = wv * tasks_per_wave, task_end = min((wv + 1) * tasks_per_wave, tasks);
  h16x8 gn, an[KS];
  auto request = [&](int task) {
    const int q = RP * WP + task * VAL - R + lane;
    gn = reinterpret_cast<const h16x8*>(du)[base + (q < plane ? q : plane - 1)];
#pragma unroll
    for (int dy = 0; dy < KS; ++dy) {
      int i = q + (dy - R) * WP;
      i = i < 0 ? 0 : (i >= plane ? plane - 1 : i);
      an[dy] = reinterpret_cast<const h16x8*>(x)[base + i];
    }
  };
  if (AHEAD && task0 < task_end) request(task0);
  for (int task = task0; task < task_end; ++task) {
    const int q = RP * WP + task * VAL - R + lane;
    const bool live = contributes && q < plane;
    if (!AHEAD) request(task);
    float g[NCH];
#pragma unroll
    for (int j = 0; j < NCH; ++j) g[j] = live ? (float)gn[c0 + j] : 0.f;
    h16x8 ac[KS];
#pragma unroll
    for (int dy = 0; dy < KS; ++dy) ac[dy] = an[dy];
    if (AHEAD && task + 1 < task_end) request(task + 1);
#pragma unroll
    for (int dy = 0; dy < KS; ++dy) {
      h16x8 a8 = ac[dy];
      if (relu_in) a8 = relu_h(a8);
#pragma unroll
      for (int j = 0; j < NCH; ++j) {
        const float a = (float)a8[c0 + j];
        if constexpr (KS == 3) {
          acc[j][dy * 3 + 0] = fmaf(lshf<-1>(a), g[j], acc[j][dy * 3 + 0]);
          acc[j][dy * 3 + 1] = fmaf(a, g[j], acc[j][dy * 3 + 1]);
          acc[j][dy * 3 + 2] = fmaf(lshf<1>(a), g[j], acc[j][dy * 3 + 2]);
        } else if constexpr (KS == 5) {
          acc[j][dy * 5 + 0] = fmaf(lshf<-2>(a), g[j], acc[j][dy * 5 + 0]);
          acc[j][dy * 5 + 1] = fmaf(lshf<-1>(a), g[j], acc[j][dy * 5 + 1]);
          acc[j][dy * 5 + 2] = fmaf(a, g[j], acc[j][dy * 5 + 2]);
          acc[j][dy * 5 + 3] = fmaf(lshf<1>(a), g[j], acc[j][dy * 5 + 3]);
          acc[j][dy * 5 + 4] = fmaf(lshf<2>(a), g[j], acc[j][dy * 5 + 4]);
        } else {
          acc[j][dy * 7 + 0] = fmaf(lshf<-3>(a), g[j], acc[j][dy * 7 + 0]);
          acc[j][dy * 7 + 1] = fmaf(lshf<-2>(a), g[j], acc[j][dy * 7 + 1]);
          acc[j][dy * 7 + 2] = fmaf(lshf<-1>(a), g[j], acc[j][dy * 7 + 2]);
          acc[j][dy * 7 + 3] = fmaf(a, g[j], acc[j][dy * 7 + 3]);
          acc[j][dy * 7 + 4] = fmaf(lshf<1>(a), g[j], acc[j][dy * 7 + 4]);
          acc[j][dy * 7 + 5] = fmaf(lshf<2>(a), g[j], acc[j][dy * 7 + 5]);
          acc[j][dy * 7 + 6] = fmaf(lshf<3>(a), g[j], acc[j][dy * 7 + 6]);
        }
      }
    }
  }
  __shared__ float red[4][NCH * KK];
#pragma unroll
  for (int j = 0; j < NCH; ++j)
#pragma unroll
    for (int t = 0; t < KK; ++t) {
      const float v = wave_sum_lane63(acc[j][t]);
      if (lane == 63) red[threadIdx.x >> 6][j * KK + t] = v;
    }
  __syncthreads();
  if (threadIdx.x < NCH * KK) {
    const int j = threadIdx.x / KK, t = threadIdx.x - j * KK;
    const int c = co * 8 + c0 + j;
    if (c < C) atomicAdd(&dW[t * C + c], red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x]);
  }
}

// ---------------------------------------------------------------- depthwise backward in ONE marching pass (k = 3), f16 octet planes
// The f16 twin of train_trunk.hip's dw_bwd_march_kernel: the input gradient dr = du (*) reversed taps (what orcai_h_sepconv computes with the
// identity pointwise factor: packed-f16 products, f16 output), its epilogue extra (EPI 2: backward sums of the BatchNorm whose pre-normalisation
// tensor is x, f32 terms; EPI 3: ReLU mask x > 0 -- the separate orcai_h_planes_relu_bwd pass) and the depthwise weight gradient (f32 accumulators,
// the products of orcai_h_dw_wgrad) from ONE pass over (du, x): a wave marches down a column strip of one channel OCTET with the three du rows and
// their two shifted copies in registers (packed f16), a step loads one du row and one x row, three steps ahead, and stores one dr row.
// BNIN: x is the pre-normalisation tensor v; y = f16(relu(fma(v, s, t))) is formed on load -- the value bn_planes_apply_h_kernel stored -- so the
// materialised y_a is not read by the backward pass at all.
// (struct InBnH: half_planes.h)

// acc = fma(f32(half HI ? upper : lower of d), y, acc)
__device__ __forceinline__ void mixacc(int hi, float& acc, uint32_t d, float y) {  // hi: a constant after unrolling
  if (hi) asm("v_fma_mix_f32 %0, %1, %2, %0 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "+v"(acc) : "v"(d), "v"(y));
  else asm("v_fma_mix_f32 %0, %1, %2, %0 op_sel:[0,0,0] op_sel_hi:[1,0,0]" : "+v"(acc) : "v"(d), "v"(y));
}

// RES: a gradient that lives on the even pixels only (the block's strided 1x1 residual branch, as compact planes [B][CO][Ho + 2][WPo][8] at the
// pooled resolution) is added to dr inside the pass, before the sums and the store -- instead of a scatter-add pass over dr afterwards, which for
// block 1 would also come too late for bn0's sums (EPI 2 with x = the entry conv's stored v0).
template <int SW, int EPI, bool BNIN, bool RES = false>
__global__ __launch_bounds__(256) void dw_bwd_march_h_kernel(const h16* __restrict__ x, const h16* __restrict__ du, int C, int H, int W, int WP, int relu_in,
                                                              const h16* __restrict__ wrev /*[CO][9][8] reversed taps*/, h16* __restrict__ dr,
                                                              float* __restrict__ dW /*[9][C]*/, double* __restrict__ shards /*EPI 2: [32][CO][16]*/, int nstrip,
                                                              int nseg, int rps, InBnH ib, int epi_relu, const h16* __restrict__ resq = nullptr, int Ho = 0, int WPo = 0) {
  static_assert(SW == 64 || SW == 32 || SW == 16, "strip lanes");
  static_assert(EPI == 0 || EPI == 2 || EPI == 3, "epilogue extras");
  static_assert(EPI != 2 || BNIN, "EPI 2: x is the pre-normalisation tensor of the BatchNorm whose backward sums are taken");
  constexpr int KK = 9, NSUB = 64 / SW;
  const int lane = threadIdx.x & 63, sl = lane % SW, sub = lane / SW;
  const int co = blockIdx.y, b = blockIdx.z;
  const int CO = (C + 7) >> 3;
  const int plane = (H + 2) * WP;
  const int64_t pbase = ((int64_t)b * CO + co) * plane;
  const h16x8* xp = reinterpret_cast<const h16x8*>(x) + pbase;
  const h16x8* dp = reinterpret_cast<const h16x8*>(du) + pbase;
  h16x8* op = reinterpret_cast<h16x8*>(dr) + pbase;
  const int task = (blockIdx.x * 4 + (threadIdx.x >> 6)) * NSUB + sub;
  const bool has_task = task < nstrip * nseg;
  const int strip = has_task ? task % nstrip : 0, seg = has_task ? task / nstrip : 0;
  const int xcol = strip * (SW - 2) - 1 + sl;
  const bool out_lane = has_task && sl >= 1 && sl <= SW - 2 && xcol < W;
  const int r_begin = seg * rps, r_end = min(r_begin + rps, H);
  float acc[8][KK];
#pragma unroll
  for (int j = 0; j < 8; ++j)
#pragma unroll
    for (int t = 0; t < KK; ++t) acc[j][t] = 0.0f;
  float s1[8], s2[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) s1[j] = s2[j] = 0.0f;
  h16x8 wt[KK];  // wave-uniform
#pragma unroll
  for (int t = 0; t < KK; ++t) wt[t] = *reinterpret_cast<const h16x8*>(wrev + ((int64_t)co * KK + t) * 8);
  float bsc[8], bsh[8], bmu[8], binv[8], bgm[8], bbt[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) bsc[j] = bsh[j] = bmu[j] = binv[j] = bgm[j] = bbt[j] = 0.0f;
  if (BNIN) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int c = co * 8 + j;
      if (c < C) {
        binv[j] = rsqrtf(ib.var[c] + ib.eps);
        bmu[j] = ib.mean[c]; bgm[j] = ib.gamma[c]; bbt[j] = ib.beta[c];
        bsc[j] = bgm[j] * binv[j];  // bn_planes_apply_h_kernel's arithmetic
        bsh[j] = bbt[j] - bmu[j] * bsc[j];
      }
    }
  }
  struct Row { h16x8 c, l, r; };
  auto pix = [&](int row) -> int {
    const int i = (row + 1) * WP + xcol;
    return i < 0 ? 0 : (i >= plane ? plane - 1 : i);
  };
  auto arrive = [&](const h16x8& raw, Row& o) {
    o.c = raw;
    o.l = lane_shift_h<-1>(raw);
    o.r = lane_shift_h<1>(raw);
  };
  h16x8 radd = zero_h();  // RES: the even-pixel gradient at this lane's pixel for the current step (zero off the even pixels)
  auto step = [&](const Row& up, const Row& mid, const Row& dn, const h16x8& x8, int row) {
    const bool live = out_lane && row < r_end;
    // input gradient: nine packed products per dword, f16 (the arithmetic class of dw_octet)
    h16x8 a = up.l * wt[0];
    a = up.c * wt[1] + a; a = up.r * wt[2] + a;
    a = mid.l * wt[3] + a; a = mid.c * wt[4] + a; a = mid.r * wt[5] + a;
    a = dn.l * wt[6] + a; a = dn.c * wt[7] + a; a = dn.r * wt[8] + a;
    if (RES) a = a + radd;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float xv = (float)x8[j];
      float y;
      if (BNIN) y = (float)(h16)fmaxf(fmaf(xv, bsc[j], bsh[j]), 0.0f);  // the f16 value the forward pass stored as y
      else y = relu_in ? fmaxf(xv, 0.0f) : xv;
      y = live ? y : 0.0f;
      // acc += f32(du half) * y as ONE v_fma_mix_f32 reading the half out of the packed row register (written as asm: the compiler otherwise
      // keeps f32 copies of all nine shifted rows alive across the three steps that use a row -- 72 more registers)
      const int dwj = j >> 1;
      mixacc(j & 1, acc[j][0], as_u(up.l)[dwj], y); mixacc(j & 1, acc[j][1], as_u(up.c)[dwj], y); mixacc(j & 1, acc[j][2], as_u(up.r)[dwj], y);
      mixacc(j & 1, acc[j][3], as_u(mid.l)[dwj], y); mixacc(j & 1, acc[j][4], as_u(mid.c)[dwj], y); mixacc(j & 1, acc[j][5], as_u(mid.r)[dwj], y);
      mixacc(j & 1, acc[j][6], as_u(dn.l)[dwj], y); mixacc(j & 1, acc[j][7], as_u(dn.c)[dwj], y); mixacc(j & 1, acc[j][8], as_u(dn.r)[dwj], y);
      if (EPI == 2) {  // bn_planes_bwd_sums_h_kernel's terms on the f16 gradient just formed
        const float xh = (xv - bmu[j]) * binv[j];
        const bool gate = !epi_relu || fmaf(xh, bgm[j], bbt[j]) > 0.0f;
        const float gg = (live && gate) ? (float)a[j] : 0.0f;
        s1[j] += gg;
        s2[j] = fmaf(gg, xh, s2[j]);
      }
      if (EPI == 3) a[j] = xv > 0.0f ? a[j] : (h16)0.0f;
    }
    if (live) op[(row + 1) * WP + xcol] = a;
  };
  if (RES) {
    if (__builtin_amdgcn_ballot_w64(has_task) != 0) {  // wave-uniform
      Row A, Bq, Cq;
      arrive(dp[pix(r_begin - 1)], A);
      arrive(dp[pix(r_begin)], Bq);
      h16x8 pg0 = dp[pix(r_begin + 1)], px0 = xp[pix(r_begin)], pg1 = dp[pix(r_begin + 2)], px1 = xp[pix(r_begin + 1)], pg2 = dp[pix(r_begin + 3)], px2 = xp[pix(r_begin + 2)];
      const h16x8* rqp = reinterpret_cast<const h16x8*>(resq) + ((int64_t)b * CO + co) * ((int64_t)(Ho + 2) * WPo);
      const bool col_even = xcol >= 0 && (xcol & 1) == 0;
      const int jq = xcol < 0 ? 0 : (xcol >> 1), jc = jq >= WPo ? WPo - 1 : jq;
      auto rload = [&](int row) -> h16x8 {  // every lane loads (pair partners the same 16 bytes); only even (row, column) keep the value
        int iq = row >> 1;
        iq = iq < 0 ? 0 : (iq >= Ho ? Ho - 1 : iq);
        return rqp[(iq + 1) * WPo + jc];
      };
      auto rkeep = [&](const h16x8& v, int row) { radd = (col_even && (row & 1) == 0) ? v : zero_h(); };
      h16x8 pr0 = rload(r_begin), pr1 = rload(r_begin + 1), pr2 = rload(r_begin + 2);
      for (int i = 0; i < rps; i += 3) {
        const int r = r_begin + i;
        { const h16x8 gr = pg0, xr = px0, rr = pr0; pg0 = dp[pix(r + 4)]; px0 = xp[pix(r + 3)]; pr0 = rload(r + 3); arrive(gr, Cq); rkeep(rr, r); step(A, Bq, Cq, xr, r); }
        { const h16x8 gr = pg1, xr = px1, rr = pr1; pg1 = dp[pix(r + 5)]; px1 = xp[pix(r + 4)]; pr1 = rload(r + 4); arrive(gr, A); rkeep(rr, r + 1); step(Bq, Cq, A, xr, r + 1); }
        { const h16x8 gr = pg2, xr = px2, rr = pr2; pg2 = dp[pix(r + 6)]; px2 = xp[pix(r + 5)]; pr2 = rload(r + 5); arrive(gr, Bq); rkeep(rr, r + 2); step(Cq, A, Bq, xr, r + 2); }
      }
    }
  } else if (__builtin_amdgcn_ballot_w64(has_task) != 0) {  // wave-uniform
    Row A, Bq, Cq;
    arrive(dp[pix(r_begin - 1)], A);
    arrive(dp[pix(r_begin)], Bq);
    h16x8 pg0 = dp[pix(r_begin + 1)], px0 = xp[pix(r_begin)], pg1 = dp[pix(r_begin + 2)], px1 = xp[pix(r_begin + 1)], pg2 = dp[pix(r_begin + 3)], px2 = xp[pix(r_begin + 2)];
    for (int i = 0; i < rps; i += 3) {
      const int r = r_begin + i;
      { const h16x8 gr = pg0, xr = px0; pg0 = dp[pix(r + 4)]; px0 = xp[pix(r + 3)]; arrive(gr, Cq); step(A, Bq, Cq, xr, r); }
      { const h16x8 gr = pg1, xr = px1; pg1 = dp[pix(r + 5)]; px1 = xp[pix(r + 4)]; arrive(gr, A); step(Bq, Cq, A, xr, r + 1); }
      { const h16x8 gr = pg2, xr = px2; pg2 = dp[pix(r + 6)]; px2 = xp[pix(r + 5)]; arrive(gr, Bq); step(Cq, A, Bq, xr, r + 2); }
    }
  }
  constexpr int NRED = 8 * KK + (EPI == 2 ? 16 : 0);
  __shared__ float red[4][NRED];
#pragma unroll
  for (int j = 0; j < 8; ++j)
#pragma unroll
    for (int t = 0; t < KK; ++t) {
      const float v = wave_sum_lane63(acc[j][t]);
      if (lane == 63) red[threadIdx.x >> 6][j * KK + t] = v;
    }
  if (EPI == 2) {
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const float v = wave_sum_lane63(j < 8 ? s1[j & 7] : s2[j & 7]);
      if (lane == 63) red[threadIdx.x >> 6][8 * KK + j] = v;
    }
  }
  __syncthreads();
  if (threadIdx.x < 8 * KK) {
    const int j = threadIdx.x / KK, t = threadIdx.x - j * KK;  // accumulator t is the REVERSED tap
    const int c = co * 8 + j;
    if (c < C) atomicAdd(&dW[(KK - 1 - t) * C + c], red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x]);
  } else if (EPI == 2 && threadIdx.x < NRED) {
    const int j = threadIdx.x - 8 * KK;  // 0..7 sum g, 8..15 sum g * xhat
    const float tot = red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
    atomicAdd(&shards[((int64_t)((blockIdx.x + 7 * b + 3 * co) & 31) * CO + co) * 16 + j], (double)tot);
  }
}

// the 32 accumulator copies [32][CO][16] -> scratch2C = dbeta[8 CO] | dgamma[8 CO] (doubles), in place by one workgroup
__global__ __launch_bounds__(256) void bwd_sums_compact_h_kernel(double* __restrict__ shards, int CO) {
  const int t = threadIdx.x;
  double tot = 0.0;
  if (t < 16 * CO) {
    const int which = t >= 8 * CO, c = which ? t - 8 * CO : t;
    for (int sh = 0; sh < 32; ++sh) tot += shards[((int64_t)sh * CO + (c >> 3)) * 16 + which * 8 + (c & 7)];
  }
  __syncthreads();
  if (t < 16 * CO) shards[t] = tot;
}

template <int SW>
int launch_dw_bwd_h(hipStream_t st, const h16* x, const h16* du, int B, int C, int H, int W, int WP, int relu_in, const h16* wrev, h16* dr, float* dW, int epi,
                    const InBnH& ib, int epi_relu, double* shards, int nstrip, const h16* resq = nullptr) {
  constexpr int NSUB = 64 / SW;
  const int CO = (C + 7) / 8;
  const int64_t per_seg = (int64_t)B * CO * nstrip;
  // segments: ~6 waves per SIMD over the chip in total.  A wave ends with the cross-lane reduction of its 72 (+16) f32 accumulators -- 617 LDS
  // permutes + 542 adds, 12 % of its instructions at 36-row segments -- so longer segments pay until the last round's imbalance takes it back:
  // 16 384 waves 16.32 ms per sweep step, 8 192 16.05-16.2, 6 144 16.11, 4 096 16.14, 2 048 16.19 (profiles/r04_ab_march_waves.log; the f32 twin is flat)
  int nseg = (int)((6144ll * NSUB + per_seg - 1) / per_seg);
  if (nseg < 1) nseg = 1;
  if (nseg > (H + 23) / 24) nseg = (H + 23) / 24;
  int rps = (H + nseg - 1) / nseg;
  rps = (rps + 2) / 3 * 3;
  nseg = (H + rps - 1) / rps;
  const int waves = (nstrip * nseg + NSUB - 1) / NSUB;
  dim3 grid((waves + 3) / 4, CO, B);
  const int Ho = (H + 1) / 2, WPo = orcai_padded_width((W + 1) / 2, 3);
  if (epi == 2 && resq)
    hipLaunchKernelGGL((dw_bwd_march_h_kernel<SW, 2, true, true>), grid, dim3(256), 0, st, x, du, C, H, W, WP, 0, wrev, dr, dW, shards, nstrip, nseg, rps, ib, epi_relu, resq, Ho, WPo);
  else if (epi == 2) hipLaunchKernelGGL((dw_bwd_march_h_kernel<SW, 2, true>), grid, dim3(256), 0, st, x, du, C, H, W, WP, 0, wrev, dr, dW, shards, nstrip, nseg, rps, ib, epi_relu, (const h16*)nullptr, 0, 0);
  else if (epi == 3) hipLaunchKernelGGL((dw_bwd_march_h_kernel<SW, 3, false>), grid, dim3(256), 0, st, x, du, C, H, W, WP, relu_in, wrev, dr, dW, shards, nstrip, nseg, rps, ib, 0, (const h16*)nullptr, 0, 0);
  else if (ib.mean) hipLaunchKernelGGL((dw_bwd_march_h_kernel<SW, 0, true>), grid, dim3(256), 0, st, x, du, C, H, W, WP, 0, wrev, dr, dW, shards, nstrip, nseg, rps, ib, 0, (const h16*)nullptr, 0, 0);
  else hipLaunchKernelGGL((dw_bwd_march_h_kernel<SW, 0, false>), grid, dim3(256), 0, st, x, du, C, H, W, WP, relu_in, wrev, dr, dW, shards, nstrip, nseg, rps, ib, 0, (const h16*)nullptr, 0, 0);
  return (int)hipGetLastError();
}

// ---------------------------------------------------------------- entry conv weight gradient with bn0 (+ReLU) backward on the fly
// dv = gamma*inv*(dy_eff - dbeta/N - xhat*dgamma/N) is formed per pixel from (dy, v, sums) and consumed at once (never written).
// Block (bx, co): octet co of the 16 entry channels (8 x k x k accumulators per lane for k = 3; two blocks per octet for k = 5, 7).
template <int KS, int NCH>
__global__ __launch_bounds__(256) void conv0_bn_wgrad_h_kernel(const float* __restrict__ in, int64_t snippet_stride, const h16* __restrict__ dy,
                                                                const h16* __restrict__ v /*[B][2][HP][WP][8]*/, int H, int W, int WP, int B,
                                                                const float* __restrict__ mean, const float* __restrict__ var, const float* __restrict__ gamma,
                                                                const float* __restrict__ beta, float eps, const double* __restrict__ dbeta,
                                                                const double* __restrict__ dgamma, float inv_count, float* __restrict__ dW /*[KS*KS][16]*/) {
  constexpr int R = KS / 2, KK = KS * KS, PARTS = 8 / NCH;
  __shared__ float red[4][NCH * KK];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int co = blockIdx.y / PARTS, c0 = (blockIdx.y % PARTS) * NCH;
  const int plane = (H + 2 * R) * WP;
  float mu[NCH], inv[NCH], g[NCH], bt[NCH], c1[NCH], c2[NCH];
#pragma unroll
  for (int k = 0; k < NCH; ++k) {
    const int c = co * 8 + c0 + k;
    mu[k] = mean[c]; inv[k] = rsqrtf(var[c] + eps); g[k] = gamma[c]; bt[k] = beta[c];
    c1[k] = (float)dbeta[c] * inv_count; c2[k] = (float)dgamma[c] * inv_count;
  }
  float acc[NCH][KK];
#pragma unroll
  for (int j = 0; j < NCH; ++j)
#pragma unroll
    for (int t = 0; t < KK; ++t) acc[j][t] = 0.0f;
  const int total = H * W;
  for (int b = 0; b < B; ++b) {
    const float* src = in + (int64_t)b * snippet_stride;
    const int64_t base = ((int64_t)b * 2 + co) * plane;
    for (int p = blockIdx.x * 256 + threadIdx.x; p < total; p += gridDim.x * 256) {
      const int y = p / W, x = p - y * W;
      const h16x8 d8 = reinterpret_cast<const h16x8*>(dy)[base + (y + R) * WP + x], v8 = reinterpret_cast<const h16x8*>(v)[base + (y + R) * WP + x];
      float gq[NCH];
#pragma unroll
      for (int k = 0; k < NCH; ++k) {
        const float xh = ((float)v8[c0 + k] - mu[k]) * inv[k];
        const float de = (fmaf(xh, g[k], bt[k]) > 0.0f) ? (float)d8[c0 + k] : 0.0f;
        gq[k] = g[k] * inv[k] * (de - c1[k] - xh * c2[k]);
      }
#pragma unroll
      for (int dyy = 0; dyy < KS; ++dyy)
#pragma unroll
        for (int dx = 0; dx < KS; ++dx) {
          const int yy = y + dyy - R, xx = x + dx - R;
          const float a = (yy >= 0 && yy < H && xx >= 0 && xx < W) ? src[yy * W + xx] : 0.0f;
#pragma unroll
          for (int j = 0; j < NCH; ++j) acc[j][dyy * KS + dx] = fmaf(a, gq[j], acc[j][dyy * KS + dx]);
        }
    }
  }
#pragma unroll
  for (int j = 0; j < NCH; ++j)
#pragma unroll
    for (int t = 0; t < KK; ++t) {
      const float s2 = wave_sum_lane63(acc[j][t]);
      if (lane == 63) red[wave][j * KK + t] = s2;
    }
  __syncthreads();
  if (threadIdx.x < NCH * KK) {
    const int j = threadIdx.x / KK, t = threadIdx.x - j * KK;
    atomicAdd(&dW[t * 16 + co * 8 + c0 + j], red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x]);
  }
}

// ---------------------------------------------------------------- f16 kernel-layout copies of the f32 master weights, one launch per step
// desc[i] = {type, src offset (floats), dst offset (halves), C, aux}:
//   0  Keras depthwise (k,k,C,1)  -> [ceil(C/8)][k*k][8]                       aux = k*k
//   1  the same with the taps reversed (input-gradient convolution)
//   2  pointwise / residual (1,1,Cin,Cout) -> A fragments [KG(Cin)][MT(Cout)][64][8]       C = Cin, aux = Cout   (forward)
//   3  its transpose -> A fragments [KG(Cout)][MT(Cin)][64][8] with row = cin, k = cout     C = Cin, aux = Cout   (input gradient)
//   4  identity matrix of C channels as A fragments [KG(C)][MT(C)][64][8] (depthwise-only passes); src unused
//   5  all-ones depthwise taps [ceil(C/8)][1][8] (pointwise-only passes); src unused
__global__ __launch_bounds__(256) void pack_weights_h_kernel(const float* __restrict__ w, const int* __restrict__ desc, h16* __restrict__ out) {
  const int* d = desc + blockIdx.x * 5;
  const int type = d[0], C = d[3], aux = d[4];
  const float* src = w + d[1];
  h16* dst = out + d[2];
  if (type <= 1) {
    const int KK = aux, CO = (C + 7) >> 3;
    for (int i = threadIdx.x; i < CO * KK * 8; i += 256) {
      const int e = i & 7, tap = (i >> 3) % KK, co = (i >> 3) / KK;
      const int c = co * 8 + e, ts = type ? KK - 1 - tap : tap;
      dst[i] = (h16)(c < C ? src[ts * C + c] : 0.0f);
    }
  } else if (type == 5) {
    const int CO = (C + 7) >> 3;
    for (int i = threadIdx.x; i < CO * 8; i += 256) dst[i] = (h16)(i < C ? 1.0f : 0.0f);
  } else {
    const int Cin = C, Cout = (type == 4) ? C : aux;
    const int Kc = (type == 3) ? Cout : Cin;   // contraction (k) channels
    const int Rc = (type == 3) ? Cin : Cout;   // row (output) channels
    const int KG = (Kc + 31) >> 5, MT = (Rc + 15) >> 4;
    for (int i = threadIdx.x; i < KG * MT * 512; i += 256) {
      const int e = i & 7, lane = (i >> 3) & 63, m = (i >> 9) % MT, kg = (i >> 9) / MT;
      const int kc = 32 * kg + 8 * (lane >> 4) + e, rc = 16 * m + (lane & 15);
      float v = 0.0f;
      if (kc < Kc && rc < Rc) v = (type == 4) ? (kc == rc ? 1.0f : 0.0f) : (type == 2 ? src[kc * Cout + rc] : src[rc * Cout + kc]);
      dst[i] = (h16)v;
    }
  }
}

// Keras Reshape layout f32 [B][H][W*C] -> f16 octet planes (gradient of the final conv's output)
__global__ __launch_bounds__(256) void feat_to_planes_h_kernel(const float* __restrict__ f, int C, int H, int W, int WP, int R, h16* __restrict__ out, int B) {
  const int CO = (C + 7) >> 3;
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t interior = (int64_t)H * W;
  if (idx >= (int64_t)B * CO * interior) return;
  const int64_t bq = idx / interior, pix = idx - bq * interior;
  const int co = (int)(bq % CO);
  const int64_t b = bq / CO;
  const int yy = (int)(pix / W), xx = (int)(pix - (int64_t)yy * W);
  const float* src = f + ((b * H + yy) * (int64_t)W + xx) * C + co * 8;
  O8 o;
#pragma unroll
  for (int k = 0; k < 8; ++k) o.v[k] = (co * 8 + k < C) ? src[k] : 0.0f;
  st8(out, bq * ((int64_t)(H + 2 * R) * WP) + (int64_t)(yy + R) * WP + xx, o);
}

// dx = (y > 0) ? dy : 0 on whole plane buffers
__global__ __launch_bounds__(256) void relu_bwd_h_kernel(const h16x8* __restrict__ dy, const h16x8* __restrict__ y, int64_t n8, h16x8* __restrict__ dx) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n8) return;
  const h16x8 d = dy[i], v = y[i];
  h16x8 o;
#pragma unroll
  for (int k = 0; k < 8; ++k) o[k] = v[k] > (h16)0 ? d[k] : (h16)0;
  dx[i] = o;
}

}  // namespace

extern "C" {

int orcai_h_bn_planes_stats(const void* v, int B, int C, int H, int W, int ksize, double* scratch2C, float* mean, float* var, void* stream) {
  if (!v || !scratch2C || !mean || !var || B <= 0 || C <= 0 || C > 64) return ORCAI_E_BADARG;
  hipStream_t st = (hipStream_t)stream;
  const int CO = (C + 7) / 8, R = ksize / 2, WP = orcai_padded_width(W, ksize);
  const int64_t plane = (int64_t)(H + 2 * R) * WP;
  if (plane >= (1ll << 31)) return ORCAI_E_UNSUPPORTED;
  if (plane < 32768) {  // small planes (f16: half the bytes of the f32 case at equal size): sharded accumulators, scratch f64[16 * ceil(C/8) * 32]
    const int nchunk = (int)((plane + 4095) / 4096);
    hipError_t e = orcai_zero::zero_async(scratch2C, sizeof(double) * 16 * CO * SUM_SHARDS, st);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(planes_sums_sharded_h_kernel, dim3((unsigned)(B * nchunk), CO), dim3(256), 0, st, (const h16*)v, CO, (int)plane, nchunk, scratch2C);
    hipLaunchKernelGGL(bn_finish_stats_sharded_h_kernel, dim3((C + 63) / 64), dim3(64), 0, st, scratch2C, C, CO, (double)B * H * W, mean, var);
    return (int)hipGetLastError();
  }
  hipError_t e = orcai_zero::zero_async(scratch2C, sizeof(double) * 16 * CO, st);
  if (e != hipSuccess) return (int)e;
  int gx = (int)((B * plane + 255) / 256);
  if (gx > 128) gx = 128;
  hipLaunchKernelGGL(planes_sums_h_kernel, dim3(gx, CO), dim3(256), 0, st, (const h16*)v, CO, plane, B, scratch2C, scratch2C + 8 * CO);
  hipLaunchKernelGGL(bn_finish_stats_h_kernel, dim3((C + 63) / 64), dim3(64), 0, st, scratch2C, scratch2C + 8 * CO, C, (double)B * H * W, mean, var);
  return (int)hipGetLastError();
}

int orcai_h_bn_finish_sharded(const double* shards, int B, int C, int H, int W, float* mean, float* var, void* stream) {
  if (!shards || !mean || !var || B <= 0 || C <= 0 || C > 64 || H <= 0 || W <= 0) return ORCAI_E_BADARG;
  hipLaunchKernelGGL(bn_finish_stats_sharded_h_kernel, dim3((C + 63) / 64), dim3(64), 0, (hipStream_t)stream, shards, C, (C + 7) / 8, (double)B * H * W, mean, var);
  return (int)hipGetLastError();
}

int orcai_h_planes_sum(const void* x, int B, int C, int H, int W, int ksize, double* scratchC, float* out, int accumulate, void* stream) {
  if (!x || !scratchC || !out || B <= 0 || C <= 0 || C > 64) return ORCAI_E_BADARG;
  hipStream_t st = (hipStream_t)stream;
  const int CO = (C + 7) / 8, R = ksize / 2, WP = orcai_padded_width(W, ksize);
  const int64_t plane = (int64_t)(H + 2 * R) * WP;
  if (plane >= (1ll << 31)) return ORCAI_E_UNSUPPORTED;
  hipError_t e = orcai_zero::zero_async(scratchC, sizeof(double) * 8 * CO, st);
  if (e != hipSuccess) return (int)e;
  int gx = (int)((B * plane + 255) / 256);
  if (gx > 128) gx = 128;
  hipLaunchKernelGGL(planes_sums_h_kernel, dim3(gx, CO), dim3(256), 0, st, (const h16*)x, CO, plane, B, scratchC, (double*)nullptr);
  hipLaunchKernelGGL(f64_to_f32_h_kernel, dim3((C + 63) / 64), dim3(64), 0, st, scratchC, out, C, accumulate);
  return (int)hipGetLastError();
}

int orcai_h_bn_planes_apply(const void* v, int B, int C, int H, int W, int ksize, const float* mean, const float* var, const float* gamma, const float* beta,
                            float eps, int relu, void* y, void* stream) {
  if (!v || !y || !mean || !var || !gamma || !beta || B <= 0 || C <= 0) return ORCAI_E_BADARG;
  const int64_t bq = (int64_t)B * ((C + 7) / 8);
  if (bq > 65535 || (int64_t)H * W >= (1ll << 31)) return ORCAI_E_UNSUPPORTED;
  hipLaunchKernelGGL(bn_planes_apply_h_kernel, dim3(blocks_for((int64_t)H * W), (unsigned)bq), dim3(256), 0, (hipStream_t)stream, (const h16*)v, C, H, W,
                     orcai_padded_width(W, ksize), ksize / 2, mean, var, gamma, beta, eps, relu, (h16*)y);
  return (int)hipGetLastError();
}

int orcai_h_bn_bwd_pointwise(const void* dy, const void* v, int B, int C, int H, int W, int ksize, const float* mean, const float* var, const float* gamma,
                             const float* beta, float eps, int relu, double* scratch2C, int sums_ready, float* dbeta, float* dgamma, const void* wtf, int Cin,
                             void* dv, void* du, void* stream) {
  if (!dy || !v || !dv || !du || !wtf || !scratch2C || !dbeta || !dgamma || B <= 0 || C <= 0 || Cin <= 0 || C > 64 || Cin > 64) return ORCAI_E_BADARG;
  hipStream_t st = (hipStream_t)stream;
  const int CO = (C + 7) / 8, R = ksize / 2, WP = orcai_padded_width(W, ksize);
  const int64_t plane = (int64_t)(H + 2 * R) * WP;
  if (plane >= (1ll << 29)) return ORCAI_E_UNSUPPORTED;
  double* db = scratch2C;
  double* dg = scratch2C + 8 * CO;
  if (!sums_ready) {
    hipError_t e = orcai_zero::zero_async(scratch2C, sizeof(double) * 16 * CO, st);
    if (e != hipSuccess) return (int)e;
    int gx = (int)((B * plane + 255) / 256);
    if (gx > 128) gx = 128;
    hipLaunchKernelGGL(bn_planes_bwd_sums_h_kernel, dim3(gx, CO), dim3(256), 0, st, (const h16*)dy, (const h16*)v, C, plane, B, mean, var, gamma, beta, eps, relu, db, dg);
  }
  const int tasks = (H * WP + 63) / 64;
  dim3 grid((tasks + 3) / 4, B);
  const float inv_count = (float)(1.0 / ((double)B * H * W));
#define ORCAI_HBBP(MT_)                                                                                                                                   \
  hipLaunchKernelGGL((bn_bwd_pw_h_kernel<MT_>), grid, dim3(256), 0, st, (const h16*)dy, (const h16*)v, C, H, W, WP, R, mean, var, gamma, beta, eps, relu, db, dg, \
                     inv_count, (const h16*)wtf, Cin, (h16*)dv, (h16*)du, tasks, magic_for(WP))
  switch ((Cin + 15) / 16) {
    case 1: ORCAI_HBBP(1); break;
    case 2: ORCAI_HBBP(2); break;
    case 3: ORCAI_HBBP(3); break;
    case 4: ORCAI_HBBP(4); break;
    default: return ORCAI_E_UNSUPPORTED;
  }
#undef ORCAI_HBBP
  hipLaunchKernelGGL(f64_to_f32_pair_h_kernel, dim3((C + 63) / 64), dim3(64), 0, st, db, dbeta, dg, dgamma, C);
  return (int)hipGetLastError();
}

int orcai_h_bn_bwd_pointwise_wgrad(const void* dy, const void* v, const void* u, int B, int C, int H, int W, int ksize, const float* mean, const float* var,
                                   const float* gamma, const float* beta, float eps, int relu, double* scratch2C, int sums_ready, float* dbeta, float* dgamma,
                                   const void* wtf, int Cin, void* du, float* dWpw, float* workspace, int64_t workspace_floats, void* stream) {
  if (!dy || !v || !u || !du || !wtf || !scratch2C || !dbeta || !dgamma || !dWpw || !workspace || B <= 0 || C <= 0 || Cin <= 0) return ORCAI_E_BADARG;
  // one output tile of dW per wave: at most 2 x 2 tiles of 16 channels (block 1 of every hyper-parameter-search width); wider layers keep the two launches
  const int MT = (Cin + 15) / 16, NT = (C + 15) / 16;
  if (MT > 2 || NT > 2 || workspace_floats < (int64_t)Cin * C) return ORCAI_E_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  const int CO = (C + 7) / 8, R = ksize / 2, WP = orcai_padded_width(W, ksize);
  const int64_t plane = (int64_t)(H + 2 * R) * WP;
  if (plane >= (1ll << 29) || (((uintptr_t)dy | (uintptr_t)v | (uintptr_t)u | (uintptr_t)du | (uintptr_t)wtf) & 15)) return ORCAI_E_UNSUPPORTED;
  double* db = scratch2C;
  double* dg = scratch2C + 8 * CO;
  if (!sums_ready) {
    hipError_t e = orcai_zero::zero_async(scratch2C, sizeof(double) * 16 * CO, st);
    if (e != hipSuccess) return (int)e;
    int gx = (int)((B * plane + 255) / 256);
    if (gx > 128) gx = 128;
    hipLaunchKernelGGL(bn_planes_bwd_sums_h_kernel, dim3(gx, CO), dim3(256), 0, st, (const h16*)dy, (const h16*)v, C, plane, B, mean, var, gamma, beta, eps, relu, db, dg);
  }
  const int64_t nchunks = (int64_t)B * ((H * WP + 255) / 256);
  int64_t grid = nchunks < 1024 ? nchunks : 1024;  // four workgroups per compute unit
  if (grid * Cin * C > workspace_floats) grid = workspace_floats / ((int64_t)Cin * C);
  const float inv_count = (float)(1.0 / ((double)B * H * W));
  void *prof0 = nullptr, *prof1 = nullptr;
  orcai_profile_take(&prof0, &prof1);  // measurement hook (orcai_profile_bracket): events around the main kernel only
  if (prof0) (void)hipEventRecord((hipEvent_t)prof0, st);
#define ORCAI_HBBPW(MT_, NT_)                                                                                                                                       \
  hipLaunchKernelGGL((bn_bwd_pw_wgrad_h_kernel<MT_, NT_>), dim3((unsigned)grid), dim3(256), 0, st, (const h16*)dy, (const h16*)v, (const h16*)u, C, H, W, WP, R, B, mean, var, \
                     gamma, beta, eps, relu, db, dg, inv_count, (const h16*)wtf, Cin, (h16*)du, workspace, magic_for(WP))
  if (MT == 1 && NT == 1) ORCAI_HBBPW(1, 1);
  else if (MT == 1) ORCAI_HBBPW(1, 2);
  else if (NT == 1) ORCAI_HBBPW(2, 1);
  else ORCAI_HBBPW(2, 2);
#undef ORCAI_HBBPW
  if (prof1) (void)hipEventRecord((hipEvent_t)prof1, st);
  hipLaunchKernelGGL(add_partials_h_kernel, dim3(blocks_for((int64_t)Cin * C), 8), dim3(256), 0, st, workspace, (int)grid, Cin * C, dWpw);
  hipLaunchKernelGGL(f64_to_f32_pair_h_kernel, dim3((C + 63) / 64), dim3(64), 0, st, db, dbeta, dg, dgamma, C);
  return (int)hipGetLastError();
}

static int h_pool_bwd_bn_impl(const void* dout, const void* ybn, int B, int C, int H, int W, int ksize, void* dy, const float* bn_gamma, const float* bn_mean,
                              const float* bn_var, float bn_eps, double* bn_sums, double* dout_sums, float* dbias, void* stream) {
  if (!dout || !ybn || !dy || B <= 0 || C <= 0 || H <= 0 || W <= 0 || C > 64) return ORCAI_E_BADARG;
  if (bn_sums && (!bn_gamma || !bn_mean || !bn_var)) return ORCAI_E_BADARG;
  if (dout_sums && (!bn_sums || !dbias)) return ORCAI_E_BADARG;
  const int Ho = (H + 1) / 2, Wo = (W + 1) / 2;
  int tot_h = (Ho - 1) * 2 + 3 - H, tot_w = (Wo - 1) * 2 + 2 - W;
  if (tot_h < 0) tot_h = 0;
  if (tot_w < 0) tot_w = 0;
  const int CO = (C + 7) / 8;
  if ((int64_t)B * CO > 65535) return ORCAI_E_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  if (bn_sums) {
    hipError_t e = orcai_zero::zero_async(bn_sums, sizeof(double) * 16 * CO, st);
    if (e != hipSuccess) return (int)e;
  }
  if (dout_sums) {
    hipError_t e = orcai_zero::zero_async(dout_sums, sizeof(double) * 8 * CO, st);
    if (e != hipSuccess) return (int)e;
  }
  const int per_bq = ((Ho + PB_ROWS - 1) / PB_ROWS) * Wo;
  dim3 grid((per_bq + 255) / 256, (unsigned)(B * CO));
  hipLaunchKernelGGL(pool_bwd_h_kernel, grid, dim3(256), 0, st, (const h16*)dout, (const h16*)ybn, C, H, W, orcai_padded_width(W, ksize), ksize / 2, Ho, Wo,
                     orcai_padded_width(Wo, ksize), tot_h / 2, tot_w / 2, (h16*)dy, bn_gamma, bn_mean, bn_var, bn_eps, bn_sums, dout_sums);
  if (dout_sums) hipLaunchKernelGGL(f64_to_f32_h_kernel, dim3((C + 63) / 64), dim3(64), 0, st, dout_sums, dbias, C, 0);
  return (int)hipGetLastError();
}

int orcai_h_pool_bwd_bn(const void* dout, const void* ybn, int B, int C, int H, int W, int ksize, void* dy, const float* bn_gamma, const float* bn_mean,
                        const float* bn_var, float bn_eps, double* bn_sums, void* stream) {
  return h_pool_bwd_bn_impl(dout, ybn, B, C, H, W, ksize, dy, bn_gamma, bn_mean, bn_var, bn_eps, bn_sums, nullptr, nullptr, stream);
}

int orcai_h_pool_bwd_bn_bias(const void* dout, const void* ybn, int B, int C, int H, int W, int ksize, void* dy, const float* bn_gamma, const float* bn_mean,
                             const float* bn_var, float bn_eps, double* bn_sums, double* dout_sums, float* dbias, void* stream) {
  if (!dout_sums || !dbias) return ORCAI_E_BADARG;
  return h_pool_bwd_bn_impl(dout, ybn, B, C, H, W, ksize, dy, bn_gamma, bn_mean, bn_var, bn_eps, bn_sums, dout_sums, dbias, stream);
}

int orcai_h_outer_reduce(const void* A, int Ca, const void* Bq, int Cb, int B, int H, int W, int ksize, int a_stride2, int Ha, int Wa, float* D, float* workspace,
                         int64_t workspace_floats, void* stream) {
  if (!A || !Bq || !D || !workspace || Ca <= 0 || Cb <= 0 || Ca > 64 || Cb > 64 || B <= 0 || workspace_floats < (int64_t)Ca * Cb) return ORCAI_E_BADARG;
  const int WP = orcai_padded_width(W, ksize), R = ksize / 2;
  const size_t lds = (size_t)256 * (((Ca + 15) / 16) * 16 + 8 + ((Cb + 15) / 16) * 16 + 8) * sizeof(h16);
  if (const hipError_t e = orcai_lds::ensure_dynamic_lds<outer_reduce_h_kernel>(lds); e != hipSuccess) return (int)e;
  const int64_t plane = (int64_t)(H + 2 * R) * WP;
  if (plane >= (1ll << 30)) return ORCAI_E_UNSUPPORTED;
  const int64_t nchunks = (int64_t)B * ((plane + 255) / 256);
  int64_t grid = nchunks < 512 ? nchunks : 512;
  if (grid * Ca * Cb > workspace_floats) grid = workspace_floats / ((int64_t)Ca * Cb);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(outer_reduce_h_kernel, dim3((unsigned)grid), dim3(256), lds, st, (const h16*)A, Ca, (const h16*)Bq, Cb, H, W, WP, R, B, a_stride2, Ha,
                     a_stride2 ? orcai_padded_width(Wa, ksize) : 0, workspace, magic_for(WP));
  hipLaunchKernelGGL(add_partials_h_kernel, dim3(blocks_for((int64_t)Ca * Cb), 8), dim3(256), 0, st, workspace, (int)grid, Ca * Cb, D);
  return (int)hipGetLastError();
}

int orcai_h_dw_wgrad(const void* x, const void* du, int B, int C, int H, int W, int ksize_planes, int ktap, int relu_in, float* dW, void* stream) {
  if (!x || !du || !dW || B <= 0 || C <= 0 || C > 64 || B > 65535 || H <= 0 || W <= 0 || ktap > ksize_planes) return ORCAI_E_BADARG;  // as orcai_dw_wgrad
  const int WP = orcai_padded_width(W, ksize_planes), RP = ksize_planes / 2;
  const int VAL = 64 - 2 * (ktap / 2);
  const int tasks = (H * WP + VAL - 1) / VAL;
  int tpw = (tasks + 7) / 8;
  if (tpw < 8) tpw = 8;
  const int parts = ktap == 3 ? 1 : 2;  // blocks per octet
  dim3 grid(((tasks + tpw - 1) / tpw + 3) / 4, parts * ((C + 7) / 8), B);
  hipStream_t st = (hipStream_t)stream;
  switch (ktap) {
    case 3: hipLaunchKernelGGL((dw_wgrad_h_kernel<3, 8>), grid, dim3(256), 0, st, (const h16*)x, (const h16*)du, C, H, W, WP, RP, relu_in, dW, tasks, tpw); break;
    case 5: hipLaunchKernelGGL((dw_wgrad_h_kernel<5, 4>), grid, dim3(256), 0, st, (const h16*)x, (const h16*)du, C, H, W, WP, RP, relu_in, dW, tasks, tpw); break;
    case 7: hipLaunchKernelGGL((dw_wgrad_h_kernel<7, 4>), grid, dim3(256), 0, st, (const h16*)x, (const h16*)du, C, H, W, WP, RP, relu_in, dW, tasks, tpw); break;
    default: return ORCAI_E_UNSUPPORTED;
  }
  return (int)hipGetLastError();
}

static int h_dw_bwd_fused_impl(const void* x, const void* du, int B, int C, int H, int W, int relu_in, const void* dw_rev, void* dr, float* dW, int epi, const float* bn_mean,
                               const float* bn_var, const float* bn_gamma, const float* bn_beta, float bn_eps, int bn_relu, double* shards, const void* resq, void* stream);

int orcai_h_dw_bwd_fused(const void* x, const void* du, int B, int C, int H, int W, int relu_in, const void* dw_rev, void* dr, float* dW, int epi, const float* bn_mean,
                         const float* bn_var, const float* bn_gamma, const float* bn_beta, float bn_eps, int bn_relu, double* shards, void* stream) {
  return h_dw_bwd_fused_impl(x, du, B, C, H, W, relu_in, dw_rev, dr, dW, epi, bn_mean, bn_var, bn_gamma, bn_beta, bn_eps, bn_relu, shards, nullptr, stream);
}

int orcai_h_dw_bwd_fused_res(const void* x, const void* du, int B, int C, int H, int W, const void* dw_rev, void* dr, float* dW, const float* bn_mean, const float* bn_var,
                             const float* bn_gamma, const float* bn_beta, float bn_eps, int bn_relu, double* shards, const void* resq, void* stream) {
  if (!resq || ((uintptr_t)resq & 15)) return ORCAI_E_BADARG;
  return h_dw_bwd_fused_impl(x, du, B, C, H, W, 0, dw_rev, dr, dW, 2, bn_mean, bn_var, bn_gamma, bn_beta, bn_eps, bn_relu, shards, resq, stream);
}

static int h_dw_bwd_fused_impl(const void* x, const void* du, int B, int C, int H, int W, int relu_in, const void* dw_rev, void* dr, float* dW, int epi, const float* bn_mean,
                               const float* bn_var, const float* bn_gamma, const float* bn_beta, float bn_eps, int bn_relu, double* shards, const void* resq, void* stream) {
  if (!x || !du || !dw_rev || !dr || !dW || B <= 0 || C <= 0 || H <= 0 || W <= 0 || (epi != 0 && epi != 2 && epi != 3)) return ORCAI_E_BADARG;
  const bool bn = bn_mean != nullptr;
  if (bn && (!bn_var || !bn_gamma || !bn_beta)) return ORCAI_E_BADARG;
  if (epi == 2 && (!bn || !shards)) return ORCAI_E_BADARG;
  if (epi == 3 && (bn || !relu_in)) return ORCAI_E_BADARG;
  const int WP = orcai_padded_width(W, 3), CO = (C + 7) / 8;
  if (B > 65535 || C > 64 || (int64_t)(H + 2) * WP >= (1ll << 27) || ((uintptr_t)x & 15) || ((uintptr_t)du & 15) || ((uintptr_t)dr & 15)) return ORCAI_E_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  InBnH ib;
  if (bn) { ib.mean = bn_mean; ib.var = bn_var; ib.gamma = bn_gamma; ib.beta = bn_beta; ib.eps = bn_eps; }
  if (epi == 2) {
    hipError_t e = orcai_zero::zero_async(shards, sizeof(double) * 16 * CO * 32, st);
    if (e != hipSuccess) return (int)e;
  }
  int best = 64, best_lanes = ((W + 61) / 62) * 64;
  if (((W + 29) / 30) * 32 < best_lanes) { best = 32; best_lanes = ((W + 29) / 30) * 32; }
  if (((W + 13) / 14) * 16 < best_lanes) { best = 16; best_lanes = ((W + 13) / 14) * 16; }
  const h16 *xh = (const h16*)x, *dh = (const h16*)du, *wh = (const h16*)dw_rev;
  int rc;
  if (best == 64) rc = launch_dw_bwd_h<64>(st, xh, dh, B, C, H, W, WP, relu_in, wh, (h16*)dr, dW, epi, ib, bn_relu, shards, (W + 61) / 62, (const h16*)resq);
  else if (best == 32) rc = launch_dw_bwd_h<32>(st, xh, dh, B, C, H, W, WP, relu_in, wh, (h16*)dr, dW, epi, ib, bn_relu, shards, (W + 29) / 30, (const h16*)resq);
  else rc = launch_dw_bwd_h<16>(st, xh, dh, B, C, H, W, WP, relu_in, wh, (h16*)dr, dW, epi, ib, bn_relu, shards, (W + 13) / 14, (const h16*)resq);
  if (rc != 0) return rc;
  if (epi == 2) hipLaunchKernelGGL(bwd_sums_compact_h_kernel, dim3(1), dim3(256), 0, st, shards, CO);
  return (int)hipGetLastError();
}

static int h_conv0_bn_bwd_impl(const float* in, int64_t snippet_stride, const void* dy, const void* v, int B, int H, int W, int ksize, const float* mean, const float* var,
                               const float* gamma, const float* beta, float eps, double* scratch2C, float* dbeta, float* dgamma, float* dW, int sums_ready, void* stream);

int orcai_h_conv0_bn_bwd(const float* in, int64_t snippet_stride, const void* dy, const void* v, int B, int H, int W, int ksize, const float* mean, const float* var,
                         const float* gamma, const float* beta, float eps, double* scratch2C, float* dbeta, float* dgamma, float* dW, void* stream) {
  return h_conv0_bn_bwd_impl(in, snippet_stride, dy, v, B, H, W, ksize, mean, var, gamma, beta, eps, scratch2C, dbeta, dgamma, dW, 0, stream);
}

int orcai_h_conv0_bn_bwd_ready(const float* in, int64_t snippet_stride, const void* dy, const void* v, int B, int H, int W, int ksize, const float* mean, const float* var,
                               const float* gamma, const float* beta, float eps, double* scratch2C, float* dbeta, float* dgamma, float* dW, void* stream) {
  return h_conv0_bn_bwd_impl(in, snippet_stride, dy, v, B, H, W, ksize, mean, var, gamma, beta, eps, scratch2C, dbeta, dgamma, dW, 1, stream);
}

static int h_conv0_bn_bwd_impl(const float* in, int64_t snippet_stride, const void* dy, const void* v, int B, int H, int W, int ksize, const float* mean, const float* var,
                               const float* gamma, const float* beta, float eps, double* scratch2C, float* dbeta, float* dgamma, float* dW, int sums_ready, void* stream) {
  if (!in || !dy || !v || !dW || !scratch2C || !dbeta || !dgamma || B <= 0) return ORCAI_E_BADARG;
  if ((int64_t)H * W >= (1ll << 30)) return ORCAI_E_BADARG;
  hipStream_t st = (hipStream_t)stream;
  const int C = 16, CO = 2, R = ksize / 2, WP = orcai_padded_width(W, ksize);
  const int64_t plane = (int64_t)(H + 2 * R) * WP;
  if (plane >= (1ll << 31)) return ORCAI_E_UNSUPPORTED;
  double* db = scratch2C;
  double* dg = scratch2C + 8 * CO;
  if (!sums_ready) {  // sums_ready: bn0's backward sums dbeta[16] | dgamma[16] are in scratch2C already (orcai_h_dw_bwd_fused_res with x = v0)
    hipError_t e = orcai_zero::zero_async(scratch2C, sizeof(double) * 16 * CO, st);
    if (e != hipSuccess) return (int)e;
    int gx = (int)((B * plane + 255) / 256);
    if (gx > 128) gx = 128;
    hipLaunchKernelGGL(bn_planes_bwd_sums_h_kernel, dim3(gx, CO), dim3(256), 0, st, (const h16*)dy, (const h16*)v, C, plane, B, mean, var, gamma, beta, eps, 1, db, dg);
  }
  const float inv_count = (float)(1.0 / ((double)B * H * W));
  dim3 grid(256, ksize == 3 ? 2 : 4);  // k = 3: one block column per octet; k = 5, 7: per half octet (accumulator registers)
  switch (ksize) {
    case 3: hipLaunchKernelGGL((conv0_bn_wgrad_h_kernel<3, 8>), grid, dim3(256), 0, st, in, snippet_stride, (const h16*)dy, (const h16*)v, H, W, WP, B, mean, var, gamma, beta, eps, db, dg, inv_count, dW); break;
    case 5: hipLaunchKernelGGL((conv0_bn_wgrad_h_kernel<5, 4>), grid, dim3(256), 0, st, in, snippet_stride, (const h16*)dy, (const h16*)v, H, W, WP, B, mean, var, gamma, beta, eps, db, dg, inv_count, dW); break;
    case 7: hipLaunchKernelGGL((conv0_bn_wgrad_h_kernel<7, 4>), grid, dim3(256), 0, st, in, snippet_stride, (const h16*)dy, (const h16*)v, H, W, WP, B, mean, var, gamma, beta, eps, db, dg, inv_count, dW); break;
    default: return ORCAI_E_UNSUPPORTED;
  }
  hipLaunchKernelGGL(f64_to_f32_pair_h_kernel, dim3(1), dim3(64), 0, st, db, dbeta, dg, dgamma, C);
  return (int)hipGetLastError();
}

int orcai_h_pack_weights(const float* w, const int* desc, int n_desc, void* out, void* stream) {
  if (!w || !desc || !out || n_desc <= 0) return ORCAI_E_BADARG;
  hipLaunchKernelGGL(pack_weights_h_kernel, dim3(n_desc), dim3(256), 0, (hipStream_t)stream, w, desc, (h16*)out);
  return (int)hipGetLastError();
}

int orcai_h_feat_to_planes(const float* f, int B, int C, int H, int W, int ksize, void* out, void* stream) {
  if (!f || !out || B <= 0 || C <= 0) return ORCAI_E_BADARG;
  const int64_t n = (int64_t)B * ((C + 7) / 8) * H * W;
  hipLaunchKernelGGL(feat_to_planes_h_kernel, dim3(blocks_for(n)), dim3(256), 0, (hipStream_t)stream, f, C, H, W, orcai_padded_width(W, ksize), ksize / 2, (h16*)out, B);
  return (int)hipGetLastError();
}

int orcai_h_planes_relu_bwd(const void* dy, const void* y, int64_t n_halves, void* dx, void* stream) {
  if (!dy || !y || !dx || n_halves <= 0 || (n_halves & 7)) return ORCAI_E_BADARG;
  hipLaunchKernelGGL(relu_bwd_h_kernel, dim3(blocks_for(n_halves / 8)), dim3(256), 0, (hipStream_t)stream, (const h16x8*)dy, (const h16x8*)y, n_halves / 8, (h16x8*)dx);
  return (int)hipGetLastError();
}

}  // extern "C"
