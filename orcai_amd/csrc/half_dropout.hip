// half_dropout.hip -- the Dropout of the f16 path between residual blocks (ResNet1DConv, architectures.py:73-97): the 0/1 mask as f16 and
// y = x * mask * scale on f16 channel-octet planes (half_planes.h).  Elementwise, 16 bytes per lane per operand: a lane owns eight
// consecutive elements; the last lane of a call whose length is not a multiple of eight stores its elements one by one.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "half_planes.h"
#include "orcai_hip.h"

using namespace orcai_half;

namespace {

inline unsigned lanes_blocks(int64_t n) { return (unsigned)(((n + 7) / 8 + 255) / 256); }

// element i of orcai_dropout_mask_dev (train_head.hip): splitmix64 of (seed, i + 1), top 24 bits against keep -- the same draw bit for bit
__device__ __forceinline__ bool keep_draw(uint64_t seed, int64_t i, float keep) {
  uint64_t z = seed + 0x9E3779B97F4A7C15ull * (uint64_t)(i + 1);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z = z ^ (z >> 31);
  const float u = (float)(z >> 40) * (1.0f / 16777216.0f);
  return u < keep;
}

__global__ __launch_bounds__(256) void dropout_mask_h_kernel(h16* __restrict__ mask, int64_t n, const uint64_t* __restrict__ counter, uint64_t seed_add, float keep) {
  const int64_t i0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 8;
  if (i0 >= n) return;
  const uint64_t seed = seed_add + counter[0] * 0xD1B54A32D192ED03ull;
  if (i0 + 8 <= n) {
    h16x8 m;
#pragma unroll
    for (int e = 0; e < 8; ++e) m[e] = keep_draw(seed, i0 + e, keep) ? (h16)1.0f : (h16)0.0f;
    *(h16x8*)(mask + i0) = m;
    return;
  }
  for (int64_t i = i0; i < n; ++i) mask[i] = keep_draw(seed, i, keep) ? (h16)1.0f : (h16)0.0f;
}

// y = f16((f32(x) * f32(mask)) * scale): the product rounded to f32, then to f16, as orcai_mask_scale followed by a conversion.  The tail goes
// through the same eight-wide arithmetic: on one element at a time hipcc contracts fptrunc(fmul) into v_fma_mixlo_f16(scale, t, 0), which
// rounds once instead of twice and turns a -0 product into +0.
__device__ __forceinline__ h16x8 mask_scale8(h16x8 a, h16x8 m, float scale) {
  h16x8 r;
#pragma unroll
  for (int e = 0; e < 8; ++e) r[e] = (h16)(((float)a[e] * (float)m[e]) * scale);
  return r;
}

// x == y is allowed (no restrict between them)
__global__ __launch_bounds__(256) void mask_scale_h_kernel(const h16* x, const h16* __restrict__ mask, float scale, int64_t n, h16* y) {
  const int64_t i0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 8;
  if (i0 >= n) return;
  if (i0 + 8 <= n) {
    *(h16x8*)(y + i0) = mask_scale8(*(const h16x8*)(x + i0), *(const h16x8*)(mask + i0), scale);
    return;
  }
  const int rem = (int)(n - i0);
  h16x8 a = {}, m = {};
  for (int e = 0; e < rem; ++e) {
    a[e] = x[i0 + e];
    m[e] = mask[i0 + e];
  }
  const h16x8 r = mask_scale8(a, m, scale);
  for (int e = 0; e < rem; ++e) y[i0 + e] = r[e];
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" {

int orcai_h_dropout_mask_dev(void* mask, int64_t n, const uint64_t* counter, uint64_t seed_add, float keep, void* stream) {
  if (!mask || !counter || n <= 0 || !aligned16(mask)) return ORCAI_E_BADARG;
  hipLaunchKernelGGL(dropout_mask_h_kernel, dim3(lanes_blocks(n)), dim3(256), 0, (hipStream_t)stream, (h16*)mask, n, counter, seed_add, keep);
  return (int)hipGetLastError();
}

int orcai_h_mask_scale(const void* x, const void* mask, float scale, int64_t n, void* y, void* stream) {
  if (!x || !mask || !y || n <= 0 || !aligned16(x) || !aligned16(mask) || !aligned16(y)) return ORCAI_E_BADARG;
  hipLaunchKernelGGL(mask_scale_h_kernel, dim3(lanes_blocks(n)), dim3(256), 0, (hipStream_t)stream, (const h16*)x, (const h16*)mask, scale, n, (h16*)y);
  return (int)hipGetLastError();
}

}  // extern "C"
