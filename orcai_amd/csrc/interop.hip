// interop.hip -- the two pieces the PyTorch custom ops (orcai_amd/torch_ops.py) need beyond the training and inference kernels:
//   orcai_sigmoid_bwd        the gradient at the logit of the heads' final sigmoid from ANY upstream gradient (the training step's own seed is the
//                            fused masked-BCE kernel, orcai_masked_bce_w);
//   orcai_prepare_inference  the folded / re-laid-out inference weights (ResNetLSTM.prepare) from the flat trainable weights and BatchNorm moving
//                            statistics already on the device: no host round trip when an optimizer changes the weights every step.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "orcai_hip.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// dz = g * (1 - p) * p, in the order of aten::sigmoid_backward (grad * (1 - out) * out): two products, no fused multiply-add to contract
__global__ __launch_bounds__(256) void sigmoid_bwd_vec_kernel(const f32x4* __restrict__ p, const f32x4* __restrict__ g, int64_t n4, f32x4* __restrict__ dz) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n4) return;
  const f32x4 q = p[i], a = g[i];
  f32x4 r;
  r.x = a.x * (1.0f - q.x) * q.x;
  r.y = a.y * (1.0f - q.y) * q.y;
  r.z = a.z * (1.0f - q.z) * q.z;
  r.w = a.w * (1.0f - q.w) * q.w;
  dz[i] = r;
}

__global__ __launch_bounds__(256) void sigmoid_bwd_kernel(const float* __restrict__ p, const float* __restrict__ g, int64_t begin, int64_t n, float* __restrict__ dz) {
  const int64_t i = begin + (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  dz[i] = g[i] * (1.0f - p[i]) * p[i];
}

unsigned blocks(int64_t n) { return (unsigned)((n + 255) / 256); }

// desc[i] = {kind, dst, count, a0, a1, a2, a3, a4} (offsets in floats):
//   kind 0  BatchNorm fold of `count` channels: scale = gamma / sqrt(var + eps), shift = beta - mean * scale (+ bias * scale), in double, rounded
//           once to float (ResNetLSTM._fold_bn); gamma = w[a0], beta = w[a1], mean = stats[a2], var = stats[a3], bias = w[a4] or none (a4 < 0);
//           scale -> out[dst + c], shift -> out[dst + roundup(count, 64) + c] (both 256-byte aligned when dst is)
//   kind 1  depthwise kernel (k, k, count, 1) at w[a0], k = a1 -> [ceil(count/4)][k*k][4] at out[dst], zero taps for the padding channels
//           (architectures.depthwise_kernel_layout)
//   kind 2  copy of `count` floats from w[a0]
//   kind 3  transposed pointwise kernel with the BatchNorm scale of its OUTPUT channel folded in (orcai_sepconv_dgrad's wts): count = Cout,
//           gamma = w[a0], var = stats[a1], pointwise [Cin = a3][Cout] at w[a2]: out[dst + co * Cin + ci] = gamma / sqrt(var + eps) * pw[ci][co],
//           the product in double, rounded once
//   kind 4  kind 1 with the taps reversed (tap t <- tap k*k - 1 - t)
//   kind 5  transpose of the [a1][a2] matrix at w[a0] (count = a1 * a2): out[dst + c * a1 + r] = w[a0 + r * a2 + c]
// One workgroup row per descriptor (blockIdx.y), a grid-stride loop over its elements.
__global__ __launch_bounds__(256) void prepare_kernel(const float* __restrict__ w, const float* __restrict__ stats, const int* __restrict__ desc, double eps,
                                                      float* __restrict__ out) {
#pragma clang fp contract(off)
  const int* d = desc + blockIdx.y * 8;
  const int kind = d[0], dst = d[1], count = d[2];
  if (kind == 0) {
    for (int c = blockIdx.x * 256 + threadIdx.x; c < count; c += gridDim.x * 256) {
      const double g = w[d[3] + c], b = w[d[4] + c], m = stats[d[5] + c], v = stats[d[6] + c];
      const double scale = g / sqrt(v + eps);
      const double ms = m * scale;
      double shift = b - ms;
      if (d[7] >= 0) {
        const double bs = (double)w[d[7] + c] * scale;
        shift = shift + bs;
      }
      out[dst + c] = (float)scale;
      out[dst + ((count + 63) & ~63) + c] = (float)shift;
    }
  } else if (kind == 1 || kind == 4) {
    const int k = d[4], kk = k * k, cq = (count + 3) / 4, n = cq * kk * 4;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
      const int j = i & 3, t = (i >> 2) % kk, q = (i >> 2) / kk, ch = 4 * q + j;
      out[dst + i] = ch < count ? w[d[3] + (kind == 4 ? kk - 1 - t : t) * count + ch] : 0.0f;
    }
  } else if (kind == 3) {
    const int cin = d[6], n = count * cin;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
      const int co = i / cin, ci = i - co * cin;
      const double g = w[d[3] + co], v = stats[d[4] + co];
      const double scale = g / sqrt(v + eps);
      out[dst + i] = (float)(scale * (double)w[d[5] + ci * count + co]);
    }
  } else if (kind == 5) {
    const int rows = d[4], cols = d[5];
    for (int i = blockIdx.x * 256 + threadIdx.x; i < count; i += gridDim.x * 256) {
      const int c = i / rows, r = i - c * rows;
      out[dst + i] = w[d[3] + r * cols + c];
    }
  } else {
    for (int i = blockIdx.x * 256 + threadIdx.x; i < count; i += gridDim.x * 256) out[dst + i] = w[d[3] + i];
  }
}

}  // namespace

extern "C" {

int orcai_sigmoid_bwd(const float* p, const float* g, int64_t n, float* dz, void* stream) {
  if (!p || !g || !dz || n < 0) return ORCAI_E_BADARG;
  if (n == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  int64_t done = 0;
  if ((((uintptr_t)p | (uintptr_t)g | (uintptr_t)dz) & 15) == 0 && n >= 4) {
    const int64_t n4 = n / 4;
    hipLaunchKernelGGL(sigmoid_bwd_vec_kernel, dim3(blocks(n4)), dim3(256), 0, st, (const f32x4*)p, (const f32x4*)g, n4, (f32x4*)dz);
    done = 4 * n4;
  }
  if (done < n) hipLaunchKernelGGL(sigmoid_bwd_kernel, dim3(blocks(n - done)), dim3(256), 0, st, p, g, done, n, dz);
  return (int)hipGetLastError();
}

int orcai_prepare_inference(const float* w, const float* stats, const int* desc, int n_desc, double eps, float* out, void* stream) {
  if (!w || !desc || !out || n_desc <= 0 || n_desc > 65535 || !(eps > 0.0)) return ORCAI_E_BADARG;
  hipLaunchKernelGGL(prepare_kernel, dim3(16, n_desc), dim3(256), 0, (hipStream_t)stream, w, stats, desc, eps, out);
  return (int)hipGetLastError();
}

}  // extern "C"
