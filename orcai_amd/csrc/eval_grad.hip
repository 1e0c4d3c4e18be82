// eval_grad.hip -- the gradient w.r.t. the input of the INFERENCE network (BatchNorm with its moving statistics, folded into per-channel
// scale / shift; no Dropout): orcai_amd/eval_grad.py.  The reference never differentiates its predict path (predict.py:265-268 calls
// model.predict); Keras would form these gradients for a frozen model behind anything trainable (architectures.py:162-241 with training=False).
//
//   orcai_sepconv_dgrad          the folded separable conv run transposed: gate, pointwise contraction with scale (.) pw^T and the depthwise conv with
//                                reversed taps in ONE pass; the pointwise product du never reaches HBM
//   orcai_rows_affine            y = [relu](x * scale[col % C] + shift[col % C]) on a row tensor (Dense-128's folded BatchNorm, kept apart from the
//                                GEMM so that the ReLU output in front of it stays available to the backward)
//   orcai_rows_affine_relu_bwd   its backward: dx = ref > 0 ? dy * scale[col % C] : 0
#include <hip/hip_runtime.h>

#include <cstdint>

#include "orcai_hip.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ f32x4 mfma16(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
__device__ __forceinline__ void swap32(float& a, float& b) {  // a's lanes 32..63 <-> b's lanes 0..31
  auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(a), __float_as_uint(b), false, false);
  a = __uint_as_float(r[0]);
  b = __uint_as_float(r[1]);
}
__device__ __forceinline__ void swap16(float& a, float& b) {  // a's odd 16-lane rows <-> b's even 16-lane rows
  auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(a), __float_as_uint(b), false, false);
  a = __uint_as_float(r[0]);
  b = __uint_as_float(r[1]);
}

// =========================================================================================
// sepconv_dgrad_kernel (k = 3).  A workgroup of 4 waves owns a strip of 64 plane columns (lane l <-> image column 62 * strip - 1 + l: 62 output
// columns and one halo column on either side) and marches down a band of image rows.  Per step
//   phase A  wave w forms ONE row of du = wts^T (gated g) for all Cin channels of the strip: per quad of g one dwordx4 load per lane (and one of
//            y_gate), the 4 x 4 transpose of 16-lane rows of model_fwd.hip's sepconv_kernel turns the quad into the four B fragments of
//            v_mfma_f32_16x16x4_f32 (k = the quad's 4 output channels of the forward conv, column = pixel), A = wts[co][ci] (row = ci).  A lane's
//            4 accumulator registers are 4 consecutive ci of one pixel = one 16-byte LDS store.  Rows outside the image are stored as zeros,
//            columns outside it are zeroed on load: the pads of g and the gates are never used.
//   phase B  wave w forms one row of dr from the three du rows around it in the LDS ring: 9 ds_read_b128 and 36 fmas per quad and lane, the
//            x_gate select, one dwordx4 store (interior pixels only).
// LDS: a ring of 8 du rows (4 written per step + the 2 + 2 the depthwise window keeps alive) x ceil(Cin/4) quads x 66 pixels x 16 bytes.
// No atomics, every dr element written by exactly one lane: bit-reproducible.
// =========================================================================================
constexpr int DG_WAVES = 4, DG_SLOTS = 8, DG_VALID = 62, DG_PITCH = 66;

template <int MTI>
__global__ __launch_bounds__(64 * DG_WAVES) void sepconv_dgrad_kernel(const float* __restrict__ g /*[B][CQo][H+2][WP][4]*/, const float* __restrict__ y_gate,
                                                                      const float* __restrict__ x_gate /*[B][CQ][H+2][WP][4]*/, const float* __restrict__ wts /*[Cout][Cin]*/,
                                                                      const float* __restrict__ dw_rev /*[CQ][9][4]*/, int Cin, int Cout, int H, int W, int WP, int strips,
                                                                      int band_rows, float* __restrict__ dr /*[B][CQ][H+2][WP][4]*/) {
  extern __shared__ float4 ring[];  // [DG_SLOTS][CQ][DG_PITCH]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int lk = lane >> 4, lj = lane & 15;
  const int b = blockIdx.y;
  const int strip = blockIdx.x % strips, band = blockIdx.x / strips;
  const int CQ = (Cin + 3) >> 2, CQo = (Cout + 3) >> 2;
  const int plane = (H + 2) * WP;
  const int x = strip * DG_VALID - 1 + lane;
  const bool xin = x >= 0 && x < W;
  const int row0 = band * band_rows;
  const int row1 = row0 + band_rows < H ? row0 + band_rows : H;
  const int nsteps = (row1 - row0 + 2 + DG_WAVES - 1) / DG_WAVES;
  const float4* gq = reinterpret_cast<const float4*>(g) + (int64_t)b * CQo * plane;
  const float4* yq = y_gate ? reinterpret_cast<const float4*>(y_gate) + (int64_t)b * CQo * plane : nullptr;
  const float4* xq = x_gate ? reinterpret_cast<const float4*>(x_gate) + (int64_t)b * CQ * plane : nullptr;
  float4* drq = reinterpret_cast<float4*>(dr) + (int64_t)b * CQ * plane;

  for (int s = 0; s < nsteps; ++s) {
    // ---- phase A: du row a (ring index rel) of this wave
    const int rel = DG_WAVES * s + wave;
    const int a = row0 - 1 + rel;
    if (a <= row1) {  // wave-uniform; du rows below row1 are nobody's halo
      float4* slot = ring + (rel & (DG_SLOTS - 1)) * CQ * DG_PITCH + 1 + lane;
      if (a < 0 || a >= H) {
        for (int q = 0; q < CQ; ++q) slot[q * DG_PITCH] = make_float4(0.f, 0.f, 0.f, 0.f);
      } else {
        f32x4 acc[MTI][4];
#pragma unroll
        for (int m = 0; m < MTI; ++m)
#pragma unroll
          for (int t = 0; t < 4; ++t) acc[m][t] = (f32x4){0.f, 0.f, 0.f, 0.f};
        const int pix = (a + 1) * WP + (xin ? x : 0);  // lanes outside the image read a valid address and discard it
        float4 nxt = gq[pix], nxy = yq ? yq[pix] : make_float4(1.f, 1.f, 1.f, 1.f);
        for (int cq = 0; cq < CQo; ++cq) {
          const float4 v = nxt, y = nxy;
          if (cq + 1 < CQo) {
            nxt = gq[(cq + 1) * plane + pix];
            if (yq) nxy = yq[(cq + 1) * plane + pix];
          }
          float d[4] = {v.x, v.y, v.z, v.w};
          const float yy[4] = {y.x, y.y, y.z, y.w};
#pragma unroll
          for (int j = 0; j < 4; ++j) d[j] = (xin && yy[j] > 0.0f && cq * 4 + j < Cout) ? d[j] : 0.0f;
          float afrag[MTI];
#pragma unroll
          for (int m = 0; m < MTI; ++m) {
            const int co = cq * 4 + lk, ci = m * 16 + lj;
            const bool ok = co < Cout && ci < Cin;
            const float av = wts[ok ? co * Cin + ci : 0];
            afrag[m] = ok ? av : 0.0f;
          }
          // d[j] = gated g of channel 4cq + j, lane = pixel -> d[t] = B fragment of column tile t (row = channel 4cq + lk, column = pixel 16t + lj)
          swap32(d[0], d[2]);
          swap32(d[1], d[3]);
          swap16(d[0], d[1]);
          swap16(d[2], d[3]);
#pragma unroll
          for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int m = 0; m < MTI; ++m) acc[m][t] = mfma16(afrag[m], d[t], acc[m][t]);
        }
        // D[row = 4 lk + r -> ci = 16 m + 4 lk + r][column lj -> pixel 16 t + lj]: the lane's 4 registers are quad 4 m + lk of that pixel
        float4* srow = ring + (rel & (DG_SLOTS - 1)) * CQ * DG_PITCH + 1;
#pragma unroll
        for (int m = 0; m < MTI; ++m) {
          const int q = m * 4 + lk;
          if (q < CQ) {
#pragma unroll
            for (int t = 0; t < 4; ++t) srow[q * DG_PITCH + 16 * t + lj] = make_float4(acc[m][t][0], acc[m][t][1], acc[m][t][2], acc[m][t][3]);
          }
        }
      }
    }
    __syncthreads();
    // ---- phase B: dr row d of this wave from du rows d - 1, d, d + 1 (ring indices d - row0 .. d - row0 + 2)
    const int d = row0 + DG_WAVES * s - 2 + wave;
    if (d >= row0 && d < row1) {
      const bool store = lane >= 1 && lane <= DG_VALID && x < W;
      const int opix = (d + 1) * WP + (store ? x : 0);
      for (int q = 0; q < CQ; ++q) {
        const float4* wq = reinterpret_cast<const float4*>(dw_rev) + q * 9;  // wave-uniform: scalar loads
        float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int dy = 0; dy < 3; ++dy) {
          const float4* src = ring + (((d - row0 + dy) & (DG_SLOTS - 1)) * CQ + q) * DG_PITCH + lane;
#pragma unroll
          for (int dx = 0; dx < 3; ++dx) {
            const float4 u = src[dx], w = wq[dy * 3 + dx];
            o.x = fmaf(w.x, u.x, o.x);
            o.y = fmaf(w.y, u.y, o.y);
            o.z = fmaf(w.z, u.z, o.z);
            o.w = fmaf(w.w, u.w, o.w);
          }
        }
        if (store) {
          if (xq) {
            const float4 xv = xq[q * plane + opix];
            o.x = xv.x > 0.0f ? o.x : 0.0f;
            o.y = xv.y > 0.0f ? o.y : 0.0f;
            o.z = xv.z > 0.0f ? o.z : 0.0f;
            o.w = xv.w > 0.0f ? o.w : 0.0f;
          }
          drq[q * plane + opix] = o;
        }
      }
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void rows_affine_kernel(const float* __restrict__ x, int64_t n, int cols, int C, const float* __restrict__ scale,
                                                          const float* __restrict__ shift, int relu, float* __restrict__ y) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int c = (int)(i % cols) % C;
  const float v = fmaf(x[i], scale[c], shift[c]);
  y[i] = relu ? fmaxf(v, 0.0f) : v;
}

__global__ __launch_bounds__(256) void rows_affine_relu_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ ref, int64_t n, int cols, int C,
                                                                   const float* __restrict__ scale, float* __restrict__ dx) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int c = (int)(i % cols) % C;
  const bool on = ref ? ref[i] > 0.0f : true;
  dx[i] = on ? dy[i] * scale[c] : 0.0f;
}

template <int MTI>
int launch_dgrad(const float* g, const float* y_gate, const float* x_gate, int B, int Cin, int Cout, int H, int W, const float* wts, const float* dw_rev, float* dr,
                 hipStream_t st) {
  const int CQ = (Cin + 3) / 4, WP = orcai_padded_width(W, 3);
  const size_t lds = (size_t)DG_SLOTS * CQ * DG_PITCH * sizeof(float4);
  static size_t lds_set = 0;  // dynamic LDS beyond the 64 KiB default needs the opt-in
  if (lds > lds_set) {
    hipError_t e = hipFuncSetAttribute((const void*)sepconv_dgrad_kernel<MTI>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return (int)e;
    lds_set = lds;
  }
  const int strips = (W + DG_VALID - 1) / DG_VALID;
  int band_rows = 32;  // 2 recomputed halo rows per band; shorter bands while the grid would leave compute units idle
  while (band_rows > 8 && (int64_t)B * strips * ((H + band_rows - 1) / band_rows) < 1024) band_rows >>= 1;
  const int bands = (H + band_rows - 1) / band_rows;
  hipLaunchKernelGGL(sepconv_dgrad_kernel<MTI>, dim3((unsigned)(strips * bands), (unsigned)B), dim3(64 * DG_WAVES), lds, st, g, y_gate, x_gate, wts, dw_rev, Cin, Cout,
                     H, W, WP, strips, band_rows, dr);
  return (int)hipGetLastError();
}

}  // namespace

extern "C" {

int orcai_sepconv_dgrad(const float* g, const float* y_gate, const float* x_gate, int B, int Cin, int Cout, int H, int W, int ksize, const float* wts, const float* dw_rev,
                        float* dr, void* stream) {
  if (!g || !wts || !dw_rev || !dr || B <= 0 || Cin <= 0 || Cout <= 0 || H <= 0 || W <= 0) return ORCAI_E_BADARG;
  if (ksize != 3 && ksize != 5 && ksize != 7) return ORCAI_E_BADARG;
  if ((((uintptr_t)g | (uintptr_t)y_gate | (uintptr_t)x_gate | (uintptr_t)dr | (uintptr_t)dw_rev) & 15) || ((uintptr_t)wts & 3)) return ORCAI_E_BADARG;
  if (ksize != 3 || Cin > 64 || Cout > 64 || B > 65535) return ORCAI_E_UNSUPPORTED;  // k = 5, 7: the caller composes the existing launchers
  const int64_t plane = (int64_t)(H + 2) * orcai_padded_width(W, 3);
  if (16 * plane >= (1ll << 31)) return ORCAI_E_UNSUPPORTED;  // 32-bit pixel offsets inside a snippet
  const int64_t wgs = (int64_t)((W + DG_VALID - 1) / DG_VALID) * ((H + 7) / 8);
  if (wgs >= (1ll << 31)) return ORCAI_E_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  switch ((Cin + 15) / 16) {
    case 1: return launch_dgrad<1>(g, y_gate, x_gate, B, Cin, Cout, H, W, wts, dw_rev, dr, st);
    case 2: return launch_dgrad<2>(g, y_gate, x_gate, B, Cin, Cout, H, W, wts, dw_rev, dr, st);
    case 3: return launch_dgrad<3>(g, y_gate, x_gate, B, Cin, Cout, H, W, wts, dw_rev, dr, st);
    default: return launch_dgrad<4>(g, y_gate, x_gate, B, Cin, Cout, H, W, wts, dw_rev, dr, st);
  }
}

int orcai_rows_affine(const float* x, int64_t M, int cols, int C, const float* scale, const float* shift, int relu, float* y, void* stream) {
  if (!x || !scale || !shift || !y || M <= 0 || cols <= 0 || C <= 0 || cols % C) return ORCAI_E_BADARG;
  const int64_t n = M * cols;
  if ((n + 255) / 256 >= (1ll << 31)) return ORCAI_E_UNSUPPORTED;
  hipLaunchKernelGGL(rows_affine_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, n, cols, C, scale, shift, relu, y);
  return (int)hipGetLastError();
}

int orcai_rows_affine_relu_bwd(const float* dy, const float* ref, int64_t M, int cols, int C, const float* scale, float* dx, void* stream) {
  if (!dy || !scale || !dx || M <= 0 || cols <= 0 || C <= 0 || cols % C) return ORCAI_E_BADARG;
  const int64_t n = M * cols;
  if ((n + 255) / 256 >= (1ll << 31)) return ORCAI_E_UNSUPPORTED;
  hipLaunchKernelGGL(rows_affine_relu_bwd_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, dy, ref, n, cols, C, scale, dx);
  return (int)hipGetLastError();
}

}  // extern "C"
