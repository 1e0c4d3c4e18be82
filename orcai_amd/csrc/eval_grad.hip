// eval_grad.hip -- the gradient w.r.t. the input of the INFERENCE network (BatchNorm with its moving statistics, folded into per-channel
// scale / shift; no Dropout): orcai_amd/eval_grad.py.  The reference never differentiates its predict path (predict.py:265-268 calls
// model.predict); Keras would form these gradients for a frozen model behind anything trainable (architectures.py:162-241 with training=False).
//
//   orcai_sepconv_dgrad          the folded separable conv run transposed: gate, pointwise contraction with scale (.) pw^T and the depthwise conv with
//                                reversed taps in ONE pass; the pointwise product du never reaches HBM
//   orcai_rows_affine            y = [relu](x * scale[col % C] + shift[col % C]) on a row tensor (Dense-128's folded BatchNorm, kept apart from the
//                                GEMM so that the ReLU output in front of it stays available to the backward)
//   orcai_rows_affine_relu_bwd   its backward: dx = ref > 0 ? dy * scale[col % C] : 0
//   orcai_sepconv_wgrad_frozen   the reductions of a folded separable conv's weight gradients (G = sum gg (x) u, sum gg, the depthwise gradient) in ONE pass over
//                                (x, g): u and du never reach HBM; per-workgroup partials added in a fixed order
//   orcai_frozen_bn_finish       weight gradients of a layer in front of a FROZEN BatchNorm from two reductions (G = sum gg (x) u, sum gg): the
//                                pointwise kernel, the bias, gamma and beta (EvalGrad.backward(wgrad=True))
//   orcai_rows_bn_frozen_wgrad   dbeta / dgamma of a frozen BatchNorm on a row tensor (Dense-128's)
//   orcai_overlap_average_bwd    the adjoint of orcai_overlap_average for a chunk of snippets: dpred = dagg / cover count (RecordingGrad.backward)
//   orcai_snippets_overlap_add   the adjoint of slicing a spectrogram into 50 %-overlapping snippets: a chunk's dx gathered and added into dspec
//   orcai_zero_fill              zero_fill.h's stream-ordered kernel fill for a caller's accumulator (dspec)
#include <hip/hip_runtime.h>

#include <cstdint>

#include "lds_optin.h"
#include "orcai_hip.h"
#include "zero_fill.h"

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

// =========================================================================================
// sepconv_wgrad_frozen_kernel (k = 3).  A workgroup of 4 waves walks over tiles of 4 image rows x 16 columns (tile = blockIdx.x, + gridDim.x, ...: a fixed
// assignment) and keeps its sums in registers until the end.  Per tile
//   load     x with its one-pixel halo (6 x 18, zero outside the image, ReLU'd when relu_in) as xs[ci][halo pixel]; gg = g gated by y_gate > 0 (zero outside the
//            image) as gs[co][pixel]: LDS images [channel][pixel], pitch 66 (bn_bwd_pw_wgrad_kernel's pattern).  The pads of the planes are never read.
//   u, du    u[ci][p] = 9 fma on the x tile (vector ALU) -> us; du = wts^T gg by v_mfma_f32_16x16x4_f32 with k = output channel (A = wts from LDS, row = ci;
//            B = gs, column = pixel; wave w owns tile row w) -> ds.  Neither reaches HBM.
//   sums     G[co][ci] += gg u^T by the same MFMA with k = pixel (A = gs, B = us; the up to 16 output tiles are dealt round-robin to the waves, 4 accumulator
//            registers each); dWdw[t][ci] += sum_p xs[ci][p + off(t)] * ds[ci][p] and dbeta[co] += sum_p gs[co][p] on the vector ALU.
// At the end every workgroup writes its Cout*Cin + Cout + 9*Cin partial sums to its own slot of the workspace; wgrad_frozen_fold_kernel adds the slots in
// index order in double.  No atomics: two launches give the same bits.
// =========================================================================================
constexpr int WF_ROWS = 4, WF_COLS = 16, WF_PIX = WF_ROWS * WF_COLS, WF_HW = WF_COLS + 2, WF_HALO = (WF_ROWS + 2) * WF_HW, WF_PITCH = WF_PIX + 2, WF_MAX_WG = 1024;

__global__ __launch_bounds__(256) void sepconv_wgrad_frozen_kernel(const float* __restrict__ x, const float* __restrict__ g, const float* __restrict__ y_gate,
                                                                   const float* __restrict__ taps /*[CQi][9][4]*/, const float* __restrict__ wts /*[Cout][Cin]*/,
                                                                   int Cin, int Cout, int H, int W, int WP, int relu_in, int TY, int TX, int ntiles,
                                                                   float* __restrict__ part /*[gridDim.x][Cout*Cin + Cout + 9*Cin]*/) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int CQi = (Cin + 3) >> 2, CQo = (Cout + 3) >> 2;
  const int MTI = (Cin + 15) >> 4, MTO = (Cout + 15) >> 4, CiP = MTI * 16, CoP = MTO * 16;
  float* xs = smem;                  // [CiP][WF_HALO]
  float* gs = xs + CiP * WF_HALO;    // [CoP][WF_PITCH]
  float* us = gs + CoP * WF_PITCH;   // [CiP][WF_PITCH]
  float* ds = us + CiP * WF_PITCH;   // [CiP][WF_PITCH]
  float* wl = ds + CiP * WF_PITCH;   // [CoP][CiP]   wts, zero-padded
  const int lds_floats = CiP * WF_HALO + (CoP + 2 * CiP) * WF_PITCH + CoP * CiP;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lk = lane >> 4, lj = lane & 15;
  for (int i = tid; i < lds_floats; i += 256) smem[i] = 0.0f;  // the rows of the channels that pad a 16-tile stay zero
  __syncthreads();
  for (int i = tid; i < Cout * Cin; i += 256) {
    const int co = i / Cin, ci = i - co * Cin;
    wl[co * CiP + ci] = wts[i];
  }
  const int64_t plane = (int64_t)(H + 2) * WP;  // float4 pixels of one channel quad of one snippet
  f32x4 accG[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) accG[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
  float accW[3] = {0.f, 0.f, 0.f};
  float accB = 0.f;
  const int ntileG = MTO * MTI;
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int b = tile / (TY * TX);
    const int rem = tile - b * (TY * TX);
    const int y0 = (rem / TX) * WF_ROWS, x0 = (rem % TX) * WF_COLS;
    // ---- load: x tile with halo, gated g tile
    for (int i = tid; i < CQi * WF_HALO; i += 256) {
      const int q = i / WF_HALO, hp = i - q * WF_HALO;
      const int iy = y0 - 1 + hp / WF_HW, ix = x0 - 1 + hp % WF_HW;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (iy >= 0 && iy < H && ix >= 0 && ix < W) v = reinterpret_cast<const float4*>(x)[((int64_t)b * CQi + q) * plane + (int64_t)(iy + 1) * WP + ix];
      float e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int c = 4 * q + j;
        float t = c < Cin ? e[j] : 0.0f;
        if (relu_in) t = fmaxf(t, 0.0f);
        xs[c * WF_HALO + hp] = t;
      }
    }
    for (int i = tid; i < CQo * WF_PIX; i += 256) {
      const int q = i / WF_PIX, p = i - q * WF_PIX;
      const int iy = y0 + p / WF_COLS, ix = x0 + p % WF_COLS;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (iy < H && ix < W) {
        const int64_t at = ((int64_t)b * CQo + q) * plane + (int64_t)(iy + 1) * WP + ix;
        v = reinterpret_cast<const float4*>(g)[at];
        if (y_gate) {
          const float4 yv = reinterpret_cast<const float4*>(y_gate)[at];
          v.x = yv.x > 0.0f ? v.x : 0.0f;
          v.y = yv.y > 0.0f ? v.y : 0.0f;
          v.z = yv.z > 0.0f ? v.z : 0.0f;
          v.w = yv.w > 0.0f ? v.w : 0.0f;
        }
      }
      float e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int j = 0; j < 4; ++j) gs[(4 * q + j) * WF_PITCH + p] = (4 * q + j) < Cout ? e[j] : 0.0f;
    }
    __syncthreads();
    // ---- u on the vector ALU
    for (int i = tid; i < CQi * 4 * WF_PIX; i += 256) {
      const int c = i / WF_PIX, p = i - c * WF_PIX;
      const float* tp = taps + (c >> 2) * 36 + (c & 3);
      const float* xp = xs + c * WF_HALO + (p / WF_COLS) * WF_HW + (p % WF_COLS);
      float a = 0.0f;
#pragma unroll
      for (int t = 0; t < 9; ++t) a = fmaf(tp[4 * t], xp[(t / 3) * WF_HW + (t % 3)], a);
      us[c * WF_PITCH + p] = a;
    }
    // ---- du = wts^T gg: wave w owns the 16 pixels of tile row w
    for (int mt = 0; mt < MTI; ++mt) {
      f32x4 acc = (f32x4){0.f, 0.f, 0.f, 0.f};
      for (int k0 = 0; k0 < CoP; k0 += 4) acc = mfma16(wl[(k0 + lk) * CiP + mt * 16 + lj], gs[(k0 + lk) * WF_PITCH + wave * 16 + lj], acc);
#pragma unroll
      for (int r = 0; r < 4; ++r) ds[(mt * 16 + 4 * lk + r) * WF_PITCH + wave * 16 + lj] = acc[r];
    }
    __syncthreads();
    // ---- G += gg u^T (k = pixel)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int t = wave + 4 * j;
      if (t < ntileG) {
        const int mo = t / MTI, mi = t - mo * MTI;
        const float* ap = gs + (mo * 16 + lj) * WF_PITCH + lk;
        const float* bp = us + (mi * 16 + lj) * WF_PITCH + lk;
#pragma unroll 4
        for (int p0 = 0; p0 < WF_PIX; p0 += 4) accG[j] = mfma16(ap[p0], bp[p0], accG[j]);
      }
    }
    // ---- dWdw and dbeta on the vector ALU
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const int q = tid + 256 * j;
      const int c = q / 9, t = q - 9 * c;
      if (c < Cin) {
        const float* xp = xs + c * WF_HALO + (t / 3) * WF_HW + (t % 3);
        const float* dp = ds + c * WF_PITCH;
        float a = accW[j];
        for (int p = 0; p < WF_PIX; ++p) a = fmaf(xp[(p / WF_COLS) * WF_HW + (p % WF_COLS)], dp[p], a);
        accW[j] = a;
      }
    }
    if (tid < Cout) {
      const float* gp = gs + tid * WF_PITCH;
      float a = accB;
      for (int p = 0; p < WF_PIX; ++p) a += gp[p];
      accB = a;
    }
    __syncthreads();  // the next tile's loads overwrite xs / gs
  }
  // ---- this workgroup's partial sums
  const int S = Cout * Cin + Cout + 9 * Cin;
  float* mine = part + (size_t)blockIdx.x * S;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int t = wave + 4 * j;
    if (t < ntileG) {
      const int mo = t / MTI, mi = t - mo * MTI;
      const int ci = mi * 16 + lj;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int co = mo * 16 + 4 * lk + r;
        if (co < Cout && ci < Cin) mine[co * Cin + ci] = accG[j][r];
      }
    }
  }
  if (tid < Cout) mine[Cout * Cin + tid] = accB;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const int q = tid + 256 * j;
    const int c = q / 9, t = q - 9 * c;
    if (c < Cin) mine[Cout * Cin + Cout + t * Cin + c] = accW[j];  // Keras (3, 3, Cin, 1)
  }
}

__global__ __launch_bounds__(256) void wgrad_frozen_fold_kernel(const float* __restrict__ part, int nwg, int Cin, int Cout, float* __restrict__ G, float* __restrict__ dbeta,
                                                                float* __restrict__ dWdw) {
  const int S = Cout * Cin + Cout + 9 * Cin;
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= S) return;
  double a = 0.0;
  for (int w = 0; w < nwg; ++w) a += (double)part[(size_t)w * S + e];
  const float v = (float)a;
  if (e < Cout * Cin) G[e] = v;
  else if (e < Cout * Cin + Cout) dbeta[e - Cout * Cin] = v;
  else dWdw[e - Cout * Cin - Cout] = v;
}

// One workgroup per layer, plain f32: a few KB of arithmetic behind orcai_outer_reduce / orcai_planes_sum.  inv is 1 / sqrtf (correctly rounded division
// and square root); every output element is written by exactly one thread.
__global__ __launch_bounds__(256) void frozen_bn_finish_kernel(const float* __restrict__ G, const float* __restrict__ sums, const float* __restrict__ pw,
                                                               const float* __restrict__ bias, const float* __restrict__ gamma, const float* __restrict__ mean,
                                                               const float* __restrict__ var, float eps, int Cin, int Cout, float* __restrict__ dWpw,
                                                               float* __restrict__ dbias, float* __restrict__ dgamma, float* __restrict__ dbeta) {
  __shared__ float scale_s[4096];  // gamma * inv per channel, formed once: dWpw and dbias see the same rounding
  for (int co = threadIdx.x; co < Cout; co += 256) {
    const float inv = 1.0f / sqrtf(var[co] + eps);
    const float sc = gamma[co] * inv;
    scale_s[co] = sc;
    const float db = sums[co];
    if (dbeta) dbeta[co] = db;
    if (dbias) dbias[co] = sc * db;
    if (G) {
      float acc = 0.0f;  // sum over pixels of gg * (pw . u) = sum_ci pw[ci][co] * G[co][ci]
      for (int ci = 0; ci < Cin; ++ci) acc = fmaf(pw[(size_t)ci * Cout + co], G[(size_t)co * Cin + ci], acc);
      const float z0 = (bias ? bias[co] : 0.0f) - mean[co];  // the conv's own bias and the moving mean are constants of the pre-normalisation tensor
      dgamma[co] = inv * fmaf(z0, db, acc);
    }
  }
  if (!G) return;
  __syncthreads();
  for (int ci = 0; ci < Cin; ++ci)
    for (int co = threadIdx.x; co < Cout; co += 256) dWpw[(size_t)ci * Cout + co] = scale_s[co] * G[(size_t)co * Cin + ci];
}

// A workgroup owns 64 columns: thread (ry, cx) adds rows ry, ry + 4, ... of column cx (coalesced over cx), the four partial sums are added in a fixed
// order through LDS: no atomics, two launches give the same bits.
__global__ __launch_bounds__(256) void rows_bn_frozen_wgrad_kernel(const float* __restrict__ dy, const float* __restrict__ x, int64_t M, int cols, int C,
                                                                   const float* __restrict__ mean, const float* __restrict__ var, float eps,
                                                                   float* __restrict__ part /*[2][cols]*/) {
  __shared__ float sb[4][64], sg[4][64];
  const int cx = threadIdx.x & 63, ry = threadIdx.x >> 6;
  const int col = blockIdx.x * 64 + cx;
  float b = 0.0f, g = 0.0f;
  if (col < cols) {
    const float mu = mean[col % C];
    for (int64_t r = ry; r < M; r += 4) {
      const float d = dy[r * cols + col];
      b += d;
      g = fmaf(d, x[r * cols + col] - mu, g);
    }
  }
  sb[ry][cx] = b;
  sg[ry][cx] = g;
  __syncthreads();
  if (ry == 0 && col < cols) {
    part[col] = (sb[0][cx] + sb[1][cx]) + (sb[2][cx] + sb[3][cx]);
    part[cols + col] = (sg[0][cx] + sg[1][cx]) + (sg[2][cx] + sg[3][cx]);
  }
}

// channel c of a row tensor with cols = W * C columns: the W columns c, c + C, ... added in order
__global__ __launch_bounds__(256) void rows_bn_frozen_fold_kernel(const float* __restrict__ part, int cols, int C, const float* __restrict__ var, float eps,
                                                                  float* __restrict__ dbeta, float* __restrict__ dgamma) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  float b = 0.0f, g = 0.0f;
  for (int col = c; col < cols; col += C) {
    b += part[col];
    g += part[cols + col];
  }
  dbeta[c] = b;
  dgamma[c] = g * (1.0f / sqrtf(var[c] + eps));
}

// =========================================================================================
// The two adjoints of the recording-level function (predict.py:244-261 slices, predict.py:276-293 averages; the forward kernel is model_fwd.hip's
// overlap_average_kernel).  Both are gathers with one thread per OUTPUT element: no atomics, two launches give the same bits.  Consecutive threads walk
// the innermost index (label / frequency bin), so reads and writes are coalesced; every index is int64_t (T * W passes 2^30 for long recordings).
// =========================================================================================
// dpred[i - i0][off][l] = dagg[i * step + off][l] / c(i * step + off), c(s) = the number of snippets 0 .. n-1 that cover step s, counted by the forward's loop
__global__ __launch_bounds__(256) void overlap_average_bwd_kernel(const float* __restrict__ dagg /*[S][L]*/, int n, int P, int L, int step, int i0, int64_t total,
                                                                   float* __restrict__ dpred /*[nb][P][L]*/) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int l = (int)(idx % L);
  const int64_t r = idx / L;
  const int off = (int)(r % P);
  const int64_t i = i0 + r / P;
  const int64_t s = i * step + off;
  int64_t i_hi = s / step;
  if (i_hi > n - 1) i_hi = n - 1;
  int64_t i_lo = (s - P + step) / step;  // ceil((s - P + 1)/step)
  if (s - P + 1 <= 0) i_lo = 0;
  int c = 0;
  for (int64_t j = i_lo; j <= i_hi; ++j) {
    const int64_t o = s - j * step;
    if (o >= 0 && o < P) ++c;
  }
  dpred[idx] = dagg[s * L + l] / (float)c;  // c >= 1: snippet i itself covers s
}

// dspec[t][w] += sum over the chunk's snippets i that cover row t, in ascending i, of dx[i - i0][t - i * shift][w]; thread <-> (t, w) of rows [t0, t0 + rows)
__global__ __launch_bounds__(256) void snippets_overlap_add_kernel(const float* __restrict__ dx /*[nb][H][W]*/, int i0, int nb, int H, int W, int shift, int64_t t0,
                                                                    int64_t total, float* __restrict__ dspec /*[T][W]*/) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int64_t t = t0 + idx / W;
  const int w = (int)(idx % W);
  int64_t i_hi = t / shift;
  if (i_hi > (int64_t)i0 + nb - 1) i_hi = (int64_t)i0 + nb - 1;
  int64_t i_lo = t - H + 1 <= 0 ? 0 : (t - H + shift) / shift;  // ceil((t - H + 1)/shift)
  if (i_lo < i0) i_lo = i0;
  float sum = 0.0f;
  for (int64_t i = i_lo; i <= i_hi; ++i) sum += dx[((i - i0) * H + (t - i * shift)) * W + w];
  const int64_t at = t * W + w;
  dspec[at] = dspec[at] + sum;
}

template <int MTI>
int launch_dgrad(const float* g, const float* y_gate, const float* x_gate, int B, int Cin, int Cout, int H, int W, const float* wts, const float* dw_rev, float* dr,
                 hipStream_t st) {
  const int CQ = (Cin + 3) / 4, WP = orcai_padded_width(W, 3);
  const size_t lds = (size_t)DG_SLOTS * CQ * DG_PITCH * sizeof(float4);
  if (const hipError_t e = orcai_lds::ensure_dynamic_lds<sepconv_dgrad_kernel<MTI>>(lds); e != hipSuccess) return (int)e;
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

int orcai_sepconv_wgrad_frozen(const float* x, const float* g, const float* y_gate, int relu_in, int B, int Cin, int Cout, int H, int W, int ksize, const float* taps,
                               const float* wts, float* G, float* dbeta, float* dWdw, float* workspace, int64_t workspace_floats, void* stream) {
  if (!x || !g || !taps || !wts || !G || !dbeta || !dWdw || !workspace || B <= 0 || Cin <= 0 || Cout <= 0 || H <= 0 || W <= 0) return ORCAI_E_BADARG;
  if (ksize != 3 && ksize != 5 && ksize != 7) return ORCAI_E_BADARG;
  if ((((uintptr_t)x | (uintptr_t)g | (uintptr_t)y_gate | (uintptr_t)taps) & 15) || (((uintptr_t)wts | (uintptr_t)G | (uintptr_t)dbeta | (uintptr_t)dWdw | (uintptr_t)workspace) & 3))
    return ORCAI_E_BADARG;
  if (ksize != 3 || Cin > 64 || Cout > 64 || B > 65535) return ORCAI_E_UNSUPPORTED;  // k = 5, 7: the caller runs compose_wgrad
  const int WP = orcai_padded_width(W, 3);
  const int64_t plane = (int64_t)(H + 2) * WP;
  if (16 * plane >= (1ll << 31)) return ORCAI_E_UNSUPPORTED;
  const int TY = (H + WF_ROWS - 1) / WF_ROWS, TX = (W + WF_COLS - 1) / WF_COLS;
  const int64_t ntiles = (int64_t)B * TY * TX;
  if (ntiles >= (1ll << 31)) return ORCAI_E_UNSUPPORTED;
  const int64_t S = (int64_t)Cout * Cin + Cout + 9 * Cin;
  const int nwg = (int)(ntiles < WF_MAX_WG ? ntiles : WF_MAX_WG);
  if (workspace_floats < nwg * S) return ORCAI_E_UNSUPPORTED;  // the size the header states
  const int CiP = (Cin + 15) / 16 * 16, CoP = (Cout + 15) / 16 * 16;
  const size_t lds = sizeof(float) * ((size_t)CiP * WF_HALO + (size_t)(CoP + 2 * CiP) * WF_PITCH + (size_t)CoP * CiP);
  if (const hipError_t e = orcai_lds::ensure_dynamic_lds<sepconv_wgrad_frozen_kernel>(lds); e != hipSuccess) return (int)e;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(sepconv_wgrad_frozen_kernel, dim3((unsigned)nwg), dim3(256), lds, st, x, g, y_gate, taps, wts, Cin, Cout, H, W, WP, relu_in, TY, TX, (int)ntiles, workspace);
  hipLaunchKernelGGL(wgrad_frozen_fold_kernel, dim3((unsigned)((S + 255) / 256)), dim3(256), 0, st, workspace, nwg, Cin, Cout, G, dbeta, dWdw);
  return (int)hipGetLastError();
}

int orcai_frozen_bn_finish(const float* G, const float* sums, const float* pw, const float* bias, const float* gamma, const float* mean, const float* var, float eps,
                           int Cin, int Cout, float* dWpw, float* dbias, float* dgamma, float* dbeta, void* stream) {
  if (!sums || !gamma || !var || Cout <= 0 || Cout > 4096) return ORCAI_E_BADARG;
  if (G && (!pw || !mean || !dWpw || !dgamma || Cin <= 0 || Cin > 4096)) return ORCAI_E_BADARG;
  if (!G && !dbias && !dbeta) return ORCAI_E_BADARG;
  hipLaunchKernelGGL(frozen_bn_finish_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, G, sums, pw, bias, gamma, mean, var, eps, Cin, Cout, dWpw, dbias, dgamma, dbeta);
  return (int)hipGetLastError();
}

int orcai_rows_bn_frozen_wgrad(const float* dy, const float* x, int64_t M, int cols, int C, const float* mean, const float* var, float eps, float* dbeta, float* dgamma,
                               float* workspace, void* stream) {
  if (!dy || !x || !mean || !var || !dbeta || !dgamma || !workspace || M <= 0 || cols <= 0 || C <= 0 || cols % C) return ORCAI_E_BADARG;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(rows_bn_frozen_wgrad_kernel, dim3((unsigned)((cols + 63) / 64)), dim3(256), 0, st, dy, x, M, cols, C, mean, var, eps, workspace);
  hipLaunchKernelGGL(rows_bn_frozen_fold_kernel, dim3((unsigned)((C + 255) / 256)), dim3(256), 0, st, workspace, cols, C, var, eps, dbeta, dgamma);
  return (int)hipGetLastError();
}

int orcai_overlap_average_bwd(const float* dagg, int n, int P, int L, int step, int64_t S, int i0, int nb, float* dpred, void* stream) {
  if (!dagg || !dpred || n <= 0 || P <= 0 || L <= 0 || step <= 0 || i0 < 0 || nb <= 0 || (int64_t)i0 + nb > n) return ORCAI_E_BADARG;
  if ((int64_t)(n - 1) * step + P > S) return ORCAI_E_BADARG;  // every step of every snippet is a row of dagg
  const int64_t total = (int64_t)nb * P * L;
  if ((total + 255) / 256 >= (1ll << 31)) return ORCAI_E_UNSUPPORTED;
  hipLaunchKernelGGL(overlap_average_bwd_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, dagg, n, P, L, step, i0, total, dpred);
  return (int)hipGetLastError();
}

int orcai_snippets_overlap_add(const float* dx, int i0, int nb, int H, int W, int shift, int64_t T, float* dspec, void* stream) {
  if (!dx || !dspec || nb <= 0 || i0 < 0 || H <= 0 || W <= 0 || shift <= 0 || (int64_t)i0 + nb > (1ll << 31) - 1) return ORCAI_E_BADARG;
  const int64_t t0 = (int64_t)i0 * shift, t1 = ((int64_t)i0 + nb - 1) * shift + H;
  if (t1 > T) return ORCAI_E_BADARG;
  const int64_t total = (t1 - t0) * W;
  if ((total + 255) / 256 >= (1ll << 31)) return ORCAI_E_UNSUPPORTED;
  hipLaunchKernelGGL(snippets_overlap_add_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, dx, i0, nb, H, W, shift, t0, total, dspec);
  return (int)hipGetLastError();
}

int orcai_zero_fill(void* p, int64_t bytes, void* stream) {
  if (!p || bytes < 0 || (bytes & 3) || ((uintptr_t)p & 3)) return ORCAI_E_BADARG;
  return (int)orcai_zero::zero_async(p, (size_t)bytes, (hipStream_t)stream);
}

}  // extern "C"
