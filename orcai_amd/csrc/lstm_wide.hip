// lstm_wide.hip -- the LSTM recurrences for units 160..256 (multiples of 32): inference, training forward and backward through time.
//
// The {32, 64, 96, 128} kernels (model_fwd.hip lstm_kernel, train_head.hip lstm_train_fwd_kernel / lstm_bwd_kernel and their _split / _h twins)
// keep one direction's recurrent matrix in registers for all T steps.  At units = 256 that matrix is U x 4U f32 = 1 MiB, twice a compute unit's
// 512 KiB of VGPRs: it cannot stay on the CU.  Here it is re-read from L2 every step instead.  All workgroups of a direction read the same 1 MiB,
// which the L2 serves to every CU of an XCD; the matrix never needs to leave it.
//
// Geometry ("Head widths"): one workgroup = one 16-row batch tile x one direction x all 4U gate columns, U / 16 waves
// (U * 4 threads: 1 024 at U = 256, four waves per SIMD).
//   forward:  wave w owns the 64 kernel columns [64w, 64w + 64) = two gate groups of 8 units (column layout of orcai_lstm_recurrent), i.e.
//             units [16w, 16w + 16); four 16-column MFMA tiles of v_mfma_f32_16x16x4_f32 over the U-long contraction h_{t-1} U.
//   backward: wave w owns units [16w, 16w + 16) and computes the 16 x 16 tile of dz_{t+1} U^T over the 4U-long contraction (lstm_bwd_kernel's
//             scheme with the U^T fragments streamed instead of resident).
// The B operand of every MFMA is read straight from global memory (L2) into registers, four k-steps per chunk, double-buffered: the next chunk's
// loads are in flight during the current chunk's MFMAs, and the first chunk of the next step is issued before the gate arithmetic.  Each element
// of U feeds exactly one MFMA of one wave per step (the batch tile is one MFMA row block), so staging it through LDS would add a write and a read
// and save nothing.  Products and sums are f32 (exact products, f32 accumulation): the accuracy of the f32-MFMA kernels of the narrow widths.
// No inter-workgroup communication, no allocation, no host synchronisation: the launches are graph-capturable.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "lds_optin.h"
#include "orcai_hip.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ f32x4 mfma16(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

// A chunk offset the compiler cannot see through: U is the same every step, and without this the loads of all steps are hoisted out of the step
// loop into registers -- the whole matrix slice of a lane, hundreds of VGPRs, spilled to scratch.
__device__ __forceinline__ void opaque(int& v) { asm volatile("" : "+s"(v)); }

// the activations and the gate stage of the narrow kernels (train_head.hip lstm_gate_stage): same functions, same arithmetic
__device__ __forceinline__ float sigmoidf_(float x) { return __builtin_amdgcn_rcpf(1.0f + __expf(-x)); }
__device__ __forceinline__ float tanhf_(float x) { return fmaf(-2.0f, __builtin_amdgcn_rcpf(__expf(2.0f * x) + 1.0f), 1.0f); }
__device__ __forceinline__ float dpp_xor8(float v) {  // lane l <- lane l ^ 8 (rotation by 8 within a row of 16 lanes)
  return __uint_as_float(__builtin_amdgcn_update_dpp(0u, __float_as_uint(v), 0x128 /*row_ror:8*/, 0xf, 0xf, true));
}
// lane (lk, lj) holds the pre-activations of rows 4 lk + r of column lj of a gate group's two tiles: tile 0 = i (lj < 8) or f, tile 1 = g or o
template <class StoreGates, class StoreState>
__device__ __forceinline__ void gate_stage(const f32x4& z0, const f32x4& z1, float (&cst)[2], int lj, StoreGates store_gates, StoreState store_state) {
  const bool low = lj < 8;
  const float m1 = low ? 2.0f : -1.0f;
  float a0[4], a1[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    a0[r] = sigmoidf_(z0[r]);
    const float rc = __builtin_amdgcn_rcpf(__expf(m1 * z1[r]) + 1.0f);
    a1[r] = low ? fmaf(-2.0f, rc, 1.0f) : rc;
    store_gates(r, a0[r], a1[r]);
  }
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const float got0 = dpp_xor8(low ? a0[2 + j] : a0[j]), got1 = dpp_xor8(low ? a1[2 + j] : a1[j]);
    const float gi = low ? a0[j] : got0, gf = low ? got0 : a0[2 + j];
    const float gg = low ? a1[j] : got1, go = low ? got1 : a1[2 + j];
    const float c = gf * cst[j] + gi * gg;
    const float h = go * tanhf_(c);
    cst[j] = c;
    store_state(j, low, h, c);  // row 4 lk + (low ? j : 2 + j)
  }
}

// TRAIN = false: inference (out only); TRAIN = true: also the gate activations and cell states in orcai_lstm_train_fwd's layouts.
template <int U, bool TRAIN>
__global__ __launch_bounds__(U * 4) void lstm_wide_fwd_kernel(const float* __restrict__ xz /*[B][T][2][4U] permuted*/, const float* __restrict__ Uw /*[2][U][4U] permuted*/,
                                                               int B, int T, float* __restrict__ out /*[B][T][2U]*/, float* __restrict__ gates /*[B][T][2][4U]*/,
                                                               float* __restrict__ cstate /*[B][T][2][U]*/) {
  static_assert(U % 32 == 0 && U <= 256, "units: a multiple of 32 up to 256");
  constexpr int HP = U + 2, CK = 4, NC = U / 4 / CK;  // CK k-steps of 4 per chunk; NC chunks per step (even: the buffer parity repeats every step)
  static_assert(NC % 2 == 0, "chunk count must be even");
  __shared__ float hbuf[2][16][HP];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lk = lane >> 4, lj = lane & 15;
  const int dir = blockIdx.y;
  const int b0 = blockIdx.x * 16;
  // B[k][col] of k-step kk, tile q: U[4 kk + lk][64 wave + 16 q + lj]
  const float* Ub = Uw + (int64_t)dir * U * 4 * U + lk * (4 * U) + wave * 64 + lj;
  float bq[2][CK][4];
  auto load_b = [&](int c, float (&dst)[CK][4]) {
    int o = (c * CK) * 4 * (4 * U);
    opaque(o);
#pragma unroll
    for (int j = 0; j < CK; ++j)
#pragma unroll
      for (int q = 0; q < 4; ++q) dst[j][q] = Ub[o + j * 4 * (4 * U) + 16 * q];
  };
  for (int i = tid; i < 2 * 16 * HP; i += U * 4) (&hbuf[0][0][0])[i] = 0.0f;
  float cst[2][2] = {{0.f, 0.f}, {0.f, 0.f}};
  __syncthreads();
  f32x4 xz_next[4];
  auto load_xz = [&](int tt) {
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int bb = b0 + lk * 4 + r;
        xz_next[q][r] = (bb < B) ? xz[(((int64_t)bb * T + tt) * 2 + dir) * (4 * U) + wave * 64 + 16 * q + lj] : 0.0f;
      }
  };
  load_xz(dir ? T - 1 : 0);
  load_b(0, bq[0]);
  for (int step = 0; step < T; ++step) {
    const int t = dir ? (T - 1 - step) : step;
    const int cur = step & 1;
    f32x4 acc[4] = {xz_next[0], xz_next[1], xz_next[2], xz_next[3]};
    if (step + 1 < T) load_xz(dir ? (T - 2 - step) : step + 1);
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      load_b((c + 1) % NC, bq[(c + 1) & 1]);  // the last chunk prefetches the next step's first one (U does not change between steps)
#pragma unroll
      for (int j = 0; j < CK; ++j) {
        const float a = hbuf[cur][lj][(c * CK + j) * 4 + lk];  // A[i = batch][k]
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[q] = mfma16(a, bq[c & 1][j][q], acc[q]);
      }
    }
#pragma unroll
    for (int g = 0; g < 2; ++g) {
      const int unit = wave * 16 + g * 8 + (lj & 7);
      gate_stage(
          acc[2 * g], acc[2 * g + 1], cst[g], lj,
          [&](int r, float g0, float g1) {
            if (!TRAIN) return;
            const int bb = b0 + lk * 4 + r;
            if (bb < B) {
              float* gp = gates + (((int64_t)bb * T + t) * 2 + dir) * (4 * U) + wave * 64 + g * 32 + lj;
              gp[0] = g0;
              gp[16] = g1;
            }
          },
          [&](int j, bool low, float h, float c) {
            const int row = lk * 4 + (low ? j : 2 + j), bb = b0 + row;
            hbuf[cur ^ 1][row][unit] = h;
            if (bb < B) {
              out[((int64_t)bb * T + t) * (2 * U) + dir * U + unit] = h;
              if (TRAIN) cstate[(((int64_t)bb * T + t) * 2 + dir) * U + unit] = c;
            }
          });
    }
    __syncthreads();
  }
}

// Backward through time (train_head.hip lstm_bwd_kernel: the same per-step arithmetic and summation order), U^T streamed from L2.
template <int U>
__global__ __launch_bounds__(U * 4) void lstm_wide_bwd_kernel(const float* __restrict__ dH /*[B][T][2U]*/, const float* __restrict__ gates, const float* __restrict__ cstate,
                                                               const float* __restrict__ Uw /*[2][U][4U] permuted*/, int B, int T,
                                                               float* __restrict__ dxz /*[B][T][2][4U] permuted*/) {
  static_assert(U % 32 == 0 && U <= 256, "units: a multiple of 32 up to 256");
  constexpr int ZP = 4 * U + 4, CK = 4, NC = U / 4 / CK;  // CK float4 k-quads per chunk (16 k-steps), NC chunks per step (even)
  static_assert(NC % 2 == 0, "chunk count must be even");
  extern __shared__ __attribute__((aligned(16))) float smem_lw[];
  float (*dzs)[16][ZP] = reinterpret_cast<float (*)[16][ZP]>(smem_lw);  // [2][16][ZP]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lk = lane >> 4, lj = lane & 15;
  const int dir = blockIdx.y;
  const int b0 = blockIdx.x * 16;
  const int unit = wave * 16 + lj;
  // B operand of k-step s: B[k = lk][j = lj] = U[unit][lk * U + s]: U consecutive floats per lane, read as float4
  const float4* urow = reinterpret_cast<const float4*>(Uw + (int64_t)dir * U * 4 * U + (int64_t)unit * (4 * U) + lk * U);
  float4 bq[2][CK];
  auto load_b = [&](int c, float4 (&dst)[CK]) {
    int o = c * CK;
    opaque(o);
#pragma unroll
    for (int j = 0; j < CK; ++j) dst[j] = urow[o + j];
  };
  float dc[4] = {0.f, 0.f, 0.f, 0.f}, dhr[4] = {0.f, 0.f, 0.f, 0.f};
  const int pl = wave * 64 + (lj >> 3) * 32 + (lj & 7);  // permuted column of gate i of this unit; f, g, o follow at +8, +16, +24
  float pg[4][4], pc[4], pcp[4], pdh[4];
  auto load_step = [&](int step) {
    const int t = dir ? step : (T - 1 - step);
    const int tprev = dir ? t + 1 : t - 1;
    const bool has_prev = dir ? (t + 1 < T) : (t > 0);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int bb = b0 + lk * 4 + r;
      const bool ok = bb < B && step < T;
      const int64_t gbase = ok ? (((int64_t)bb * T + t) * 2 + dir) * (4 * U) + pl : 0;
      pg[r][0] = ok ? gates[gbase] : 0.f; pg[r][1] = ok ? gates[gbase + 8] : 0.f;
      pg[r][2] = ok ? gates[gbase + 16] : 0.f; pg[r][3] = ok ? gates[gbase + 24] : 0.f;
      pc[r] = ok ? cstate[(((int64_t)bb * T + t) * 2 + dir) * U + unit] : 0.f;
      pcp[r] = (ok && has_prev) ? cstate[(((int64_t)bb * T + tprev) * 2 + dir) * U + unit] : 0.f;
      pdh[r] = ok ? dH[((int64_t)bb * T + t) * (2 * U) + dir * U + unit] : 0.f;
    }
  };
  load_step(0);
  load_b(0, bq[0]);
  for (int step = 0; step < T; ++step) {
    const int t = dir ? step : (T - 1 - step);
    const int cur = step & 1;
    float cg[4][4], cc[4], ccp[4], cdh[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      cc[r] = pc[r]; ccp[r] = pcp[r]; cdh[r] = pdh[r];
#pragma unroll
      for (int q = 0; q < 4; ++q) cg[r][q] = pg[r][q];
    }
    load_step(step + 1);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float gi = cg[r][0], gf = cg[r][1], gg = cg[r][2], go = cg[r][3];
      const float c = cc[r], cp = ccp[r];
      const float dh = cdh[r] + dhr[r];
      const float tc = tanhf_(c);
      const float dO = dh * tc;
      const float dct = dc[r] + dh * go * (1.0f - tc * tc);
      dc[r] = dct * gf;
      float* zr = &dzs[cur][lk * 4 + r][pl];  // rows past B carry zero gates, hence zero dz
      zr[0] = dct * gg * gi * (1.0f - gi);
      zr[8] = dct * cp * gf * (1.0f - gf);
      zr[16] = dct * gi * (1.0f - gg * gg);
      zr[24] = dO * go * (1.0f - go);
    }
    __syncthreads();  // dz[cur] of every wave is visible; buffer cur^1 is free again after the next barrier
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int row = i * 4 + lk, bb = b0 + row;
      const float4 v = *reinterpret_cast<const float4*>(&dzs[cur][row][wave * 64 + lj * 4]);
      if (bb < B) *reinterpret_cast<float4*>(dxz + (((int64_t)bb * T + t) * 2 + dir) * (4 * U) + wave * 64 + lj * 4) = v;
    }
    f32x4 acc[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
    const float* arow = &dzs[cur][lj][lk * U];  // A[i = batch lj][k = lk] of k-step s = dz[lj][lk*U + s]
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      load_b((c + 1) % NC, bq[(c + 1) & 1]);
#pragma unroll
      for (int j = 0; j < CK; ++j) {
        const float4 a = *reinterpret_cast<const float4*>(arow + 4 * (c * CK + j));
        const float4 b = bq[c & 1][j];
        acc[0] = mfma16(a.x, b.x, acc[0]);
        acc[1] = mfma16(a.y, b.y, acc[1]);
        acc[2] = mfma16(a.z, b.z, acc[2]);
        acc[3] = mfma16(a.w, b.w, acc[3]);
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) dhr[r] = (acc[0][r] + acc[1][r]) + (acc[2][r] + acc[3][r]);
  }
}

template <int U>
hipError_t launch_fwd(const float* xz, const float* Uw, int B, int T, float* out, float* gates, float* cstate, hipStream_t st) {
  const dim3 grid((B + 15) / 16, 2);
  if (gates)
    hipLaunchKernelGGL((lstm_wide_fwd_kernel<U, true>), grid, dim3(U * 4), 0, st, xz, Uw, B, T, out, gates, cstate);
  else
    hipLaunchKernelGGL((lstm_wide_fwd_kernel<U, false>), grid, dim3(U * 4), 0, st, xz, Uw, B, T, out, gates, cstate);
  return hipGetLastError();
}

template <int U>
hipError_t launch_bwd(const float* dH, const float* gates, const float* cstate, const float* Uw, int B, int T, float* dxz, hipStream_t st) {
  const size_t lds = (size_t)2 * 16 * (4 * U + 4) * sizeof(float);  // 83 456 B at U = 160 ... 131 584 B at U = 256: above 64 KiB
  if (const hipError_t e = orcai_lds::ensure_dynamic_lds<lstm_wide_bwd_kernel<U>>(lds); e != hipSuccess) return e;
  hipLaunchKernelGGL(lstm_wide_bwd_kernel<U>, dim3((B + 15) / 16, 2), dim3(U * 4), lds, st, dH, gates, cstate, Uw, B, T, dxz);
  return hipGetLastError();
}

}  // namespace

// Internal entry points of orcai_lstm_recurrent / orcai_lstm_train_fwd / orcai_lstm_bwd and their orcai_h_ twins for 128 < units <= 256
// (multiples of 32); the callers have checked the pointers and B, T > 0.  gates == NULL: inference (out only).  Hidden: not part of the
// library's C ABI (include/orcai_hip.h lists every exported symbol).
__attribute__((visibility("hidden"))) int lstm_wide_fwd_launch(const float* xz, const float* Uw, int B, int T, int units, float* out, float* gates, float* cstate, void* stream) {
  if (gates && !cstate) return ORCAI_E_BADARG;
  hipStream_t st = (hipStream_t)stream;
  switch (units) {
    case 160: return (int)launch_fwd<160>(xz, Uw, B, T, out, gates, cstate, st);
    case 192: return (int)launch_fwd<192>(xz, Uw, B, T, out, gates, cstate, st);
    case 224: return (int)launch_fwd<224>(xz, Uw, B, T, out, gates, cstate, st);
    case 256: return (int)launch_fwd<256>(xz, Uw, B, T, out, gates, cstate, st);
    default: return ORCAI_E_BADARG;
  }
}

__attribute__((visibility("hidden"))) int lstm_wide_bwd_launch(const float* dH, const float* gates, const float* cstate, const float* Uw, int B, int T, int units, float* dxz, void* stream) {
  if (((uintptr_t)Uw | (uintptr_t)dxz) & 15) return ORCAI_E_BADARG;  // float4 reads of U rows, float4 stores of dxz rows
  hipStream_t st = (hipStream_t)stream;
  switch (units) {  // the > 64 KiB LDS opt-in happens on a device's first call per width, which is never inside a capture (lds_optin.h)
    case 160: return (int)launch_bwd<160>(dH, gates, cstate, Uw, B, T, dxz, st);
    case 192: return (int)launch_bwd<192>(dH, gates, cstate, Uw, B, T, dxz, st);
    case 224: return (int)launch_bwd<224>(dH, gates, cstate, Uw, B, T, dxz, st);
    case 256: return (int)launch_bwd<256>(dH, gates, cstate, Uw, B, T, dxz, st);
    default: return ORCAI_E_BADARG;
  }
}
