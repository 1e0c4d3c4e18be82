// pcen.hip -- per-channel energy normalisation (spectrogram parameter "pcen"; orcai_amd/pcen.py holds the definition and its float64 specification).
//
//   S = scale E,  M[0] = S[0],  M[t] = a M[t-1] + b S[t],  out = (S (eps + M)^-gain + bias)^power - bias^power
//
// The smoother is a first-order recursion along time, [T, K] row-major with K contiguous: a chunked scan, ORCAI_PCEN_CHUNK frames per chunk, in three
// launches.  Lanes run across columns: thread = one (chunk, column) chain, flat index chunk * K + column, so a wave's 64 lanes read 64 consecutive
// floats of a row whatever K is (171 needs no padding); only the lanes that straddle two chunks split a row access in two.
//   1  pcen_partial_kernel   per (chunk j, column): the chain m = fma(a, m, b s) over the chunk from m = 0 -- for chunk 0 from M[0] = S[0] --> P[j][k]
//   2  pcen_carry_kernel     per column, in chunk order: C[0] = P[0], C[j] = fma(a^L_j, C[j-1], P[j]), L_j the chunk's own length (the last one is short)
//   3  pcen_apply_kernel     per (chunk, column): the chain again from C[j-1], the PCEN value written over the energy just read
// Every sum has one fixed order (no atomics, nothing depends on the grid), so the same input gives the same bytes on every launch.
// HBM: x read twice and written once, 2 x 4 bytes per (chunk, column) of partials and carries.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "orcai_hip.h"

namespace {

constexpr int L = ORCAI_PCEN_CHUNK;
constexpr int UNROLL = 8;  // row loads in flight per chain ahead of the dependent fma chain

struct PcenArgs {
  float a, b, scale, gain, bias, power, eps;
};

__device__ __forceinline__ float hw_pow(float x, float p) {  // x^p = exp2(p log2 x) on v_log_f32 / v_exp_f32: log2(0) = -inf, exp2(-inf) = 0
  return __builtin_amdgcn_exp2f(p * __builtin_amdgcn_logf(x));
}

// One chain over frames [t0, t0 + len) of column k.  APPLY = false: returns the end state.  APPLY = true: also writes the PCEN values in place.
// first: the chain starts the recording, M[t0] = S[t0], and m_in is ignored.
template <bool APPLY>
__device__ __forceinline__ float pcen_chain(float* __restrict__ x, int64_t t0, int len, int K, int k, float m_in, bool first, const PcenArgs& p) {
  float* col = x + t0 * (int64_t)K + k;
  // bias^power by the very instructions that form the value below: a zero energy gives fma(0, r, bias) = bias and therefore exactly 0
  const float bias_pow = hw_pow(p.bias, p.power);
  float m = m_in;
  int i = 0;
  auto step = [&](float e, int ii) {
    const float s = p.scale * e;
    m = (first && ii == 0) ? s : fmaf(p.a, m, p.b * s);
    if constexpr (APPLY) {
      const float r = hw_pow(p.eps + m, -p.gain);
      col[(int64_t)ii * K] = hw_pow(fmaf(s, r, p.bias), p.power) - bias_pow;
    }
  };
  for (; i + UNROLL <= len; i += UNROLL) {
    float e[UNROLL];
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) e[u] = col[(int64_t)(i + u) * K];
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) step(e[u], i + u);
  }
  for (; i < len; ++i) step(col[(int64_t)i * K], i);
  return m;
}

__global__ __launch_bounds__(256) void pcen_partial_kernel(float* __restrict__ x, int64_t T, int K, int64_t n_chains, PcenArgs p, float* __restrict__ partial) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= n_chains) return;
  const int64_t j = idx / K;
  const int k = (int)(idx - j * K);
  const int64_t t0 = j * L;
  const int len = (int)(T - t0 < L ? T - t0 : L);
  partial[idx] = pcen_chain<false>(x, t0, len, K, k, 0.0f, j == 0, p);
}

// K threads in all; the partials of a column are independent loads (a batch is requested whole before its dependent chain runs).
__global__ __launch_bounds__(64) void pcen_carry_kernel(const float* __restrict__ partial, float* __restrict__ carry, int64_t n_chunks, int K, float a_chunk, float a_last) {
  const int k = blockIdx.x * 64 + threadIdx.x;
  if (k >= K) return;
  constexpr int B = 16;
  float c = partial[k];
  carry[k] = c;
  int64_t j = 1;
  for (; j + B <= n_chunks - 1; j += B) {  // full chunks only: the last chunk (index n_chunks - 1) may be short
    float q[B];
#pragma unroll
    for (int u = 0; u < B; ++u) q[u] = partial[(j + u) * K + k];
#pragma unroll
    for (int u = 0; u < B; ++u) {
      c = fmaf(a_chunk, c, q[u]);
      carry[(j + u) * K + k] = c;
    }
  }
  for (; j < n_chunks; ++j) {
    c = fmaf(j == n_chunks - 1 ? a_last : a_chunk, c, partial[j * K + k]);
    carry[j * K + k] = c;
  }
}

__global__ __launch_bounds__(256) void pcen_apply_kernel(float* __restrict__ x, int64_t T, int K, int64_t n_chains, PcenArgs p, const float* __restrict__ carry) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= n_chains) return;
  const int64_t j = idx / K;
  const int k = (int)(idx - j * K);
  const int64_t t0 = j * L;
  const int len = (int)(T - t0 < L ? T - t0 : L);
  const float m_in = j > 0 ? carry[idx - K] : 0.0f;
  pcen_chain<true>(x, t0, len, K, k, m_in, j == 0, p);
}

// ---------------------------------------------------------------- backward (orcai_pcen_bwd; definition in include/orcai_hip.h)
// g = dL/dout -> dE = dL/dE with p_lo / p_hi constants read from stats[2..3].  The smoother's adjoint is the same first-order recursion run BACKWARD
// in time, lambda[t] = q[t] + a lambda[t+1]: a second chunked scan, mirrored.  Six launches, the layout and the thread-per-(chunk, column) of the forward:
//   1  pcen_partial_kernel       as the forward (E is only read)
//   2  pcen_carry_kernel         as the forward
//   3  pcen_bwd_local_kernel     the forward chain from C[j-1], step by step the instructions of pcen_chain<true> -- so y, and with it the clip's
//                                gate, is the forward's bit for bit -- then h, d = h r (direct path) and q = -gain d S / (eps + M) (dL/dM, local) --> two planes
//   4  pcen_rpartial_kernel      per (chunk j, column): lambda = fma(a, lambda, q[t]) from 0, last frame of the chunk to its first --> R[j][k]
//   5  pcen_rcarry_kernel        per column, chunks descending: D[last] = R[last], D[j] = fma(a^L_j, D[j+1], R[j]); every j < last is a full chunk
//   6  pcen_bwd_apply_kernel     the reverse chain again from D[j+1], dE[t] = scale (d[t] + b lambda[t]), and scale (d[0] + lambda[0]) at frame 0
// HBM: E read twice, g once, d and q written once, q read twice, d once, dE written once: 9 passes of T K floats.
template <bool APPLY>
__device__ __forceinline__ float pcen_rchain(const float* __restrict__ dplane, const float* __restrict__ qplane, float* __restrict__ dE, int64_t t0, int len, int K, int k,
                                             float lam_in, bool first, const PcenArgs& p) {
  const int64_t base = t0 * (int64_t)K + k;
  float lam = lam_in;
  int i = len - 1;
  auto step = [&](float q, float d, int ii) {
    lam = fmaf(p.a, lam, q);
    if constexpr (APPLY) dE[base + (int64_t)ii * K] = p.scale * ((first && ii == 0) ? d + lam : fmaf(p.b, lam, d));
  };
  for (; i - UNROLL + 1 >= 0; i -= UNROLL) {
    float q[UNROLL], d[UNROLL];
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      q[u] = qplane[base + (int64_t)(i - u) * K];
      d[u] = APPLY ? dplane[base + (int64_t)(i - u) * K] : 0.0f;
    }
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) step(q[u], d[u], i - u);
  }
  for (; i >= 0; --i) step(qplane[base + (int64_t)i * K], APPLY ? dplane[base + (int64_t)i * K] : 0.0f, i);
  return lam;
}

__global__ __launch_bounds__(256) void pcen_bwd_local_kernel(const float* __restrict__ x, const float* __restrict__ gout, const float* __restrict__ stats, int64_t T, int K,
                                                              int64_t n_chains, PcenArgs p, const float* __restrict__ carry, float* __restrict__ dplane,
                                                              float* __restrict__ qplane) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= n_chains) return;
  const int64_t j = idx / K;
  const int k = (int)(idx - j * K);
  const int64_t t0 = j * L;
  const int len = (int)(T - t0 < L ? T - t0 : L);
  const bool first = j == 0;
  const float p_lo = stats[2], p_hi = stats[3];
  const float range = p_hi - p_lo;
  const int64_t base = t0 * (int64_t)K + k;
  const float bias_pow = hw_pow(p.bias, p.power);
  float m = j > 0 ? carry[idx - K] : 0.0f;
  int i = 0;
  auto step = [&](float e, float g, int ii) {
    const float s = p.scale * e;  // down to y: pcen_chain<true>
    m = (first && ii == 0) ? s : fmaf(p.a, m, p.b * s);
    const float em = p.eps + m;
    const float r = hw_pow(em, -p.gain);
    const float u = fmaf(s, r, p.bias);
    const float y = hw_pow(u, p.power) - bias_pow;
    const bool open = y > p_lo && y < p_hi;  // clip_normalize_kernel's clamp leaves y as it is exactly there
    const float h = (g / range) * p.power * hw_pow(u, p.power - 1.0f);
    const float d = open ? h * r : 0.0f;  // selects: h may be inf or NaN where the gate is shut (u = 0, p_hi = p_lo)
    dplane[base + (int64_t)ii * K] = d;
    qplane[base + (int64_t)ii * K] = open ? -p.gain * (d * (s / em)) : 0.0f;
  };
  for (; i + UNROLL <= len; i += UNROLL) {
    float e[UNROLL], g[UNROLL];
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      e[u] = x[base + (int64_t)(i + u) * K];
      g[u] = gout[base + (int64_t)(i + u) * K];
    }
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) step(e[u], g[u], i + u);
  }
  for (; i < len; ++i) step(x[base + (int64_t)i * K], gout[base + (int64_t)i * K], i);
}

__global__ __launch_bounds__(256) void pcen_rpartial_kernel(const float* __restrict__ qplane, int64_t T, int K, int64_t n_chains, PcenArgs p, float* __restrict__ rpartial) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= n_chains) return;
  const int64_t j = idx / K;
  const int k = (int)(idx - j * K);
  const int64_t t0 = j * L;
  const int len = (int)(T - t0 < L ? T - t0 : L);
  rpartial[idx] = pcen_rchain<false>(nullptr, qplane, nullptr, t0, len, K, k, 0.0f, false, p);
}

// pcen_carry_kernel mirrored: chunks in descending order, every multiplier a^256 (the short last chunk starts the chain and multiplies nothing).
__global__ __launch_bounds__(64) void pcen_rcarry_kernel(const float* __restrict__ rpartial, float* __restrict__ rcarry, int64_t n_chunks, int K, float a_chunk) {
  const int k = blockIdx.x * 64 + threadIdx.x;
  if (k >= K) return;
  constexpr int B = 16;
  float c = rpartial[(n_chunks - 1) * K + k];
  rcarry[(n_chunks - 1) * K + k] = c;
  int64_t j = n_chunks - 2;
  for (; j - B + 1 >= 0; j -= B) {
    float q[B];
#pragma unroll
    for (int u = 0; u < B; ++u) q[u] = rpartial[(j - u) * K + k];
#pragma unroll
    for (int u = 0; u < B; ++u) {
      c = fmaf(a_chunk, c, q[u]);
      rcarry[(j - u) * K + k] = c;
    }
  }
  for (; j >= 0; --j) {
    c = fmaf(a_chunk, c, rpartial[j * K + k]);
    rcarry[j * K + k] = c;
  }
}

__global__ __launch_bounds__(256) void pcen_bwd_apply_kernel(const float* __restrict__ dplane, const float* __restrict__ qplane, int64_t T, int K, int64_t n_chains,
                                                              int64_t n_chunks, PcenArgs p, const float* __restrict__ rcarry, float* __restrict__ dE) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= n_chains) return;
  const int64_t j = idx / K;
  const int k = (int)(idx - j * K);
  const int64_t t0 = j * L;
  const int len = (int)(T - t0 < L ? T - t0 : L);
  const float lam_in = j + 1 < n_chunks ? rcarry[idx + K] : 0.0f;
  pcen_rchain<true>(dplane, qplane, dE, t0, len, K, k, lam_in, j == 0, p);
}

}  // namespace

extern "C" {

size_t orcai_pcen_scratch_bytes(int64_t n_frames, int k) {
  if (n_frames <= 0 || k <= 0) return 0;
  const int64_t n_chunks = (n_frames + L - 1) / L;
  return (size_t)(2 * n_chunks * k) * sizeof(float);
}

// ev: null, or four events recorded around the three launches (orcai_pcen_stage_ms).
static int pcen_launch(float* x, int64_t n_frames, int k, float a, float b, float scale, float gain, float bias, float power, float eps, void* scratch, void* stream,
                       hipEvent_t* ev) {
  if (!x || !scratch || n_frames <= 0 || k <= 0 || ((uintptr_t)x & 3) || ((uintptr_t)scratch & 3)) return ORCAI_E_BADARG;
  if (!(a >= 0.0f && a < 1.0f) || !(b > 0.0f && b <= 1.0f) || !(scale > 0.0f) || !(gain >= 0.0f && gain <= 1.0f) || !(bias >= 0.0f) ||
      !(power > 0.0f && power <= 1.0f) || !(eps > 0.0f))
    return ORCAI_E_BADARG;
  const int64_t n_chunks = (n_frames + L - 1) / L;
  const int64_t n_chains = n_chunks * k;
  const int64_t blocks = (n_chains + 255) / 256;
  if (blocks > 0x7fffffff) return ORCAI_E_UNSUPPORTED;
  const int last_len = (int)(n_frames - (n_chunks - 1) * L);
  const float a_chunk = (float)std::pow((double)a, (double)L), a_last = (float)std::pow((double)a, (double)last_len);
  const PcenArgs p{a, b, scale, gain, bias, power, eps};
  float* partial = (float*)scratch;
  float* carry = partial + n_chains;
  hipStream_t st = (hipStream_t)stream;
  if (ev) (void)hipEventRecord(ev[0], st);
  hipLaunchKernelGGL(pcen_partial_kernel, dim3((unsigned)blocks), dim3(256), 0, st, x, n_frames, k, n_chains, p, partial);
  if (ev) (void)hipEventRecord(ev[1], st);
  hipLaunchKernelGGL(pcen_carry_kernel, dim3((unsigned)((k + 63) / 64)), dim3(64), 0, st, (const float*)partial, carry, n_chunks, k, a_chunk, a_last);
  if (ev) (void)hipEventRecord(ev[2], st);
  hipLaunchKernelGGL(pcen_apply_kernel, dim3((unsigned)blocks), dim3(256), 0, st, x, n_frames, k, n_chains, p, (const float*)carry);
  if (ev) (void)hipEventRecord(ev[3], st);
  return (int)hipGetLastError();
}

int orcai_pcen(float* x, int64_t n_frames, int k, float a, float b, float scale, float gain, float bias, float power, float eps, void* scratch, void* stream) {
  return pcen_launch(x, n_frames, k, a, b, scale, gain, bias, power, eps, scratch, stream, nullptr);
}

int orcai_pcen_stage_ms(float* x, int64_t n_frames, int k, float a, float b, float scale, float gain, float bias, float power, float eps, void* scratch, void* stream,
                        float stage_ms[3]) {
  if (!stage_ms) return ORCAI_E_BADARG;
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
  hipError_t e = hipSuccess;
  for (int i = 0; i < 4 && e == hipSuccess; ++i) e = hipEventCreate(&ev[i]);
  int rc = (int)e;
  if (!rc) rc = pcen_launch(x, n_frames, k, a, b, scale, gain, bias, power, eps, scratch, stream, ev);
  if (!rc) rc = (int)hipEventSynchronize(ev[3]);
  for (int i = 0; i < 3 && !rc; ++i) rc = (int)hipEventElapsedTime(&stage_ms[i], ev[i], ev[i + 1]);
  for (int i = 0; i < 4; ++i)
    if (ev[i]) (void)hipEventDestroy(ev[i]);
  return rc;
}

size_t orcai_pcen_bwd_scratch_bytes(int64_t n_frames, int k) {
  if (n_frames <= 0 || k <= 0) return 0;
  const int64_t n_chunks = (n_frames + L - 1) / L;
  return (size_t)(4 * n_chunks * k + 2 * n_frames * k) * sizeof(float);
}

// ev: null, or seven events recorded around the six launches (orcai_pcen_bwd_stage_ms).
static int pcen_bwd_launch(const float* E, const float* gout, const float* stats_dev, int64_t n_frames, int k, float a, float b, float scale, float gain, float bias,
                           float power, float eps, float* dE, void* scratch, void* stream, hipEvent_t* ev) {
  if (!E || !gout || !stats_dev || !dE || !scratch || n_frames <= 0 || k <= 0) return ORCAI_E_BADARG;
  if (((uintptr_t)E & 3) || ((uintptr_t)gout & 3) || ((uintptr_t)stats_dev & 3) || ((uintptr_t)dE & 3) || ((uintptr_t)scratch & 3)) return ORCAI_E_BADARG;
  if (!(a >= 0.0f && a < 1.0f) || !(b > 0.0f && b <= 1.0f) || !(scale > 0.0f) || !(gain >= 0.0f && gain <= 1.0f) || !(bias >= 0.0f) ||
      !(power > 0.0f && power <= 1.0f) || !(eps > 0.0f))
    return ORCAI_E_BADARG;
  const int64_t n_chunks = (n_frames + L - 1) / L;
  const int64_t n_chains = n_chunks * k;
  const int64_t blocks = (n_chains + 255) / 256;
  if (blocks > 0x7fffffff) return ORCAI_E_UNSUPPORTED;
  const int last_len = (int)(n_frames - (n_chunks - 1) * L);
  const float a_chunk = (float)std::pow((double)a, (double)L), a_last = (float)std::pow((double)a, (double)last_len);
  const PcenArgs p{a, b, scale, gain, bias, power, eps};
  float* partial = (float*)scratch;
  float* carry = partial + n_chains;
  float* rpartial = carry + n_chains;
  float* rcarry = rpartial + n_chains;
  float* dplane = rcarry + n_chains;
  float* qplane = dplane + n_frames * (int64_t)k;
  const dim3 grid((unsigned)blocks), cols((unsigned)((k + 63) / 64));
  hipStream_t st = (hipStream_t)stream;
  int n_ev = 0;
  auto mark = [&]() {
    if (ev) (void)hipEventRecord(ev[n_ev++], st);
  };
  mark();
  hipLaunchKernelGGL(pcen_partial_kernel, grid, dim3(256), 0, st, const_cast<float*>(E), n_frames, k, n_chains, p, partial);  // APPLY = false: reads only
  mark();
  hipLaunchKernelGGL(pcen_carry_kernel, cols, dim3(64), 0, st, (const float*)partial, carry, n_chunks, k, a_chunk, a_last);
  mark();
  hipLaunchKernelGGL(pcen_bwd_local_kernel, grid, dim3(256), 0, st, E, gout, stats_dev, n_frames, k, n_chains, p, (const float*)carry, dplane, qplane);
  mark();
  hipLaunchKernelGGL(pcen_rpartial_kernel, grid, dim3(256), 0, st, (const float*)qplane, n_frames, k, n_chains, p, rpartial);
  mark();
  hipLaunchKernelGGL(pcen_rcarry_kernel, cols, dim3(64), 0, st, (const float*)rpartial, rcarry, n_chunks, k, a_chunk);
  mark();
  hipLaunchKernelGGL(pcen_bwd_apply_kernel, grid, dim3(256), 0, st, (const float*)dplane, (const float*)qplane, n_frames, k, n_chains, n_chunks, p, (const float*)rcarry, dE);
  mark();
  return (int)hipGetLastError();
}

int orcai_pcen_bwd(const float* E, const float* gout, const float* stats_dev, int64_t n_frames, int k, float a, float b, float scale, float gain, float bias,
                   float power, float eps, float* dE, void* scratch, void* stream) {
  return pcen_bwd_launch(E, gout, stats_dev, n_frames, k, a, b, scale, gain, bias, power, eps, dE, scratch, stream, nullptr);
}

int orcai_pcen_bwd_stage_ms(const float* E, const float* gout, const float* stats_dev, int64_t n_frames, int k, float a, float b, float scale, float gain, float bias,
                            float power, float eps, float* dE, void* scratch, void* stream, float stage_ms[6]) {
  if (!stage_ms) return ORCAI_E_BADARG;
  hipEvent_t ev[7] = {};
  hipError_t e = hipSuccess;
  for (int i = 0; i < 7 && e == hipSuccess; ++i) e = hipEventCreate(&ev[i]);
  int rc = (int)e;
  if (!rc) rc = pcen_bwd_launch(E, gout, stats_dev, n_frames, k, a, b, scale, gain, bias, power, eps, dE, scratch, stream, ev);
  if (!rc) rc = (int)hipEventSynchronize(ev[6]);
  for (int i = 0; i < 6 && !rc; ++i) rc = (int)hipEventElapsedTime(&stage_ms[i], ev[i], ev[i + 1]);
  for (int i = 0; i < 7; ++i)
    if (ev[i]) (void)hipEventDestroy(ev[i]);
  return rc;
}

size_t orcai_pcen_spectrogram_bwd_scratch_bytes(int64_t n_frames, int k) {
  if (n_frames <= 0 || k <= 0) return 0;
  return orcai_pcen_bwd_scratch_bytes(n_frames, k) + (size_t)(2 * ((n_frames * k + 3) & ~(int64_t)3)) * sizeof(float);
}

int orcai_pcen_spectrogram_bwd(const float* pcm, int64_t n_samples, int n_fft, int hop, int64_t n_frames, int k, const int* band_lo, const int* band_hi,
                               const int* band_off, const float* weights, int n_weights, float a, float b, float scale, float gain, float bias, float power,
                               float eps, const float* gout, const float* stats_dev, float* dpcm, void* scratch, void* stream) {
  if (!pcm || !gout || !stats_dev || !dpcm || !scratch || k < 1 || n_frames <= 0 || ((uintptr_t)scratch & 15) || ((uintptr_t)gout & 3) || ((uintptr_t)stats_dev & 3) ||
      ((uintptr_t)dpcm & 3))
    return ORCAI_E_BADARG;  // what the later steps would refuse, before the first one runs
  if (!(a >= 0.0f && a < 1.0f) || !(b > 0.0f && b <= 1.0f) || !(scale > 0.0f) || !(gain >= 0.0f && gain <= 1.0f) || !(bias >= 0.0f) ||
      !(power > 0.0f && power <= 1.0f) || !(eps > 0.0f))
    return ORCAI_E_BADARG;
  // scratch: E | dE, each n_frames * k floats rounded up to 16 bytes (orcai_stft_energy writes float4), then orcai_pcen_bwd's own
  const int64_t plane = (n_frames * (int64_t)k + 3) & ~(int64_t)3;
  float* E = (float*)scratch;
  float* dE = E + plane;
  void* scan = dE + plane;
  int e = band_lo ? orcai_stft_mel_energy(pcm, n_samples, n_fft, hop, n_frames, k, band_lo, band_hi, band_off, weights, n_weights, E, stream)
                  : orcai_stft_energy(pcm, n_samples, n_fft, hop, n_frames, k, E, stream);
  if (e) return e;  // every refusal of the transform's arguments lands here, before anything is launched
  e = orcai_pcen_bwd(E, gout, stats_dev, n_frames, k, a, b, scale, gain, bias, power, eps, dE, scan, stream);
  if (e) return e;
  return band_lo ? orcai_stft_mel_energy_bwd(pcm, n_samples, n_fft, hop, n_frames, k, band_lo, band_hi, band_off, weights, n_weights, dE, dpcm, stream)
                 : orcai_stft_energy_bwd(pcm, n_samples, n_fft, hop, n_frames, k, dE, dpcm, stream);
}

int orcai_make_pcen_spectrogram(const float* pcm, int64_t n_samples, int n_fft, int hop, int64_t n_frames, int k, const int* band_lo, const int* band_hi,
                                const int* band_off, const float* weights, int n_weights, float a, float b, float scale, float gain, float bias, float power,
                                float eps, int64_t rank_lo, int64_t rank_hi, float* out, void* scratch, void* workspace, void* stream) {
  const int64_t n = n_frames * (int64_t)k;
  if (!workspace || !out || !scratch || k < 1 || n_frames <= 0 || rank_lo < 0 || rank_hi < 0 || rank_lo >= n || rank_hi >= n)
    return ORCAI_E_BADARG;  // what the later steps would refuse, before the first one runs
  int e = orcai_frontend_reset(workspace, stream);
  if (e) return e;
  e = band_lo ? orcai_stft_mel_energy(pcm, n_samples, n_fft, hop, n_frames, k, band_lo, band_hi, band_off, weights, n_weights, out, stream)
              : orcai_stft_energy(pcm, n_samples, n_fft, hop, n_frames, k, out, stream);
  if (e) return e;
  e = orcai_pcen(out, n_frames, k, a, b, scale, gain, bias, power, eps, scratch, stream);
  if (e) return e;
  e = orcai_quantile_select_radix(out, n, rank_lo, rank_hi, workspace, stream);  // PCEN values crowd below 0.125, the level-1 map's single bucket
  if (e) return e;
  e = orcai_frontend_finalize(0, 0.0f, workspace, stream);
  if (e) return e;
  return orcai_clip_normalize(out, n, workspace, stream);
}

}  // extern "C"
