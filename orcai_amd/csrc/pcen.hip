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
  e = orcai_hist_level1(out, n, workspace, stream);
  if (e) return e;
  e = orcai_quantile_select(out, n, rank_lo, rank_hi, workspace, stream);
  if (e) return e;
  e = orcai_frontend_finalize(0, 0.0f, workspace, stream);
  if (e) return e;
  return orcai_clip_normalize(out, n, workspace, stream);
}

}  // extern "C"
