// resample.hip -- rational-ratio polyphase resampler for gfx950.
//
// Replaces the resampling half of librosa.load(sr=...) (reference src/orcAI/spectrogram.py:23-27, which uses
// libsoxr "soxr_hq").  soxr is not available in this image, so bit parity with it is impossible ("parity
// unpinned"); this is a Kaiser-windowed-sinc polyphase filter (64 zero crossings, beta 14.77,
// roll-off 0.9475) whose table is designed on the host in float64 (orcai_amd/resample.py).
//   out[n] = sum_j x[i0 - half + 1 + j] * table[phase][j],   i0 = floor(n*M/L), phase = (n*M) mod L
#include <hip/hip_runtime.h>

#include <cstdint>

#include "orcai_hip.h"

namespace {

__global__ __launch_bounds__(256) void resample_kernel(const float* __restrict__ x, int64_t n_in, float* __restrict__ out, int64_t n_out, int L, int M,
                                                        const float* __restrict__ table /*[L][ntaps]*/, int ntaps) {
  const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (n >= n_out) return;
  const int64_t num = n * (int64_t)M;
  const int64_t i0 = num / L;
  const int ph = (int)(num - i0 * L);
  const float* h = table + (int64_t)ph * ntaps;
  const int64_t k0 = i0 - ntaps / 2 + 1;
  float acc0 = 0.f, acc1 = 0.f, acc2 = 0.f, acc3 = 0.f;  // 4 partial sums: shorter dependency chains, fixed order
  if (k0 >= 0 && k0 + ntaps <= n_in) {
    const float* xp = x + k0;
    for (int j = 0; j < ntaps; j += 4) {
      acc0 = fmaf(xp[j], h[j], acc0);
      acc1 = fmaf(xp[j + 1], h[j + 1], acc1);
      acc2 = fmaf(xp[j + 2], h[j + 2], acc2);
      acc3 = fmaf(xp[j + 3], h[j + 3], acc3);
    }
  } else {
    for (int j = 0; j < ntaps; j += 4) {
      const int64_t k = k0 + j;
      acc0 = fmaf((k >= 0 && k < n_in) ? x[k] : 0.f, h[j], acc0);
      acc1 = fmaf((k + 1 >= 0 && k + 1 < n_in) ? x[k + 1] : 0.f, h[j + 1], acc1);
      acc2 = fmaf((k + 2 >= 0 && k + 2 < n_in) ? x[k + 2] : 0.f, h[j + 2], acc2);
      acc3 = fmaf((k + 3 >= 0 && k + 3 < n_in) ? x[k + 3] : 0.f, h[j + 3], acc3);
    }
  }
  out[n] = (acc0 + acc1) + (acc2 + acc3);
}

// The adjoint: dx[k] = sum_n dout[n] * table[(n*M) mod L][k - (floor(n*M/L) - ntaps/2 + 1)] over the outputs n whose window holds k, i.e. (h = ntaps/2)
// floor(n*M/L) in [k - h, k + h - 1], i.e. n in [ceil((k-h)*L/M), ceil((k+h)*L/M)).  Gather form: one lane owns one k and adds its terms in ascending n.
//
// Layout.  For ONE k the terms walk through the table with a stride of M mod L rows, so a lane that ran its own n-range would touch a different cache line
// with every load, and so would its 63 neighbours.  Instead the n-loop is WAVE-uniform: a wave owns 64 consecutive k and walks the union of their
// n-ranges; n, the phase, floor(n*M/L) and dout[n] live in scalar registers, and the 64 lanes read 64 consecutive taps table[phase][j0 + lane] of one row,
// one coalesced load.  The price is the lanes whose k lies outside the window of the current n: of the (64 + ntaps)*L/M steps of a wave a lane uses
// ntaps*L/M (2/3 at 128 taps, 4/5 at 280).  The steps whose window covers all 64 lanes (floor(n*M/L) in [kb + 63 - h, kb + h - 1]) run without the
// per-lane test; the steps before and after clamp the tap index and select 0.  Nothing is staged in LDS, so there is no table size the kernel refuses;
// the table (1 KB .. a few 100 KB) is read through L1/L2.  Phase and floor(n*M/L) advance by addition (no 64-bit division in the loop); every product of a
// sample index with L or M is 64-bit.
// `c` is the tap of the current n that weighs the wave's first k: h - 1 - (floor(n*M/L) - kb); lane l reads tap c + l.
template <bool CHECK>
__device__ __forceinline__ float resample_bwd_steps(float acc, int64_t n, int64_t n_end, int& ph, int& c, int lane, int L, int Mq, int Mr, int ntaps,
                                                    const float* __restrict__ dout, const float* __restrict__ table) {
  // the row base (CHECK) or the address of tap c (otherwise) advances by one of two uniform strides: no multiplication in the loop
  const float* p = table + ((int64_t)ph * ntaps + (CHECK ? 0 : c));
  const int64_t step = (int64_t)Mr * ntaps - (CHECK ? 0 : Mq), step_wrap = step - (int64_t)L * ntaps - (CHECK ? 0 : 1);
  auto one = [&](int64_t m) {
    if (CHECK) {
      // Neither load may feed the select directly: the compiler turns a select on a loaded value into a branch around the load with a wait of its own,
      // one per step.  The tap is loaded at a clamped index and always multiplied; dout[n] passes through readfirstlane (it is uniform: a register copy).
      const int j = lane + c;
      const float d = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, dout[m])));
      acc = fmaf((unsigned)j < (unsigned)ntaps ? d : 0.f, p[(unsigned)min(max(j, 0), ntaps - 1)], acc);
    } else {
      acc = fmaf(dout[m], p[(unsigned)lane], acc);  // a uniform base and the lane: no address arithmetic per lane
    }
    ph += Mr;
    c -= Mq;
    const bool wrap = ph >= L;
    p += wrap ? step_wrap : step;
    if (wrap) {
      ph -= L;
      --c;
    }
  };
  for (; n + 4 <= n_end; n += 4) {  // unrolled by hand (readfirstlane is convergent: the compiler would not): four loads in flight
    one(n);
    one(n + 1);
    one(n + 2);
    one(n + 3);
  }
  for (; n < n_end; ++n) one(n);
  return acc;
}

__device__ __forceinline__ int64_t ceil_mul_div(int64_t a, int L, int M) {  // ceil(a*L/M) for a >= 0
  return (a * (int64_t)L + (M - 1)) / M;
}

__global__ __launch_bounds__(256) void resample_bwd_kernel(const float* __restrict__ dout, int64_t n_out, float* __restrict__ dx, int64_t n_in, int L, int M,
                                                            const float* __restrict__ table /*[L][ntaps]*/, int ntaps) {
  const int64_t kb = (int64_t)blockIdx.x * 256 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x & ~63u));  // the wave's first k: uniform
  if (kb >= n_in) return;
  const int lane = (int)(threadIdx.x & 63u);
  const int h = ntaps / 2;
  // [n0, n3): every n whose window meets [kb, kb + 63]; [n1, n2): those whose window covers all of it (empty for short filters); clipped to [0, n_out)
  auto first_n = [&](int64_t a) -> int64_t { return a <= 0 ? 0 : min(ceil_mul_div(a, L, M), n_out); };
  const int64_t n0 = first_n(kb - h), n3 = first_n(kb + 63 + h);
  const int64_t n1 = min(max(first_n(kb + 63 - h), n0), n3), n2 = min(max(first_n(kb + h), n1), n3);
  const int64_t num = n0 * (int64_t)M, i0 = num / L;
  int ph = (int)(num - i0 * L);
  int c = h - 1 - (int)(i0 - kb);  // |i0 - kb| <= h + 63 + M/L
  const int Mq = M / L, Mr = M % L;
  float acc = 0.f;
  acc = resample_bwd_steps<true>(acc, n0, n1, ph, c, lane, L, Mq, Mr, ntaps, dout, table);
  acc = resample_bwd_steps<false>(acc, n1, n2, ph, c, lane, L, Mq, Mr, ntaps, dout, table);
  acc = resample_bwd_steps<true>(acc, n2, n3, ph, c, lane, L, Mq, Mr, ntaps, dout, table);
  if (kb + lane < n_in) dx[kb + lane] = acc;
}

}  // namespace

extern "C" int orcai_resample_polyphase_bwd(const float* dout, int64_t n_out, float* dx, int64_t n_in, int L, int M, const float* table, int ntaps,
                                            void* stream) {
  if (!dout || !dx || !table || n_in <= 0 || n_out <= 0 || L <= 0 || M <= 0 || ntaps <= 0 || (ntaps & 3)) return ORCAI_E_BADARG;
  hipLaunchKernelGGL(resample_bwd_kernel, dim3((unsigned)((n_in + 255) / 256)), dim3(256), 0, (hipStream_t)stream, dout, n_out, dx, n_in, L, M, table, ntaps);
  return (int)hipGetLastError();
}

extern "C" int orcai_resample_polyphase(const float* x, int64_t n_in, float* out, int64_t n_out, int L, int M, const float* table, int ntaps,
                                        void* stream) {
  if (!x || !out || !table || n_in <= 0 || n_out <= 0 || L <= 0 || M <= 0 || ntaps <= 0 || (ntaps & 3)) return ORCAI_E_BADARG;
  hipLaunchKernelGGL(resample_kernel, dim3((unsigned)((n_out + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, n_in, out, n_out, L, M, table, ntaps);
  return (int)hipGetLastError();
}
