// augment.hip -- training augmentation on the GPU for gfx950: SpecAugment-style time / frequency masks, a random level shift and
// snippet mixing, behind the training dataset (orcai_amd/augment.py is the specification: plan_ref / apply_ref).
//
// Two launches per batch, no atomics, nothing allocated, nothing synchronised:
//   augment_plan_kernel   one thread per snippet draws int32 plan[B][ORCAI_AUGMENT_PLAN_WORDS] from the 64-bit batch key with the
//                         counter-based generator of dropout_mask_kernel (train_head.hip): draw j of snippet b is
//                         splitmix64_finalise(key + 0x9E3779B97F4A7C15 * (b * ORCAI_AUGMENT_DRAWS + j + 1)).
//   augment_apply_kernel  one streaming pass over x, one snippet per blockIdx.y: the workgroup expands its snippet's plan into a row-mask
//                         and a column-mask image in LDS (one byte per row / column), then every element is one (or, mixed, two) loads,
//                         max / add / clamp, two LDS byte lookups and one store; 16-byte accesses when the three blocks it touches are
//                         16-byte aligned and H * W is a multiple of 4 (the choice gather_snippets_kernel makes), scalar otherwise.  The
//                         last workgroup of a snippet also writes its S * L labels.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "orcai_hip.h"

namespace {

constexpr int kMaxMasks = ORCAI_AUGMENT_MAX_MASKS;
constexpr int kDraws = ORCAI_AUGMENT_DRAWS;
constexpr int kPlanWords = ORCAI_AUGMENT_PLAN_WORDS;
constexpr int kMaxH = ORCAI_AUGMENT_MAX_H;
constexpr int kMaxW = ORCAI_AUGMENT_MAX_W;
// plan words (the header states the layout)
constexpr int kPartner = 0, kShift = 1, kNTime = 2, kNFreq = 3, kTime0 = 4, kFreq0 = kTime0 + 2 * kMaxMasks;
// draw slots of a snippet
constexpr int kDrawMix = 0, kDrawPartner = 1, kDrawShift = 2, kDrawTime0 = 3, kDrawFreq0 = kDrawTime0 + 2 * kMaxMasks;
static_assert(kFreq0 + 2 * kMaxMasks == kPlanWords, "plan layout");
static_assert(kDrawFreq0 + 2 * kMaxMasks <= kDraws, "draw slots");

__device__ __forceinline__ uint64_t draw(uint64_t key, int b, int j) {
  uint64_t z = key + 0x9E3779B97F4A7C15ull * (uint64_t)((int64_t)b * kDraws + j + 1);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
__device__ __forceinline__ int draw_int(uint64_t z, int n) { return (int)(((z >> 32) * (uint64_t)n) >> 32); }  // in [0, n)
__device__ __forceinline__ float draw_uniform(uint64_t z) { return (float)(z >> 40) * (1.0f / 16777216.0f); }  // in [0, 1)

__global__ __launch_bounds__(64) void augment_plan_kernel(uint64_t key, int B, int H, int W, int time_masks, int time_mask_rows, int freq_masks,
                                                          int freq_mask_bins, float level_shift, float mix_probability, int32_t* __restrict__ plan) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
  int32_t* p = plan + (int64_t)b * kPlanWords;
  const bool mixed = B > 1 && draw_uniform(draw(key, b, kDrawMix)) < mix_probability;
  p[kPartner] = mixed ? (int)(((int64_t)b + 1 + draw_int(draw(key, b, kDrawPartner), B - 1)) % B) : -1;
  const float u = draw_uniform(draw(key, b, kDrawShift));
  p[kShift] = __float_as_int(__fmul_rn(u + u - 1.0f, level_shift));  // u + u - 1 is exact; one rounding, in the product
  p[kNTime] = time_masks;
  p[kNFreq] = freq_masks;
  for (int k = 0; k < kMaxMasks; ++k) {
    int start = 0, height = 0;
    if (k < time_masks) {
      height = draw_int(draw(key, b, kDrawTime0 + 2 * k), time_mask_rows + 1);
      start = draw_int(draw(key, b, kDrawTime0 + 2 * k + 1), H - height + 1);
    }
    p[kTime0 + 2 * k] = start;
    p[kTime0 + 2 * k + 1] = height;
    start = height = 0;
    if (k < freq_masks) {
      height = draw_int(draw(key, b, kDrawFreq0 + 2 * k), freq_mask_bins + 1);
      start = draw_int(draw(key, b, kDrawFreq0 + 2 * k + 1), W - height + 1);
    }
    p[kFreq0 + 2 * k] = start;
    p[kFreq0 + 2 * k + 1] = height;
  }
}

// 1 where index i lies in one of the n (start, height) pairs at s_plan[first ...]
__device__ __forceinline__ uint8_t in_any(const int32_t* s_plan, int first, int n, int i) {
  uint8_t m = 0;
  for (int k = 0; k < n; ++k) m |= (uint8_t)((unsigned)(i - s_plan[first + 2 * k]) < (unsigned)s_plan[first + 2 * k + 1]);
  return m;
}

__device__ __forceinline__ float shift_clamp(float v, float shift) { return fminf(fmaxf(v + shift, 0.0f), 1.0f); }

__global__ __launch_bounds__(256) void augment_apply_kernel(const float* __restrict__ x_in, const float* __restrict__ y_in, const int32_t* __restrict__ plan,
                                                            float* __restrict__ x_out, float* __restrict__ y_out, int H, int W, int S, int L, float mask_value,
                                                            int flags) {
  __shared__ int32_t s_plan[kPlanWords];
  __shared__ uint8_t s_row[kMaxH];
  __shared__ uint8_t s_col[kMaxW];
  const int b = blockIdx.y, B = gridDim.y, tid = threadIdx.x;
  if (tid < kPlanWords) s_plan[tid] = plan[(int64_t)b * kPlanWords + tid];
  __syncthreads();
  // the plan is the caller's memory: counts and the partner are clamped to what the images and x_in hold
  const int nt = min(max(s_plan[kNTime], 0), kMaxMasks), nf = min(max(s_plan[kNFreq], 0), kMaxMasks);
  for (int r = tid; r < H; r += 256) s_row[r] = in_any(s_plan, kTime0, nt, r);
  for (int c = tid; c < W; c += 256) s_col[c] = in_any(s_plan, kFreq0, nf, c);
  __syncthreads();

  const bool mixed = s_plan[kPartner] >= 0 && s_plan[kPartner] < B;
  const int partner = mixed ? s_plan[kPartner] : b;
  const float shift = __int_as_float(s_plan[kShift]);
  const bool shifted = (flags & ORCAI_AUGMENT_LEVEL_SHIFT) != 0;
  const int n = H * W;  // <= kMaxH * kMaxW
  const float* src = x_in + (int64_t)b * n;
  const float* oth = x_in + (int64_t)partner * n;
  float* dst = x_out + (int64_t)b * n;
  const bool vec = ((((uintptr_t)src | (uintptr_t)oth | (uintptr_t)dst) & 15) == 0) && (n & 3) == 0;
  if (vec) {
    const int n4 = n >> 2;
    for (int i = blockIdx.x * 256 + tid; i < n4; i += gridDim.x * 256) {
      const float4 a = reinterpret_cast<const float4*>(src)[i];
      float v[4] = {a.x, a.y, a.z, a.w};
      if (mixed) {
        const float4 p = reinterpret_cast<const float4*>(oth)[i];
        v[0] = fmaxf(v[0], p.x), v[1] = fmaxf(v[1], p.y), v[2] = fmaxf(v[2], p.z), v[3] = fmaxf(v[3], p.w);
      }
      int r = (i * 4) / W, c = i * 4 - r * W;  // the four elements may straddle a row end
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (shifted) v[k] = shift_clamp(v[k], shift);
        if (s_row[r] | s_col[c]) v[k] = mask_value;
        if (++c == W) c = 0, ++r;  // r == H only after the snippet's last element: not read again
      }
      reinterpret_cast<float4*>(dst)[i] = make_float4(v[0], v[1], v[2], v[3]);
    }
  } else {
    for (int i = blockIdx.x * 256 + tid; i < n; i += gridDim.x * 256) {
      float v = src[i];
      if (mixed) v = fmaxf(v, oth[i]);
      if (shifted) v = shift_clamp(v, shift);
      const int r = i / W, c = i - r * W;
      if (s_row[r] | s_col[c]) v = mask_value;
      dst[i] = v;
    }
  }

  if (blockIdx.x != gridDim.x - 1) return;
  // labels: mixed = 1 if either has 1, else -1 (MASK_VALUE) if either has -1, else 0; a step whose rows are all time-masked becomes -1
  const int factor = H / S;
  const bool mask_labels = (flags & ORCAI_AUGMENT_MASK_LABELS) != 0;
  const float* ya = y_in + (int64_t)b * S * L;
  const float* yp = y_in + (int64_t)partner * S * L;
  float* yo = y_out + (int64_t)b * S * L;
  for (int i = tid; i < S * L; i += 256) {
    float y = ya[i];
    if (mixed) {
      const float p = yp[i];
      y = (y == 1.0f || p == 1.0f) ? 1.0f : ((y == -1.0f || p == -1.0f) ? -1.0f : 0.0f);
    }
    if (mask_labels) {
      const int s = i / L;
      uint8_t covered = 1;
      for (int k = 0; k < factor; ++k) covered &= s_row[s * factor + k];
      if (covered) y = -1.0f;
    }
    yo[i] = y;
  }
}

bool overlap(const void* a, const void* b, int64_t bytes) {
  const uintptr_t p = (uintptr_t)a, q = (uintptr_t)b;
  return p < q + (uintptr_t)bytes && q < p + (uintptr_t)bytes;
}

}  // namespace

extern "C" {

int orcai_augment_plan(uint64_t batch_key, int B, int H, int W, int time_masks, int time_mask_rows, int freq_masks, int freq_mask_bins, float level_shift,
                       float mix_probability, int32_t* plan, void* stream) {
  if (!plan || B <= 0 || H <= 0 || W <= 0 || time_masks < 0 || freq_masks < 0) return ORCAI_E_BADARG;
  if (time_mask_rows < 0 || time_mask_rows > H || freq_mask_bins < 0 || freq_mask_bins > W) return ORCAI_E_BADARG;
  if (!(level_shift >= 0.0f && level_shift <= 1.0f) || !(mix_probability >= 0.0f && mix_probability <= 1.0f)) return ORCAI_E_BADARG;
  if (time_masks > kMaxMasks || freq_masks > kMaxMasks || H > kMaxH || W > kMaxW || B > 65535) return ORCAI_E_UNSUPPORTED;
  hipLaunchKernelGGL(augment_plan_kernel, dim3((B + 63) / 64), dim3(64), 0, (hipStream_t)stream, batch_key, B, H, W, time_masks, time_mask_rows, freq_masks,
                     freq_mask_bins, level_shift, mix_probability, plan);
  return (int)hipGetLastError();
}

int orcai_augment_apply(const float* x_in, const float* y_in, const int32_t* plan, float* x_out, float* y_out, int B, int H, int W, int S, int L, float mask_value,
                        int flags, void* stream) {
  if (!x_in || !y_in || !plan || !x_out || !y_out || B <= 0 || H <= 0 || W <= 0 || S <= 0 || L <= 0) return ORCAI_E_BADARG;
  if (H % S || !std::isfinite(mask_value) || (flags & ~(ORCAI_AUGMENT_LEVEL_SHIFT | ORCAI_AUGMENT_MASK_LABELS))) return ORCAI_E_BADARG;
  if (H > kMaxH || W > kMaxW || B > 65535 || (int64_t)S * L > INT32_MAX) return ORCAI_E_UNSUPPORTED;
  const int64_t n = (int64_t)H * W;
  // out of place: a workgroup reads its partner's block of x_in while another one writes that snippet's block of x_out
  if (overlap(x_in, x_out, (int64_t)B * n * 4) || overlap(y_in, y_out, (int64_t)B * S * L * 4)) return ORCAI_E_BADARG;
  int gx = (int)((n / 4 + 255) / 256);
  if (gx > 64) gx = 64;
  if (gx < 1) gx = 1;
  hipLaunchKernelGGL(augment_apply_kernel, dim3(gx, B), dim3(256), 0, (hipStream_t)stream, x_in, y_in, plan, x_out, y_out, H, W, S, L, mask_value, flags);
  return (int)hipGetLastError();
}

}  // extern "C"
