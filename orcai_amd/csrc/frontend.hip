// frontend.hip -- STFT / dB / exact quantile clip / normalise for gfx950 (MI355X).
//
// Replaces the arithmetic of /root/reference/src/orcAI/spectrogram.py:34-39 (librosa.stft),
// :51-53 (amplitude_to_db(ref=np.max)) and :58-87 (preprocess_spectrogram).
//
// Data flow (one recording):
//   pass A  stft_db_kernel      PCM f32 -> L[t][k] = 10*log10(max(|X|^2,1e-10)), k < k_crop   (HBM: R pcm, W L)
//                               + max |X|^2 over all 257 bins (atomicMax) + level-1 histogram of L (LDS)
//   scan1   select_scan1_kernel level-1 histogram -> key interval of each wanted rank
//   pass C  hist2_kernel        re-read L, histogram the keys inside the two intervals (<= 2 rounds)
//   scan2   select_scan2_kernel interval -> exact key
//   (values that are not dB, the PCEN routes: radix_hist_kernel<1..3> / radix_scan_kernel<1..3> instead of the four steps above -- three reads
//    of the array, one key digit each, whatever the values; orcai_quantile_select_radix)
//   final   clip_normalize      in place: max(L - ref_db, -80) -> clip -> (v - lo)/(hi - lo)     (HBM: R L, W out)
//   backward spectrogram_bwd     dL/dout -> dL/dpcm with ref_db / lo / hi held constant (orcai_spectrogram_bwd)   (HBM: R pcm, R g, W dpcm)
//
// The order statistic is selected on the un-referenced values L: v = max(L - ref_db, -80) is monotone
// non-decreasing in L, so the k-th smallest v is that function of the k-th smallest L (exact).
//
// STFT kernel layout: a wavefront (64 lanes) transforms 4 consecutive frames at once, 16 lanes per
// frame.  A 512-point real frame is packed as 256 complex points z[n] = x[2n] + i x[2n+1] and
// transformed as 16 x 16 (four-step): FFT-16 in registers over n2 (n = n1 + 16 n2, n1 = lane),
// twiddle W256^(n1 k2), 16x16 transpose through a wave-private padded LDS tile, FFT-16 in registers
// over n1, then the real-FFT split with the mirrored bin fetched by ds_bpermute.  The 4 frames' 171
// kept bins are staged in the same LDS tile and leave as one contiguous 2736-byte run of dwordx4 stores.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <type_traits>
#include <cstring>
#include <mutex>

#include "lds_optin.h"
#include "orcai_hip.h"
#include "select_key.h"  // f2key / key2f
#include "zero_fill.h"

namespace {

constexpr int NFFT = 512;
constexpr int NB1 = 2561;    // level-1 buckets: 1280 negative + 1 around zero + 1280 positive
constexpr int NB1_PAD = 2568;
constexpr int NB2 = 65536;   // level-2 bins per round
constexpr int NB2C = NB2 / 256;
constexpr float AMIN_POW = 1e-10f;
constexpr float DB_PER_LOG2 = 3.0102999566398120f;  // 10*log10(2)

struct SelState {
  uint32_t klo;       // first key of the current interval
  uint32_t done;      // 1 once the interval is a single key
  uint64_t width;     // number of keys in the interval
  uint64_t rank;      // 0-based rank of the wanted element inside the interval
};

struct Workspace {
  uint32_t hist1[NB1_PAD];
  uint32_t hist2[2][NB2];
  uint32_t hist2c[2][NB2C];  // coarse: one counter per 256 fine bins
  SelState sel[2];
  uint32_t pmax_bits;  // max |X|^2 (non-negative float, so uint order == float order)
  uint32_t use_ref;
  float ref_db;        // 10*log10(max(pmax, 1e-10))
  float floor_db;      // -top_db
  float p_lo, p_hi;    // clip bounds in final dB
  float sel_raw[2];    // selected raw order statistics
};

__device__ float g_window[NFFT];
__device__ float2 g_tw256[256];  // [k2*16 + n1] = exp(-2 pi i n1 k2 / 256)
__device__ float2 g_tw512[260];  // [k] = (cos, sin)(2 pi k / 512), k = 0..256

__device__ __forceinline__ float power_to_db(float p) {
  return __builtin_amdgcn_logf(fmaxf(p, AMIN_POW)) * DB_PER_LOG2;
}
// Monotone map key -> level-1 bucket: 128 buckets per octave for 0.125 <= |x| < 128, one bucket around 0.
__device__ __forceinline__ int bucket1(uint32_t key) {
  // k16 <  0x3D00 -> 0;  0x3D00..0x41FF -> k16 - 0x3D00;  0x4200..0xBDFF -> 1280;  0xBE00..0xC2FF -> 1281 + (k16 - 0xBE00);  above -> 2560
  const int k16 = (int)(key >> 16);
  const int lo = min(max(k16 - 0x3D00, 0), 1280);
  const int hi = 1281 + min(k16 - 0xBE00, 0x4FF);
  return k16 >= 0xBE00 ? hi : lo;
}
// The same bucket straight from the float (bucket1(f2key(f)) == bucket1f(f) for every float; tests/test_host_logic.py restates both and checks all 2^16
// high halves): magnitude bits m16 = bits[30:16], t = clamp(m16 - 0x3DFF, 0, 0x500) counts 1/128-octave steps above 0.125 (0 below),
// bucket = 1280 +- t by the sign.  7 integer instructions instead of 13 in the STFT kernel's per-bin tail.
__device__ __forceinline__ int bucket1f(float f) {
  const int u = (int)__float_as_uint(f);
  const int sgn = u >> 31;  // 0 or -1
  const int m16 = (int)(((uint32_t)u >> 16) & 0x7FFFu);  // v_bfe_u32
  const int t = min(max(m16 - 0x3DFF, 0), 0x500);         // v_med3_i32
  return 1280 + ((t ^ sgn) - sgn);
}
__device__ __forceinline__ void bucket1_range(int b, uint32_t& klo, uint64_t& width) {
  if (b == 0) { klo = 0u; width = 0x3D010000ull; }
  else if (b < 1280) { klo = (0x3D00u + (uint32_t)b) << 16; width = 65536ull; }
  else if (b == 1280) { klo = 0x42000000u; width = 0xBE000000ull - 0x42000000ull; }
  else if (b < 2560) { klo = (0xBE00u + (uint32_t)(b - 1281)) << 16; width = 65536ull; }
  else { klo = 0xC2FF0000u; width = 0x100000000ull - 0xC2FF0000ull; }
}
__device__ __forceinline__ int shift_for(uint64_t width) {
  int s = 0;
  while ((width >> s) > (uint64_t)NB2) ++s;
  return s;
}

// ---------------------------------------------------------------- FFT-16 in registers, packed complex arithmetic
// A complex number is one aligned register pair (re, im); every butterfly add / subtract is ONE v_pk_add_f32, a multiplication by
// -i or +i is folded into the add that consumes it through the operand selectors of VOP3P (op_sel / op_sel_hi pick which half of a
// source feeds which half of the result, neg_lo / neg_hi negate it), and a complex multiplication is v_pk_mul_f32 + v_pk_fma_f32.
// Written as inline asm: left to itself the compiler keeps re[] / im[] apart and spends a fifth of the kernel's vector instructions
// on register moves that assemble packed operands.
typedef float c2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ c2 add_mi(c2 a, c2 b) {  // a - i b = (a.re + b.im, a.im - b.re)
  c2 r;
  asm("v_pk_add_f32 %0, %1, %2 op_sel:[0,1] op_sel_hi:[1,0] neg_hi:[0,1]" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
__device__ __forceinline__ c2 add_pi(c2 a, c2 b) {  // a + i b = (a.re - b.im, a.im + b.re)
  c2 r;
  asm("v_pk_add_f32 %0, %1, %2 op_sel:[0,1] op_sel_hi:[1,0] neg_lo:[0,1]" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
__device__ __forceinline__ c2 cmulv(c2 a, c2 w) {  // a * w, w = (wr, wi) in a VGPR pair
  c2 t, r;
  asm("v_pk_mul_f32 %0, %1, %2 op_sel:[0,0] op_sel_hi:[1,0]" : "=v"(t) : "v"(a), "v"(w));                                  // (a.re wr, a.im wr)
  asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel:[1,1,0] op_sel_hi:[0,1,1] neg_lo:[0,1,0]" : "=v"(r) : "v"(a), "v"(w), "v"(t));  // (-a.im wi + ., a.re wi + .)
  return r;
}
__device__ __forceinline__ c2 cmuls(c2 a, c2 w) {  // the same with a wave-uniform constant in an SGPR pair
  c2 t, r;
  asm("v_pk_mul_f32 %0, %1, %2 op_sel:[0,0] op_sel_hi:[1,0]" : "=v"(t) : "v"(a), "s"(w));
  asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel:[1,1,0] op_sel_hi:[0,1,1] neg_lo:[0,1,0]" : "=v"(r) : "v"(a), "s"(w), "v"(t));
  return r;
}
__device__ __forceinline__ void bfly4(c2& a, c2& b, c2& c, c2& d) {
  const c2 t0 = a + c, t1 = a - c, t2 = b + d, t3 = b - d;
  a = t0 + t2;
  c = t0 - t2;
  b = add_mi(t1, t3);
  d = add_pi(t1, t3);
}
// In-place forward FFT-16; output bin k ends up at position P16(k).
#define P16(k) (4 * ((k) & 3) + ((k) >> 2))
__device__ __forceinline__ void fft16(c2 (&x)[16]) {
  constexpr float C1 = 0.92387953251128674f, S1 = 0.38268343236508977f, R2 = 0.70710678118654752f;
#pragma unroll
  for (int a = 0; a < 4; ++a) bfly4(x[a], x[a + 4], x[a + 8], x[a + 12]);
  // position a + 4q holds y[a][q]; multiply by W16^(a q)
  x[1 + 4] = cmuls(x[1 + 4], (c2){C1, -S1});     // a=1,q=1 : W^1
  x[1 + 8] = cmuls(x[1 + 8], (c2){R2, -R2});     // a=1,q=2 : W^2
  x[1 + 12] = cmuls(x[1 + 12], (c2){S1, -C1});   // a=1,q=3 : W^3
  x[2 + 4] = cmuls(x[2 + 4], (c2){R2, -R2});     // a=2,q=1 : W^2
  x[2 + 8] = add_mi((c2){0.f, 0.f}, x[2 + 8]);   // a=2,q=2 : W^4 = -i
  x[2 + 12] = cmuls(x[2 + 12], (c2){-R2, -R2});  // a=2,q=3 : W^6
  x[3 + 4] = cmuls(x[3 + 4], (c2){S1, -C1});     // a=3,q=1 : W^3
  x[3 + 8] = cmuls(x[3 + 8], (c2){-R2, -R2});    // a=3,q=2 : W^6
  x[3 + 12] = cmuls(x[3 + 12], (c2){-C1, S1});   // a=3,q=3 : W^9
#pragma unroll
  for (int q = 0; q < 4; ++q) bfly4(x[4 * q], x[4 * q + 1], x[4 * q + 2], x[4 * q + 3]);
}

constexpr int ROW_BYTES = 144;               // 16 complex (128 B) + 16 B pad: conflict-free b128 row reads
constexpr int FRAME_BYTES = 16 * ROW_BYTES;  // 2304
constexpr int WAVE_BYTES = 4 * FRAME_BYTES;  // 9216, also holds the 4 x k_crop output staging (<= 4112 B)

constexpr int STFT_BLOCKS = 1536;  // persistent workgroups of the STFT launch: six per compute unit, three resident (profiles/r03_ab_stft_blocks.log: 768 -> 1536 = -3 %)

struct __attribute__((aligned(16))) StftLds {
  unsigned char tile[4][WAVE_BYTES];  // per wave: PCM staging (5 hops) -> 16x16 transpose tile -> output staging
  float2 tw256[256];
  float2 tw512[260];
  float2 win2[256];                   // (w[2n], w[2n+1])
  uint32_t hist[NB1_PAD];
};

__device__ __forceinline__ void wave_lds_fence() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// FAST_ONLY: every group in [g_begin, g_end) is known (by the launcher) to satisfy the fast-path conditions for all four of its
// waves, so the generic body is not even instantiated (134 VGPRs and no spills instead of 168 + spills).  KC > 0: k_crop is the
// compile-time constant KC (171 for orcai-V1), which removes the per-bin crop branches from the real-FFT split.
//
// MEL (orcai_stft_mel_db): the same transform with a mel epilogue instead of the crop.  k_crop_arg is n_mels.  The 257 powers of each of the wave's four
// frames are parked in the wave's tile (MEL_PSTRIDE floats per frame: 272 = 16 mod 64, so the four frames' 16 lanes write 64 different banks), the 64
// lanes then sum the 4 x n_mels bands (task = frame * n_mels + band, one lane per task, bins in ascending order: a fixed order, no atomics on values)
// from the band table and the packed weights, both resident in LDS (MelLds) for the life of the workgroup, and stage the dB values BEHIND the powers
// in the same tile (4352 + 4 x 256 x 4 = 8448 <= 9216 B), from where they leave as the linear path's do.  The running maximum tracks the band powers.
constexpr int MEL_MAX = 256;       // bands
constexpr int MEL_W_LDS = 1024;    // packed weights the 512-point kernel keeps in LDS (triangles over 257 bins have at most 514)
constexpr int MEL_PSTRIDE = 272;   // floats between the parked power rows of a wave's frames

struct MelBands {  // kernel argument, by value: band m covers bins [lo, lo + n) with weights w[off .. off + n)
  uint16_t lo[MEL_MAX], n[MEL_MAX], off[MEL_MAX];
};
struct MelLds {
  float w[MEL_W_LDS];
  uint16_t lo[MEL_MAX], n[MEL_MAX], off[MEL_MAX];
};

//
// ENERGY (orcai_stft_energy / orcai_stft_mel_energy, the input of orcai_pcen): the same transform, staging and stores with a linear epilogue -- the
// magnitude |X[k]| = sqrt(4 |X|^2) / 2 of the kept bins, or the band power acc as it stands -- and neither running maximum nor histogram (ws is unused
// and may be null).  A separate instantiation: the dB ones compile to what they were.
template <bool EVEN_HOP, bool FAST_ONLY, int KC, bool MEL, bool ENERGY = false>
__device__ __forceinline__ void stft_db_body(const float* __restrict__ pcm, int64_t n_samples, int hop, int64_t n_frames, int k_crop_arg,
                                             float* __restrict__ out, Workspace* __restrict__ ws, int64_t g_begin, int64_t g_end,
                                             const MelBands* __restrict__ mel_bands, const float* __restrict__ mel_w, int n_weights) {
  static_assert(!MEL || KC == 0, "the mel epilogue has no compile-time crop");
  const int k_crop = KC > 0 ? KC : k_crop_arg;
  __shared__ StftLds lds;
  MelLds* mel = nullptr;
  if constexpr (MEL) {
    __shared__ MelLds mel_lds;
    mel = &mel_lds;
    for (int i = threadIdx.x; i < n_weights; i += 256) mel_lds.w[i] = mel_w[i];
    for (int i = threadIdx.x; i < k_crop; i += 256) {
      mel_lds.lo[i] = mel_bands->lo[i];
      mel_lds.n[i] = mel_bands->n[i];
      mel_lds.off[i] = mel_bands->off[i];
    }
  }
  const int tid = threadIdx.x;
  const int wave = tid >> 6;
  const int lane = tid & 63;
  const int l16 = lane & 15;  // n1, later k2
  const int fsub = lane >> 4; // frame within the wave

  for (int i = tid; i < 256; i += 256) lds.tw256[i] = g_tw256[i];
  for (int i = tid; i < 257; i += 256) lds.tw512[i] = g_tw512[i];
  if constexpr (!ENERGY)
    for (int i = tid; i < NB1_PAD; i += 256) lds.hist[i] = 0u;

  for (int i = tid; i < 256; i += 256) lds.win2[i] = *reinterpret_cast<const float2*>(&g_window[2 * i]);
  __syncthreads();

  unsigned char* my_tile = lds.tile[wave];
  unsigned char* my_frame = my_tile + fsub * FRAME_BYTES;
  float pmax = 0.0f;

  // One group of 4 frames per wave.  FAST (compile-time): hop 256, all 4 frames inside the recording, the 1280 samples they
  // cover inside the PCM array and 16-byte aligned -> no per-element predicates anywhere in the body.
  auto process = [&](auto fast_tag, int64_t t0w, const float4& p0, const float4& p1, const float4& p2, const float4& p3, const float4& p4 /*FAST_ONLY: this group's 5 x 16 B per lane, requested one group ahead*/) {
    constexpr bool FAST = decltype(fast_tag)::value;
    const int64_t t = t0w + fsub;
    const bool valid = FAST ? true : (t < n_frames);
    const int64_t s0 = t * (int64_t)hop - (NFFT / 2);

    c2 z[16];
    // The wave's 4 frames cover padded samples [hop*t0w, hop*(t0w+3) + 512): for the default hop 256 that is one
    // contiguous run of 1280 floats, fetched as 5 dwordx4 per lane (1 KiB per instruction) into the wave's tile.
    const int64_t w0 = t0w * (int64_t)hop - (NFFT / 2);  // first sample the wave needs
    if constexpr (FAST) {
      float* st = reinterpret_cast<float*>(my_tile);
      const float4* gp = reinterpret_cast<const float4*>(pcm + w0);
      if constexpr (FAST_ONLY) {
        reinterpret_cast<float4*>(st)[lane] = p0;
        reinterpret_cast<float4*>(st)[lane + 64] = p1;
        reinterpret_cast<float4*>(st)[lane + 128] = p2;
        reinterpret_cast<float4*>(st)[lane + 192] = p3;
        reinterpret_cast<float4*>(st)[lane + 256] = p4;
      } else {
#pragma unroll
        for (int u = 0; u < 5; ++u) reinterpret_cast<float4*>(st)[lane + 64 * u] = gp[lane + 64 * u];
      }
      wave_lds_fence();
      const float* fr = st + fsub * 256;
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const c2 v = *reinterpret_cast<const c2*>(fr + 2 * (l16 + 16 * j));
        const c2 w = *reinterpret_cast<const c2*>(&lds.win2[l16 + 16 * j]);
        z[j] = v * w;  // (x[2n] w[2n], x[2n+1] w[2n+1]): the 512-point real frame packed as 256 complex points
      }
      wave_lds_fence();  // staging reads done before the tile is reused for the transpose
    } else {
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const int64_t sidx = s0 + 2 * (l16 + 16 * j);
        const float x0 = (valid && sidx >= 0 && sidx < n_samples) ? pcm[sidx] : 0.0f;
        const float x1 = (valid && sidx + 1 >= 0 && sidx + 1 < n_samples) ? pcm[sidx + 1] : 0.0f;
        const float2 w = lds.win2[l16 + 16 * j];
        z[j] = (c2){x0 * w.x, x1 * w.y};
      }
    }

    // step 1: FFT-16 over n2 -> Y[n1][k2] at position P16(k2); step 2: twiddle W256^(n1 k2)
    fft16(z);
#pragma unroll
    for (int k2 = 1; k2 < 16; ++k2) z[P16(k2)] = cmulv(z[P16(k2)], *reinterpret_cast<const c2*>(&lds.tw256[k2 * 16 + l16]));
    // step 3: transpose through the wave-private tile: row k2, column n1
#pragma unroll
    for (int k2 = 0; k2 < 16; ++k2) *reinterpret_cast<c2*>(my_frame + k2 * ROW_BYTES + l16 * 8) = z[P16(k2)];
    wave_lds_fence();
#pragma unroll
    for (int h = 0; h < 8; ++h) {
      const float4 v = *reinterpret_cast<const float4*>(my_frame + l16 * ROW_BYTES + h * 16);
      z[2 * h] = (c2){v.x, v.y};
      z[2 * h + 1] = (c2){v.z, v.w};
    }
    // step 4: FFT-16 over n1 -> Z[16 k1 + k2] at position P16(k1), lane = k2
    fft16(z);
    wave_lds_fence();  // all lanes have read the tile before it is reused as output staging

    // step 5: real-FFT split.  A = Z[k], B = Z[256-k] (lane (16-k2)&15, register 15-k1 for k2 != 0, (16-k1)&15 for k2 == 0): every lane
    // parks its 16 bins in the wave's tile ([frame][k] complex, 2 KiB + 128 B per frame) and reads the mirrored ones back with a per-lane address --
    // 16 ds_write_b64 + 16 ds_read_b64 (both conflict-free: the 16 lanes of a frame touch 16 consecutive bins) where round 2 had 32
    // ds_bpermute + 32 selects for the k2 == 0 lane.
    //   2 X[k] = (A + conj B) + (c - i s)(-i)(A - conj B)        with (c, s) = tw512[k]
    // in packed form: E = A + conj B, O = (A.im + B.im, B.re - A.re), 2 X = E + (c O.re + s O.im, c O.im - s O.re); power = |2X|^2 / 4:
    // the 1/4 is applied once to the running maximum and, in the dB value, to the argument of the logarithm's clamp (0.25 s >= 1e-10
    // <=> s >= 4e-10) and as log2(s) - 2 (exact scaling by a power of two; the sum rounds like log2(0.25 s) up to one ulp).
    c2* zt = reinterpret_cast<c2*>(my_tile + fsub * 2176);  // 257 bins (Z[256] = Z[0]) + pad: frames 0 / 1 (and 2 / 3) of a half-wave land in different bank halves
#pragma unroll
    for (int k1 = 0; k1 < 16; ++k1) zt[16 * k1 + l16] = z[P16(k1)];
    if (l16 == 0) zt[256] = z[P16(0)];  // so that bin 256 - k needs no wrap: the mirrored address is one per-lane base + a compile-time offset
    wave_lds_fence();
    const c2* zm = zt + (16 - l16);  // Z[256 - (16 k1 + k2)] = zm[16 (15 - k1)]
    float Lk[(KC > 0 ? (KC + 15) / 16 : 16)];  // MEL: 4 |X|^2 of the lane's 16 bins
    const c2 z0 = z[P16(0)];
#pragma unroll
    for (int k1 = 0; k1 < 16; ++k1) {
      const c2 A = z[P16(k1)];
      const int k = 16 * k1 + l16;
      const c2 Bv = zm[16 * (15 - k1)];
      const c2 cs = *reinterpret_cast<const c2*>(&lds.tw512[k]);
      c2 E, O, P, T;
      asm("v_pk_add_f32 %0, %1, %2 neg_hi:[0,1]" : "=v"(E) : "v"(A), "v"(Bv));                                              // (A.re + B.re, A.im - B.im)
      asm("v_pk_add_f32 %0, %1, %2 op_sel:[1,1] op_sel_hi:[0,0] neg_hi:[1,0]" : "=v"(O) : "v"(A), "v"(Bv));                 // (A.im + B.im, B.re - A.re)
      asm("v_pk_mul_f32 %0, %1, %2 op_sel:[0,0] op_sel_hi:[1,0]" : "=v"(T) : "v"(O), "v"(cs));                              // (c O.re, c O.im)
      asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel:[1,1,0] op_sel_hi:[0,1,1] neg_hi:[0,1,0]" : "=v"(P) : "v"(O), "v"(cs), "v"(T));  // (s O.im + ., -s O.re + .)
      const c2 X2 = E + P;
      const float p4 = fmaf(X2.x, X2.x, X2.y * X2.y);  // 4 |X|^2
      if constexpr (MEL) {
        Lk[k1] = p4;
      } else if constexpr (ENERGY) {
        if (KC > 0 ? (16 * k1 < KC) : true) Lk[k1] = 0.5f * sqrtf(p4);  // |X|
      } else {
        if (valid) pmax = fmaxf(pmax, p4);
        if (KC > 0 ? (16 * k1 < KC) : true) Lk[KC > 0 ? k1 : k1] = (__builtin_amdgcn_logf(fmaxf(p4, 4.0f * AMIN_POW)) - 2.0f) * DB_PER_LOG2;
      }
    }
    float Lnyq = 0.0f;
    if (l16 == 0) {  // Nyquist bin 256: X = Re Z0 - Im Z0
      const float x = z0.x - z0.y;
      const float p4 = 4.0f * x * x;
      if constexpr (MEL) {
        Lnyq = p4;
      } else if constexpr (ENERGY) {
        Lnyq = 0.5f * sqrtf(p4);
      } else {
        if (valid) pmax = fmaxf(pmax, p4);
        Lnyq = (__builtin_amdgcn_logf(fmaxf(p4, 4.0f * AMIN_POW)) - 2.0f) * DB_PER_LOG2;
      }
    }
    wave_lds_fence();  // every mirrored read is done before the tile becomes the output staging
    if constexpr (MEL) {
      float* pw = reinterpret_cast<float*>(my_tile) + fsub * MEL_PSTRIDE;  // |X|^2 (the exact quarter of what the loop tracked); frames past the end hold zeros
#pragma unroll
      for (int k1 = 0; k1 < 16; ++k1) pw[16 * k1 + l16] = 0.25f * Lk[k1];
      if (l16 == 0) pw[256] = 0.25f * Lnyq;
      wave_lds_fence();  // the band sums read every lane's powers
      float* stage = reinterpret_cast<float*>(my_tile) + 4 * MEL_PSTRIDE;  // behind the powers: no band sum reads what another lane stages
      const int nm = k_crop;
      for (int idx = lane; idx < 4 * nm; idx += 64) {
        const int f = (idx >= nm) + (idx >= 2 * nm) + (idx >= 3 * nm);
        const int m = idx - f * nm;
        const float* w = mel->w + mel->off[m];
        const float* p = reinterpret_cast<const float*>(my_tile) + f * MEL_PSTRIDE + mel->lo[m];
        const int nk = mel->n[m];
        float acc = 0.0f;
        for (int j = 0; j < nk; ++j) acc = fmaf(w[j], p[j], acc);  // ascending bins: the same order on every launch
        if constexpr (ENERGY) {
          stage[idx] = acc;
        } else {
          const float L = power_to_db(acc);
          stage[idx] = L;
          if (FAST || t0w + f < n_frames) {
            pmax = fmaxf(pmax, acc);
            atomicAdd(&lds.hist[bucket1f(L)], 1u);
          }
        }
      }
    } else {
    float* stage = reinterpret_cast<float*>(my_tile) + fsub * k_crop;
#pragma unroll
    for (int k1 = 0; k1 < (KC > 0 ? (KC + 15) / 16 : 16); ++k1) {
      const int k = 16 * k1 + l16;
      if (k < k_crop) {
        stage[k] = Lk[k1];
        if constexpr (!ENERGY)
          if (valid) atomicAdd(&lds.hist[bucket1f(Lk[k1])], 1u);
      }
    }
    if (l16 == 0 && 256 < k_crop) {
      stage[256] = Lnyq;
      if constexpr (!ENERGY)
        if (valid) atomicAdd(&lds.hist[bucket1f(Lnyq)], 1u);
    }
    }
    wave_lds_fence();

    // step 6: the wave's valid frames are one contiguous run of out[]
    int64_t nv = n_frames - t0w;
    nv = nv < 0 ? 0 : (nv > 4 ? 4 : nv);
    const int count = (int)nv * k_crop;
    float* dst = out + t0w * (int64_t)k_crop;  // 16-byte aligned: t0w % 4 == 0
    const float* src = reinterpret_cast<const float*>(my_tile) + (MEL ? 4 * MEL_PSTRIDE : 0);
    const int n4 = count >> 2;
    for (int i = lane; i < n4; i += 64) reinterpret_cast<float4*>(dst)[i] = reinterpret_cast<const float4*>(src)[i];
    for (int i = (n4 << 2) + lane; i < count; i += 64) dst[i] = src[i];
    // The staging tile may be overwritten once its reads have returned (the stores carry their data in registers).  An LDS-only wait:
    // wave_lds_fence() here made every group end by waiting for its own output stores to be acknowledged (a release fence drains vmcnt).
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
  };
  if constexpr (FAST_ONLY) {
    // The PCM of the NEXT group is requested before the current one is transformed (a wave otherwise starts every group by waiting a full
    // HBM round trip with only two other waves of its SIMD to cover it): two register sets, the loop unrolled by two so that no set with
    // loads in flight is ever moved; the request past the last group is clamped to the last one (unconditional, never used).
    const int64_t G = gridDim.x, g_last = g_end - 1;
    auto base = [&](int64_t g) {
      const int64_t gc = g < g_end ? g : g_last;
      return reinterpret_cast<const float4*>(pcm + (((gc << 4) + (wave << 2)) * (int64_t)hop - (NFFT / 2))) + lane;
    };
    int64_t g = g_begin + blockIdx.x;
    if (g < g_end) {
      const float4* gp = base(g);
      float4 a0 = gp[0], a1 = gp[64], a2 = gp[128], a3 = gp[192], a4 = gp[256];
      while (true) {
        gp = base(g + G);
        const float4 b0 = gp[0], b1 = gp[64], b2 = gp[128], b3 = gp[192], b4 = gp[256];
        process(std::true_type{}, (g << 4) + (wave << 2), a0, a1, a2, a3, a4);
        g += G;
        if (g >= g_end) break;
        gp = base(g + G);
        a0 = gp[0]; a1 = gp[64]; a2 = gp[128]; a3 = gp[192]; a4 = gp[256];
        process(std::true_type{}, (g << 4) + (wave << 2), b0, b1, b2, b3, b4);
        g += G;
        if (g >= g_end) break;
      }
    }
  } else {
    for (int64_t g = g_begin + blockIdx.x; g < g_end; g += gridDim.x) {
      const int64_t t0w = (g << 4) + (wave << 2);  // first frame of this wave
      const int64_t w0 = t0w * (int64_t)hop - (NFFT / 2);
      const bool fast = EVEN_HOP && hop == 256 && w0 >= 0 && ((w0 & 3) == 0) && (w0 + 1280 <= n_samples) && (t0w + 3 < n_frames);
      const float4 none = make_float4(0.f, 0.f, 0.f, 0.f);
      if (fast) process(std::true_type{}, t0w, none, none, none, none, none);  // wave-uniform
      else process(std::false_type{}, t0w, none, none, none, none, none);
    }
  }

  if constexpr (ENERGY) return;
  // wave max -> one atomic per wave
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) pmax = fmaxf(pmax, __shfl_xor(pmax, off, 64));
  if (lane == 0) atomicMax(&ws->pmax_bits, __float_as_uint(MEL ? pmax : 0.25f * pmax));  // the linear loop tracked 4 |X|^2 (exact scaling), the mel one band powers
  __syncthreads();
  for (int i = tid; i < NB1; i += 256) {
    uint32_t c = lds.hist[i];
    if (c) atomicAdd(&ws->hist1[i], c);
  }
}

template <bool EVEN_HOP, bool FAST_ONLY, int KC>
__global__ __launch_bounds__(256, 3) void stft_db_kernel(const float* __restrict__ pcm, int64_t n_samples, int hop, int64_t n_frames,
                                                       int k_crop_arg, float* __restrict__ out, Workspace* __restrict__ ws, int64_t g_begin,
                                                       int64_t g_end) {
  stft_db_body<EVEN_HOP, FAST_ONLY, KC, false>(pcm, n_samples, hop, n_frames, k_crop_arg, out, ws, g_begin, g_end, nullptr, nullptr, 0);
}

// The mel variant: 58 944 B of LDS (StftLds + MelLds), two workgroups per compute unit where the linear kernel has three.
template <bool EVEN_HOP, bool FAST_ONLY>
__global__ __launch_bounds__(256, 2) void stft_mel_kernel(const float* __restrict__ pcm, int64_t n_samples, int hop, int64_t n_frames, int n_mels,
                                                        float* __restrict__ out, Workspace* __restrict__ ws, int64_t g_begin, int64_t g_end,
                                                        const MelBands bands, const float* __restrict__ weights, int n_weights) {
  stft_db_body<EVEN_HOP, FAST_ONLY, 0, true>(pcm, n_samples, hop, n_frames, n_mels, out, ws, g_begin, g_end, &bands, weights, n_weights);
}

// The energy variants (ENERGY above): same launch bounds, same LDS, no workspace.
template <bool EVEN_HOP, bool FAST_ONLY, int KC>
__global__ __launch_bounds__(256, 3) void stft_energy_kernel(const float* __restrict__ pcm, int64_t n_samples, int hop, int64_t n_frames, int k_crop_arg,
                                                           float* __restrict__ out, int64_t g_begin, int64_t g_end) {
  stft_db_body<EVEN_HOP, FAST_ONLY, KC, false, true>(pcm, n_samples, hop, n_frames, k_crop_arg, out, nullptr, g_begin, g_end, nullptr, nullptr, 0);
}

template <bool EVEN_HOP, bool FAST_ONLY>
__global__ __launch_bounds__(256, 2) void stft_mel_energy_kernel(const float* __restrict__ pcm, int64_t n_samples, int hop, int64_t n_frames, int n_mels,
                                                               float* __restrict__ out, int64_t g_begin, int64_t g_end, const MelBands bands,
                                                               const float* __restrict__ weights, int n_weights) {
  stft_db_body<EVEN_HOP, FAST_ONLY, 0, true, true>(pcm, n_samples, hop, n_frames, n_mels, out, nullptr, g_begin, g_end, &bands, weights, n_weights);
}

// ---------------------------------------------------------------- STFT + dB for any power-of-two transform size (the reference reads nfft
// from the parameter file, spectrogram.py:34-39; every shipped file says 512 and runs stft_db_kernel above).  Plain and slow by comparison: one
// workgroup per frame, the windowed frame (centred, zero padding, periodic Hann: librosa.stft's defaults) bit-reversed into LDS, log2(nfft) radix-2
// stages with a barrier each, twiddles by sincospif; L for the first k_crop bins, max |X|^2 over ALL 1 + nfft/2 bins.  The level-1 histogram is
// taken by hist1_kernel in a second pass over L (the 512-point kernel builds it on the fly).
constexpr int NFFT_ANY_MAX = 4096;

// ENERGY (stft_any_energy_kernel): |X[k]| of the kept bins instead of dB, no maximum, ws unused.
template <bool ENERGY>
__device__ __forceinline__ void stft_any_body(const float* __restrict__ pcm, int64_t n_samples, int n_fft, int log2n, int hop, int64_t n_frames, int k_crop,
                                              float* __restrict__ out_db, Workspace* __restrict__ ws) {
  __shared__ float2 buf[NFFT_ANY_MAX];
  __shared__ float wmax[4];
  const int tid = threadIdx.x;
  const int half = n_fft >> 1;
  float pmax = 0.0f;
  for (int64_t t = blockIdx.x; t < n_frames; t += gridDim.x) {
    const int64_t s0 = t * hop - half;
    for (int n = tid; n < n_fft; n += 256) {
      const int64_t i = s0 + n;
      const float x = (i >= 0 && i < n_samples) ? pcm[i] : 0.0f;
      // periodic Hann as sin^2(pi n / N) (n / N is exact): 0.5 - 0.5 cos(2 pi n / N) in f32 cancels at the window's ends and leaves an ABSOLUTE error
      // of 2^-25 there -- 1e-4 of w[34] at N = 4096 (tests/test_stft_gpu.py, impulses)
      const float sw = sinpif((float)n / (float)n_fft);
      buf[__brev((uint32_t)n) >> (32 - log2n)] = make_float2(x * (sw * sw), 0.0f);
    }
    __syncthreads();
    for (int st = 1; st <= log2n; ++st) {
      const int hm = 1 << (st - 1);
      for (int j = tid; j < half; j += 256) {
        const int k = j & (hm - 1);
        const int i0 = ((j >> (st - 1)) << st) + k, i1 = i0 + hm;
        float sn, cs;
        sincospif(-(float)k / (float)hm, &sn, &cs);  // exp(-2 pi i k / (2 hm))
        const float2 a = buf[i0], b = buf[i1];
        const float2 tb = make_float2(fmaf(b.x, cs, -b.y * sn), fmaf(b.x, sn, b.y * cs));
        buf[i0] = make_float2(a.x + tb.x, a.y + tb.y);
        buf[i1] = make_float2(a.x - tb.x, a.y - tb.y);
      }
      __syncthreads();
    }
    for (int k = tid; k <= half; k += 256) {
      const float2 z = buf[k];
      const float p = fmaf(z.x, z.x, z.y * z.y);
      if constexpr (ENERGY) {
        if (k < k_crop) out_db[t * (int64_t)k_crop + k] = sqrtf(p);
      } else {
        pmax = fmaxf(pmax, p);
        if (k < k_crop) out_db[t * (int64_t)k_crop + k] = power_to_db(p);
      }
    }
    __syncthreads();
  }
  if constexpr (ENERGY) return;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) pmax = fmaxf(pmax, __shfl_xor(pmax, o, 64));
  if ((tid & 63) == 0) wmax[tid >> 6] = pmax;
  __syncthreads();
  if (tid == 0) atomicMax(&ws->pmax_bits, __float_as_uint(fmaxf(fmaxf(wmax[0], wmax[1]), fmaxf(wmax[2], wmax[3]))));
}

__global__ __launch_bounds__(256) void stft_any_kernel(const float* __restrict__ pcm, int64_t n_samples, int n_fft, int log2n, int hop, int64_t n_frames, int k_crop,
                                                        float* __restrict__ out_db, Workspace* __restrict__ ws) {
  stft_any_body<false>(pcm, n_samples, n_fft, log2n, hop, n_frames, k_crop, out_db, ws);
}

__global__ __launch_bounds__(256) void stft_any_energy_kernel(const float* __restrict__ pcm, int64_t n_samples, int n_fft, int log2n, int hop, int64_t n_frames,
                                                               int k_crop, float* __restrict__ out) {
  stft_any_body<true>(pcm, n_samples, n_fft, log2n, hop, n_frames, k_crop, out, nullptr);
}

// ---------------------------------------------------------------- STFT + mel + dB for the powers of two from 128 to 4096 (orcai_stft_mel_db away from the
// tuned 512-point kernel).  stft_any_kernel's transform, then |X|^2 of all 1 + nfft/2 bins parked in LDS and one WAVE per band: lane l adds bins
// lo + l, lo + l + 64, ... in ascending order and the 64 partial sums meet in a fixed butterfly, so two launches give the same bits.  Weights come
// from global memory (a few KiB, cached), the band table from the kernel argument.  max M as stft_any_kernel leaves max |X|^2; the level-1 histogram
// is orcai_hist_level1's second pass.
// ENERGY (stft_mel_any_energy_kernel): the band power as summed, no dB and no maximum, ws unused.
template <bool ENERGY>
__device__ __forceinline__ void stft_mel_any_body(const float* __restrict__ pcm, int64_t n_samples, int n_fft, int log2n, int hop, int64_t n_frames,
                                                  int n_mels, float* __restrict__ out_db, Workspace* __restrict__ ws, const MelBands& bands,
                                                  const float* __restrict__ weights) {
  __shared__ float2 buf[NFFT_ANY_MAX];
  __shared__ float pw[NFFT_ANY_MAX / 2 + 1];
  __shared__ float wmax[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int half = n_fft >> 1;
  float pmax = 0.0f;
  for (int64_t t = blockIdx.x; t < n_frames; t += gridDim.x) {
    const int64_t s0 = t * hop - half;
    for (int n = tid; n < n_fft; n += 256) {
      const int64_t i = s0 + n;
      const float x = (i >= 0 && i < n_samples) ? pcm[i] : 0.0f;
      const float sw = sinpif((float)n / (float)n_fft);  // periodic Hann as sin^2(pi n / N), as stft_any_kernel
      buf[__brev((uint32_t)n) >> (32 - log2n)] = make_float2(x * (sw * sw), 0.0f);
    }
    __syncthreads();
    for (int st = 1; st <= log2n; ++st) {
      const int hm = 1 << (st - 1);
      for (int j = tid; j < half; j += 256) {
        const int k = j & (hm - 1);
        const int i0 = ((j >> (st - 1)) << st) + k, i1 = i0 + hm;
        float sn, cs;
        sincospif(-(float)k / (float)hm, &sn, &cs);
        const float2 a = buf[i0], b = buf[i1];
        const float2 tb = make_float2(fmaf(b.x, cs, -b.y * sn), fmaf(b.x, sn, b.y * cs));
        buf[i0] = make_float2(a.x + tb.x, a.y + tb.y);
        buf[i1] = make_float2(a.x - tb.x, a.y - tb.y);
      }
      __syncthreads();
    }
    for (int k = tid; k <= half; k += 256) {
      const float2 z = buf[k];
      pw[k] = fmaf(z.x, z.x, z.y * z.y);
    }
    __syncthreads();
    for (int m = wave; m < n_mels; m += 4) {  // wave-uniform
      const int lo = bands.lo[m], nk = bands.n[m];
      const float* w = weights + bands.off[m];
      float acc = 0.0f;
      for (int j = lane; j < nk; j += 64) acc = fmaf(w[j], pw[lo + j], acc);
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);  // a + b == b + a: every lane holds the same bits
      if (lane == 0) out_db[t * (int64_t)n_mels + m] = ENERGY ? acc : power_to_db(acc);
      pmax = fmaxf(pmax, acc);
    }
    __syncthreads();
  }
  if constexpr (ENERGY) return;
  if (lane == 0) wmax[wave] = pmax;
  __syncthreads();
  if (tid == 0) atomicMax(&ws->pmax_bits, __float_as_uint(fmaxf(fmaxf(wmax[0], wmax[1]), fmaxf(wmax[2], wmax[3]))));
}

__global__ __launch_bounds__(256) void stft_mel_any_kernel(const float* __restrict__ pcm, int64_t n_samples, int n_fft, int log2n, int hop, int64_t n_frames,
                                                            int n_mels, float* __restrict__ out_db, Workspace* __restrict__ ws, const MelBands bands,
                                                            const float* __restrict__ weights) {
  stft_mel_any_body<false>(pcm, n_samples, n_fft, log2n, hop, n_frames, n_mels, out_db, ws, bands, weights);
}

__global__ __launch_bounds__(256) void stft_mel_any_energy_kernel(const float* __restrict__ pcm, int64_t n_samples, int n_fft, int log2n, int hop, int64_t n_frames,
                                                                   int n_mels, float* __restrict__ out, const MelBands bands, const float* __restrict__ weights) {
  stft_mel_any_body<true>(pcm, n_samples, n_fft, log2n, hop, n_frames, n_mels, out, nullptr, bands, weights);
}

// ---------------------------------------------------------------- STFT + dB for ANY transform size 2 .. 4096 (odd, 500, 1000 ...: the reference passes
// whatever the parameter file says to librosa.stft, spectrogram.py:34-39; no shipped file uses one).  A direct DFT, O(nfft^2) per frame: one workgroup per
// frame, the windowed frame and the nfft twiddles exp(-2 pi i j / nfft) as float64 in dynamic LDS (96 KB at 4096), thread = bin, the twiddle index stepped
// by k modulo nfft, float64 accumulation (numpy's rfft, which librosa calls, is float64 too).  Completeness, not speed: ~1 s per hour of audio at nfft 1000.
__global__ __launch_bounds__(256) void stft_dft_kernel(const float* __restrict__ pcm, int64_t n_samples, int n_fft, int hop, int64_t n_frames, int k_crop,
                                                        float* __restrict__ out_db, Workspace* __restrict__ ws) {
  extern __shared__ __attribute__((aligned(16))) double dft_lds[];  // [n_fft] frame, then [n_fft][2] twiddles
  __shared__ float wmax[4];
  double* xw = dft_lds;
  double2* tw = reinterpret_cast<double2*>(dft_lds + n_fft + (n_fft & 1));
  const int tid = threadIdx.x;
  const int half = n_fft >> 1;
  for (int j = tid; j < n_fft; j += 256) {
    double sn, cs;
    sincospi(2.0 * (double)j / (double)n_fft, &sn, &cs);
    tw[j] = make_double2(cs, -sn);
  }
  __syncthreads();
  float pmax = 0.0f;
  for (int64_t t = blockIdx.x; t < n_frames; t += gridDim.x) {
    const int64_t s0 = t * hop - half;
    for (int n = tid; n < n_fft; n += 256) {
      const int64_t i = s0 + n;
      const double x = (i >= 0 && i < n_samples) ? (double)pcm[i] : 0.0;
      xw[n] = x * (0.5 - 0.5 * tw[n].x);  // periodic Hann
    }
    __syncthreads();
    for (int k = tid; k <= half; k += 256) {
      double re = 0.0, im = 0.0;
      int idx = 0;
      for (int n = 0; n < n_fft; ++n) {
        const double2 w = tw[idx];
        const double x = xw[n];
        re = fma(x, w.x, re);
        im = fma(x, w.y, im);
        idx += k;
        idx -= idx >= n_fft ? n_fft : 0;
      }
      const float fr = (float)re, fi = (float)im;  // complex64, as librosa stores the transform
      const float p = fmaf(fr, fr, fi * fi);
      pmax = fmaxf(pmax, p);
      if (k < k_crop) out_db[t * (int64_t)k_crop + k] = power_to_db(p);
    }
    __syncthreads();
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) pmax = fmaxf(pmax, __shfl_xor(pmax, o, 64));
  if ((tid & 63) == 0) wmax[tid >> 6] = pmax;
  __syncthreads();
  if (tid == 0) atomicMax(&ws->pmax_bits, __float_as_uint(fmaxf(fmaxf(wmax[0], wmax[1]), fmaxf(wmax[2], wmax[3]))));
}

// ---------------------------------------------------------------- generic level-1 histogram
__global__ __launch_bounds__(256) void hist1_kernel(const float* __restrict__ x, int64_t n, Workspace* __restrict__ ws) {
  __shared__ uint32_t h[NB1_PAD];
  for (int i = threadIdx.x; i < NB1_PAD; i += 256) h[i] = 0u;
  __syncthreads();
  const int64_t n4 = n >> 2;
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += stride) {
    float4 v = reinterpret_cast<const float4*>(x)[i];
    atomicAdd(&h[bucket1(f2key(v.x))], 1u);
    atomicAdd(&h[bucket1(f2key(v.y))], 1u);
    atomicAdd(&h[bucket1(f2key(v.z))], 1u);
    atomicAdd(&h[bucket1(f2key(v.w))], 1u);
  }
  if (blockIdx.x == 0) {
    for (int64_t i = (n4 << 2) + threadIdx.x; i < n; i += 256) atomicAdd(&h[bucket1(f2key(x[i]))], 1u);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < NB1; i += 256) {
    uint32_t c = h[i];
    if (c) atomicAdd(&ws->hist1[i], c);
  }
}

// ---------------------------------------------------------------- block-wide "which bin holds rank r"
// 1024 threads; hist has nb bins; returns (bin, exclusive prefix of that bin) to every thread.
// If zero_after, bins are reset to 0 after being read (ready for the next round).
__device__ void find_bin(uint32_t* hist, int nb, uint64_t rank, bool zero_after, int& bin_out, uint64_t& prefix_out) {
  __shared__ uint64_t wave_tot[16];
  __shared__ int s_bin;
  __shared__ uint64_t s_prefix;
  const int tid = threadIdx.x;
  const int per = (nb + 1023) / 1024;
  const int b0 = tid * per;
  uint64_t sum = 0;
  for (int i = 0; i < per; ++i) {
    int b = b0 + i;
    if (b < nb) sum += hist[b];
  }
  // inclusive scan of `sum` over the block
  uint64_t incl = sum;
  const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    uint64_t o = __shfl_up(incl, off, 64);
    if (lane >= off) incl += o;
  }
  if (lane == 63) wave_tot[wave] = incl;
  if (tid == 0) { s_bin = nb - 1; s_prefix = 0; }
  __syncthreads();
  uint64_t base = 0;
  for (int w = 0; w < wave; ++w) base += wave_tot[w];
  const uint64_t excl = base + incl - sum;
  if (rank >= excl && rank < excl + sum) {
    uint64_t run = excl;
    for (int i = 0; i < per; ++i) {
      int b = b0 + i;
      if (b >= nb) break;
      uint64_t c = hist[b];
      if (rank < run + c) { s_bin = b; s_prefix = run; break; }
      run += c;
    }
  }
  __syncthreads();
  bin_out = s_bin;
  prefix_out = s_prefix;
  if (zero_after) {
    for (int i = 0; i < per; ++i) {
      int b = b0 + i;
      if (b < nb) hist[b] = 0u;
    }
  }
  __syncthreads();
}

__global__ __launch_bounds__(1024) void select_scan1_kernel(Workspace* __restrict__ ws, int64_t rank_lo, int64_t rank_hi) {
  for (int q = 0; q < 2; ++q) {
    int bin; uint64_t prefix;
    const uint64_t rank = (uint64_t)(q == 0 ? rank_lo : rank_hi);
    find_bin(ws->hist1, NB1, rank, false, bin, prefix);
    if (threadIdx.x == 0) {
      uint32_t klo; uint64_t width;
      bucket1_range(bin, klo, width);
      ws->sel[q].klo = klo;
      ws->sel[q].width = width;
      ws->sel[q].rank = rank - prefix;
      ws->sel[q].done = (width == 1) ? 1u : 0u;
    }
  }
}

// One element against both pending intervals.  All 64 lanes of the wave call this together.
__device__ __forceinline__ void hist2_add(uint32_t key, bool live, const SelState& s0, const SelState& s1, int sh0, int sh1, int lane,
                                          Workspace* __restrict__ ws) {
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const SelState& s = q ? s1 : s0;
    if (s.done) continue;  // wave-uniform
    const uint32_t d = key - s.klo;
    const bool in = live && key >= s.klo && (uint64_t)d < s.width;
    const uint32_t bin = d >> (q ? sh1 : sh0);
    const unsigned long long mask = __ballot(in);
    if (mask == 0ull) continue;
    const int first = __ffsll((long long)mask) - 1;
    const uint32_t b0 = __shfl(bin, first, 64);
    const bool uniform = __all(!in || bin == b0);
    if (uniform) {  // ties / constant input: one atomic per wave instead of 64 on one address
      if (lane == first) {
        const uint32_t c = (uint32_t)__popcll(mask);
        atomicAdd(&ws->hist2[q][b0], c);
        atomicAdd(&ws->hist2c[q][b0 >> 8], c);
      }
    } else if (in) {
      atomicAdd(&ws->hist2[q][bin], 1u);
      atomicAdd(&ws->hist2c[q][bin >> 8], 1u);
    }
  }
}

__global__ __launch_bounds__(256) void hist2_kernel(const float* __restrict__ x, int64_t n, Workspace* __restrict__ ws) {
  const SelState s0 = ws->sel[0], s1 = ws->sel[1];
  if (s0.done && s1.done) return;
  const int sh0 = shift_for(s0.width), sh1 = shift_for(s1.width);
  const int lane = threadIdx.x & 63;
  const int64_t stride = (int64_t)gridDim.x * 256;
  const int64_t n4 = n >> 2;
  const int64_t n4_round = ((n4 + stride - 1) / stride) * stride;  // whole waves stay in the loop for the ballots
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4_round; i += stride) {
    const bool live = i < n4;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (live) v = reinterpret_cast<const float4*>(x)[i];
    hist2_add(f2key(v.x), live, s0, s1, sh0, sh1, lane, ws);
    hist2_add(f2key(v.y), live, s0, s1, sh0, sh1, lane, ws);
    hist2_add(f2key(v.z), live, s0, s1, sh0, sh1, lane, ws);
    hist2_add(f2key(v.w), live, s0, s1, sh0, sh1, lane, ws);
  }
  if (blockIdx.x == 0 && threadIdx.x < 64) {  // tail (< 4 elements), one full wave
    const int64_t i = (n4 << 2) + threadIdx.x;
    const bool live = i < n;
    hist2_add(live ? f2key(x[i]) : 0u, live, s0, s1, sh0, sh1, lane, ws);
  }
}

__global__ __launch_bounds__(1024) void select_scan2_kernel(Workspace* __restrict__ ws) {
  for (int q = 0; q < 2; ++q) {
    SelState s = ws->sel[q];
    if (s.done) continue;  // uniform across the block
    const int sh = shift_for(s.width);
    int cbin, bin; uint64_t cprefix, prefix;
    find_bin(ws->hist2c[q], NB2C, s.rank, false, cbin, cprefix);              // which group of 256 fine bins
    find_bin(ws->hist2[q] + cbin * 256, 256, s.rank - cprefix, false, bin, prefix);  // which bin inside it
    bin += cbin * 256;
    prefix += cprefix;
    if (threadIdx.x == 0) {
      const uint64_t off = (uint64_t)bin << sh;
      uint64_t w = 1ull << sh;
      if (off + w > s.width) w = s.width - off;
      ws->sel[q].klo = s.klo + (uint32_t)off;
      ws->sel[q].width = w;
      ws->sel[q].rank = s.rank - prefix;
      ws->sel[q].done = (w == 1) ? 1u : 0u;
    }
    __syncthreads();
  }
}

// ---------------------------------------------------------------- radix select (orcai_quantile_select_radix)
// Three digit passes over the 32-bit key, most significant first: bits [31:21], [20:10], [9:0] (2048 / 2048 / 1024 bins).  Each pass reads x once,
// histograms the digit of the elements whose higher digits equal the prefix found so far into LDS, and adds its non-zero bins to the global histogram
// (integer sums: independent of launch order); a one-workgroup scan then turns the histogram into (digit, rank inside it) per rank.  Unlike the
// level-1 map above, nothing here depends on where the values lie.  The global histograms live at the start of Workspace::hist2, in pass order:
// [2048] shared by both ranks | [2][2048] | [2][1024]; one image serves both ranks of a later pass while their prefixes are equal.
constexpr int RADIX_WORDS = 2048 + 2 * 2048 + 2 * 1024;
__host__ __device__ constexpr int radix_shift(int pass) { return pass == 1 ? 21 : pass == 2 ? 10 : 0; }
__host__ __device__ constexpr int radix_bins(int pass) { return pass == 3 ? 1024 : 2048; }
__host__ __device__ constexpr int radix_offset(int pass) { return pass == 1 ? 0 : pass == 2 ? 2048 : 3 * 2048; }
// Do keys a and b agree above the digit of `pass`?
template <int PASS>
__device__ __forceinline__ bool radix_same_prefix(uint32_t a, uint32_t b) {
  if (PASS == 1) return true;
  return ((a ^ b) >> (PASS == 2 ? 21 : 10)) == 0u;
}

// One element into one LDS image.  All 64 lanes of the wave call this together; hist2_add's shortcut: when every taking lane hits the same bin
// (ties, constant input, PCEN's exact +0.0), one lane adds the population count instead of 64 atomics serialising on one address.
__device__ __forceinline__ void radix_add(uint32_t* __restrict__ h, uint32_t bin, bool in, int lane) {
  const unsigned long long mask = __ballot(in);
  if (mask == 0ull) return;
  const int first = __ffsll((long long)mask) - 1;
  const uint32_t b0 = (uint32_t)__builtin_amdgcn_readlane((int)bin, first);
  if (__ballot(in && bin != b0) == 0ull) {
    if (lane == first) atomicAdd(&h[b0], (uint32_t)__popcll(mask));
  } else if (in) {
    atomicAdd(&h[bin], 1u);
  }
}

template <int PASS>
__global__ __launch_bounds__(256) void radix_hist_kernel(const float* __restrict__ x, int64_t n, Workspace* __restrict__ ws) {
  constexpr int SH = radix_shift(PASS), NB = radix_bins(PASS), IMAGES = PASS == 1 ? 1 : 2;
  __shared__ uint32_t h[IMAGES * NB];
  uint32_t k0 = 0u, k1 = 0u;
  bool on0 = true, on1 = false;
  if (PASS > 1) {
    const SelState s0 = ws->sel[0], s1 = ws->sel[1];
    if (s0.done && s1.done) return;
    k0 = s0.klo;
    k1 = s1.klo;
    on0 = !s0.done;
    on1 = !s1.done && !(on0 && radix_same_prefix<PASS>(k0, k1));  // equal prefixes: image 0 is the histogram of both ranks
  }
  for (int i = threadIdx.x; i < IMAGES * NB; i += 256) h[i] = 0u;
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const auto add = [&](uint32_t key, bool live) {
    const uint32_t bin = (key >> SH) & (uint32_t)(NB - 1);
    if (PASS == 1) {
      radix_add(h, bin, live, lane);
    } else {
      if (on0) radix_add(h, bin, live && radix_same_prefix<PASS>(key, k0), lane);       // on0 / on1 are uniform across the grid
      if (on1) radix_add(h + NB, bin, live && radix_same_prefix<PASS>(key, k1), lane);
    }
  };
  const int64_t stride = (int64_t)gridDim.x * 256;
  const int64_t n4 = n >> 2;
  const int64_t n4_round = ((n4 + stride - 1) / stride) * stride;  // whole waves stay in the loop for the ballots
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4_round; i += stride) {
    const bool live = i < n4;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (live) v = reinterpret_cast<const float4*>(x)[i];
    add(f2key(v.x), live);
    add(f2key(v.y), live);
    add(f2key(v.z), live);
    add(f2key(v.w), live);
  }
  if (blockIdx.x == 0 && threadIdx.x < 64) {  // tail (< 4 elements), one full wave
    const int64_t i = (n4 << 2) + threadIdx.x;
    const bool live = i < n;
    add(live ? f2key(x[i]) : 0u, live);
  }
  __syncthreads();
  uint32_t* __restrict__ g = &ws->hist2[0][0] + radix_offset(PASS);
  for (int i = threadIdx.x; i < IMAGES * NB; i += 256) {
    const uint32_t c = h[i];
    if (c) atomicAdd(&g[i], c);
  }
}

// 1024 threads, one workgroup: the digit of `PASS` of each pending rank.  Pass 1 writes sel[] whole (nothing of an earlier select survives);
// after pass 3 sel[q] = {the key, done = 1, width = 1}: the state select_scan2_kernel leaves.
template <int PASS>
__global__ __launch_bounds__(1024) void radix_scan_kernel(Workspace* __restrict__ ws, int64_t rank_lo, int64_t rank_hi) {
  constexpr int SH = radix_shift(PASS), NB = radix_bins(PASS);
  SelState s[2];
  for (int q = 0; q < 2; ++q) {
    if (PASS == 1) {
      s[q].klo = 0u;
      s[q].done = 0u;
      s[q].width = 1ull << 32;
      s[q].rank = (uint64_t)(q == 0 ? rank_lo : rank_hi);
    } else {
      s[q] = ws->sel[q];
    }
  }
  __syncthreads();  // every thread holds both states before thread 0 writes the first
  const bool shared = !s[0].done && radix_same_prefix<PASS>(s[0].klo, s[1].klo);  // as radix_hist_kernel decided
  uint32_t* g = &ws->hist2[0][0] + radix_offset(PASS);
  for (int q = 0; q < 2; ++q) {
    if (s[q].done) continue;  // uniform across the block
    int bin; uint64_t prefix;
    find_bin(g + ((q == 1 && !shared) ? NB : 0), NB, s[q].rank, false, bin, prefix);
    if (threadIdx.x == 0) {
      ws->sel[q].klo = s[q].klo | ((uint32_t)bin << SH);
      ws->sel[q].width = 1ull << SH;
      ws->sel[q].rank = s[q].rank - prefix;
      ws->sel[q].done = SH == 0 ? 1u : 0u;
    }
  }
}

__device__ __forceinline__ float sub_rounded_once(float a, float b) {  // a - b that is never fused into the multiplication that produced b
#pragma clang fp contract(off)
  return a - b;
}

__global__ void finalize_kernel(Workspace* __restrict__ ws, int use_ref, float top_db) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const float lo = key2f(ws->sel[0].klo), hi = key2f(ws->sel[1].klo);
  ws->sel_raw[0] = lo;
  ws->sel_raw[1] = hi;
  ws->use_ref = (uint32_t)use_ref;
  if (use_ref) {
    const float ref_db = power_to_db(__uint_as_float(ws->pmax_bits));
    ws->ref_db = ref_db;
    ws->floor_db = -top_db;
    ws->p_lo = fmaxf(lo - ref_db, -top_db);
    ws->p_hi = fmaxf(hi - ref_db, -top_db);
  } else {
    ws->ref_db = 0.0f;
    ws->floor_db = -INFINITY;
    ws->p_lo = lo;
    ws->p_hi = hi;
  }
}

// use_ref = 2 (the mel route), a kernel of its own so that finalize_kernel's code stays what it is: the bound is the clipped value of the selected
// element bit for bit -- x - ref_db rounded once, as clip_normalize_kernel computes it -- where finalize_kernel fuses the subtraction into the
// multiplication that forms ref_db.
__global__ void finalize_once_kernel(Workspace* __restrict__ ws, float top_db) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const float lo = key2f(ws->sel[0].klo), hi = key2f(ws->sel[1].klo);
  const float ref_db = power_to_db(__uint_as_float(ws->pmax_bits));
  ws->sel_raw[0] = lo;
  ws->sel_raw[1] = hi;
  ws->use_ref = 2u;
  ws->ref_db = ref_db;
  ws->floor_db = -top_db;
  ws->p_lo = fmaxf(sub_rounded_once(lo, ref_db), -top_db);
  ws->p_hi = fmaxf(sub_rounded_once(hi, ref_db), -top_db);
}

__device__ __forceinline__ float norm1(float x, float ref_db, float floor_db, float lo, float hi, float range) {
  float v = fmaxf(x - ref_db, floor_db);
  v = fminf(fmaxf(v, lo), hi);
  return (v - lo) / range;
}

__global__ __launch_bounds__(256) void clip_normalize_kernel(float* __restrict__ x, int64_t n, const Workspace* __restrict__ ws) {
  const float ref_db = ws->ref_db, floor_db = ws->floor_db, lo = ws->p_lo, hi = ws->p_hi;
  const float range = hi - lo;
  const int64_t n4 = n >> 2;
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += stride) {
    float4 v = reinterpret_cast<float4*>(x)[i];
    v.x = norm1(v.x, ref_db, floor_db, lo, hi, range);
    v.y = norm1(v.y, ref_db, floor_db, lo, hi, range);
    v.z = norm1(v.z, ref_db, floor_db, lo, hi, range);
    v.w = norm1(v.w, ref_db, floor_db, lo, hi, range);
    reinterpret_cast<float4*>(x)[i] = v;
  }
  if (blockIdx.x == 0)
    for (int64_t i = (n4 << 2) + threadIdx.x; i < n; i += 256) x[i] = norm1(x[i], ref_db, floor_db, lo, hi, range);
}

__global__ __launch_bounds__(256) void db_reference_kernel(float* __restrict__ x, int64_t n, const Workspace* __restrict__ ws) {
  const float ref_db = ws->ref_db, floor_db = ws->floor_db;  // set by finalize_kernel(use_ref = 1)
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) x[i] = fmaxf(x[i] - ref_db, floor_db);
}

// [F,T] -> [T,K]: 32x32 tiles through LDS
__global__ __launch_bounds__(256) void crop_transpose_kernel(const float* __restrict__ in, int64_t n_freq, int64_t n_frames, int f_lo, int K,
                                                              float* __restrict__ out) {
  __shared__ float tile[32][33];
  const int64_t t0 = (int64_t)blockIdx.x * 32;
  const int k0 = blockIdx.y * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
  for (int r = ty; r < 32; r += 8) {
    const int k = k0 + r;
    const int64_t t = t0 + tx;
    tile[r][tx] = (k < K && t < n_frames) ? in[(int64_t)(f_lo + k) * n_frames + t] : 0.0f;
  }
  __syncthreads();
  for (int r = ty; r < 32; r += 8) {
    const int64_t t = t0 + r;
    const int k = k0 + tx;
    if (k < K && t < n_frames) out[t * K + k] = tile[tx][r];
  }
}

// ---------------------------------------------------------------- backward of the spectrogram w.r.t. the audio (orcai_spectrogram_bwd; definition in
// include/orcai_hip.h).  A GROUP of NT threads -- a wavefront for n_fft <= 512, the whole workgroup above -- owns a run of `run` consecutive output
// samples and walks over every frame that touches it, in frame order: the windowed frame goes through a radix-2 decimation-in-frequency transform in
// LDS (natural order in, X[k] at the bit-reversed position out), the complex gradient G[k] = (dRe, dIm) replaces X[k] where it stands (zero for
// k > n_fft/2 and k >= k_crop), a decimation-in-time transform with conjugated twiddles takes the bit-reversed positions back to natural order -- the
// real part of sum_k G[k] exp(+2 pi i k n / N) is the Hermitian-to-real inverse of the half spectrum -- and w[n] * Re lands in the group's LDS
// accumulator.  One thread owns one n per frame and frames follow each other behind a group barrier, so every output sample is summed in frame
// order by plain adds: no float atomics, identical bits on every launch.  Frames that straddle two runs are transformed by both groups (the halo:
// (run + n_fft) / run of the transforms, 1.25 for 512 / 2048); nothing but pcm, g and the three statistics is read and nothing but dpcm written.
template <int NT>
__device__ __forceinline__ void group_sync() {
  if constexpr (NT == 64) wave_lds_fence();
  else __syncthreads();
}

constexpr float DB_GRAD = 4.3429448190325183f;  // 10 / ln 10

// The body is spectrogram_bwd_body.inc, included as text in the two kernels below (see there for why it is no function).
// MEL (orcai_mel_spectrogram_bwd): the same two transforms with the filterbank between them; k_crop is n_mels.  With X[k] standing in buf, SUB lanes per
// band (1 for the wave-per-run kernel, a wavefront for the workgroup-per-run one) add w[j] |X[lo + j]|^2 in ascending j, strided by SUB, and meet in a
// fixed butterfly; the band's dM -- three gates, g / range * 10 / (ln 10 M) -- replaces the sum in the group's n_mels floats.  G[k] is then a GATHER:
// triangles m and m + 2 never overlap (the launcher refuses a table where they do), so a bin has at most one band of each parity, and a table built once
// per workgroup names them: per bin and parity the band (a byte, 0xFF = none) and the index of its weight in the packed weights.  dP[k] = w_even dM_even
// + w_odd dM_odd in that order.  The table, the band arrays and dM live in LDS behind the accumulators; the weights are read from global memory (a few
// KiB, read-only, shared by every frame of every workgroup) in both steps.
struct MelBwdLds {
  float* dM;                   // per group: [n_mels]
  uint16_t *widx_e, *widx_o;   // [n_bins]: index into weights of the bin's even / odd band, 0xFFFF = none (n_weights <= 65535)
  uint16_t *lo, *n, *off;      // [n_mels]
  uint8_t *band_e, *band_o;    // [n_bins]: m >> 1 of the bin's even / odd band
};
constexpr size_t mel_bwd_lds_bytes(int groups, int n_fft, int n_mels) {
  const size_t nb = (size_t)(n_fft / 2 + 4) & ~(size_t)3;  // 1 + n_fft / 2 bins, padded to a multiple of 4
  return (size_t)groups * n_mels * sizeof(float) + 2 * nb * sizeof(uint16_t) + 3 * (size_t)n_mels * sizeof(uint16_t) + 2 * nb;
}

template <int NT>
__global__ __launch_bounds__(256) void spectrogram_bwd_kernel(const float* __restrict__ pcm, int64_t n_samples, int n_fft, int log2n, int hop, int64_t n_frames,
                                                               int k_crop, const float* __restrict__ gout, const float* __restrict__ stats, float top_db,
                                                               float* __restrict__ dpcm, int run, int64_t n_runs) {
  extern __shared__ float4 bwd_lds[];
  constexpr bool MEL = false;
  constexpr bool ENERGY = false;
  const MelBands* const bands = nullptr;
  const float* const weights = nullptr;
  constexpr bool DENOISE = false;
  const float* const floor = nullptr;
#include "spectrogram_bwd_body.inc"
}

// The linear epilogue (orcai_stft_energy_bwd): gout is dL/d|X[k]|.  A kernel of its own, so that the dB kernel above compiles to what it was.
template <int NT>
__global__ __launch_bounds__(256) void stft_energy_bwd_kernel(const float* __restrict__ pcm, int64_t n_samples, int n_fft, int log2n, int hop, int64_t n_frames,
                                                               int k_crop, const float* __restrict__ gout, float* __restrict__ dpcm, int run, int64_t n_runs) {
  extern __shared__ float4 bwd_lds[];
  constexpr bool MEL = false;
  constexpr bool ENERGY = true;
  const MelBands* const bands = nullptr;
  const float* const weights = nullptr;
  constexpr bool DENOISE = false;
  const float* const floor = nullptr;
  const float* const stats = nullptr;
  const float top_db = 0.0f;
#include "spectrogram_bwd_body.inc"
}

template <int NT>
__global__ __launch_bounds__(256) void mel_spectrogram_bwd_kernel(const float* __restrict__ pcm, int64_t n_samples, int n_fft, int log2n, int hop, int64_t n_frames,
                                                                   int n_mels, const float* __restrict__ gout, const float* __restrict__ stats, float top_db,
                                                                   float* __restrict__ dpcm, int run, int64_t n_runs, const MelBands bands_by_value,
                                                                   const float* __restrict__ weights) {
  extern __shared__ float4 bwd_lds[];
  constexpr bool MEL = true;
  constexpr bool ENERGY = false;
  const MelBands* const bands = &bands_by_value;
  const int k_crop = n_mels;
  constexpr bool DENOISE = false;
  const float* const floor = nullptr;
#include "spectrogram_bwd_body.inc"
}

// orcai_stft_mel_energy_bwd: gout is dL/dM[m], the band power's gradient; the gather and everything behind it are the dB kernel's.
template <int NT>
__global__ __launch_bounds__(256) void stft_mel_energy_bwd_kernel(const float* __restrict__ pcm, int64_t n_samples, int n_fft, int log2n, int hop, int64_t n_frames,
                                                                   int n_mels, const float* __restrict__ gout, float* __restrict__ dpcm, int run, int64_t n_runs,
                                                                   const MelBands bands_by_value, const float* __restrict__ weights) {
  extern __shared__ float4 bwd_lds[];
  constexpr bool MEL = true;
  constexpr bool ENERGY = true;
  const MelBands* const bands = &bands_by_value;
  const int k_crop = n_mels;
  constexpr bool DENOISE = false;
  const float* const floor = nullptr;
  const float* const stats = nullptr;
  const float top_db = 0.0f;
#include "spectrogram_bwd_body.inc"
}

// orcai_denoised_spectrogram_bwd, linear and mel: the dB kernels with the per-channel floor in their clip gates (DENOISE in the body).  Kernels of their
// own, as the energy ones are, so that the plain kernels compile to what they were; launch geometry and LDS are those of the plain twin.
template <int NT>
__global__ __launch_bounds__(256) void denoised_spectrogram_bwd_kernel(const float* __restrict__ pcm, int64_t n_samples, int n_fft, int log2n, int hop, int64_t n_frames,
                                                                        int k_crop, const float* __restrict__ gout, const float* __restrict__ stats, float top_db,
                                                                        float* __restrict__ dpcm, int run, int64_t n_runs, const float* __restrict__ floor) {
  extern __shared__ float4 bwd_lds[];
  constexpr bool MEL = false;
  constexpr bool ENERGY = false;
  constexpr bool DENOISE = true;
  const MelBands* const bands = nullptr;
  const float* const weights = nullptr;
#include "spectrogram_bwd_body.inc"
}

template <int NT>
__global__ __launch_bounds__(256) void denoised_mel_spectrogram_bwd_kernel(const float* __restrict__ pcm, int64_t n_samples, int n_fft, int log2n, int hop,
                                                                            int64_t n_frames, int n_mels, const float* __restrict__ gout,
                                                                            const float* __restrict__ stats, float top_db, float* __restrict__ dpcm, int run,
                                                                            int64_t n_runs, const MelBands bands_by_value, const float* __restrict__ weights,
                                                                            const float* __restrict__ floor) {
  extern __shared__ float4 bwd_lds[];
  constexpr bool MEL = true;
  constexpr bool ENERGY = false;
  constexpr bool DENOISE = true;
  const MelBands* const bands = &bands_by_value;
  const int k_crop = n_mels;
#include "spectrogram_bwd_body.inc"
}

__global__ void stats_dev_kernel(const Workspace* __restrict__ ws, float* __restrict__ out) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  out[0] = __uint_as_float(ws->pmax_bits);
  out[1] = ws->ref_db;
  out[2] = ws->p_lo;
  out[3] = ws->p_hi;
  out[4] = ws->sel_raw[0];
  out[5] = ws->sel_raw[1];
}

std::once_flag g_tables_once;
int g_tables_err = 0;

void init_tables() {
  static float window[NFFT];
  static float2 tw256[256];
  static float2 tw512[260];
  const double PI = 3.14159265358979323846;
  for (int n = 0; n < NFFT; ++n) window[n] = (float)(0.5 - 0.5 * std::cos(2.0 * PI * n / NFFT));  // periodic Hann
  for (int k2 = 0; k2 < 16; ++k2)
    for (int n1 = 0; n1 < 16; ++n1) {
      const double a = -2.0 * PI * (double)(n1 * k2) / 256.0;
      tw256[k2 * 16 + n1] = make_float2((float)std::cos(a), (float)std::sin(a));
    }
  for (int k = 0; k < 260; ++k) {
    const double a = 2.0 * PI * (double)k / 512.0;
    tw512[k] = make_float2((float)std::cos(a), (float)std::sin(a));
  }
  hipError_t e = hipMemcpyToSymbol(HIP_SYMBOL(g_window), window, sizeof(window));
  if (e == hipSuccess) e = hipMemcpyToSymbol(HIP_SYMBOL(g_tw256), tw256, sizeof(tw256));
  if (e == hipSuccess) e = hipMemcpyToSymbol(HIP_SYMBOL(g_tw512), tw512, sizeof(tw512));
  g_tables_err = (int)e;
}

inline int grid_for(int64_t n_units) {
  int64_t g = n_units;
  if (g > 256 * 8) g = 256 * 8;
  if (g < 1) g = 1;
  return (int)g;
}

inline int ilog2(int n_fft) {  // of a power of two
  int log2n = 0;
  while ((1 << log2n) < n_fft) ++log2n;
  return log2n;
}

// One workgroup per frame (per group of 16 frames for the 512-point kernels), at most `cap`: the kernels stride over the rest.
inline dim3 frames_grid(int64_t n_frames, int64_t cap) { return dim3((unsigned)(n_frames < cap ? n_frames : cap)); }

// The band table is HOST memory: checked here, handed to the kernels by value.  Bands of equal parity may overlap (only the backward minds).
int pack_mel_bands(const int* band_lo, const int* band_hi, const int* band_off, int n_mels, int n_fft, int n_weights, MelBands& bands) {
  std::memset(&bands, 0, sizeof(bands));
  const int n_bins = 1 + n_fft / 2;
  for (int m = 0; m < n_mels; ++m) {
    const int lo = band_lo[m], hi = band_hi[m], off = band_off[m];
    if (lo < 0 || hi < lo || hi > n_bins || off < 0 || off > n_weights - (hi - lo)) return ORCAI_E_BADARG;
    bands.lo[m] = (uint16_t)lo;
    bands.n[m] = (uint16_t)(hi - lo);
    bands.off[m] = (uint16_t)off;
  }
  return 0;
}

// The interior groups [g_lo, g_hi) of a 512-point launch, the only ones the FAST_ONLY kernel may run (it reads pcm without bounds checks, 16 bytes
// at a time): all 16 frames of the group exist and the samples of every wave lie inside the recording, 16-byte aligned (hop 256 only) --
// t0w >= 1 for the first wave of the group, so g >= 1; (16g + 12) * 256 + 1024 <= n_samples and 16g + 15 < n_frames for the last.
// g_lo == g_hi == n_groups when there are none; g_lo == 1 when there are.
void stft_interior_groups(int64_t n_samples, int hop, int64_t n_frames, int64_t n_groups, int64_t& g_lo, int64_t& g_hi) {
  g_lo = g_hi = n_groups;
  if (hop != 256) return;
  g_lo = 1;
  const int64_t by_samples = n_samples >= 4096 ? ((n_samples - 1024) / 256 - 12) / 16 + 1 : 0;  // groups g with (16g+12)*256+1024 <= n_samples
  const int64_t by_frames = n_frames >= 16 ? (n_frames - 16) / 16 + 1 : 0;                       // groups g with 16g + 15 < n_frames
  g_hi = by_samples < by_frames ? by_samples : by_frames;
  if (g_hi > n_groups) g_hi = n_groups;
  if (g_hi < g_lo) g_lo = g_hi = n_groups;  // no interior: everything goes through the mixed kernel
}

// The launches of a tuned 512-point kernel over the groups of 16 frames: an odd hop is one launch of the <false, false> instantiation; an even hop
// with an interior is the fast kernel on it, then the mixed <true, false> one on the leading and on the trailing edge; without one, the mixed kernel
// on everything.  launch(variant, grid, g_begin, g_end) names the entry's kernels and arguments.  Called after every argument refusal.
enum class Stft512 { ANY_HOP, FAST, MIXED };  // <EVEN_HOP, FAST_ONLY> = <false, false>, <true, true>, <true, false>

template <class Launch>
int launch_stft512(int64_t n_samples, int hop, int64_t n_frames, Launch&& launch) {
  std::call_once(g_tables_once, init_tables);  // no-op: orcai_frontend_workspace_bytes() already ran it (kept for callers that size the workspace themselves)
  if (g_tables_err) return g_tables_err;
  const int64_t n_groups = (n_frames + 15) / 16;
  const auto run = [&](Stft512 variant, int64_t g_begin, int64_t g_end) { launch(variant, frames_grid(g_end - g_begin, STFT_BLOCKS), g_begin, g_end); };
  int64_t g_lo, g_hi;
  stft_interior_groups(n_samples, hop, n_frames, n_groups, g_lo, g_hi);
  if ((hop & 1) != 0) {
    run(Stft512::ANY_HOP, 0, n_groups);
  } else if (g_hi > g_lo) {
    run(Stft512::FAST, g_lo, g_hi);
    run(Stft512::MIXED, 0, g_lo);  // never empty: g_lo == 1
    if (g_hi < n_groups) run(Stft512::MIXED, g_hi, n_groups);
  } else {
    run(Stft512::MIXED, 0, n_groups);
  }
  return (int)hipGetLastError();
}

// The launch geometry of the four backward kernels.  Run of output samples per group: 2048 for the wave-per-run kernel (LDS 2 KiB twiddles +
// 4 x (4 + 8) KiB at 512: three workgroups per compute unit), 4 n_fft for the workgroup-per-run kernel, n_fft at 4096 (twiddles + frame +
// accumulator = 64 KiB, the most a launch gets without opting in).  n_mels = 0: the linear routes; otherwise the mel gather's LDS comes on top.
struct BwdPlan {
  bool wave;   // n_fft <= 512: the <64> instantiation, a wave per run and four runs per workgroup; else <256>, a workgroup per run
  int run;     // output samples per run
  int groups;  // runs per workgroup
  size_t lds;  // dynamic LDS bytes of the launch
  int64_t n_runs(int64_t n_samples) const { return (n_samples + run - 1) / run; }
  dim3 grid(int64_t n_samples) const {
    const int64_t blocks = (n_runs(n_samples) + groups - 1) / groups;
    return dim3((unsigned)(blocks < 256 * 12 ? blocks : 256 * 12));
  }
};

BwdPlan bwd_plan(int n_fft, int n_mels) {
  BwdPlan p;
  p.wave = n_fft <= 512;
  p.run = p.wave ? 2048 : (n_fft == 4096 ? 4096 : 4 * n_fft);
  p.groups = p.wave ? 4 : 1;
  p.lds = sizeof(float2) * (size_t)(n_fft / 2) + (size_t)p.groups * (sizeof(float2) * (size_t)n_fft + sizeof(float) * (size_t)p.run) +
          (n_mels ? mel_bwd_lds_bytes(p.groups, n_fft, n_mels) : 0);
  return p;
}

// The launchers behind orcai_spectrogram_bwd (ENERGY = false) and orcai_stft_energy_bwd (ENERGY = true: stats_dev and top_db are not looked at).
// DENOISE (orcai_denoised_spectrogram_bwd, linear route): the same checks and the same plan, the kernel with the floor f32[k_crop] in its gates.
template <bool ENERGY, bool DENOISE = false>
int spectrogram_bwd_launch(const float* pcm, int64_t n_samples, int n_fft, int hop, int64_t n_frames, int k_crop, const float* gout, const float* stats_dev,
                           float top_db, float* dpcm, void* stream, const float* floor = nullptr) {
  static_assert(!(ENERGY && DENOISE), "the energy epilogue has no clip gates");
  if (!pcm || !gout || (!ENERGY && !stats_dev) || !dpcm || n_samples <= 0 || hop <= 0 || n_frames <= 0 || k_crop < 1 || n_fft < 2) return ORCAI_E_BADARG;
  if (DENOISE && !floor) return ORCAI_E_BADARG;
  if (n_fft < 32 || n_fft > NFFT_ANY_MAX || (n_fft & (n_fft - 1))) return ORCAI_E_UNSUPPORTED;  // powers of two from 32 to 4096 only
  if (k_crop > 1 + n_fft / 2 || n_frames != 1 + n_samples / hop) return ORCAI_E_BADARG;         // librosa's centred frame count (n_fft is even)
  const BwdPlan p = bwd_plan(n_fft, 0);
  if (p.lds > 64 * 1024) return ORCAI_E_UNSUPPORTED;  // (never: 64 KiB at n_fft = 4096 is the largest request)
  const dim3 grid = p.grid(n_samples);
  const int64_t n_runs = p.n_runs(n_samples);
  const int log2n = ilog2(n_fft);
  hipStream_t st = (hipStream_t)stream;
  if constexpr (ENERGY) {
    if (p.wave) hipLaunchKernelGGL((stft_energy_bwd_kernel<64>), grid, dim3(256), p.lds, st, pcm, n_samples, n_fft, log2n, hop, n_frames, k_crop, gout, dpcm, p.run, n_runs);
    else hipLaunchKernelGGL((stft_energy_bwd_kernel<256>), grid, dim3(256), p.lds, st, pcm, n_samples, n_fft, log2n, hop, n_frames, k_crop, gout, dpcm, p.run, n_runs);
  } else if constexpr (DENOISE) {
    if (p.wave)
      hipLaunchKernelGGL((denoised_spectrogram_bwd_kernel<64>), grid, dim3(256), p.lds, st, pcm, n_samples, n_fft, log2n, hop, n_frames, k_crop, gout, stats_dev, top_db, dpcm,
                         p.run, n_runs, floor);
    else
      hipLaunchKernelGGL((denoised_spectrogram_bwd_kernel<256>), grid, dim3(256), p.lds, st, pcm, n_samples, n_fft, log2n, hop, n_frames, k_crop, gout, stats_dev, top_db, dpcm,
                         p.run, n_runs, floor);
  } else {
    if (p.wave)
      hipLaunchKernelGGL((spectrogram_bwd_kernel<64>), grid, dim3(256), p.lds, st, pcm, n_samples, n_fft, log2n, hop, n_frames, k_crop, gout, stats_dev, top_db, dpcm, p.run,
                         n_runs);
    else
      hipLaunchKernelGGL((spectrogram_bwd_kernel<256>), grid, dim3(256), p.lds, st, pcm, n_samples, n_fft, log2n, hop, n_frames, k_crop, gout, stats_dev, top_db, dpcm, p.run,
                         n_runs);
  }
  return (int)hipGetLastError();
}

// Likewise behind orcai_mel_spectrogram_bwd and orcai_stft_mel_energy_bwd, and with DENOISE behind orcai_denoised_spectrogram_bwd's mel route.
template <bool ENERGY, bool DENOISE = false>
int mel_spectrogram_bwd_launch(const float* pcm, int64_t n_samples, int n_fft, int hop, int64_t n_frames, int n_mels, const int* band_lo, const int* band_hi,
                               const int* band_off, const float* weights, int n_weights, const float* gout, const float* stats_dev, float top_db, float* dpcm,
                               void* stream, const float* floor = nullptr) {
  static_assert(!(ENERGY && DENOISE), "the energy epilogue has no clip gates");
  if (!pcm || !band_lo || !band_hi || !band_off || !weights || !gout || (!ENERGY && !stats_dev) || !dpcm || (DENOISE && !floor)) return ORCAI_E_BADARG;
  if (n_samples <= 0 || hop <= 0 || n_frames <= 0 || n_fft < 2 || n_mels < 8 || n_mels > MEL_MAX || n_weights < 1 || n_weights > 65535) return ORCAI_E_BADARG;
  if (((uintptr_t)pcm & 15) || ((uintptr_t)weights & 15) || ((uintptr_t)gout & 3) || ((uintptr_t)stats_dev & 3) || ((uintptr_t)dpcm & 3)) return ORCAI_E_BADARG;
  if (n_fft < 128 || n_fft > NFFT_ANY_MAX || (n_fft & (n_fft - 1))) return ORCAI_E_UNSUPPORTED;
  if (n_frames != 1 + n_samples / hop) return ORCAI_E_BADARG;  // librosa's centred frame count (n_fft is even)
  MelBands bands;
  if (const int e = pack_mel_bands(band_lo, band_hi, band_off, n_mels, n_fft, n_weights, bands)) return e;
  // The per-bin gather has one even-band and one odd-band entry: bands of equal parity must not share a bin.  Checked against the running end of the
  // non-empty bands of each parity, so an empty band between two overlapping ones hides nothing.
  int end[2] = {0, 0};
  for (int m = 0; m < n_mels; ++m) {
    if (band_hi[m] == band_lo[m]) continue;
    if (band_lo[m] < end[m & 1]) return ORCAI_E_UNSUPPORTED;
    end[m & 1] = band_hi[m];
  }
  const BwdPlan p = bwd_plan(n_fft, n_mels);
  constexpr size_t LDS_MAX = 64 * 1024 + mel_bwd_lds_bytes(1, NFFT_ANY_MAX, MEL_MAX);  // the request at n_fft = 4096 with 256 bands: 80 408 B, two per compute unit
  if (p.lds > LDS_MAX) return ORCAI_E_UNSUPPORTED;  // (never)
  if (p.wave && p.lds > 64 * 1024) return ORCAI_E_UNSUPPORTED;  // (never: the wave-per-run kernel asks for at most 58 392 B and does not opt in)
  if (p.lds > 64 * 1024) {  // n_fft = 4096, and 2048 with more than 202 bands
    hipError_t e;
    if constexpr (ENERGY) e = orcai_lds::ensure_dynamic_lds<stft_mel_energy_bwd_kernel<256>>(LDS_MAX);
    else if constexpr (DENOISE) e = orcai_lds::ensure_dynamic_lds<denoised_mel_spectrogram_bwd_kernel<256>>(LDS_MAX);
    else e = orcai_lds::ensure_dynamic_lds<mel_spectrogram_bwd_kernel<256>>(LDS_MAX);
    if (e != hipSuccess) return (int)e;
  }
  const dim3 grid = p.grid(n_samples);
  const int64_t n_runs = p.n_runs(n_samples);
  const int log2n = ilog2(n_fft);
  hipStream_t st = (hipStream_t)stream;
  if constexpr (ENERGY) {
    if (p.wave)
      hipLaunchKernelGGL((stft_mel_energy_bwd_kernel<64>), grid, dim3(256), p.lds, st, pcm, n_samples, n_fft, log2n, hop, n_frames, n_mels, gout, dpcm, p.run, n_runs, bands,
                         weights);
    else
      hipLaunchKernelGGL((stft_mel_energy_bwd_kernel<256>), grid, dim3(256), p.lds, st, pcm, n_samples, n_fft, log2n, hop, n_frames, n_mels, gout, dpcm, p.run, n_runs, bands,
                         weights);
  } else if constexpr (DENOISE) {
    if (p.wave)
      hipLaunchKernelGGL((denoised_mel_spectrogram_bwd_kernel<64>), grid, dim3(256), p.lds, st, pcm, n_samples, n_fft, log2n, hop, n_frames, n_mels, gout, stats_dev, top_db,
                         dpcm, p.run, n_runs, bands, weights, floor);
    else
      hipLaunchKernelGGL((denoised_mel_spectrogram_bwd_kernel<256>), grid, dim3(256), p.lds, st, pcm, n_samples, n_fft, log2n, hop, n_frames, n_mels, gout, stats_dev, top_db,
                         dpcm, p.run, n_runs, bands, weights, floor);
  } else {
    if (p.wave)
      hipLaunchKernelGGL((mel_spectrogram_bwd_kernel<64>), grid, dim3(256), p.lds, st, pcm, n_samples, n_fft, log2n, hop, n_frames, n_mels, gout, stats_dev, top_db, dpcm,
                         p.run, n_runs, bands, weights);
    else
      hipLaunchKernelGGL((mel_spectrogram_bwd_kernel<256>), grid, dim3(256), p.lds, st, pcm, n_samples, n_fft, log2n, hop, n_frames, n_mels, gout, stats_dev, top_db, dpcm,
                         p.run, n_runs, bands, weights);
  }
  return (int)hipGetLastError();
}

}  // namespace

extern "C" {

size_t orcai_frontend_workspace_bytes(void) {
  // Setup call (every caller needs it before it can allocate the workspace): the window / twiddle tables are uploaded here, with a
  // synchronous hipMemcpyToSymbol, so that no later call -- orcai_frontend_reset, orcai_stft_db, ... -- does anything but enqueue
  // work on the caller's stream (hipGraph-capturable from the first call on).  An upload error is reported by orcai_stft_db.
  std::call_once(g_tables_once, init_tables);
  return (sizeof(Workspace) + 255) & ~(size_t)255;
}

int orcai_frontend_reset(void* workspace, void* stream) {
  if (!workspace) return ORCAI_E_BADARG;
  return (int)orcai_zero::zero_async(workspace, sizeof(Workspace), (hipStream_t)stream);
}

int orcai_stft_db(const float* pcm, int64_t n_samples, int n_fft, int hop, int64_t n_frames, int k_crop, float* out_db, void* workspace,
                  void* stream) {
  if (!pcm || !out_db || !workspace || n_samples <= 0 || hop <= 0 || k_crop < 1 || n_fft < 2 || k_crop > 1 + n_fft / 2) return ORCAI_E_BADARG;
  if (n_frames != 1 + (n_samples - (n_fft & 1)) / hop) return ORCAI_E_BADARG;  // librosa, center = True: 1 + (n + 2 (n_fft / 2) - n_fft) / hop
  if (((uintptr_t)out_db & 15) || ((uintptr_t)pcm & 15)) return ORCAI_E_BADARG;
  Workspace* ws = (Workspace*)workspace;
  hipStream_t st = (hipStream_t)stream;
  if (n_fft != NFFT) {  // any other size up to 4096: the plain radix-2 kernel (powers of two from 32) or the direct transform, + a separate level-1 histogram pass
    if (n_fft > NFFT_ANY_MAX) return ORCAI_E_UNSUPPORTED;
    if (n_fft < 32 || (n_fft & (n_fft - 1))) {  // not a power of two (or a tiny one): the direct transform
      const size_t lds = sizeof(double) * ((size_t)n_fft + (n_fft & 1) + 2 * (size_t)n_fft);
      if (lds > 48 * 1024)
        if (const hipError_t e = orcai_lds::ensure_dynamic_lds<stft_dft_kernel>(3 * NFFT_ANY_MAX * sizeof(double)); e != hipSuccess) return (int)e;
      hipLaunchKernelGGL(stft_dft_kernel, frames_grid(n_frames, 256 * 4), dim3(256), lds, st, pcm, n_samples, n_fft, hop, n_frames, k_crop, out_db, ws);
    } else {
      hipLaunchKernelGGL(stft_any_kernel, frames_grid(n_frames, 256 * 16), dim3(256), 0, st, pcm, n_samples, n_fft, ilog2(n_fft), hop, n_frames, k_crop, out_db, ws);
    }
    if (const hipError_t e = hipGetLastError(); e != hipSuccess) return (int)e;
    return orcai_hist_level1(out_db, n_frames * (int64_t)k_crop, workspace, stream);
  }
  return launch_stft512(n_samples, hop, n_frames, [&](Stft512 variant, dim3 grid, int64_t g_begin, int64_t g_end) {
    const auto go = [&](auto kernel) { hipLaunchKernelGGL(kernel, grid, dim3(256), 0, st, pcm, n_samples, hop, n_frames, k_crop, out_db, ws, g_begin, g_end); };
    if (variant == Stft512::ANY_HOP) go(stft_db_kernel<false, false, 0>);
    else if (variant == Stft512::MIXED) go(stft_db_kernel<true, false, 0>);
    else if (k_crop == 171) go(stft_db_kernel<true, true, 171>);
    else go(stft_db_kernel<true, true, 0>);
  });
}

int orcai_stft_occupancy(void) {  // workgroups of stft_db_kernel<true, true, 171> the runtime says fit one compute unit (LDS: 52 KiB each)
  int n = -1;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, (const void*)stft_db_kernel<true, true, 171>, 256, 0) != hipSuccess) return -1;
  return n;
}

int orcai_stft_mel_db(const float* pcm, int64_t n_samples, int n_fft, int hop, int64_t n_frames, int n_mels, const int* band_lo, const int* band_hi,
                      const int* band_off, const float* weights, int n_weights, float* out_db, void* workspace, void* stream) {
  if (!pcm || !band_lo || !band_hi || !band_off || !weights || !out_db || !workspace) return ORCAI_E_BADARG;
  if (n_samples <= 0 || hop <= 0 || n_fft < 2 || n_mels < 8 || n_mels > MEL_MAX || n_weights < 1 || n_weights > 65535) return ORCAI_E_BADARG;
  if (((uintptr_t)out_db & 15) || ((uintptr_t)pcm & 15) || ((uintptr_t)weights & 15)) return ORCAI_E_BADARG;
  if (n_fft < 128 || n_fft > NFFT_ANY_MAX || (n_fft & (n_fft - 1))) return ORCAI_E_UNSUPPORTED;
  if (n_frames != 1 + n_samples / hop) return ORCAI_E_BADARG;  // librosa's centred frame count (n_fft is even)
  MelBands bands;
  if (const int e = pack_mel_bands(band_lo, band_hi, band_off, n_mels, n_fft, n_weights, bands)) return e;
  Workspace* ws = (Workspace*)workspace;
  hipStream_t st = (hipStream_t)stream;
  if (n_fft != NFFT || n_weights > MEL_W_LDS) {  // (512 with a table wider than the tuned kernel's LDS copy -- no triangular one is -- runs here too)
    hipLaunchKernelGGL(stft_mel_any_kernel, frames_grid(n_frames, 256 * 16), dim3(256), 0, st, pcm, n_samples, n_fft, ilog2(n_fft), hop, n_frames, n_mels, out_db, ws,
                       bands, weights);
    if (const hipError_t e = hipGetLastError(); e != hipSuccess) return (int)e;
    return orcai_hist_level1(out_db, n_frames * (int64_t)n_mels, workspace, stream);
  }
  return launch_stft512(n_samples, hop, n_frames, [&](Stft512 variant, dim3 grid, int64_t g_begin, int64_t g_end) {
    const auto go = [&](auto kernel) {
      hipLaunchKernelGGL(kernel, grid, dim3(256), 0, st, pcm, n_samples, hop, n_frames, n_mels, out_db, ws, g_begin, g_end, bands, weights, n_weights);
    };
    if (variant == Stft512::ANY_HOP) go(stft_mel_kernel<false, false>);
    else if (variant == Stft512::MIXED) go(stft_mel_kernel<true, false>);
    else go(stft_mel_kernel<true, true>);
  });
}

int orcai_stft_mel_occupancy(void) {  // workgroups of stft_mel_kernel<true, true> the runtime says fit one compute unit
  int n = -1;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, (const void*)stft_mel_kernel<true, true>, 256, 0) != hipSuccess) return -1;
  return n;
}

int orcai_stft_energy(const float* pcm, int64_t n_samples, int n_fft, int hop, int64_t n_frames, int k_crop, float* out, void* stream) {
  if (!pcm || !out || n_samples <= 0 || hop <= 0 || k_crop < 1 || n_fft < 2 || k_crop > 1 + n_fft / 2) return ORCAI_E_BADARG;
  if (((uintptr_t)out & 15) || ((uintptr_t)pcm & 15)) return ORCAI_E_BADARG;
  if (n_fft < 32 || n_fft > NFFT_ANY_MAX || (n_fft & (n_fft - 1))) return ORCAI_E_UNSUPPORTED;  // the direct transform has no energy epilogue
  if (n_frames != 1 + n_samples / hop) return ORCAI_E_BADARG;  // librosa's centred frame count (n_fft is even)
  hipStream_t st = (hipStream_t)stream;
  if (n_fft != NFFT) {
    hipLaunchKernelGGL(stft_any_energy_kernel, frames_grid(n_frames, 256 * 16), dim3(256), 0, st, pcm, n_samples, n_fft, ilog2(n_fft), hop, n_frames, k_crop, out);
    return (int)hipGetLastError();
  }
  return launch_stft512(n_samples, hop, n_frames, [&](Stft512 variant, dim3 grid, int64_t g_begin, int64_t g_end) {
    const auto go = [&](auto kernel) { hipLaunchKernelGGL(kernel, grid, dim3(256), 0, st, pcm, n_samples, hop, n_frames, k_crop, out, g_begin, g_end); };
    if (variant == Stft512::ANY_HOP) go(stft_energy_kernel<false, false, 0>);
    else if (variant == Stft512::MIXED) go(stft_energy_kernel<true, false, 0>);
    else if (k_crop == 171) go(stft_energy_kernel<true, true, 171>);
    else go(stft_energy_kernel<true, true, 0>);
  });
}

int orcai_stft_mel_energy(const float* pcm, int64_t n_samples, int n_fft, int hop, int64_t n_frames, int n_mels, const int* band_lo, const int* band_hi,
                          const int* band_off, const float* weights, int n_weights, float* out, void* stream) {
  if (!pcm || !band_lo || !band_hi || !band_off || !weights || !out) return ORCAI_E_BADARG;
  if (n_samples <= 0 || hop <= 0 || n_fft < 2 || n_mels < 8 || n_mels > MEL_MAX || n_weights < 1 || n_weights > 65535) return ORCAI_E_BADARG;
  if (((uintptr_t)out & 15) || ((uintptr_t)pcm & 15) || ((uintptr_t)weights & 15)) return ORCAI_E_BADARG;
  if (n_fft < 128 || n_fft > NFFT_ANY_MAX || (n_fft & (n_fft - 1))) return ORCAI_E_UNSUPPORTED;
  if (n_frames != 1 + n_samples / hop) return ORCAI_E_BADARG;
  MelBands bands;
  if (const int e = pack_mel_bands(band_lo, band_hi, band_off, n_mels, n_fft, n_weights, bands)) return e;
  hipStream_t st = (hipStream_t)stream;
  if (n_fft != NFFT || n_weights > MEL_W_LDS) {
    hipLaunchKernelGGL(stft_mel_any_energy_kernel, frames_grid(n_frames, 256 * 16), dim3(256), 0, st, pcm, n_samples, n_fft, ilog2(n_fft), hop, n_frames, n_mels, out, bands,
                       weights);
    return (int)hipGetLastError();
  }
  return launch_stft512(n_samples, hop, n_frames, [&](Stft512 variant, dim3 grid, int64_t g_begin, int64_t g_end) {
    const auto go = [&](auto kernel) {
      hipLaunchKernelGGL(kernel, grid, dim3(256), 0, st, pcm, n_samples, hop, n_frames, n_mels, out, g_begin, g_end, bands, weights, n_weights);
    };
    if (variant == Stft512::ANY_HOP) go(stft_mel_energy_kernel<false, false>);
    else if (variant == Stft512::MIXED) go(stft_mel_energy_kernel<true, false>);
    else go(stft_mel_energy_kernel<true, true>);
  });
}

int orcai_hist_level1(const float* x, int64_t n, void* workspace, void* stream) {
  if (!x || !workspace || n <= 0 || ((uintptr_t)x & 15)) return ORCAI_E_BADARG;
  int grid = grid_for((n / 4 + 255) / 256);
  hipLaunchKernelGGL(hist1_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, x, n, (Workspace*)workspace);
  return (int)hipGetLastError();
}

int orcai_quantile_select(const float* x, int64_t n, int64_t rank_lo, int64_t rank_hi, void* workspace, void* stream) {
  if (!x || !workspace || n <= 0 || rank_lo < 0 || rank_hi < 0 || rank_lo >= n || rank_hi >= n) return ORCAI_E_BADARG;
  Workspace* ws = (Workspace*)workspace;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(select_scan1_kernel, dim3(1), dim3(1024), 0, s, ws, rank_lo, rank_hi);
  if ((uintptr_t)x & 15) return ORCAI_E_BADARG;
  int grid = grid_for((n / 4 + 255) / 256);
  for (int round = 0; round < 2; ++round) {  // a level-1 bucket is at most 2^31 keys wide: two 16-bit rounds
    hipError_t e = orcai_zero::zero_async(ws->hist2, sizeof(ws->hist2) + sizeof(ws->hist2c), s);  // hist2c follows hist2
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(hist2_kernel, dim3(grid), dim3(256), 0, s, x, n, ws);
    hipLaunchKernelGGL(select_scan2_kernel, dim3(1), dim3(1024), 0, s, ws);
  }
  return (int)hipGetLastError();
}

int orcai_quantile_select_radix(const float* x, int64_t n, int64_t rank_lo, int64_t rank_hi, void* workspace, void* stream) {
  if (!x || !workspace || n <= 0 || n >= ((int64_t)1 << 32) || rank_lo < 0 || rank_hi < 0 || rank_lo >= n || rank_hi >= n || ((uintptr_t)x & 15))
    return ORCAI_E_BADARG;  // the bins are u32
  Workspace* ws = (Workspace*)workspace;
  hipStream_t s = (hipStream_t)stream;
  static_assert(RADIX_WORDS * sizeof(uint32_t) <= sizeof(ws->hist2), "the radix histograms live in hist2");
  const hipError_t e = orcai_zero::zero_async(ws->hist2, RADIX_WORDS * sizeof(uint32_t), s);  // all three passes' histograms; hist1 and pmax_bits stay
  if (e != hipSuccess) return (int)e;
  const int grid = grid_for((n / 4 + 255) / 256);
  hipLaunchKernelGGL(radix_hist_kernel<1>, dim3(grid), dim3(256), 0, s, x, n, ws);
  hipLaunchKernelGGL(radix_scan_kernel<1>, dim3(1), dim3(1024), 0, s, ws, rank_lo, rank_hi);
  hipLaunchKernelGGL(radix_hist_kernel<2>, dim3(grid), dim3(256), 0, s, x, n, ws);
  hipLaunchKernelGGL(radix_scan_kernel<2>, dim3(1), dim3(1024), 0, s, ws, rank_lo, rank_hi);
  hipLaunchKernelGGL(radix_hist_kernel<3>, dim3(grid), dim3(256), 0, s, x, n, ws);
  hipLaunchKernelGGL(radix_scan_kernel<3>, dim3(1), dim3(1024), 0, s, ws, rank_lo, rank_hi);
  return (int)hipGetLastError();
}

int orcai_frontend_finalize(int use_ref, float top_db, void* workspace, void* stream) {
  if (!workspace) return ORCAI_E_BADARG;
  if (use_ref == 2) hipLaunchKernelGGL(finalize_once_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (Workspace*)workspace, top_db);
  else hipLaunchKernelGGL(finalize_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (Workspace*)workspace, use_ref, top_db);
  return (int)hipGetLastError();
}

int orcai_clip_normalize(float* x, int64_t n, const void* workspace, void* stream) {
  if (!x || !workspace || n <= 0 || ((uintptr_t)x & 15)) return ORCAI_E_BADARG;
  int grid = grid_for((n / 4 + 255) / 256);
  hipLaunchKernelGGL(clip_normalize_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, x, n, (const Workspace*)workspace);
  return (int)hipGetLastError();
}

int orcai_db_reference(float* x, int64_t n, const void* workspace, void* stream) {
  if (!x || !workspace || n <= 0) return ORCAI_E_BADARG;
  int grid = grid_for((n + 255) / 256);
  hipLaunchKernelGGL(db_reference_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, x, n, (const Workspace*)workspace);
  return (int)hipGetLastError();
}

int orcai_crop_transpose(const float* in_ft, int64_t n_freq, int64_t n_frames, int f_lo, int f_hi, float* out_tf, void* stream) {
  if (!in_ft || !out_tf || n_freq <= 0 || n_frames <= 0 || f_lo < 0 || f_hi <= f_lo || f_hi > n_freq) return ORCAI_E_BADARG;
  const int K = f_hi - f_lo;
  dim3 grid((unsigned)((n_frames + 31) / 32), (unsigned)((K + 31) / 32));
  hipLaunchKernelGGL(crop_transpose_kernel, grid, dim3(256), 0, (hipStream_t)stream, in_ft, n_freq, n_frames, f_lo, K, out_tf);
  return (int)hipGetLastError();
}

int orcai_frontend_stats_host(const void* workspace, float stats_host[6], void* stream) {
  if (!workspace || !stats_host) return ORCAI_E_BADARG;
  Workspace* h = new Workspace;
  hipError_t e = hipMemcpyAsync(h, workspace, sizeof(Workspace), hipMemcpyDeviceToHost, (hipStream_t)stream);
  if (e == hipSuccess) e = hipStreamSynchronize((hipStream_t)stream);
  if (e == hipSuccess) {
    float pm;
    std::memcpy(&pm, &h->pmax_bits, 4);
    stats_host[0] = pm;
    stats_host[1] = h->ref_db;
    stats_host[2] = h->p_lo;
    stats_host[3] = h->p_hi;
    stats_host[4] = h->sel_raw[0];
    stats_host[5] = h->sel_raw[1];
  }
  delete h;
  return (int)e;
}

int orcai_frontend_stats_dev(const void* workspace, float* stats_dev, void* stream) {
  if (!workspace || !stats_dev) return ORCAI_E_BADARG;
  hipLaunchKernelGGL(stats_dev_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (const Workspace*)workspace, stats_dev);
  return (int)hipGetLastError();
}

int orcai_spectrogram_bwd(const float* pcm, int64_t n_samples, int n_fft, int hop, int64_t n_frames, int k_crop, const float* gout, const float* stats_dev,
                          float top_db, float* dpcm, void* stream) {
  return spectrogram_bwd_launch<false>(pcm, n_samples, n_fft, hop, n_frames, k_crop, gout, stats_dev, top_db, dpcm, stream);
}

int orcai_stft_energy_bwd(const float* pcm, int64_t n_samples, int n_fft, int hop, int64_t n_frames, int k_crop, const float* gE, float* dpcm, void* stream) {
  return spectrogram_bwd_launch<true>(pcm, n_samples, n_fft, hop, n_frames, k_crop, gE, nullptr, 0.0f, dpcm, stream);
}

int orcai_mel_spectrogram_bwd(const float* pcm, int64_t n_samples, int n_fft, int hop, int64_t n_frames, int n_mels, const int* band_lo, const int* band_hi,
                              const int* band_off, const float* weights, int n_weights, const float* gout, const float* stats_dev, float top_db, float* dpcm,
                              void* stream) {
  return mel_spectrogram_bwd_launch<false>(pcm, n_samples, n_fft, hop, n_frames, n_mels, band_lo, band_hi, band_off, weights, n_weights, gout, stats_dev, top_db, dpcm,
                                           stream);
}

int orcai_stft_mel_energy_bwd(const float* pcm, int64_t n_samples, int n_fft, int hop, int64_t n_frames, int n_mels, const int* band_lo, const int* band_hi,
                              const int* band_off, const float* weights, int n_weights, const float* gE, float* dpcm, void* stream) {
  return mel_spectrogram_bwd_launch<true>(pcm, n_samples, n_fft, hop, n_frames, n_mels, band_lo, band_hi, band_off, weights, n_weights, gE, nullptr, 0.0f, dpcm, stream);
}

int orcai_mel_spectrogram_bwd_occupancy(int n_fft, int n_mels) {  // workgroups of the mel backward the runtime says fit one compute unit; -1 on refusal
  if (n_fft < 128 || n_fft > NFFT_ANY_MAX || (n_fft & (n_fft - 1)) || n_mels < 8 || n_mels > MEL_MAX) return -1;
  const BwdPlan p = bwd_plan(n_fft, n_mels);
  int n = -1;
  const hipError_t e = p.wave ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, (const void*)mel_spectrogram_bwd_kernel<64>, 256, p.lds)
                              : hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, (const void*)mel_spectrogram_bwd_kernel<256>, 256, p.lds);
  return e == hipSuccess ? n : -1;
}

int orcai_denoised_spectrogram_bwd(const float* pcm, int64_t n_samples, int n_fft, int hop, int64_t n_frames, int k, const int* band_lo, const int* band_hi,
                                   const int* band_off, const float* weights, int n_weights, const float* gout, const float* stats_dev, const float* profile,
                                   float top_db, float* dpcm, void* stream) {
  if (!pcm || !gout || !stats_dev || !profile || !dpcm) return ORCAI_E_BADARG;
  if (((uintptr_t)pcm & 3) || ((uintptr_t)gout & 3) || ((uintptr_t)stats_dev & 3) || ((uintptr_t)profile & 3) || ((uintptr_t)dpcm & 3)) return ORCAI_E_BADARG;
  if (!band_lo)  // the linear route: k is k_crop, the other band arguments are not looked at
    return spectrogram_bwd_launch<false, true>(pcm, n_samples, n_fft, hop, n_frames, k, gout, stats_dev, top_db, dpcm, stream, profile);
  return mel_spectrogram_bwd_launch<false, true>(pcm, n_samples, n_fft, hop, n_frames, k, band_lo, band_hi, band_off, weights, n_weights, gout, stats_dev, top_db, dpcm,
                                                 stream, profile);
}

int orcai_denoised_spectrogram_bwd_occupancy(int n_fft, int n_mels) {  // n_mels = 0: the linear route; -1 on refusal
  if (n_fft < (n_mels ? 128 : 32) || n_fft > NFFT_ANY_MAX || (n_fft & (n_fft - 1)) || (n_mels && (n_mels < 8 || n_mels > MEL_MAX))) return -1;
  const BwdPlan p = bwd_plan(n_fft, n_mels);
  const void* f = n_mels ? (p.wave ? (const void*)denoised_mel_spectrogram_bwd_kernel<64> : (const void*)denoised_mel_spectrogram_bwd_kernel<256>)
                         : (p.wave ? (const void*)denoised_spectrogram_bwd_kernel<64> : (const void*)denoised_spectrogram_bwd_kernel<256>);
  int n = -1;
  return hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, f, 256, p.lds) == hipSuccess ? n : -1;
}

int orcai_make_spectrogram(const float* pcm, int64_t n_samples, int n_fft, int hop, int64_t n_frames, int k_crop, int64_t rank_lo,
                           int64_t rank_hi, float top_db, float* out, void* workspace, void* stream) {
  int e = orcai_frontend_reset(workspace, stream);
  if (e) return e;
  e = orcai_stft_db(pcm, n_samples, n_fft, hop, n_frames, k_crop, out, workspace, stream);
  if (e) return e;
  const int64_t n = n_frames * (int64_t)k_crop;
  e = orcai_quantile_select(out, n, rank_lo, rank_hi, workspace, stream);
  if (e) return e;
  e = orcai_frontend_finalize(1, top_db, workspace, stream);
  if (e) return e;
  return orcai_clip_normalize(out, n, workspace, stream);
}

int orcai_make_mel_spectrogram(const float* pcm, int64_t n_samples, int n_fft, int hop, int64_t n_frames, int n_mels, const int* band_lo, const int* band_hi,
                               const int* band_off, const float* weights, int n_weights, int64_t rank_lo, int64_t rank_hi, float top_db, float* out,
                               void* workspace, void* stream) {
  const int64_t n = n_frames * (int64_t)n_mels;
  if (!workspace || !out || n_mels < 8 || n_mels > MEL_MAX || n_frames <= 0 || rank_lo < 0 || rank_hi < 0 || rank_lo >= n || rank_hi >= n)
    return ORCAI_E_BADARG;  // what the later steps would refuse, before the first one runs
  int e = orcai_frontend_reset(workspace, stream);
  if (e) return e;
  e = orcai_stft_mel_db(pcm, n_samples, n_fft, hop, n_frames, n_mels, band_lo, band_hi, band_off, weights, n_weights, out, workspace, stream);
  if (e) return e;
  e = orcai_quantile_select(out, n, rank_lo, rank_hi, workspace, stream);
  if (e) return e;
  e = orcai_frontend_finalize(2, top_db, workspace, stream);
  if (e) return e;
  return orcai_clip_normalize(out, n, workspace, stream);
}

}  // extern "C"
