// pcm_convert.h -- one WAV sample, as the integer it is in the file, -> the bits of the f32 libsndfile's float read gives for it
// (orcai_amd/wavio.py read_wav is the host statement of the same table).  Integer arithmetic and exact float operations only, so host and device,
// and any denormal mode, give the same bits.
#pragma once

#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ORCAI_HD __host__ __device__ __forceinline__
#else
#define ORCAI_HD inline
#endif

namespace orcai_pcm {

enum Format : int { U8 = 0, S16 = 1, S24 = 2, S32 = 3, F32 = 4, F64 = 5, NUM_FORMATS = 6 };

ORCAI_HD int bytes_per_sample(int format) { return format == U8 ? 1 : format == S16 ? 2 : format == S24 ? 3 : format == F64 ? 8 : 4; }

ORCAI_HD uint32_t float_bits(float f) { return __builtin_bit_cast(uint32_t, f); }

// The f32 nearest to the f64 with bits b, ties to even: what a cast does (numpy's astype(np.float32)), spelled in integers so that f32 subnormals
// do not depend on the denormal mode.  Overflow -> +-inf; a NaN stays a NaN (quiet, leading payload bits kept).
ORCAI_HD uint32_t f64_bits_to_f32_bits(uint64_t b) {
  const uint32_t sign = (uint32_t)(b >> 63) << 31;
  const int e = (int)((b >> 52) & 0x7ff);
  uint64_t m = b & ((1ull << 52) - 1);
  if (e == 0x7ff) return sign | (m ? (0x7fc00000u | (uint32_t)(m >> 29)) : 0x7f800000u);
  const int E = e - 1023 + 127;  // the biased f32 exponent
  if (E >= 255) return sign | 0x7f800000u;
  if (E <= 0) {                  // below the smallest f32 normal: in units of 2^-149
    if (E < -24) return sign;    // under half of the smallest subnormal (f64 zeros and subnormals land here too)
    m |= 1ull << 52;
    const int shift = 30 - E;    // 30..54
    uint64_t q = m >> shift;
    const uint64_t rem = m & ((1ull << shift) - 1), half = 1ull << (shift - 1);
    if (rem > half || (rem == half && (q & 1))) ++q;
    return sign | (uint32_t)q;   // q == 2^23 is the smallest normal, in its own encoding
  }
  const uint64_t q = m >> 29;
  const uint32_t rem = (uint32_t)m & 0x1fffffffu;
  uint32_t r = ((uint32_t)E << 23) | (uint32_t)q;
  if (rem > 0x10000000u || (rem == 0x10000000u && (q & 1))) ++r;  // a carry out of the mantissa raises the exponent, up to inf
  return sign | r;
}

// v: the sample's bytes, little-endian, zero-extended (F64: all 64 bits).
template <int FORMAT>
ORCAI_HD uint32_t sample_to_f32_bits(uint64_t v) {
  if (FORMAT == U8) return float_bits((float)((int)(uint32_t)v - 128) * 0x1p-7f);                  // exact
  if (FORMAT == S16) return float_bits((float)(int16_t)(uint16_t)v * 0x1p-15f);                    // exact
  if (FORMAT == S24) return float_bits((float)((int32_t)((uint32_t)v << 8) >> 8) * 0x1p-23f);      // 24 bits: exact
  if (FORMAT == S32) return float_bits((float)(int32_t)(uint32_t)v * 0x1p-31f);                    // the cast rounds (nearest even), the scale is exact
  if (FORMAT == F32) return (uint32_t)v;
  return f64_bits_to_f32_bits(v);
}

}  // namespace orcai_pcm
