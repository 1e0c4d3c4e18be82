// wav_decode.hip -- the sample decode of the predict path for gfx950: the data chunk of a WAV file, as it lies in the file, -> one channel as f32
// (orcai_pcm_decode, described first) or every channel as f32 planes (orcai_pcm_decode_planar, at its kernel below).
//
// Replaces the soundfile half of librosa.load(mono=False) and the channel pick (reference src/orcAI/spectrogram.py:23-31).  Every WAV sample format
// converts to f32 exactly or with one rounding (pcm_convert.h), so the output equals orcai_amd.wavio.read_wav bit for bit.
//
// Layout (one channel).  A lane owns a RUN of 16 consecutive frames.  A run is 16 * frame_bytes bytes, so every run starts at a multiple of 16 from the base
// whatever the sample width (1, 2, 3, 4, 8 bytes) and the channel count: a run is `frame_bytes` aligned 16-byte words.  The byte offset of frame f's
// sample inside its run, f * frame_bytes + channel * bytes_per_sample, is the same for every lane, so which word a sample sits in and where is
// wave-uniform: a lane loads a word (global_load_dwordx4) only when the sample leaves the word it holds -- mono PCM16 reads 2 words per run, a wide
// frame reads the one word that holds its sample and skips the rest.  Only a 3-byte sample can straddle two words.  16 floats leave as four float4
// stores.  No byte-wise loads, no LDS.  The run that holds the last frame takes the guarded path when it is not full: it loads only words that hold
// a byte of a valid frame (inside n_frames * frame_bytes rounded up to 16) and writes its floats one by one.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "orcai_hip.h"
#include "pcm_convert.h"

namespace {

using namespace orcai_pcm;

constexpr int RUN = 16;  // frames per lane

struct RunWords {
  const uint4* base;  // the run's first word
  int have;           // index of the word in `cur` (-1: none yet)
  uint4 cur;
  __device__ __forceinline__ uint32_t dword(int byte_off) {  // the aligned dword that holds byte_off
    const int wi = byte_off >> 4;
    if (wi != have) {
      cur = base[wi];
      have = wi;
    }
    const int d = (byte_off >> 2) & 3;
    return d == 0 ? cur.x : d == 1 ? cur.y : d == 2 ? cur.z : cur.w;
  }
};

template <int FORMAT>
__device__ __forceinline__ float sample_at(RunWords& w, int off) {  // off: byte offset of the sample in the run, a multiple of its width
  uint64_t v;
  if (FORMAT == U8) {
    v = (w.dword(off) >> ((off & 3) * 8)) & 0xffu;
  } else if (FORMAT == S16) {
    v = (w.dword(off) >> ((off & 2) * 8)) & 0xffffu;
  } else if (FORMAT == S24) {
    const int sh = (off & 3) * 8;
    uint32_t x = w.dword(off) >> sh;
    if (sh > 8) x |= w.dword(off + 2) << (32 - sh);  // the sample's last byte lies in the next dword (possibly the next word)
    v = x & 0xffffffu;
  } else if (FORMAT == F64) {
    const uint32_t lo = w.dword(off);
    v = ((uint64_t)w.dword(off + 4) << 32) | lo;
  } else {
    v = w.dword(off);
  }
  return __builtin_bit_cast(float, sample_to_f32_bits<FORMAT>(v));
}

template <int FORMAT>
__global__ __launch_bounds__(256) void pcm_decode_kernel(const uint4* __restrict__ words, int64_t n_frames, int frame_bytes, int sample_off,
                                                          float* __restrict__ out) {
  const int64_t run = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t first = run * RUN;
  if (first >= n_frames) return;
  RunWords w{words + run * frame_bytes, -1, {}};  // 64-bit: run * frame_bytes words = first * frame_bytes bytes
  if (first + RUN <= n_frames) {
    float4* o = reinterpret_cast<float4*>(out + first);
#pragma unroll
    for (int q = 0; q < RUN / 4; ++q) {
      float4 r;
      r.x = sample_at<FORMAT>(w, (4 * q + 0) * frame_bytes + sample_off);
      r.y = sample_at<FORMAT>(w, (4 * q + 1) * frame_bytes + sample_off);
      r.z = sample_at<FORMAT>(w, (4 * q + 2) * frame_bytes + sample_off);
      r.w = sample_at<FORMAT>(w, (4 * q + 3) * frame_bytes + sample_off);
      o[q] = r;
    }
  } else {
    const int rest = (int)(n_frames - first);
    for (int f = 0; f < rest; ++f) out[first + f] = sample_at<FORMAT>(w, f * frame_bytes + sample_off);
  }
}

template <int FORMAT>
int launch(const void* frames, int64_t n_frames, int channels, int channel, float* out, unsigned blocks, hipStream_t stream) {
  const int bps = bytes_per_sample(FORMAT);
  hipLaunchKernelGGL(pcm_decode_kernel<FORMAT>, dim3(blocks), dim3(256), 0, stream, static_cast<const uint4*>(frames), n_frames, channels * bps, channel * bps,
                     out);
  return (int)hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------------------------------------
// Every channel from one read of the bytes (orcai_pcm_decode_planar): out f32 [channels][stride].
//
// A workgroup owns a TILE of `tile` consecutive frames (a multiple of 16, so the tile starts at a multiple of 16 bytes whatever the frame is) of at
// most LDS_BYTES.  It copies the tile's 16-byte words from the file's bytes to LDS as they lie, each word read once and the loads of a wave contiguous;
// then, plane after plane, thread t converts frames t, t + 256, ... from LDS and stores them: consecutive lanes write consecutive floats of one plane.
// The conversion is pcm_convert.h's, on the same zero-extended little-endian integer orcai_pcm_decode hands it.  Frames behind n_frames are neither
// converted nor stored (the words that hold none of their bytes are not loaded either), so the up to three pad floats of a plane stay untouched.
constexpr int LDS_BYTES = 32768;

template <int FORMAT>
__device__ __forceinline__ float lds_sample(const uint32_t* lds, int off) {  // off: byte offset of the sample in the tile, a multiple of its width
  uint64_t v;
  if (FORMAT == U8) {
    v = (lds[off >> 2] >> ((off & 3) * 8)) & 0xffu;
  } else if (FORMAT == S16) {
    v = (lds[off >> 2] >> ((off & 2) * 8)) & 0xffffu;
  } else if (FORMAT == S24) {
    const int sh = (off & 3) * 8;
    uint32_t x = lds[off >> 2] >> sh;
    if (sh > 8) x |= lds[(off >> 2) + 1] << (32 - sh);  // the sample's last byte(s) lie in the next dword: still inside the sample, so inside the tile
    v = x & 0xffffffu;
  } else if (FORMAT == F64) {
    v = ((uint64_t)lds[(off >> 2) + 1] << 32) | lds[off >> 2];
  } else {
    v = lds[off >> 2];
  }
  return __builtin_bit_cast(float, sample_to_f32_bits<FORMAT>(v));
}

template <int FORMAT>
__global__ __launch_bounds__(256) void pcm_decode_planar_kernel(const uint4* __restrict__ words, int64_t n_frames, int channels, int tile, int64_t total_words,
                                                                 int64_t stride, float* __restrict__ out) {
  __shared__ uint4 lds4[LDS_BYTES / 16];
  constexpr int bps = FORMAT == U8 ? 1 : FORMAT == S16 ? 2 : FORMAT == S24 ? 3 : FORMAT == F64 ? 8 : 4;
  const int frame_bytes = channels * bps;
  const int64_t f0 = (int64_t)blockIdx.x * tile;        // first frame of the tile
  const int tile_words = tile * frame_bytes / 16;       // <= LDS_BYTES / 16 (the launcher's choice of `tile`)
  const int64_t w0 = f0 / 16 * frame_bytes;             // f0 * frame_bytes / 16 without the 64-bit product's intermediate: f0 is a multiple of 16
  for (int w = threadIdx.x; w < tile_words && w0 + w < total_words; w += 256) lds4[w] = words[w0 + w];
  __syncthreads();
  const uint32_t* lds = reinterpret_cast<const uint32_t*>(lds4);
  const int64_t rest = n_frames - f0;
  const int frames = rest < tile ? (int)rest : tile;
  for (int c = 0; c < channels; ++c) {
    float* o = out + c * stride + f0;
    for (int f = threadIdx.x; f < frames; f += 256) o[f] = lds_sample<FORMAT>(lds, f * frame_bytes + c * bps);
  }
}

template <int FORMAT>
int launch_planar(const void* frames, int64_t n_frames, int channels, int64_t stride, float* out, hipStream_t stream) {
  const int frame_bytes = channels * bytes_per_sample(FORMAT);  // <= 512
  int tile = (LDS_BYTES / frame_bytes) & ~15;                   // >= 64 frames
  if (tile > 4096) tile = 4096;
  const int64_t blocks = (n_frames + tile - 1) / tile;
  if (blocks > 0x7fffffff) return ORCAI_E_UNSUPPORTED;
  const int64_t total_words = (n_frames * frame_bytes + 15) / 16;  // the words that hold a byte of a valid frame
  hipLaunchKernelGGL(pcm_decode_planar_kernel<FORMAT>, dim3((unsigned)blocks), dim3(256), 0, stream, static_cast<const uint4*>(frames), n_frames, channels, tile,
                     total_words, stride, out);
  return (int)hipGetLastError();
}

}  // namespace

extern "C" int orcai_pcm_decode(const void* frames, int64_t n_frames, int channels, int channel, int format, float* out, void* stream) {
  if (!frames || !out || (reinterpret_cast<uintptr_t>(frames) & 15) || (reinterpret_cast<uintptr_t>(out) & 15)) return ORCAI_E_BADARG;
  if (n_frames <= 0 || channels < 1 || channels > 64 || channel < 0 || channel >= channels || format < 0 || format >= NUM_FORMATS) return ORCAI_E_BADARG;
  const int64_t blocks = (n_frames + RUN * 256 - 1) / (RUN * 256);
  if (blocks > 0x7fffffff) return ORCAI_E_UNSUPPORTED;  // 2^43 frames: beyond any device memory
  hipStream_t s = (hipStream_t)stream;
  switch (format) {
    case U8: return launch<U8>(frames, n_frames, channels, channel, out, (unsigned)blocks, s);
    case S16: return launch<S16>(frames, n_frames, channels, channel, out, (unsigned)blocks, s);
    case S24: return launch<S24>(frames, n_frames, channels, channel, out, (unsigned)blocks, s);
    case S32: return launch<S32>(frames, n_frames, channels, channel, out, (unsigned)blocks, s);
    case F32: return launch<F32>(frames, n_frames, channels, channel, out, (unsigned)blocks, s);
    default: return launch<F64>(frames, n_frames, channels, channel, out, (unsigned)blocks, s);
  }
}

extern "C" int orcai_pcm_decode_planar(const void* frames, int64_t n_frames, int channels, int format, float* out, int64_t stride, void* stream) {
  if (!frames || !out || (reinterpret_cast<uintptr_t>(frames) & 15) || (reinterpret_cast<uintptr_t>(out) & 15)) return ORCAI_E_BADARG;
  if (n_frames <= 0 || channels < 1 || channels > 64 || format < 0 || format >= NUM_FORMATS || stride < n_frames || (stride & 3)) return ORCAI_E_BADARG;
  hipStream_t s = (hipStream_t)stream;
  switch (format) {
    case U8: return launch_planar<U8>(frames, n_frames, channels, stride, out, s);
    case S16: return launch_planar<S16>(frames, n_frames, channels, stride, out, s);
    case S24: return launch_planar<S24>(frames, n_frames, channels, stride, out, s);
    case S32: return launch_planar<S32>(frames, n_frames, channels, stride, out, s);
    case F32: return launch_planar<F32>(frames, n_frames, channels, stride, out, s);
    default: return launch_planar<F64>(frames, n_frames, channels, stride, out, s);
  }
}
