/*
 * orcai_hip.h -- C ABI of liborcai_hip.so, the MI355X (gfx950) implementation of
 * orcAI's spectrogram -> label hot path.
 *
 * The reference (ethz-tb/orcAI v1.0.3) is pure Python and has no FFI layer; its
 * hot-path arithmetic is delegated to librosa/numpy/Keras calls.  Each entry
 * point below names the reference call site (file:line under
 * /root/reference/src/orcAI/) whose arithmetic it replaces.  INTEGRATION.md
 * shows the ctypes binding a maintainer of the reference would add.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless its name ends in _host;
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream);
 *   - the caller owns and allocates every buffer (no ownership transfer);
 *   - the return value is a hipError_t as int (0 = hipSuccess), or a negative
 *     ORCAI_E_* code for argument errors detected on the host before launch;
 *   - nothing here allocates, frees or synchronises, so every call may be
 *     captured into a hipGraph.  The only exceptions are the *_host readback
 *     helpers, which synchronise the stream and say so, and the setup call
 *     orcai_frontend_workspace_bytes(), which uploads the front end's constant
 *     tables once (synchronously) before any capturable call can be made.
 */
#ifndef ORCAI_HIP_H
#define ORCAI_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ORCAI_E_BADARG (-1)      /* null pointer, non-positive size, misaligned buffer */
#define ORCAI_E_UNSUPPORTED (-2) /* parameter combination the HIP path does not implement */

/* library identification: "orcai_hip <version> gfx950" */
const char* orcai_version(void);

/* ------------------------------------------------------------------------------------------
 * Front end (spectrogram.py:15-87)
 * ------------------------------------------------------------------------------------------ */

/* Bytes of device workspace the front-end calls need (histograms + selection state).
 * The workspace must be 256-byte aligned.  SETUP CALL: also uploads the Hann window and the FFT twiddle tables to device
 * constants (once per process, synchronous), so that every later front-end call only enqueues work on `stream`. */
size_t orcai_frontend_workspace_bytes(void);

/* Zero the workspace (histograms, running max, selection state).  Must precede each
 * recording's orcai_stft_db / orcai_hist_level1. */
int orcai_frontend_reset(void* workspace, void* stream);

/* Sample decode: the data chunk of a RIFF/WAVE file as it lies in the file (interleaved little-endian frames), on the device -> the samples of ONE
 * channel as f32, with libsndfile's float scaling (the soundfile half of librosa.load(mono=False) + the channel pick, spectrogram.py:23-31).
 *   format     0 U8   (x - 128) / 128          3 S32  x * 2^-31, rounded once (round to nearest even)
 *              1 S16  x * 2^-15                4 F32  the bits, untouched (NaN payloads and signed zeros included)
 *              2 S24  x * 2^-23 (sign-extended) 5 F64  one round-to-nearest-even cast: overflow -> +-inf, f32 subnormals kept
 *   frames     n_frames frames of `channels` samples; 16-byte aligned, and READABLE up to n_frames * frame_bytes ROUNDED UP TO 16
 *              (frame_bytes = channels * bytes per sample): every load is an aligned 16-byte word, the last one may reach past the last
 *              frame (those bytes are read and ignored; they need not be initialised)
 *   channels   1..64;  channel  0-based, in [0, channels)
 *   out        f32[n_frames], 16-byte aligned; exactly n_frames floats are written
 * Every conversion is exact or rounds once, so out equals the host decode (orcai_amd.wavio.read_wav) bit for bit.  One lane decodes 16 consecutive
 * frames: their bytes start at a multiple of 16 for every format and channel count, the stores are 16 bytes wide, no LDS.  Byte offsets are 64-bit.
 * ORCAI_E_BADARG: null or misaligned pointer, n_frames <= 0, channels outside 1..64, channel outside [0, channels), unknown format. */
int orcai_pcm_decode(const void* frames, int64_t n_frames, int channels, int channel, int format, float* out, void* stream);

/* The same decode for EVERY channel from one read of the bytes: frames, n_frames, channels, format as orcai_pcm_decode.
 *   out        f32[channels][stride], 16-byte aligned: plane c holds the n_frames samples of channel c, bit for bit what
 *              orcai_pcm_decode(..., channel = c, ...) writes; the stride - n_frames floats behind them are not written
 *   stride     floats between planes: >= n_frames and a multiple of 4, so that every plane starts 16-byte aligned (roundup(n_frames, 4))
 * A workgroup copies a tile of frames (a multiple of 16 frames, at most 32 KiB) to LDS with aligned 16-byte loads, every word of the file once, and
 * converts it plane after plane with consecutive lanes storing consecutive floats of a plane.
 * ORCAI_E_BADARG: null or misaligned pointer, n_frames <= 0, channels outside 1..64, unknown format, stride < n_frames or not a multiple of 4. */
int orcai_pcm_decode_planar(const void* frames, int64_t n_frames, int channels, int format, float* out, int64_t stride, void* stream);

/* Rational polyphase resampler (the resampling half of librosa.load(sr=...), spectrogram.py:23-27; libsoxr itself
 * is absent, so this stage cannot be bit-compared: parity unpinned).
 *   out[n] = sum_j x[floor(n*M/L) - ntaps/2 + 1 + j] * table[(n*M) mod L][j]; table f32[L][ntaps], ntaps % 4 == 0. */
int orcai_resample_polyphase(const float* x, int64_t n_in, float* out, int64_t n_out, int L, int M, const float* table, int ntaps, void* stream);

/* The adjoint of orcai_resample_polyphase with the same table: the gradient w.r.t. the audio at its native rate (the resampler is linear,
 * so this is its whole backward; the reference has no counterpart, it never differentiates librosa.load).
 *   dx[k] = sum_n dout[n] * table[(n*M) mod L][k - (floor(n*M/L) - ntaps/2 + 1)]
 * over the outputs n in [0, n_out) whose window holds k: n in [ceil((k - ntaps/2)*L/M), ceil((k + ntaps/2)*L/M)).
 *   dout f32[n_out], dx f32[n_in]: EVERY element of dx is written (the caller does not zero it); n_out is the forward's output length.
 * Gather form, one owner per dx[k] adding in ascending n, no float atomics: two launches give the same bits.  Every (L, M, ntaps) the forward
 * accepts runs (nothing is staged in LDS, so no table is too large); ORCAI_E_BADARG for what the forward rejects (null pointer, non-positive
 * size, ntaps % 4 != 0).  Index arithmetic is 64-bit. */
int orcai_resample_polyphase_bwd(const float* dout, int64_t n_out, float* dx, int64_t n_in, int L, int M, const float* table, int ntaps, void* stream);

/* librosa.stft(n_fft=512, hop_length=hop, window="hann", center=True, pad_mode="constant")
 * followed by the first half of amplitude_to_db (spectrogram.py:34-39, :51-53):
 *   out_db[t*k_crop + k] = 10*log10(max(|X[k,t]|^2, 1e-10))          k in [0, k_crop)
 * (the reference level, max-80 floor and normalisation are applied by orcai_clip_normalize).
 * Also accumulates into the workspace: max |X|^2 over ALL 257 bins and all frames, and the
 * level-1 selection histogram of the values written.
 *   pcm        f32[n_samples], mono, already at the target sampling rate
 *   n_frames   must equal 1 + (n_samples - (n_fft & 1)) / hop  (librosa's centred frame count; 1 + n_samples / hop for even n_fft)
 *   k_crop     1..1 + n_fft/2 leading rFFT bins to keep (171 for orcai-V1: first bin with f >= 16 kHz)
 *   out_db     f32[n_frames * k_crop], layout [frame][bin]  (the transposed layout
 *              preprocess_spectrogram returns, spectrogram.py:86)
 * n_fft = 512 (every shipped parameter file) runs the tuned kernel; any other power of two from 32 to 4096 a plain
 * one-workgroup-per-frame radix-2 kernel, every other size from 2 to 4096 (odd ones too) a direct float64 transform, O(n_fft^2)
 * per frame -- both followed by a separate level-1 histogram pass (same outputs); n_fft > 4096 is ORCAI_E_UNSUPPORTED.
 * With n_fft != 512 "ALL 257 bins" reads "all 1 + n_fft/2 bins". */
int orcai_stft_db(const float* pcm, int64_t n_samples, int n_fft, int hop, int64_t n_frames, int k_crop,
                  float* out_db, void* workspace, void* stream);

/* Level-1 selection histogram of an arbitrary f32 array (used when the dB array comes from the
 * caller, i.e. the drop-in preprocess_spectrogram(spectrogram, ...) entry, spectrogram.py:58). */
int orcai_stft_occupancy(void);     /* workgroups of the STFT kernel per compute unit as the runtime computes it */
int orcai_hist_level1(const float* x, int64_t n, void* workspace, void* stream);

/* Exact order statistics: the rank_lo-th and rank_hi-th smallest (0-based) of x[0..n), i.e. what
 * np.percentile(x, q, method="nearest") returns for the indices computed on the host
 * (spectrogram.py:70-75).  Requires the level-1 histogram of exactly these n values to be in
 * the workspace.  Results stay in the workspace (see orcai_frontend_stats_host). */
int orcai_quantile_select(const float* x, int64_t n, int64_t rank_lo, int64_t rank_hi, void* workspace, void* stream);

/* The same exact order statistics by a radix select on the monotone key, for values that are not dB: three passes over x (key bits [31:21],
 * [20:10], [9:0]), each a histogram in LDS whose non-zero bins are added to the workspace, and a one-workgroup scan after each.  The cost is
 * three reads of x wherever the values lie; orcai_quantile_select's depends on its level-1 map, cut for 0.125 <= |x| < 128.  The order is the
 * key's: -0.0 before +0.0, +-inf and subnormals ordinary values.  Needs NO orcai_hist_level1 and no orcai_frontend_reset before it: it clears
 * what it uses (the start of the level-2 histogram area) and leaves the level-1 histogram and pmax alone.  On return the workspace holds exactly
 * what orcai_quantile_select leaves, so orcai_frontend_finalize, orcai_clip_normalize and the statistics calls run unchanged behind it.
 * Asynchronous on stream, no allocation, hipGraph-capturable.  ORCAI_E_BADARG, before anything is launched: null x or workspace, n <= 0 or
 * n >= 2^32 (the bins are u32), a rank outside [0, n), x not 16-byte aligned.  rank_lo > rank_hi is allowed.  What orcai_make_pcen_spectrogram
 * selects with. */
int orcai_quantile_select_radix(const float* x, int64_t n, int64_t rank_lo, int64_t rank_hi, void* workspace, void* stream);

/* Turn the selected raw order statistics into clip bounds.
 *   use_ref = 1: values are un-referenced dB from orcai_stft_db; ref_db = 10*log10(max(pmax,1e-10)),
 *                bound = max(selected - ref_db, -top_db)                    (spectrogram.py:51-53)
 *   use_ref = 2: as 1 with selected - ref_db rounded ONCE in f32 (use_ref = 1 fuses it into the multiplication that forms ref_db), so that the
 *                bound is bit for bit the value orcai_clip_normalize gives the selected element: what orcai_make_mel_spectrogram uses
 *   use_ref = 0: values already are final dB (drop-in preprocess entry): bound = selected. */
int orcai_frontend_finalize(int use_ref, float top_db, void* workspace, void* stream);

/* In place: v = max(x - ref_db, -top_db) (when use_ref), clip to [p_lo, p_hi], (v - p_lo)/(p_hi - p_lo)
 * (spectrogram.py:78-83).  Bounds are read from the workspace on the device. */
int orcai_clip_normalize(float* x, int64_t n, const void* workspace, void* stream);

/* In place: x = max(x - ref_db, -top_db): the dB array calculate_spectrogram returns
 * (spectrogram.py:51-53). */
int orcai_db_reference(float* x, int64_t n, const void* workspace, void* stream);

/* [F, T] -> [T, f_hi - f_lo] crop + transpose (spectrogram.py:68, :86) for the drop-in
 * preprocess_spectrogram entry whose input is the reference's [freq, time] layout. */
int orcai_crop_transpose(const float* in_ft, int64_t n_freq, int64_t n_frames, int f_lo, int f_hi, float* out_tf, void* stream);

/* Synchronises `stream` and copies {pmax, ref_db, p_lo, p_hi, sel_lo_raw, sel_hi_raw} to the host. */
int orcai_frontend_stats_host(const void* workspace, float stats_host[6], void* stream);

/* One call = reset + stft_db + select + finalize + clip_normalize: the whole of make_spectrogram
 * (spectrogram.py:90-147) after file decode.  rank_lo/rank_hi as for orcai_quantile_select with
 * n = n_frames * k_crop. */
int orcai_make_spectrogram(const float* pcm, int64_t n_samples, int n_fft, int hop, int64_t n_frames, int k_crop,
                           int64_t rank_lo, int64_t rank_hi, float top_db, float* out, void* workspace, void* stream);

/* Mel front end (no counterpart in the reference; semantics are librosa's documented defaults, parity unpinned):
 *   S[k,t] = |stft(pcm, n_fft, hop, hann, center=True, zero padding)|^2,   M[m,t] = sum_k W[m][k] S[k,t],
 *   out_db[t*n_mels + m] = 10*log10(max(M[m,t], 1e-10))
 * fused: the linear spectrum never goes to memory.  W is a SPARSE band table: band m covers the FFT bins [band_lo[m], band_hi[m]) with the f32
 * weights weights[band_off[m] .. band_off[m] + band_hi[m] - band_lo[m]) (orcai_amd.mel.band_table builds it from librosa.filters.mel's triangles).
 *   band_lo, band_hi, band_off   int[n_mels] in HOST memory: read and checked during the call, handed to the kernels by value (nothing to keep alive)
 *   weights    f32[n_weights] on the device, 16-byte aligned, 1 <= n_weights <= 65535
 *   n_mels     8..256;  n_frames = 1 + n_samples / hop
 *   out_db     f32[n_frames * n_mels], layout [frame][band], 16-byte aligned
 * The workspace is left exactly as orcai_stft_db leaves it -- the level-1 histogram of the values written and, in the slot of max |X|^2, the maximum
 * of M as a POWER (orcai_frontend_finalize(1, top_db) turns it into ref_db = 10*log10(max(max M, 1e-10)): power_to_db(ref=np.max, amin=1e-10)) --
 * so orcai_quantile_select, orcai_frontend_finalize(1, .) and orcai_clip_normalize run unchanged behind it.  A band sum adds its bins in a fixed
 * order and there are no float atomics on values: two calls give the same bytes.
 * n_fft = 512: a mel epilogue of the tuned STFT kernel (powers, band table and weights in LDS; same three launch routes); the other powers of two
 * from 128 to 4096 (and 512 with more than 1024 weights): one workgroup per frame + a separate level-1 histogram pass.
 * ORCAI_E_BADARG (nothing launched, nothing written): null or misaligned pointer, non-positive size, n_mels outside 8..256, n_weights outside
 * 1..65535, n_frames other than 1 + n_samples / hop, a band with band_lo < 0, band_hi < band_lo, band_hi > 1 + n_fft/2 or weights outside
 * [0, n_weights).  ORCAI_E_UNSUPPORTED: n_fft that is no power of two from 128 to 4096. */
int orcai_stft_mel_db(const float* pcm, int64_t n_samples, int n_fft, int hop, int64_t n_frames, int n_mels, const int* band_lo, const int* band_hi,
                      const int* band_off, const float* weights, int n_weights, float* out_db, void* workspace, void* stream);
int orcai_stft_mel_occupancy(void); /* workgroups of the 512-point mel kernel per compute unit as the runtime computes it */

/* One call = reset + stft_mel_db + select + finalize(2, top_db) + clip_normalize: orcai_make_spectrogram for the mel route.  rank_lo / rank_hi as for
 * orcai_quantile_select with n = n_frames * n_mels; out f32[n_frames * n_mels] in [0, 1]. */
int orcai_make_mel_spectrogram(const float* pcm, int64_t n_samples, int n_fft, int hop, int64_t n_frames, int n_mels, const int* band_lo,
                               const int* band_hi, const int* band_off, const float* weights, int n_weights, int64_t rank_lo, int64_t rank_hi,
                               float top_db, float* out, void* workspace, void* stream);

/* The statistics of the front-end run that just finished on `stream`, {pmax, ref_db, p_lo, p_hi, sel_lo_raw, sel_hi_raw} as
 * orcai_frontend_stats_host returns them, copied by a one-thread launch into the caller's device buffer f32[6]: no host
 * synchronisation (capturable).  The workspace is overwritten by the next recording, the copy is the caller's to keep -- it is what
 * orcai_spectrogram_bwd reads, so the backward never reruns the selection. */
int orcai_frontend_stats_dev(const void* workspace, float* stats_dev, void* stream);

/* Gradient of orcai_make_spectrogram w.r.t. the audio (the reference has no counterpart: spectrogram.py:90-147 is numpy / librosa and is
 * never differentiated).  With out = (clip(v, p_lo, p_hi) - p_lo) / (p_hi - p_lo), v = max(db - ref_db, -top_db),
 * db = 10 log10(max(P, 1e-10)), P = Re^2 + Im^2 of the centred, zero-padded, Hann-windowed STFT, and g = dL/dout:
 *   g_db    = g / (p_hi - p_lo)  where P > 1e-10, db - ref_db > -top_db and p_lo < v < p_hi (all strict); 0 otherwise
 *   dP      = g_db * 10 / (ln 10 * P);  dRe[k] = 2 Re[k] dP, dIm[k] = 2 Im[k] dP for k < k_crop, 0 for the bins above
 *   dframe_t[n] = w[n] * sum_k (dRe[k] cos(2 pi k n / N) - dIm[k] sin(2 pi k n / N)),  N = n_fft
 *   dpcm[s] = sum over the frames t that cover s of dframe_t[s - t * hop + N/2]   (positions in the zero padding receive nothing)
 * The three global statistics ref_db, p_lo, p_hi are HELD CONSTANT: mathematically they depend on the data, but only through single STFT
 * bins (the maximum-power bin, the two order-statistic bins), and that dependence is ill-defined under ties.
 *   pcm, n_samples, n_fft, hop, n_frames, k_crop   as for orcai_stft_db (the forward's arguments; Re / Im are recomputed, the forward stores dB only)
 *   gout       f32[n_frames * k_crop], layout [frame][bin]
 *   stats_dev  f32[6] from orcai_frontend_stats_dev after the forward of the same pcm (ref_db, p_lo, p_hi are read on the device)
 *   dpcm       f32[n_samples]: every element is WRITTEN (nothing accumulated, no need to clear it); summed without float atomics in a
 *              fixed order, so two launches give identical bits
 * n_fft: powers of two from 32 to 4096 (512 included); every other size is ORCAI_E_UNSUPPORTED (the forward keeps running them).  hop is
 * arbitrary (it need not divide n_fft).  ORCAI_E_BADARG: null pointer, non-positive size, k_crop outside 1..1 + n_fft/2, n_frames other than
 * librosa's 1 + n_samples / hop. */
int orcai_spectrogram_bwd(const float* pcm, int64_t n_samples, int n_fft, int hop, int64_t n_frames, int k_crop, const float* gout,
                          const float* stats_dev, float top_db, float* dpcm, void* stream);

/* Gradient of orcai_make_mel_spectrogram w.r.t. the audio.  Notation as above and at orcai_stft_mel_db.  With Re, Im, P = Re^2 + Im^2 the centred,
 * zero-padded, periodic-Hann STFT, M[m] = sum_k W[m][k] P[k], Ldb = 10 log10(max(M, 1e-10)), v = max(Ldb - ref_db, -top_db),
 * out = (clip(v, p_lo, p_hi) - p_lo) / (p_hi - p_lo) and g = dL/dout, f32[n_frames][n_mels]:
 *   g_L[m]  = g[m] / (p_hi - p_lo)  where M[m] > 1e-10, Ldb - ref_db > -top_db and p_lo < v < p_hi (all strict); 0 otherwise
 *   dM[m]   = g_L[m] * 10 / (ln 10 * M[m])
 *   dP[k]   = sum_m W[m][k] dM[m]                      (a bin lies under at most two triangles)
 *   dRe[k]  = 2 Re[k] dP[k],  dIm[k] = 2 Im[k] dP[k]
 *   dframe_t[n] = w[n] * sum_k (dRe[k] cos(2 pi k n / N) - dIm[k] sin(2 pi k n / N)),  N = n_fft
 *   dpcm[s] = sum over the frames t that cover s of dframe_t[s - t * hop + N/2]
 * ref_db, p_lo and p_hi are HELD CONSTANT, as in orcai_spectrogram_bwd and for the same reason; they are read on the device from stats_dev.  M, Re
 * and Im are recomputed from pcm (the forward stores nothing but out).  The filterbank weights receive no gradient.
 *   pcm, n_samples, n_fft, hop, n_frames, n_mels, band_lo, band_hi, band_off, weights, n_weights   exactly as for orcai_stft_mel_db: the band arrays
 *              in HOST memory (read and checked during the call, handed to the kernel by value), weights on the device
 *   gout       f32[n_frames * n_mels], layout [frame][band]
 *   stats_dev  f32[6] from orcai_frontend_stats_dev after the forward of the same pcm
 *   dpcm       f32[n_samples]: every element is WRITTEN, nothing is accumulated in memory; no float atomics -- a band sum adds its bins in a fixed
 *              order and dP[k] is gathered per bin, even band first, then the odd one -- so two launches give identical bytes
 * The gather keeps ONE even-numbered and ONE odd-numbered band per bin (built per workgroup in LDS from the band arrays; no extra pointer): two
 * non-empty bands of equal parity must not share a bin, i.e. band_hi[m] <= band_lo[m + 2] -- what every table of orcai_amd.mel.band_table
 * satisfies.  n_fft: the powers of two from 128 to 4096, as the mel forward; hop is arbitrary.  At n_fft = 4096 (and 2048 with more than 202 bands) the launch asks
 * for more than 64 KiB of LDS: the first such call per device must come outside a stream capture.
 * ORCAI_E_BADARG (nothing launched, nothing written): null pointer, pcm or weights not 16-byte aligned, non-positive size, n_mels outside 8..256,
 * n_weights outside 1..65535, n_frames other than 1 + n_samples / hop, a band with band_lo < 0, band_hi < band_lo, band_hi > 1 + n_fft/2 or weights
 * outside [0, n_weights).  ORCAI_E_UNSUPPORTED (likewise): n_fft that is no power of two from 128 to 4096; two bands of equal parity that overlap. */
int orcai_mel_spectrogram_bwd(const float* pcm, int64_t n_samples, int n_fft, int hop, int64_t n_frames, int n_mels, const int* band_lo,
                              const int* band_hi, const int* band_off, const float* weights, int n_weights, const float* gout,
                              const float* stats_dev, float top_db, float* dpcm, void* stream);
int orcai_mel_spectrogram_bwd_occupancy(int n_fft, int n_mels); /* workgroups of that launch per compute unit as the runtime computes it; -1 if refused */

/* PCEN front end (spectrogram parameter "pcen"; no counterpart in the reference; semantics are librosa.pcen's, parity unpinned; the float64
 * specification is orcai_amd.pcen.pcen_ref).
 *
 * Linear energies out of the STFT, the input of orcai_pcen: orcai_stft_db / orcai_stft_mel_db with a linear epilogue, and neither running maximum
 * nor histogram (hence no workspace):
 *   orcai_stft_energy       out[t*k_crop + k] = |X[k,t]|, k < k_crop: the magnitude the dB step takes the logarithm of
 *   orcai_stft_mel_energy   out[t*n_mels + m] = M[m,t] = sum_k W[m][k] |X[k,t]|^2: the band power, summed in orcai_stft_mel_db's order
 * Arguments as for orcai_stft_db / orcai_stft_mel_db.  n_fft: the powers of two from 32 (mel: 128) to 4096 -- 512 runs the tuned kernel, the
 * others the one-workgroup-per-frame kernel; every other size is ORCAI_E_UNSUPPORTED (the direct transform has no energy epilogue).
 * ORCAI_E_BADARG as for the dB calls. */
int orcai_stft_energy(const float* pcm, int64_t n_samples, int n_fft, int hop, int64_t n_frames, int k_crop, float* out, void* stream);
int orcai_stft_mel_energy(const float* pcm, int64_t n_samples, int n_fft, int hop, int64_t n_frames, int n_mels, const int* band_lo, const int* band_hi,
                          const int* band_off, const float* weights, int n_weights, float* out, void* stream);

/* Frames per chunk of orcai_pcen's scan.  Part of the ABI: the f32 result depends on where the chunks end. */
#define ORCAI_PCEN_CHUNK 256

/* Per-channel energy normalisation of x = f32[n_frames][k] non-negative energies, IN PLACE:
 *   S = scale x,  M[0] = S[0],  M[t] = a M[t-1] + b S[t],  x <- (S (eps + M)^-gain + bias)^power - bias^power
 * The recursion along time runs as a chunked scan, ORCAI_PCEN_CHUNK frames per chunk, in three launches: per (chunk, column) the chain
 * m = fma(a, m, b S) over the chunk from m = 0 (chunk 0: from M[0] = S[0]); per column the carries in chunk order, C[0] = P[0],
 * C[j] = fma(a^L_j, C[j-1], P[j]) with L_j the chunk's own length and a^L_j computed in float64 on the host; per (chunk, column) the chain again
 * from C[j-1], the result written over the energy just read.  The powers are exp2(p log2 .) on the hardware's exp2 / log2; bias^power is formed on
 * the device by the same instructions, so x = 0 in a channel whose M is finite gives exactly 0.  No float atomics and a fixed order everywhere: the
 * same input gives the same bytes on every launch.
 *   a, b       the smoother, 0 <= a < 1, 0 < b <= 1 (orcai_amd.pcen.smoother: b from the time constant in frames, a = 1 - b)
 *   scale > 0, 0 <= gain <= 1, bias >= 0, 0 < power <= 1, eps > 0
 *   scratch    orcai_pcen_scratch_bytes(n_frames, k) bytes on the device, 4-byte aligned: f32[ceil(n_frames / 256)][k] partials, then as many carries
 * ORCAI_E_BADARG (nothing launched): null or misaligned pointer, non-positive size, a parameter outside its range. */
size_t orcai_pcen_scratch_bytes(int64_t n_frames, int k);
int orcai_pcen(float* x, int64_t n_frames, int k, float a, float b, float scale, float gain, float bias, float power, float eps, void* scratch,
               void* stream);
/* orcai_pcen with HIP events around its three launches: stage_ms = {partials, carries, apply} in milliseconds.  A measuring tool (tools/time_pcen.py):
 * it SYNCHRONISES on the last event, so it is not capturable. */
int orcai_pcen_stage_ms(float* x, int64_t n_frames, int k, float a, float b, float scale, float gain, float bias, float power, float eps, void* scratch,
                        void* stream, float stage_ms[3]);

/* One call = reset + stft_energy (band_lo null) or stft_mel_energy + pcen + orcai_quantile_select_radix + finalize(0) + clip_normalize:
 * orcai_make_spectrogram for a spectrogram parameter with "pcen" set (the same bytes as with hist_level1 + orcai_quantile_select: both are exact).  k is k_crop or n_mels; the band arguments as for orcai_stft_mel_db, all ignored when band_lo is null.
 * The percentile clip runs on the PCEN values: no dB reference, no top_db.  rank_lo / rank_hi as for orcai_quantile_select with n = n_frames * k;
 * out f32[n_frames * k] in [0, 1].  No host synchronisation; orcai_frontend_stats_dev behind it reports p_lo / p_hi as PCEN values (pmax and ref_db 0). */
int orcai_make_pcen_spectrogram(const float* pcm, int64_t n_samples, int n_fft, int hop, int64_t n_frames, int k, const int* band_lo, const int* band_hi,
                                const int* band_off, const float* weights, int n_weights, float a, float b, float scale, float gain, float bias,
                                float power, float eps, int64_t rank_lo, int64_t rank_hi, float* out, void* scratch, void* workspace, void* stream);

/* Gradient of the PCEN front end w.r.t. the audio.  Notation as at orcai_pcen and orcai_spectrogram_bwd.  Forward: E the magnitude |X[k,t]| (linear
 * route) or the band power (mel route), S = scale E, M the smoother, r = (eps + M)^-gain, u = S r + bias, y = u^power - bias^power,
 * out = (clip(y, p_lo, p_hi) - p_lo) / (p_hi - p_lo).  With g = dL/dout, and p_lo / p_hi read on the device from stats_dev[2..3] and HELD CONSTANT:
 *   g_y[t]  = g[t] / (p_hi - p_lo)  where p_lo < y[t] < p_hi (both strict); exactly 0 otherwise (a select, never 0 * inf)
 *   h[t]    = g_y[t] power u[t]^(power - 1)
 *   d[t]    = h[t] r[t]                                    the direct path into S[t]
 *   q[t]    = -gain h[t] S[t] r[t] / (eps + M[t])          dL/dM[t], local part
 *   lam[T-1] = q[T-1];  lam[t] = q[t] + a lam[t+1]         the smoother's adjoint: the recursion BACKWARD in time
 *   dE[t]   = scale (d[t] + b lam[t]) for t >= 1;  dE[0] = scale (d[0] + lam[0])      (M[0] = S[0]: coefficient 1, not b)
 * A clipped or silent element has d = q = 0 and still receives b lam from later frames.  The PCEN parameters, the filterbank and the two statistics get
 * no gradient; there is no second derivative and no f16 path.
 *
 * orcai_pcen_bwd is that map g -> dE alone: E f32[n_frames][k] (const, not overwritten), gout and dE likewise; EVERY element of dE is written.  y and M
 * are recomputed by the forward's instructions at the forward's chunk boundaries (ORCAI_PCEN_CHUNK), so the gate agrees bit for bit with what
 * orcai_clip_normalize clipped.  Six launches: the forward's partials and carries; the forward chain again writing d and q; per (chunk, column) the
 * reverse partial R[j] = the chain lam = fma(a, lam, q[t]) from 0, last frame of the chunk to its first; per column D[last] = R[last],
 * D[j] = fma(a^256, D[j+1], R[j]) in descending chunk order (a^256 in float64 on the host); the reverse chain again from D[j+1] writing dE.  One fixed
 * order everywhere and no float atomics: the same input gives the same bytes on every launch.
 *   scratch    orcai_pcen_bwd_scratch_bytes(n_frames, k) bytes on the device, 4-byte aligned: four f32[ceil(n_frames / 256)][k] (partials, carries and
 *              their reverse counterparts), then the planes d and q, f32[n_frames][k] each
 * ORCAI_E_BADARG (nothing launched, dE untouched): as orcai_pcen, and a null or misaligned E, gout, stats_dev or dE. */
size_t orcai_pcen_bwd_scratch_bytes(int64_t n_frames, int k);
int orcai_pcen_bwd(const float* E, const float* gout, const float* stats_dev, int64_t n_frames, int k, float a, float b, float scale, float gain, float bias,
                   float power, float eps, float* dE, void* scratch, void* stream);
/* orcai_pcen_bwd with HIP events around its six launches: stage_ms = {partials, carries, local, reverse partials, reverse carries, apply}.  A measuring
 * tool (tools/time_pcen_grad.py): it SYNCHRONISES on the last event, so it is not capturable. */
int orcai_pcen_bwd_stage_ms(const float* E, const float* gout, const float* stats_dev, int64_t n_frames, int k, float a, float b, float scale, float gain,
                            float bias, float power, float eps, float* dE, void* scratch, void* stream, float stage_ms[6]);

/* From the gradient w.r.t. the energies to the samples: orcai_spectrogram_bwd / orcai_mel_spectrogram_bwd with a linear epilogue in place of the dB
 * gates and the 10 / (ln 10 P) factor -- the same kernels' text, two more instantiations; neither stats_dev nor top_db.
 *   orcai_stft_energy_bwd      gE = dL/d|X[k,t]| f32[n_frames][k_crop]: dRe[k] = gE[k] Re[k] / |X[k]|, dIm[k] = gE[k] Im[k] / |X[k]|, both exactly 0
 *                              where |X[k]| = 0 (a select) and for the bins from k_crop on
 *   orcai_stft_mel_energy_bwd  gE = dL/dM[m,t] f32[n_frames][n_mels]: dP[k] = sum_m W[m][k] gE[m], gathered even band first, then the odd one;
 *                              dRe = 2 Re dP, dIm = 2 Im dP
 * then the inverse transform and the frame-ordered overlap-add of orcai_spectrogram_bwd: every element of dpcm is written, no float atomics, two
 * launches give identical bytes.  Sizes (32, mel 128, to 4096), alignment, refusals and the LDS opt-in as for the two dB backwards. */
int orcai_stft_energy_bwd(const float* pcm, int64_t n_samples, int n_fft, int hop, int64_t n_frames, int k_crop, const float* gE, float* dpcm, void* stream);
int orcai_stft_mel_energy_bwd(const float* pcm, int64_t n_samples, int n_fft, int hop, int64_t n_frames, int n_mels, const int* band_lo, const int* band_hi,
                              const int* band_off, const float* weights, int n_weights, const float* gE, float* dpcm, void* stream);

/* One call = stft_energy (band_lo null) or stft_mel_energy into scratch (the forward keeps nothing but out) + pcen_bwd + the matching energy backward:
 * the gradient of orcai_make_pcen_spectrogram w.r.t. pcm.  Arguments as there; gout f32[n_frames * k]; stats_dev from orcai_frontend_stats_dev after
 * the forward of the same pcm; dpcm f32[n_samples], every element written.  scratch: orcai_pcen_spectrogram_bwd_scratch_bytes(n_frames, k) bytes,
 * 16-byte aligned (E and dE, f32[n_frames * k] each rounded up to 16 bytes, then orcai_pcen_bwd's).  No host synchronisation.  Refusals are those of
 * the steps; the transform's arguments are refused by the first step, before anything is launched. */
size_t orcai_pcen_spectrogram_bwd_scratch_bytes(int64_t n_frames, int k);
int orcai_pcen_spectrogram_bwd(const float* pcm, int64_t n_samples, int n_fft, int hop, int64_t n_frames, int k, const int* band_lo, const int* band_hi,
                               const int* band_off, const float* weights, int n_weights, float a, float b, float scale, float gain, float bias, float power,
                               float eps, const float* gout, const float* stats_dev, float* dpcm, void* scratch, void* stream);

/* Segmented select: out[c] = the rank-th smallest (0-based) of column c of x = f32[rows][cols] (row-major, as the front end writes [frame][bin]), for
 * every column in one call.  Exact for any f32 data without NaN.  The order is the monotone key's of orcai_quantile_select_radix (-0.0 before +0.0,
 * +-inf and subnormals ordinary values) and the value returned is the selected key's float: bit for bit what orcai_quantile_select_radix returns on
 * that column alone.  Four passes over x, one 8-bit digit of the key each, most significant first: a workgroup owns 32 adjacent columns (a row piece
 * is 128 contiguous bytes; with fewer than 17 columns the lanes of a row shrink to the next power of two) and strides over row tiles with a capped
 * grid; an element counts into its column's LDS histogram (u32[32][257], 32.1 KiB) only when its higher digits equal ITS OWN COLUMN's prefix; the
 * non-zero bins are then added to the global u32[cols][256] with integer atomics, and one wave per column turns its histogram into (digit, remaining
 * rank) and clears it.  Four reads of x wherever the values lie, no global atomic per element, no float atomics: two launches give the same bytes.
 *   scratch    orcai_column_select_scratch_bytes(cols) bytes on the device, 4-byte aligned: the histograms, the per-column state {prefix, rank} and
 *              f32[cols] that this call leaves alone (orcai_make_denoised_spectrogram's profile when the caller passes none).  The call clears what
 *              it accumulates into and writes its state whole: a stale or never-cleared scratch gives the same result, no reset call in front.
 *   out        f32[cols]; nothing else is written, and the front end's workspace is not touched.
 * Asynchronous on stream, no allocation, no host synchronisation, hipGraph-capturable; static LDS below 64 KiB, so no opt-in.  ORCAI_E_BADARG, before
 * anything is launched: null x, out or scratch; rows <= 0 or rows >= 2^32 (the bins are u32); cols outside 1..4096; rank outside [0, rows); a pointer
 * that is not 4-byte aligned.  cols need not be a multiple of anything and rows need not be 16-byte multiples (every load is one dword).
 * orcai_column_select_scratch_bytes is 0 for cols outside 1..4096. */
size_t orcai_column_select_scratch_bytes(int cols);
int orcai_column_select(const float* x, int64_t rows, int cols, int64_t rank, float* out, void* scratch, void* stream);

/* In place: x[t][c] = x[t][c] - m[c] in f32 (one rounding), x = f32[rows][cols], m = f32[cols].  One streaming pass, every element read and written
 * once: 16-byte accesses from the first 16-byte boundary of x on, scalar accesses in front of it and behind the last whole 16 bytes.
 * ORCAI_E_BADARG: null or not 4-byte aligned x or m, rows and cols as for orcai_column_select. */
int orcai_subtract_columns(float* x, int64_t rows, int cols, const float* m, void* stream);

/* The dB front end with a per-channel noise floor removed (the spectrogram parameter "denoise"): every column of the referenced dB spectrogram minus its
 * own order statistic over the recording (rank_col; the median for quantile 0.5), then the global percentile clip and the normalisation.  One call =
 *   orcai_frontend_reset, orcai_stft_db (band_lo null; k = k_crop) or orcai_stft_mel_db (k = n_mels), orcai_frontend_finalize(1, top_db),
 *   orcai_db_reference                       -> V = max(dB - ref_db, -top_db) in out
 *   orcai_column_select(V, n_frames, k, rank_col) -> m,   orcai_subtract_columns -> Y = V - m
 *   orcai_quantile_select_radix(Y, rank_lo, rank_hi), orcai_frontend_finalize(0), orcai_clip_normalize
 * in this order, byte for byte.  The clip runs on the denoised values Y, so rank_lo / rank_hi keep their meaning (n = n_frames * k); the radix select
 * because Y is not dB-shaped.  The band arguments as for orcai_stft_mel_db, all ignored when band_lo is null.
 *   profile    f32[k] or null: receives m, the recording's noise profile in referenced dB
 *   scratch    orcai_column_select_scratch_bytes(k) bytes, 4-byte aligned;  out f32[n_frames * k] in [0, 1], 16-byte aligned
 * No host synchronisation.  orcai_frontend_stats_dev behind it reports pmax of the STFT and p_lo / p_hi as values of Y; ref_db reads 0 there, as the
 * last finalize leaves it for orcai_clip_normalize (the STFT's is 10 log10(max(pmax, 1e-10))).  ORCAI_E_BADARG before anything is launched for what the
 * select and clip steps would refuse; the transform's own refusals are those of the STFT entry, unchanged.  Its gradient w.r.t. the audio is
 * orcai_denoised_spectrogram_bwd below (orcai_spectrogram_bwd and orcai_mel_spectrogram_bwd do not know the floor and are not it). */
int orcai_make_denoised_spectrogram(const float* pcm, int64_t n_samples, int n_fft, int hop, int64_t n_frames, int k, const int* band_lo, const int* band_hi,
                                    const int* band_off, const float* weights, int n_weights, int64_t rank_col, int64_t rank_lo, int64_t rank_hi, float top_db,
                                    float* out, float* profile, void* scratch, void* workspace, void* stream);

/* The time-varying noise floor (the spectrogram parameter "denoise" with "segment" set).  The rows of x = f32[rows][cols] are cut into
 * S = max(1, rows / seg_rows) segments: segment s < S - 1 is rows [s seg_rows, (s + 1) seg_rows), the last one [(S - 1) seg_rows, rows) -- it absorbs the
 * remainder, so it has seg_rows .. 2 seg_rows - 1 rows (all the rows when S == 1, which may be fewer than seg_rows).
 *
 * orcai_segment_column_select: out[s][c] = the rank-th smallest of column c inside segment s (rank_last-th inside the last segment), bit for bit what
 * orcai_column_select(x + s seg_rows cols, n_s, cols, rank_s) returns.  Two routes with the same bytes, chosen by one rule
 * (orcai_segment_column_select_route: 1 fused, 0 loop): while 61 ns x the rows of the longest segment <= 45 us x S (a lone workgroup's time per row of its
 * slab against the launches of one orcai_column_select, both measured: DESIGN 4.25) ONE launch in which a workgroup owns one (segment, 32 adjacent
 * columns), keeps the u32[32][257] histogram and the columns' {prefix, rank} in LDS (33.2 KiB static, no opt-in), runs all four digit passes itself and
 * re-reads its own slab (n_s rows x 128 bytes) between them: no global histogram, no global atomics, out written with ordinary stores; columns of a
 * partial group idle their lanes (no lane packing).  Few, long segments would leave most compute units idle while each workgroup walks megabytes, and the
 * entry loops over orcai_column_select on the row ranges instead, through scratch.  orcai_segment_column_select_fused runs the one-launch route whatever the rule says
 * (the measurement's and the tests' handle; no scratch).
 *   rank       0 <= rank < seg_rows, read for the segments in front of the last (not checked when S == 1);  rank_last  0 <= rank_last < rows of the last
 *   out        f32[S][cols];  scratch  orcai_segment_column_select_scratch_bytes(rows, cols, seg_rows) bytes, 4-byte aligned: orcai_column_select's
 *              histograms and state, then f32[S][cols] this call leaves alone (orcai_make_segment_denoised_spectrogram's profile when none is passed)
 * Asynchronous, no allocation, no host synchronisation.  ORCAI_E_BADARG before anything is launched: a null or not 4-byte aligned pointer, rows < 1 or
 * >= 2^32, cols outside 1..4096, seg_rows < 1, a rank outside its segment.  The scratch size is 0 and the route ORCAI_E_BADARG for such sizes. */
size_t orcai_segment_column_select_scratch_bytes(int64_t rows, int cols, int64_t seg_rows);
int orcai_segment_column_select_route(int64_t rows, int cols, int64_t seg_rows);
int orcai_segment_column_select(const float* x, int64_t rows, int cols, int64_t seg_rows, int64_t rank, int64_t rank_last, float* out, void* scratch,
                                void* stream);
int orcai_segment_column_select_fused(const float* x, int64_t rows, int cols, int64_t seg_rows, int64_t rank, int64_t rank_last, float* out, void* stream);

/* In place: x[t][c] = fl32(x[t][c] - F[t][c]), F the floors m = f32[S][cols] interpolated linearly in time between the segment centres and held constant
 * outside the first and the last.  In doubled integer coordinates u = 2 t and c2_s = 2 s seg_rows + n_s - 1 (n_s the rows of segment s):
 *   u <= c2_0: F = m[0];   u >= c2_{S-1}: F = m[S-1];   else with c2_s <= u < c2_{s+1}:
 *   a = (float)((double)(u - c2_s) / (double)(c2_{s+1} - c2_s)),   F = fl32(m[s] + fl32(a * fl32(m[s+1] - m[s])))   -- no fused multiply-add
 * which is orcai_amd/denoise.py's segment_denoise_ref byte for byte; with S == 1 the bytes of orcai_subtract_columns.  One streaming pass shaped as
 * orcai_subtract_columns' (16-byte accesses from the first 16-byte boundary of x, scalars in front and behind); {s, a} is computed in the kernel, once
 * per 16-byte piece and again only where the piece crosses into the next row.  ORCAI_E_BADARG: null or not 4-byte aligned x or m, rows, cols and
 * seg_rows as above. */
int orcai_subtract_segment_floor(float* x, int64_t rows, int cols, int64_t seg_rows, const float* m, void* stream);

/* orcai_make_denoised_spectrogram with orcai_segment_column_select(V, n_frames, k, seg_rows, rank_seg, rank_seg_last) -> m and
 * orcai_subtract_segment_floor in place of orcai_column_select and orcai_subtract_columns; every other step, their order and the statistics contract
 * are that entry's, byte for byte.  profile: f32[S][k] or null.  scratch: orcai_segment_column_select_scratch_bytes(n_frames, k, seg_rows) bytes.
 * Forward only: orcai_denoised_spectrogram_bwd is the gradient of the global floor, not of this one. */
int orcai_make_segment_denoised_spectrogram(const float* pcm, int64_t n_samples, int n_fft, int hop, int64_t n_frames, int k, const int* band_lo,
                                            const int* band_hi, const int* band_off, const float* weights, int n_weights, int64_t seg_rows, int64_t rank_seg,
                                            int64_t rank_seg_last, int64_t rank_lo, int64_t rank_hi, float top_db, float* out, float* profile, void* scratch,
                                            void* workspace, void* stream);

/* Gradient of orcai_make_denoised_spectrogram w.r.t. the audio.  Notation as at orcai_spectrogram_bwd (band_lo null) and orcai_mel_spectrogram_bwd
 * (band_lo set); dB is 10 log10(max(P, 1e-10)) on the linear route and 10 log10(max(M[m], 1e-10)) on the mel route.  With
 *   v = max(dB - ref_db, -top_db),  y = v - m[k] (f32, one rounding),  out = (clip(y, p_lo, p_hi) - p_lo) / (p_hi - p_lo)  and  g = dL/dout:
 *   g_db[t][k] = g[t][k] / (p_hi - p_lo)  where P (or M) > 1e-10, dB - ref_db > -top_db and p_lo < fl32(v - m[k]) < p_hi (all strict); 0 otherwise
 * and everything behind g_db -- dP or dM, the mel gather, dRe and dIm, the inverse transform, the window and the frame-ordered overlap sum into dpcm --
 * is that of the plain entry of the route, unchanged.  The gate forms v - m[k] first, in f32, and then compares, as the forward's clip does; the floor is
 * never folded into the bounds.
 * The floor m[k] is HELD CONSTANT, like ref_db, p_lo and p_hi and for the reason given at orcai_spectrogram_bwd: it is an order statistic of channel k,
 * depends on the data through a single STFT bin (band) of that channel, and that dependence is ill-defined under ties.  There is no gradient "through
 * the median".
 *   pcm ... n_weights   as for orcai_make_denoised_spectrogram: band_lo null selects the linear route with k = k_crop (the other band arguments are then
 *              ignored); otherwise the band arrays in HOST memory and the packed weights on the device, k = n_mels
 *   gout       f32[n_frames * k], layout [frame][channel]
 *   stats_dev  f32[6] from orcai_frontend_stats_dev after orcai_make_denoised_spectrogram of the same pcm.  Its ref_db slot reads 0 there, so ref_db is
 *              recomputed on the device from stats_dev[0] = pmax, 10 log10(max(pmax, 1e-10)) as orcai_frontend_finalize computes it; stats_dev[1] is
 *              never read.  p_lo and p_hi (values of y) are stats_dev[2] and [3].
 *   profile    f32[k] on the device: m, what the forward wrote to its `profile`
 *   dpcm       f32[n_samples]: every element is WRITTEN; no float atomics, two launches give identical bytes
 * No allocation, no host synchronisation; the launch geometry and the LDS request are the plain entry's (the floor is read through the cache), so the
 * first call per device with more than 64 KiB of LDS (mel, n_fft = 4096) must come outside a stream capture.  With profile all zero and the statistics
 * of the plain forward the bytes are those of orcai_spectrogram_bwd / orcai_mel_spectrogram_bwd.
 * Refusals come before anything is launched and leave dpcm untouched.  ORCAI_E_BADARG: a null pcm, gout, stats_dev, profile or dpcm, one of them not
 * 4-byte aligned, and what the route's plain entry answers with it (sizes, n_frames other than 1 + n_samples / hop, the mel route's alignment and band
 * checks).  ORCAI_E_UNSUPPORTED: n_fft that is no power of two from 32 (linear) or 128 (mel) to 4096; two mel bands of equal parity that overlap. */
int orcai_denoised_spectrogram_bwd(const float* pcm, int64_t n_samples, int n_fft, int hop, int64_t n_frames, int k, const int* band_lo, const int* band_hi,
                                   const int* band_off, const float* weights, int n_weights, const float* gout, const float* stats_dev, const float* profile,
                                   float top_db, float* dpcm, void* stream);
int orcai_denoised_spectrogram_bwd_occupancy(int n_fft, int n_mels); /* workgroups of that launch per compute unit as the runtime computes it (n_mels = 0: the linear route); -1 if refused */


/* ------------------------------------------------------------------------------------------
 * Model forward, inference (architectures.py:162-241 as executed by model.predict, predict.py:265-268)
 * Activations are planar fp32 [snippet][channel][H = time][W = freq].  BatchNormalization is folded on
 * the host into per-channel (scale, shift): scale = gamma*rsqrt(var + 1e-3),
 * shift = beta - mean*scale + conv_bias*scale.
 * ------------------------------------------------------------------------------------------ */

/* Padded plane layout used by every convolutional activation tensor: an H x W plane is stored as HP x WP floats,
 * HP = H + 2*(k/2) (k/2 zero rows above and below), WP = orcai_padded_width(W, k) = roundup4(W + k/2) (zero columns
 * on the right); image pixel (y, x) is at (y + k/2)*WP + x.  The CALLER zero-fills the buffers once; the kernels
 * never write the pads, so "same" zero padding costs no bounds checks and every tile halo is one contiguous run. */
int orcai_padded_width(int W, int ksize);

/* Knob of the separable-conv launcher for k = 3 launches with plane or x-pooled output (the inference trunk, the training forward
 * with its depthwise-output store, the input-gradient passes).  1 (default): the LDS-shared-row kernels -- sepconv_tile_kernel (a
 * workgroup of 8 waves owns 8 image rows x 64 columns; the tile's 10 input rows per channel quad are fetched once by LDS-DMA) on the
 * "strip" route, sepconv_ftile_kernel (8 consecutive windows of the flat plane share one contiguous range of rows) on the "flat"
 * route; 2: no strips; 0: the one-window-per-wave sepconv_kernel everywhere.  Which shape takes which route is stated once, in
 * orcai_amd/csrc/sep_route.h, and reported by orcai_sepconv_route.  All three perform the same arithmetic in the same order
 * (bit-identical results).  Returns the previous value; values outside [0, 2] only query.  Process-wide, not thread-safe. */
int orcai_sepconv_tile_mode(int mode);

/* The route of a k = 3 launch on R = 1 planes under the current orcai_sepconv_tile_mode: 0 window, 1 strip, 2 flat.  Pure host code,
 * no GPU call.  half: 0 the f32 launcher, 1 the f16 one.  extras: 0 none, 1 depthwise-output store, 2 + output statistics
 * (orcai_[h_]sepconv[_planes]_stats), 3 + BatchNorm folded on load (..._stats_bn), 4 / 5 epi 2 / 3 of orcai_sepconv_planes_epi (f32
 * only).  The entry points with extras >= 2 return ORCAI_E_UNSUPPORTED exactly where this says window.  ORCAI_E_BADARG on nonsense. */
int orcai_sepconv_route(int half, int Cin, int Cout, int H, int W, int out_layout, int extras);

/* Same kind of knob for orcai_conv0_sepconv: windows per wave (>= 1; the next window's inputs are prefetched while the current
 * one is computed).  Returns the previous value; values outside [1, 64] only query. */
int orcai_entry_windows(int windows_per_wave);

/* orcai_conv0_sepconv on planes at least two 62-column strips wide with Cout in 17..32: waves per workgroup of the strip-tile
 * variant (conv0_sep_tile_kernel: every entry-activation row is computed once per tile and shared through LDS), 10 (default) or 16;
 * 0 = conv0_sep_kernel everywhere.  Bit-identical either way.  Returns the previous value; other values only query. */
int orcai_entry_tile(int waves);

/* Conv2D(16, k, padding="same") + BN + ReLU on the 1-channel spectrogram (architectures.py:164-168).
 *   in              f32, UNPADDED: snippet b starts at in + b*snippet_stride and is [H][W] row-major.  For the sliding
 *                   50 % overlap view of a [T][W] spectrogram use snippet_stride = (H/2)*W: no snippet copy is
 *                   materialised (predict.py:253-261 makes one)
 *   w               f32[k*k][16] (Keras kernel (k,k,1,16) flattened); scale/shift f32[16]
 *   out             f32[B][16][HP][WP] padded planes */
int orcai_conv0_bn_relu(const float* in, int64_t snippet_stride, int B, int H, int W, int ksize, const float* w, const float* scale,
                        const float* shift, float* out, void* stream);

/* Entry convolution fused into the first separable convolution, k = 3, inference (architectures.py:164-179):
 *   Conv2D(16, 3, same) + BN + ReLU  ->  ReLU -> SeparableConv2D(Cout, 3, same) -> BN -> [ReLU]
 * = orcai_conv0_bn_relu followed by orcai_sepconv_bn(relu_in = 1, out_layout = 0), bit for bit, without the 16-channel entry
 * activation ever reaching HBM.  in / snippet_stride / w0 / scale0 / shift0 as for orcai_conv0_bn_relu; dw f32[4][9][4] (channel-quad layout, see orcai_sepconv_bn),
 * pw f32[16][Cout], scale / shift f32[Cout] as for orcai_sepconv_bn; out: padded channel-quad planes of Cout channels.
 *   prev_sub (may be NULL)  f32[B][4][ceil(H/2)][ceil(W/2)][4]: the entry activation at pixels (2i, 2j) only -- all that the
 *                           strided 1x1 residual convolution of block 1 reads (orcai_pool_res_add with flag 2). */
int orcai_conv0_sepconv(const float* in, int64_t snippet_stride, int B, int H, int W, const float* w0, const float* scale0, const float* shift0,
                        const float* dw, const float* pw, const float* scale, const float* shift, int Cout, int relu_out, float* out, float* prev_sub,
                        void* stream);

/* [ReLU] -> SeparableConv2D(Cout, k, same) -> BN -> [ReLU]   (architectures.py:174-189, :198-206)
 *   in   f32[B][ceil(Cin/4)][HP][WP][4] padded channel-quad planes
 *   dw   f32[ceil(Cin/4)][k*k][4]   channel-quad layout: element (q, tap, j) = Keras depthwise kernel (k,k,Cin,1) at
 *        [tap / k][tap % k][4q + j][0], zero for channels >= Cin (what the kernels read with scalar loads; 16-byte aligned)
 *   pw   f32[Cin][Cout]  (Keras pointwise kernel (1,1,Cin,Cout))
 *   out_layout 0: padded channel-quad planes;  1: f32[B][H][W*Cout] with feature = x*Cout + c, i.e. Keras
 *   Reshape((-1, W*C)) of the NHWC tensor (architectures.py:208);  2: x-pooled f32[B][CQout][H][roundup4(ceil(W/2))][4]:
 *   element (y, j) = max over the column pair (2j, 2j+1) -- the first half of the MaxPooling2D((3,2), 2, "same") that
 *   follows (architectures.py:190), consumed by orcai_pool_res_add(xpooled = 1).  Cout <= 64, k in {3,5,7}. */
int orcai_sepconv_bn(const float* in, int B, int Cin, int H, int W, int ksize, int relu_in, const float* dw, const float* pw, const float* scale,
                     const float* shift, int Cout, int relu_out, int out_layout, float* out, void* stream);

/* MaxPooling2D((3,2), strides 2, "same")(s) + Conv2D(C, 1, strides 2, "same")(prev)   (architectures.py:190-196)
 *   xpooled is a flag word.  Bit 0: s is the x-pooled tensor written by orcai_sepconv_bn(out_layout = 2) instead of padded
 *   channel-quad planes of C channels.  Bit 1: prev is the compact subsample f32[B][ceil(Cp/4)][ceil(H/2)][ceil(W/2)][4] of
 *   pixels (2i, 2j) written by orcai_conv0_sepconv instead of padded channel-quad planes of Cp channels.  wr f32[Cp][C], br f32[C]
 *   -> out f32[B][C][ceil(H/2) + 2*(k/2)][orcai_padded_width(ceil(W/2), k)] padded planes */
int orcai_pool_res_add(const float* s, const float* prev, int B, int C, int Cp, int H, int W, int ksize, const float* wr, const float* br,
                       float* out, int xpooled, void* stream);
/* orcai_pool_res_add (xpooled bit 0 set) over B windows of one recording, each output row stored into the per-snippet planes that hold it
 * (50 %-overlapping snippets whose first blocks are computed once per recording row).  Window b's output row r is
 * recording row R = base + b * img_step + r of this stage; R is row R - k * period of snippet k = R / period and row R - (k-1) * period of
 * snippet k - 1.  A row is stored only for r_lo <= r < r_hi (also r < r_lo for a window starting at recording row 0: the first snippet's
 * own top edge), and only into rows keep_lo <= y < keep_hi of snippets 0 <= k < nsnip.
 *   out f32[nsnip][ceil(C/4)][Hd + 2*(k/2)][orcai_padded_width(ceil(W/2), k)][4] padded planes (pads untouched), Hd = 2 * period.
 * Bit for bit the values orcai_pool_res_add writes for the same window.  ORCAI_E_UNSUPPORTED, before anything is launched, for every
 * shape orcai_pool_res_add does not run on its x-pooled kernel. */
int orcai_pool_res_add_scatter(const float* s, const float* prev, int B, int C, int Cp, int H, int W, int ksize, const float* wr, const float* br,
                               float* out, int xpooled, int Hd, int nsnip, int period, int base, int img_step, int r_lo, int r_hi, int keep_lo,
                               int keep_hi, void* stream);
/* orcai_pool_res_add_scatter with up to ORCAI_ROW_FAMILIES destination families instead of the snippets: window b's output row r is recording
 * row R = base + b * img_step + r, stored for r_lo <= r < r_hi (also r < r_lo for a window starting at recording row 0) into row
 * y = R - offset - j * period of image j of every family, for 0 <= j < count and keep_lo <= y < keep_hi.  Image j of a family holds
 * recording rows [offset + j * period, offset + j * period + Hd); out f32[count][ceil(C/4)][Hd + 2*(k/2)][orcai_padded_width(ceil(W/2), k)][4]
 * padded planes (pads untouched).  `fams` is a HOST array, read during the call.  Bit for bit the values orcai_pool_res_add writes for the
 * same window.  ORCAI_E_UNSUPPORTED, before anything is launched, for every shape orcai_pool_res_add does not run on its x-pooled kernel,
 * more than ORCAI_ROW_FAMILIES families, or a family with keep_hi - keep_lo > 2 * period (a row in more than two of its images). */
#define ORCAI_ROW_FAMILIES 4
typedef struct {
  float* out;
  int Hd, period, offset, count, keep_lo, keep_hi;
} orcai_row_family;
int orcai_pool_res_add_scatter_families(const float* s, const float* prev, int B, int C, int Cp, int H, int W, int ksize, const float* wr,
                                        const float* br, int xpooled, int base, int img_step, int r_lo, int r_hi, const orcai_row_family* fams,
                                        int nfam, void* stream);
/* A residual block's second separable convolution WITH the block's tail in its epilogue (architectures.py:172-196, predict.py:265-268):
 *   out = MaxPooling2D((3,2), strides 2, "same")(scale * SepConv(relu_in ? relu(in) : in) + shift [relu_out]) + Conv2D(C, 1, strides 2)(prev) + br
 * = orcai_sepconv_bn(out_layout = 2) followed by orcai_pool_res_add(xpooled bit 0), bit for bit, without the x-pooled tensor in HBM.
 *   in f32[B][ceil(Cin/4)][H+2][orcai_padded_width(W,3)][4] planes, dw f32[ceil(Cin/4)][9][4], pw f32[Cin][C], scale / shift f32[C] (folded BatchNorm);
 *   prev: the block input, padded planes of Cp channels at H x W, or (prev_compact) its (2i, 2j) subsample f32[B][ceil(Cp/4)][H/2][ceil(W/2)][4];
 *   wr f32[Cp][C], br f32[C] -> out f32[B][ceil(C/4)][H/2 + 2][orcai_padded_width(ceil(W/2),3)][4] padded planes (pads untouched).
 * ORCAI_E_UNSUPPORTED (the caller runs the two launches) unless ksize == 3, 17 <= C <= 32, 17 <= Cin <= 32, Cp <= 16, H even and the plane is wide
 * enough for 60-column strips (orcai-V1 block 1).  orcai_pool_fused(nt): tiles of 8 conv rows a workgroup marches over (default 8); 0 switches the
 * fused tail off; < 0 queries; returns the previous value. */
int orcai_sepconv_pool_res(const float* in, const float* prev, int B, int Cin, int C, int Cp, int H, int W, int ksize, int relu_in, const float* dw, const float* pw,
                           const float* scale, const float* shift, int relu_out, const float* wr, const float* br, float* out, int prev_compact, void* stream);
int orcai_pool_fused(int nt);
int orcai_pool_vertical(int on); /* experiments: 1 (default) = the inference pooling kernel on stacked tiles (4 output rows x 16 columns per wave: the row two windows share is loaded once) where the pooled plane is >= 40 columns wide; 0 = flat 64-pixel windows everywhere; < 0 queries; returns the previous value.  Bit-identical results. */

/* C[M][N] = act(A[M][K] * Bm[K][N] + bias[N]) [* scale[N] + shift[N]]; act 0 = identity, 1 = ReLU; bias/scale/shift may be NULL.
 * Used for the LSTM input projections x*W + b (architectures.py:210-229) and Dense(128, relu) + BN (:231-237). */
int orcai_gemm_bias_act(const float* A, const float* Bm, const float* bias, const float* scale, const float* shift, float* C, int64_t M, int N,
                        int K, int act, void* stream);

/* Both directions of one Bidirectional(LSTM(units, return_sequences=True)) given xz = x*W + b.
 *   xz  f32[B][T][2][4*units], Uw f32[2][units][4*units], both with the gate columns in the kernel's order:
 *       column 32*w + 16*nt + j  <-  Keras column (2*nt + (j>>3))*units + 8*w + (j&7)     (gate order i,f,c,o)
 *   out f32[B][T][2*units] = concat(forward, backward) at each time step.  units a multiple of 32 in [32, 256]: up to 128 the recurrent
 *   matrix stays in registers; 160..256 run the L2-streamed f32-MFMA family of csrc/lstm_wide.hip (for either orcai_lstm_split setting, and
 *   for the orcai_h_ twins of the training entries below); the training backward then needs Uw and dxz 16-byte aligned (ORCAI_E_BADARG). */
int orcai_lstm_recurrent(const float* xz, const float* Uw, int B, int T, int units, float* out, void* stream);

/* out[M][N] = sigmoid(x[M][K] * w[K][N] + b[N]),  1 <= N <= 64   (architectures.py:239) */
int orcai_dense_sigmoid(const float* x, const float* w, const float* bias, int64_t M, int K, int N, float* out, void* stream);

/* predict.py:276-293: overlay the n snippet predictions [n][P][L] at offsets i*step, count overlaps, divide.
 *   agg f64[S][L], cnt f64[S];  float64 accumulation in snippet order (bit-exact with the numpy loop). */
int orcai_overlap_average(const float* pred, int n, int P, int L, int step, int64_t S, double* agg, double* cnt, void* stream);

/* orcai_overlap_average over a table of R recordings in one launch (several recordings through one detector pass: orcai_amd/batch.py).
 *   pred  f32[n_total][P][L]: the snippets of all recordings, recording r's at pred[first_r .. first_r + n_r)
 *   table int64[R][4] ON THE DEVICE, row r = {first_r, n_r, S_r, row_r}: row_0 = 0, row_{r+1} = row_r + S_r, S_total = the sum of S_r
 *   agg   f64[S_total][L], cnt f64[S_total]: rows row_r .. row_r + S_r are, bit for bit, what orcai_overlap_average(pred + first_r*P*L, n_r, P, L,
 *         step, S_r, ...) writes for recording r alone, the zero-count steps behind its last snippet included.
 * One thread per output element (binary search of its recording on row_r), no atomics: deterministic.  The table's contents are not checked.
 * ORCAI_E_BADARG: a null pointer, R < 1, non-positive P / L / step / S_total.  ORCAI_E_UNSUPPORTED: S_total * L needs 2^31 or more workgroups. */
int orcai_overlap_average_ragged(const float* pred, int P, int L, int step, const int64_t* table, int R, int64_t S_total, double* agg, double* cnt,
                                 void* stream);

/* predict.py:298-340 and the duration filter of :14-159: label intervals from the averaged probabilities of R recordings, in the order of the
 * label file (compute_binary_predictions + compute_labels, with _check_duration's verdict per interval).
 *   agg, cnt   f64[S_total][L], f64[S_total]: what orcai_overlap_average (R = 1, table = {0, n, S, 0}) or orcai_overlap_average_ragged writes
 *   table      int64[R][4] ON THE DEVICE, the ragged launcher's; only S_r and row_r are read.  1 <= L <= 64.
 *   per recording r, over rows row_r .. row_r + S_r:  thr_r = threshold / max(cnt) (one f64 division; no rows or a zero maximum: no runs);
 *              b[s][l] = agg[s][l] > thr_r (strict, NaN is false); a run is a maximal stretch of ones of one column INSIDE the recording
 *   runs       int32[capacity][4] = {start_row, stop_row (inclusive), label, status}, rows counted from row_r, 16-byte aligned.  Recording r's runs
 *              are runs[offsets[r] .. offsets[r + 1]), ascending by (start_row, stop_row, label_rank[label], label): the order of the stable
 *              sort_values(by=["start", "stop", "label"]) when label_rank int[L] is the string order of the label names.
 *   status     limits f64[L][2] = {min, max} seconds per label, NULL: every status 0.  d = (double)((stop_row - start_row) * tpo) * frame_seconds;
 *              1 (too short) if d < min, else 2 (too long) if d > max, else 0.
 *   offsets    int64[R + 1]; offsets[R], the number of runs found, is always written.  Runs at positions >= capacity are counted and not stored
 *              (the caller retries with a larger buffer); capacity = L * ceil(S_total / 2) + R always suffices.
 *   workspace  orcai_extract_labels_workspace_bytes(L, R, S_total) bytes, 256-byte aligned (0 for sizes the call refuses).
 * Six launches on `stream` (labels.hip: row tile 256 rows, scan tile 64 row tiles); none iterates over the length of a run.  Output positions are
 * computed by scans, not claimed: no atomics, two calls write the same bytes.  The table's contents are not checked (rows tile [0, S_total) in
 * ascending order, as the ragged launcher wants them).
 * ORCAI_E_BADARG: a null agg / cnt / table / label_rank / runs / offsets / workspace, L outside 1..64, R < 1, S_total < 1, capacity < 0, tpo < 1,
 * a workspace smaller than the size function answers, misaligned runs or workspace.  ORCAI_E_UNSUPPORTED (nothing launched): 2^31 or more row tiles. */
int orcai_extract_labels(const double* agg, const double* cnt, int L, const int64_t* table, int R, int64_t S_total, double threshold,
                         const int* label_rank, const double* limits, double frame_seconds, int tpo, int* runs, int64_t capacity, int64_t* offsets,
                         void* workspace, size_t workspace_bytes, void* stream);
size_t orcai_extract_labels_workspace_bytes(int L, int R, int64_t S_total);

/* orcai_extract_labels with one decision threshold per label (`orcai predict --thresholds`): the same arguments, thresholds f64[L] ON THE DEVICE in
 * place of the scalar.  thr_r[l] = thresholds[l] / max(cnt) over the rows of recording r (one f64 division per label; no rows or a zero maximum: no
 * runs), b[s][l] = agg[s][l] > thr_r[l] (strict, NaN is false); everything behind the threshold stage -- runs, order, status, offsets, workspace, the
 * six launches -- is orcai_extract_labels' own code, so with every threshold equal to t the output is byte for byte that of the scalar call with t.
 * ORCAI_E_BADARG / ORCAI_E_UNSUPPORTED as there, and ORCAI_E_BADARG for a null thresholds. */
int orcai_extract_labels_per_label(const double* agg, const double* cnt, int L, const int64_t* table, int R, int64_t S_total, const double* thresholds,
                                   const int* label_rank, const double* limits, double frame_seconds, int tpo, int* runs, int64_t capacity,
                                   int64_t* offsets, void* workspace, size_t workspace_bytes, void* stream);

/* orcai_extract_labels_per_label with hysteresis and gap merging (`orcai predict --high-thresholds --merge-gap`): the same arguments plus
 * high_thresholds f64[L] and gap_rows int32[L], both ON THE DEVICE.  Per recording r and label l, with max = max(cnt) over the recording's rows:
 *   lo[s] = agg[s][l] > thresholds[l] / max,  hi[s] = lo[s] && agg[s][l] > high_thresholds[l] / max  (one f64 division each, strict, NaN is false);
 *   1. candidates are the maximal stretches of lo inside the recording;  2. a candidate is kept iff one of its rows has hi set;
 *   3. kept runs of one column and recording are joined while next.start - prev.stop - 1 <= gap_rows[l] (transitively; dropped candidates in the gap
 *      do not matter; runs of different recordings are never joined; a gap below 1 joins nothing);
 *   4. order, status (the duration verdict on the joined run), offsets, capacity bound and output format are orcai_extract_labels' own.
 * With high_thresholds == thresholds and every gap 0 the output is byte for byte that of orcai_extract_labels_per_label.  Twelve launches on `stream`
 * (labels.hip): keep flags come from prefix counts of the hi rows, chain ends from nearest-set-bit scans over the kept candidates of a column; no lane
 * walks a run, a gap or a chain, no atomics, two calls write the same bytes.
 *   workspace  orcai_extract_labels_refined_workspace_bytes(L, R, S_total) bytes, 256-byte aligned (0 for sizes the call refuses).
 * ORCAI_E_BADARG as orcai_extract_labels_per_label, and for a null high_thresholds or gap_rows.  ORCAI_E_UNSUPPORTED (nothing launched):
 * S_total >= 2^31 (candidate rows are kept as int32). */
int orcai_extract_labels_refined(const double* agg, const double* cnt, int L, const int64_t* table, int R, int64_t S_total, const double* thresholds,
                                 const double* high_thresholds, const int* gap_rows, const int* label_rank, const double* limits, double frame_seconds,
                                 int tpo, int* runs, int64_t capacity, int64_t* offsets, void* workspace, size_t workspace_bytes, void* stream);
size_t orcai_extract_labels_refined_workspace_bytes(int L, int R, int64_t S_total);

/* A score for every interval an extraction call found (`orcai predict --scores`).  The call goes behind orcai_extract_labels,
 * orcai_extract_labels_per_label or orcai_extract_labels_refined on the same stream and reads agg, table, runs, offsets and capacity as that call
 * left them on the device; only min(offsets[R], capacity) runs are scored.  The recording of run i is found by a binary search of i in offsets.
 * The contract, shared with the host route (orcai_amd/scores.py): for a run of label l in recording r over rows start_row .. stop_row inclusive
 * (counted inside the recording, as runs stores them; for a merged run the rows of its gaps count), with p[s] = agg[row_r + s][l]:
 *   peak      the largest p[s], as the f64 it is; NaN rows are skipped (a gap row may be NaN, a start row never is: NaN is above no threshold).
 *   peak_row  the lowest row s that attains peak: ties go to the earlier row.
 *   sum_q32   the sum of q[s] = rint(min(max(p[s], 0), 1) * 2^32) (round-half-even, NaN gives 0) as an unsigned 64-bit integer.  The scaling by a power
 *             of two and the rint are exact and integer addition is associative, so every order of reduction gives the same bits; a run of fewer than
 *             2^31 rows sums to less than 2^63.
 *   mean      is NOT written: the caller forms sum_q32 / (n_rows * 2^32) in f64, within 2^-33 of the exact mean of the clamped rows by definition.
 *   scores    24 bytes per run, in run order: {f64 peak, u64 sum_q32, i64 peak_row}, 8-byte aligned, `capacity` rows.  (A run whose rows are all NaN,
 *             which no extraction call produces: peak NaN, peak_row -1.)
 *   eager     NULL, or room for eager_runs rows of the same layout: the rows of the first eager_runs runs are written there AS WELL, so that a caller
 *             can keep them next to the head of its run buffer and fetch both in one copy.
 *   workspace orcai_interval_scores_workspace_bytes(L, R, S_total) bytes, 256-byte aligned (0 for sizes the call refuses).
 * Two launches on `stream` (labels.hip).  Row tiles of 256 rows are cut on the GLOBAL rows of agg.  The first launch reads every tile's 256 x L slab
 * once and leaves per (tile, label) the maximum, its first row and the q32 sum; the second gives every run 16 lanes, which share its head piece (at most
 * 255 rows), the table entries of its whole tiles and its tail piece (at most 255 rows).  No lane walks a run; agg is read once by the first launch and,
 * element for element, at most once more by the second.  No atomics: two calls write the same bytes.
 * ORCAI_E_BADARG: a null agg / table / runs / offsets / scores / workspace, L outside 1..64, R < 1, S_total < 1, capacity < 0, eager_runs < 0, a
 * workspace smaller than the size function answers, misaligned runs, scores, eager or workspace.  ORCAI_E_UNSUPPORTED (nothing launched):
 * S_total >= 2^31 (global rows are kept as int32). */
int orcai_interval_scores(const double* agg, int L, const int64_t* table, int R, int64_t S_total, const int* runs, const int64_t* offsets,
                          int64_t capacity, void* scores, void* eager, int64_t eager_runs, void* workspace, size_t workspace_bytes, void* stream);
size_t orcai_interval_scores_workspace_bytes(int L, int R, int64_t S_total);

/* test.py:37-225: the integer counts behind the three tables of `orcai test` (compute_confusion_table, compute_misclassification_tables) for one
 * batch; the host forms the tables' float64 values from them (orcai_amd/device_tables.py).
 *   p, y       f32[M][L], M = snippets * time steps: probabilities, and labels in {0, 1, mask_value = -1}.  1 <= L <= 64.
 *   The call ADDS to conf and mis: the caller zeroes both once per dataset (orcai_zero_fill) and every batch accumulates into them.
 *   conf       int64[L][4] = {TN, FP, FN, TP} per label over the elements with y != mask_value; predicted = p >= 0.5f (NaN: not predicted), the truth
 *              tests are y == 0 and y == 1.
 *   mis        int64[2][L+1][L+1][L].  Direction d = 0 (true_pred): matrix 1 = the labels truncated to int, matrix 2 = the prediction bits; d = 1
 *              (pred_true): the roles swapped.  Per row and direction, with ones1 / ones2 the columns equal to 1 and n1 / n2 their counts:
 *              n1 > 1: the row is skipped.  n1 == 1: src = that column a, and the row is skipped if matrix2[row][a] == -1.  n1 == 0: src = L (NOLABEL).
 *              n2 > 0: mis[d][src][c][n2 - 1] += 1 for every c of ones2; else mis[d][src][L][0] += 1.
 *              A table cell is sum over n of mis[d][src][c][n - 1] / n: the n2 axis keeps the 1 / n2 shares of the host route as integers.
 * One launch on `stream` (test_tables.hip), one lane per row; no workspace, no allocation, no synchronisation.  Integer adds only, 64-bit global
 * accumulators: the result does not depend on the order of execution and two runs from equal buffers leave the same bytes.  Counts are reduced per
 * workgroup first -- ballots for conf and for the NOLABEL -> NOLABEL bin of both directions, an LDS histogram of the other bins for L <= 16 -- and
 * only non-zero workgroup totals reach global memory; for L > 16 the rows outside that one bin add straight to global memory.
 * ORCAI_E_BADARG: a null p / y / conf / mis, M < 1, L outside 1..64.  ORCAI_E_UNSUPPORTED (nothing launched): 2^31 or more workgroups. */
int orcai_test_counts(const float* p, const float* y, int64_t M, int L, float mask_value, int64_t* conf, int64_t* mis, void* stream);

/* The integer counts of the threshold sweep of `orcai test --threshold-sweep` for one batch (orcai_amd/threshold_sweep.py forms TP / FP / FN / TN per
 * threshold, the ROC and PR curves and their areas from them: the MaskedAUC of reference architectures.py:289-304 as a test-time report).
 *   p, y        f32[M][L] as for orcai_test_counts.  1 <= L <= 64.
 *   thresholds  f32[T] ON THE DEVICE, strictly ascending (not checked; any table leaves k inside 0..T).  1 <= T <= 1024.
 *   hist        int64[L][2][T + 1].  For every element (row, l) with y != mask_value and y == 0 or y == 1 (its class c): k = the number of j with
 *               p > thresholds[j] -- strict, in f32, found by searching the table itself, so a probability equal to an entry lies below it; a NaN
 *               gives k = 0 -- and hist[l][c][k] += 1.  Every other label value is ignored.
 *   The call ADDS to hist: the caller zeroes it once per dataset (orcai_zero_fill).  Predicted positive at threshold j is k >= j + 1.
 * One launch on `stream` (test_tables.hip); no workspace, no allocation, no synchronisation.  Integer adds only, 64-bit global accumulators: the
 * result does not depend on the order of execution and two runs from equal buffers leave the same bytes.  grid = (row workgroups, label tiles): a
 * workgroup keeps the u32 image [label tile][2][T + 1] of its tile in LDS beside the table (tile = min(L, 16, what fits into 64 KiB): 16 labels and
 * 25.9 KiB at T = 200, 7 labels and 60.1 KiB at T = 1024), and only its non-zero bins reach global memory, one 64-bit atomic add each.
 * ORCAI_E_BADARG: a null p / y / thresholds / hist, M < 1, L outside 1..64, T outside 1..1024.  ORCAI_E_UNSUPPORTED (nothing launched): 2^31 or more
 * row workgroups. */
int orcai_threshold_counts(const float* p, const float* y, int64_t M, int L, float mask_value, const float* thresholds, int T, int64_t* hist,
                           void* stream);

/* ------------------------------------------------------------------------------------------
 * Training (train.py:155-219: Adam(lr) + MaskedBinaryCrossentropy + MaskedBinaryAccuracy; architectures.py:210-286)
 * "Row tensors" are f32[M][cols] row-major, M = snippets * time steps.
 * ------------------------------------------------------------------------------------------ */

/* C[M][N] (=|+=) alpha * sum_k A(m,k) B(k,n) + beta_w * Wreg[m][n] with A(m,k) = A[m*sam + k*sak], B(k,n) = B[k*sbk + n*sbn]:
 * weight gradients (A^T B), input gradients (A B^T) and the L2 term 2*lambda*W of kernel_regularizer=l2 (architectures.py:215,225,235). */
int orcai_gemm_strided(const float* A, int64_t sam, int64_t sak, const float* B, int64_t sbk, int64_t sbn, float* C, int M, int N, int K, float alpha,
                       int accumulate, const float* Wreg, float beta_w, void* stream);

/* out[c] (=|+=) sum_m x[m][c]  (bias gradients) */
int orcai_colsum(const float* x, int M, int C, float* out, int accumulate, void* stream);

/* BatchNormalization in training mode on a row tensor whose channel is (column % C): batch mean / biased variance,
 * y = [relu]((x - mean) * gamma * rsqrt(var + eps) + beta), and its backward (dbeta, dgamma, dx) with the optional ReLU folded in.
 * Up to 2 048 columns / 512 channels the two reductions (orcai_bn_rows_stats, orcai_bn_rows_bwd) read row slabs with coalesced loads and fold the slabs'
 * partial sums in a fixed order through one device array inside the library: bit-reproducible, but at most ONE of these two launchers may be in flight per
 * device (calls on one stream are ordered and fine) -- the restriction orcai_lstm_bwd has. */
int orcai_bn_rows_stats(const float* x, int M, int cols, int C, float* mean, float* var, void* stream);
int orcai_bn_rows_apply(const float* x, int M, int cols, int C, const float* mean, const float* var, const float* gamma, const float* beta, float eps,
                        int relu, float* y, void* stream);
int orcai_bn_rows_bwd(const float* dy, const float* x, int M, int cols, int C, const float* mean, const float* var, const float* gamma, const float* beta,
                      float eps, int relu, float* dbeta, float* dgamma, float* dx, void* stream);

/* Dropout: mask[i] in {0,1} from a counter-based generator (seed, i); y = x * mask * scale (forward and backward). */
int orcai_dropout_mask(float* mask, int64_t n, uint64_t seed, float keep, void* stream);
int orcai_mask_scale(const float* x, const float* mask, float scale, int64_t n, float* y, void* stream);
/* dx = dy * (y > 0) */
int orcai_relu_bwd(const float* dy, const float* y, int64_t n, float* dx, void* stream);

/* MaskedBinaryCrossentropy / MaskedBinaryAccuracy (architectures.py:262-286): acc3 = {sum of BCE, unmasked count, correct count}
 * (f64, device); dz (may be NULL) = d(mean BCE)/d(logit of the final sigmoid). */
int orcai_masked_bce(const float* p, const float* y, int64_t n, float mask_value, double* acc3, float* dz, void* stream);
/* The same with Keras' class_weight semantics (train.py:125-136, 214: model.fit(class_weight=...)): Keras turns class_weight into a
 * sample weight per (snippet, step) -- class_weight[argmax over labels of y_true] -- and multiplies the SCALAR loss of
 * MaskedBinaryCrossentropy by the batch mean of those weights.  loss_weight (may be NULL = 1) points to that one device float:
 * acc3[0] and dz are multiplied by it.  grad_scale > 0 multiplies dz only (static loss scale of the f16 path, undone in
 * orcai_adam_step's gscale). */
int orcai_masked_bce_w(const float* p, const float* y, int64_t n, float mask_value, double* acc3, float* dz, const float* loss_weight, float grad_scale,
                       void* stream);
/* out += lambda * sum w^2   (value of the L2 penalty) */
int orcai_l2_value(const float* w, int64_t n, float lambda, double* out, void* stream);

/* Keras-3 Adam on flat buffers: g is scaled by gscale first (1/world_size after an all-reduce(sum)); step is 1-based. */
int orcai_adam_step(float* w, const float* g, float* m, float* v, int64_t n, float lr, float b1, float b2, float eps, int step, float gscale, void* stream);

/* Training forward of one Bidirectional(LSTM): as orcai_lstm_recurrent, plus the gate activations (i,f,g,o, permuted columns)
 * f32[B][T][2][4*units] and cell states f32[B][T][2][units] the backward pass needs. */
int orcai_lstm_split(int on); /* 1 (default): the f32 path's LSTM recurrences (inference, training forward and backward) run their recurrent product on f16 MFMA with every operand split as hi + lo / 4096 (f32 accuracy, 24 MFMAs of 16 cycles per step instead of 64 of 32); 0: v_mfma_f32_16x16x4_f32; < 0 queries; returns the previous value */
int orcai_lstm_train_fwd(const float* xz, const float* Uw, int B, int T, int units, float* out, float* gates, float* cstate, void* stream);
/* The f16 path's twin (same arguments, f32 tensors): the recurrent product on v_mfma_f32_16x16x32_f16 with h and U rounded to f16,
 * f32 accumulation on the f32 input projection, gates / cell state / outputs in f32; orcai_h_lstm_bwd likewise for the recurrent
 * term dz U^T of orcai_lstm_bwd (dz rounded to f16 for the product only; dxz is written in f32).  units 160..256 run the f32 wide
 * family, bit for bit the f32 entries' results.  Pinned down by tests/test_half_lstm_gpu.py:
 *   - The f16 operand is the f32 product (o tanh c, resp. dz) rounded ONCE to f16 (v_fma_mixlo_f16), not the stored f32 value rounded
 *     again: where the stored value is an exact f16 midpoint (2^-13 of the elements) the operand may be either neighbour.
 *   - f16-subnormal A/B operands are KEPT by v_mfma_f32_16x16x32_f16 on gfx950 (measured on an MI355X: the kernels match a float64
 *     reference that keeps them to 4e-7 / 2e-7 of max|dxz|, and miss one that flushes them by up to 0.2 of max|dxz|).
 *   - Forward: h, gates and cell states within 2.5e-4 of the f32 entry (what rounding h and U to f16 costs over 46 steps).
 *   - Backward: dz is cast to f16 WITHOUT rescaling, so dH is expected loss-scaled (half.LOSS_SCALE = 1024: max|dH| is 27 .. 270 in
 *     training).  With dH = s x standard normal (max|dH| ~ 4.5 s; float64 reference on the CPU, units 64, T 46), the error of dxz
 *     relative to max|dxz| is 7e-5 .. 1e-4 for s in [1e-3, 3] (the cost of f16 operands alone), 3e-4 at s = 1e-4, 3e-3 at 1e-5,
 *     3e-2 at 1e-6, 0.14 at 1e-7, and for s <= 1e-9 every dz rounds to zero: the recurrent term is lost (back-propagation through
 *     time is silently truncated to one step).  Keep max|dH| >= 4e-3.  There is no saturation either: |dz| > 65504 becomes inf. */
int orcai_h_lstm_train_fwd(const float* xz, const float* Uw, int B, int T, int units, float* out, float* gates, float* cstate, void* stream);
int orcai_h_lstm_bwd(const float* dH, const float* gates, const float* cstate, const float* Uw, int B, int T, int units, float* dxz, void* stream);
/* Backward through time: dH f32[B][T][2*units] (gradient of the layer output) -> dxz f32[B][T][2][4*units] (permuted columns).
 * With orcai_lstm_split(1) the launch rescales dz by a power of two taken from max|dH| (two tiny launches in front of the recurrence); that scale
 * travels through one device global, so at most ONE orcai_lstm_bwd may be in flight per device (calls on one stream are ordered and fine;
 * concurrent calls on two streams of the same device are not supported).  Device-symbol addresses and the > 64 KiB LDS opt-ins are looked up
 * per device on the device's first call, which must not be inside a stream capture.  dz is saturated at 2^15 x the largest incoming gradient
 * before the f16 split: exploding recurrences are clipped, never turned into inf / NaN. */
int orcai_lstm_bwd(const float* dH, const float* gates, const float* cstate, const float* Uw, int B, int T, int units, float* dxz, void* stream);
/* hprev[b][t][dir][u] = h[b][t-1 (dir 0) | t+1 (dir 1)][dir*units + u], 0 at the sequence start: left operand of dU = hprev^T dxz. */
int orcai_lstm_hprev(const float* h, int B, int T, int units, float* hprev, void* stream);

/* conv0 with a selectable ReLU (training forward stores the pre-BatchNorm output: scale = 1, shift = bias, relu = 0). */
int orcai_conv0_affine(const float* in, int64_t snippet_stride, int B, int H, int W, int ksize, const float* w, const float* scale, const float* shift,
                       int relu, float* out, void* stream);

/* ResNet1DConv head, backward (architectures.py:100-115; Keras differentiates these inside model.fit, train.py:201-219):
 * orcai_freq_mean_bwd: dfeat[m][x*C + c] = dfm[m][c] / W (gradient of ReduceFrequencyMean on the Keras Reshape layout).
 * orcai_conv1d_bwd: x [B][T][C], w [K][C][L], dz [B][T][L] = gradient at the pre-sigmoid output; dW [K][C][L] is ACCUMULATED
 * (zero it first), dx [B][T][C] is written.  The bias gradient is the column sum of dz (orcai_colsum). */
int orcai_freq_mean_bwd(const float* dfm, int64_t M, int W, int C, float* dfeat, void* stream);
int orcai_conv1d_bwd(const float* x, const float* w, const float* dz, int B, int T, int C, int K, int L, float* dW, float* dx, void* stream);

/* Training-data path (replaces DataLoader.__getitem__ io.py:128-147 + reshape_labels io.py:101-126 and the
 * materialised tf.data snapshot io.py:187-218).  store: [total_rows][cols] f32 resident in HBM (recordings concatenated along time);
 * row_starts: device int64[B], first store row of each snippet (caller guarantees start + rows <= total_rows).
 * orcai_gather_snippets: out[b] = rows [start_b, start_b + rows) of the store, as [B][rows][cols].
 * orcai_downsample_labels: out[b][s][l] = round_half_even(mean over the `factor` rows of group s); rows % factor != 0 -> BADARG. */
int orcai_gather_snippets(const float* store, const int64_t* row_starts, int B, int rows, int cols, float* out, void* stream);
int orcai_downsample_labels(const float* labels, const int64_t* row_starts, int B, int rows, int L, int factor, float* out, void* stream);

/* ResNet1DConv head (architectures.py:10-15 ReduceFrequencyMean, :107-115 Conv1D(num_labels, kernel_size = 36, "same", sigmoid)).
 * orcai_freq_mean: feat [M][W*C] in the Keras Reshape layout (feature = x*C + c) -> out [M][C] = mean over x.
 * orcai_conv1d_sigmoid: x [B][T][C], w [K][C][L] (Keras Conv1D kernel layout), bias [L] -> out [B][T][L];
 * "same" padding as TensorFlow: (K-1)/2 zero steps before, K/2 after. */
int orcai_freq_mean(const float* feat, int64_t M, int W, int C, float* out, void* stream);
int orcai_conv1d_sigmoid(const float* x, const float* w, const float* bias, int B, int T, int C, int K, int L, float* out, void* stream);

/* orcai_sepconv_bn with the tap size (ktap in {1,3,5,7}) decoupled from the padding of the planes (ksize_planes >= ktap), used by the
 * backward pass: ktap = 1 is a pure pointwise conv (input gradient through the pointwise weights), out_layout 3 scatter-ADDS the
 * result to pixel (2y, 2x) of planes of an H2 x W2 image (input gradient of the stride-2 1x1 residual conv). */
int orcai_sepconv_planes(const float* in, int B, int Cin, int H, int W, int ksize_planes, int ktap, int relu_in, const float* dw, const float* pw,
                         const float* scale, const float* shift, int Cout, int relu_out, int out_layout, int H2, int W2, float* out, void* stream);
/* The same, additionally storing the depthwise output u (planes of Cin channels, u_out may be NULL): the training forward keeps u
 * because the pointwise weight gradient is sum_pixels u (x) dv (architectures.py:176-189 differentiated by Keras inside model.fit). */
int orcai_sepconv_planes_u(const float* in, int B, int Cin, int H, int W, int ksize_planes, int ktap, int relu_in, const float* dw, const float* pw,
                           const float* scale, const float* shift, int Cout, int relu_out, int out_layout, int H2, int W2, float* out, float* u_out,
                           void* stream);

/* BatchNormalization (training) on padded channel-quad planes: batch mean / biased variance (scratch: f64[8*ceil(C/4)*32] for
 * orcai_bn_planes_stats -- 32 accumulator copies for its small-plane pass --, f64[8*ceil(C/4)] for the other entry points),
 * y = [relu](v*s + t) at interior pixels, backward (dbeta, dgamma, dv) with the optional ReLU folded in. */
int orcai_bn_planes_stats(const float* v, int B, int C, int H, int W, int ksize, double* scratch, float* mean, float* var, void* stream);

/* Training forward of a k = 3 separable convolution with the BatchNorm batch statistics of its output reduced in the kernel's epilogue
 * (train.py:155-219 runs keras' SeparableConv2D -> BatchNormalization(training=True)): = orcai_sepconv_planes_u(ksize_planes = ktap = 3,
 * relu_out = 0, out_layout = 0) followed by the sums of orcai_bn_planes_stats, without the read pass over `out`.
 *   shards   f64[32][ceil(Cout/4)][8] accumulator copies (zeroed here); orcai_bn_finish_sharded turns them into mean / biased variance
 * Only the shapes the LDS-tile kernels take (orcai_sepconv_route(0, ..., 0, 2) != 0; sep_route.h states the rule): ORCAI_E_UNSUPPORTED
 * otherwise, with nothing touched, and the caller runs the two calls above.  Per-workgroup partial sums are f32 (512 pixels), accumulated
 * in f64. */
int orcai_sepconv_planes_stats(const float* in, int B, int Cin, int H, int W, int relu_in, const float* dw, const float* pw, const float* scale, const float* shift,
                               int Cout, float* out, float* u_out, double* shards, void* stream);
/* orcai_sepconv_planes_stats whose input planes hold the PRE-normalisation tensor v of the BatchNorm (+ ReLU) in front of the conv
 * (architectures.py:176-183: bn_a + ReLU feed the second separable conv of a block): y = max(fma(v, gamma * inv, beta - mean * gamma * inv), 0)
 * is formed on load -- the arithmetic of orcai_bn_planes_apply, bit for bit -- and zero outside the image, so the normalised tensor is never
 * written or re-read.  Same refusal rule (ORCAI_E_UNSUPPORTED before anything is touched). */
int orcai_sepconv_planes_stats_bn(const float* v_in, int B, int Cin, int H, int W, const float* in_mean, const float* in_var, const float* in_gamma, const float* in_beta,
                                  float in_eps, const float* dw, const float* pw, const float* scale, const float* shift, int Cout, float* out, float* u_out, double* shards,
                                  void* stream);
/* The input-gradient pass of a k = 3 separable conv (flipped depthwise taps, identity pointwise factor, plane output) with an epilogue that
 * reads a reference tensor `ref` of the OUTPUT's layout where it stores (train.py:201-219: inside Keras' backward):
 *   epi 2: the output is the gradient dy of a BatchNorm whose pre-normalisation input is ref: the BatchNorm backward sums
 *          dbeta = sum g, dgamma = sum g * xhat (g = relu ? dy * [gamma * xhat + beta > 0] : dy) are reduced where dy is stored and left in
 *          `shards` as scratch2C = dbeta[4 CQo] | dgamma[4 CQo] doubles (shards: 32 * 8 * CQo doubles of workspace): the next
 *          orcai_bn_bwd_pointwise(_wgrad) call takes sums_ready = 1 and the read pass over (dy, v) is gone;
 *   epi 3: out = ref > 0 ? out : 0 (the ReLU in front of the conv, folded: no separate orcai_planes_relu_bwd pass).
 * ORCAI_E_UNSUPPORTED (before anything is touched) for shapes the LDS-tile kernels do not take (orcai_sepconv_route(0, ..., 0, 2 + epi)
 * == 0): the caller runs the separate passes. */
int orcai_sepconv_planes_epi(const float* in, int B, int Cin, int H, int W, const float* dw, const float* pw, const float* scale, const float* shift, int Cout, float* out,
                             int epi, const float* ref, const float* mean, const float* var, const float* gamma, const float* beta, float eps, int relu, double* shards,
                             void* stream);
int orcai_bn_finish_sharded(const double* shards, int B, int C, int H, int W, float* mean, float* var, void* stream);
/* The f16 twins (octet planes; shards f64[32][ceil(Cout/8)][16]; flat-tile kernel, any plane width and channel count it handles; the sums are
 * taken on the f32 values before their rounding to f16). */
int orcai_h_sepconv_stats(const void* in, int B, int Cin, int H, int W, int relu_in, const void* dw, const void* pwf, const float* scale, const float* shift, int Cout,
                          void* out, void* u_out, double* shards, void* stream);
/* orcai_h_sepconv_stats whose input planes hold the PRE-normalisation tensor v of a BatchNorm + ReLU (the f16 twin of orcai_sepconv_planes_stats_bn):
 * y = f16(relu(fma(v, gamma * rsqrt(var + eps), beta - mean * ...))) is formed on load -- the value orcai_h_bn_planes_apply stores, bit for bit -- and zero
 * outside the image, so the training forward never materialises y_a (architectures.py:172-189 in training mode). */
int orcai_h_sepconv_stats_bn(const void* v_in, int B, int Cin, int H, int W, const float* in_mean, const float* in_var, const float* in_gamma, const float* in_beta,
                             float in_eps, const void* dw, const void* pwf, const float* scale, const float* shift, int Cout, void* out, void* u_out, double* shards,
                             void* stream);
int orcai_h_bn_finish_sharded(const double* shards, int B, int C, int H, int W, float* mean, float* var, void* stream);
int orcai_bn_planes_apply(const float* v, int B, int C, int H, int W, int ksize, const float* mean, const float* var, const float* gamma, const float* beta,
                          float eps, int relu, float* y, void* stream);
int orcai_bn_planes_bwd(const float* dy, const float* v, int B, int C, int H, int W, int ksize, const float* mean, const float* var, const float* gamma,
                        const float* beta, float eps, int relu, double* scratch, float* dbeta, float* dgamma, float* dv, void* stream);
/* Kernel-layout copies of trunk weights from the flat parameter buffer in one launch: desc = n_desc x {type, src offset, dst offset,
 * C, aux} (device int32): type 0 depthwise (k,k,C,1) -> [ceil(C/4)][k*k][4] (aux = k*k), type 1 the same with reversed taps,
 * type 2 pointwise (1,1,C,aux) -> transposed [aux][C]. */
int orcai_pack_weights(const float* w, const int* desc, int n_desc, float* out, void* stream);
/* Backward of the entry block Conv2D(16) -> BatchNormalization -> ReLU (architectures.py:162-168): dbeta / dgamma of bn0 and the
 * conv weight gradient dW0[tap][16] (accumulated) from dy = gradient at the ReLU output and v = pre-BN conv output.  The BN input
 * gradient is formed on the fly and never written (the entry conv has no input gradient). */
int orcai_conv0_bn_bwd(const float* in, int64_t snippet_stride, const float* dy, const float* v, int B, int H, int W, int ksize, const float* mean,
                       const float* var, const float* gamma, const float* beta, float eps, double* scratch, float* dbeta, float* dgamma, float* dW,
                       void* stream);
/* The entry conv + bn0 of the training forward WITHOUT the pre-normalisation tensor v0 in HBM (architectures.py:164-168; train.py:201-219):
 *   orcai_conv0_stats     first pass: v0 = fma(conv, scale, shift) is formed as orcai_conv0_affine forms it, only its batch statistics leave
 *                         the kernel (shards: 32 * 4 * 8 doubles, the layout orcai_bn_finish_sharded(C = 16) reads);
 *   orcai_conv0_affine_bn second pass: the conv recomputed from the 1-channel input, then y0 = [relu](fma(v0, gamma * inv, beta - mean * gamma * inv))
 *                         -- the two roundings of orcai_conv0_affine + orcai_bn_planes_apply, so y0 is bit for bit what those launches wrote;
 *   orcai_conv0_bn_bwd_x  orcai_conv0_bn_bwd with v0 rebuilt per pixel from the input taps (w0 [k*k][16], bias [16]) instead of read; dW accumulates. */
int orcai_conv0_stats(const float* in, int64_t snippet_stride, int B, int H, int W, int ksize, const float* w, const float* scale, const float* shift, double* shards,
                      void* stream);
int orcai_conv0_affine_bn(const float* in, int64_t snippet_stride, int B, int H, int W, int ksize, const float* w, const float* scale, const float* shift,
                          const float* bn_mean, const float* bn_var, const float* bn_gamma, const float* bn_beta, float bn_eps, int relu, float* out, void* stream);
int orcai_conv0_bn_bwd_x(const float* in, int64_t snippet_stride, const float* dy, int B, int H, int W, int ksize, const float* w0, const float* bias, const float* mean,
                         const float* var, const float* gamma, const float* beta, float eps, double* scratch2C /*>= 1024 doubles*/, float* dbeta, float* dgamma, float* dW,
                         float* workspace /*per-workgroup partial weight gradients*/, int64_t workspace_floats, void* stream);
/* Training forward / backward of the pooling with the BatchNormalization in front of it applied on the fly (architectures.py:
 * 189-196): `s` / `ybn` hold the PRE-BN tensor v; BN(v) = fma(v, gamma*rsqrt(var+eps), beta - mean*that) is monotone per channel,
 * so the maximum (and its position) is taken on v and transformed once.  BN(v) is never materialised. */
int orcai_pool_res_add_bn(const float* s, const float* prev, int B, int C, int Cp, int H, int W, int ksize, const float* wr, const float* br, float* out,
                          int xpooled, const float* bn_mean, const float* bn_var, const float* bn_gamma, const float* bn_beta, float bn_eps, void* stream);
/* bn_sums != NULL (device f64[8*ceil(C/4)], zeroed by the call): additionally accumulates sum dy and sum dy*xhat per channel, the two
 * reductions of that BatchNorm's backward, so orcai_bn_bwd_pointwise(sums_ready = 1) need not read dy and v for them. */
int orcai_pool_bwd_bn(const float* dout, const float* v, int B, int C, int H, int W, int ksize, float* dy, const float* bn_gamma, const float* bn_mean,
                      const float* bn_var, float bn_eps, double* bn_sums, void* stream);
/* orcai_pool_bwd_bn that also reduces dbias[c] = sum over snippets and pixels of dout[c] -- the bias gradient of the block's residual 1x1
 * convolution, whose output gradient dout is (architectures.py:190-196) -- where the pooling backward reads every dout value exactly once;
 * dout_sums: 4 * ceil(C/4) doubles of workspace.  Replaces an orcai_planes_sum pass over dout. */
int orcai_pool_bwd_bn_bias(const float* dout, const float* ybn, int B, int C, int H, int W, int ksize, float* dy, const float* bn_gamma, const float* bn_mean,
                           const float* bn_var, float bn_eps, double* bn_sums, double* dout_sums, float* dbias, void* stream);
/* orcai_bn_planes_bwd fused with the input gradient through the pointwise weights of the separable conv that produced v:
 * dbeta / dgamma as above, dv (may alias dy) = BN input gradient, du = Wpw dv with wt = pointwise^T [C][Cin] (planes of Cin
 * channels).  One pass over dy and v instead of bn apply + a pointwise conv pass that re-reads dv. */
int orcai_bn_bwd_pointwise(const float* dy, const float* v, int B, int C, int H, int W, int ksize, const float* mean, const float* var, const float* gamma,
                           const float* beta, float eps, int relu, double* scratch, int sums_ready, float* dbeta, float* dgamma, const float* wt, int Cin,
                           float* dv, float* du, void* stream);
/* orcai_bn_bwd_pointwise + the pointwise weight gradient of the same separable conv in ONE pass (train.py:201-219 computes these inside Keras):
 * dv is formed per pixel, multiplied by the transposed pointwise weights (du) AND contracted with the depthwise output u of the forward
 * pass (dWpw[ci][co] += sum_pixels u[ci] dv[co]); dv itself is never written.  workspace: per-wave partial products
 * (>= 4 * Cin * C floats per workgroup).  ORCAI_E_UNSUPPORTED (before anything is touched) when ceil(Cin/16) + ceil(C/16) > 6: the caller
 * then runs orcai_bn_bwd_pointwise and orcai_outer_reduce. */
int orcai_pw_wgrad_tiles(int tiles); /* experiments: widest layer (in 16-channel tiles, both operands) the fused entry accepts, 0 = never; < 0 queries; returns the previous value */
int orcai_bn_bwd_pointwise_wgrad(const float* dy, const float* v, const float* u, int B, int C, int H, int W, int ksize, const float* mean, const float* var,
                                 const float* gamma, const float* beta, float eps, int relu, double* scratch2C, int sums_ready, float* dbeta, float* dgamma,
                                 const float* wt, int Cin, float* du, float* dWpw, float* workspace, int64_t workspace_floats, void* stream);
/* out[c] (=|+=) sum over snippets and pixels of x[c] (bias gradients); scratch: f64[4*ceil(C/4)] */
int orcai_planes_sum(const float* x, int B, int C, int H, int W, int ksize, double* scratch, float* out, int accumulate, void* stream);
/* gradient of MaxPooling2D((3,2), 2, "same"): dy[y][x] = sum of dout over the windows whose maximum is ybn[y][x] */
int orcai_pool_bwd(const float* dout, const float* ybn, int B, int C, int H, int W, int ksize, float* dy, void* stream);
/* D[ca][cb] += sum over snippets and pixels of A[ca][p] * Bq[cb][p] (pointwise / residual weight gradients); with a_stride2 the A planes
 * are an Ha x Wa image sampled at (2i, 2j) for pixel (i, j) of the H x W image of Bq.  workspace: device scratch for the per-workgroup
 * partial products (up to 512 * Ca * Cb floats are used; fewer workgroups run if it is smaller). */
int orcai_outer_reduce(const float* A, int Ca, const float* Bq, int Cb, int B, int H, int W, int ksize, int a_stride2, int Ha, int Wa, float* D,
                       float* workspace, int64_t workspace_floats, void* stream);
/* dW[tap][c] += sum r[c][p + off(tap)] * du[c][p], r = relu_in ? relu(x) : x  (depthwise weight gradient, written in the Keras
 * kernel layout (k, k, C, 1), i.e. straight into the flat gradient buffer) */
int orcai_dw_wgrad(const float* x, const float* du, int B, int C, int H, int W, int ksize_planes, int ktap, int relu_in, float* dW, void* stream);
int orcai_dw_wgrad_march(int on); /* experiments: 1 (default) = k = 3 launches on planes >= 100 pixels wide run the row-marching kernel (every byte requested once); 0 = the flat-window kernel everywhere; < 0 queries; returns the previous value */
/* the same (k = 3) with r = the BatchNorm + ReLU of the pre-normalisation tensor v, formed on load (see orcai_sepconv_planes_stats_bn) */
int orcai_dw_wgrad_bn(const float* v, const float* du, int B, int C, int H, int W, const float* in_mean, const float* in_var, const float* in_gamma, const float* in_beta,
                      float in_eps, float* dW, void* stream);
/* Depthwise backward of a k = 3 separable conv in ONE pass over (du, x) (replaces orcai_sepconv_planes_epi + orcai_dw_wgrad[_bn]; Keras: the
 * DepthwiseConv2D half of SeparableConv2D's gradient, reference architectures.py:66-86 trained by train.py:201-219):
 *   dr = du (*) reversed depthwise taps (dw_rev: [ceil(C/4)][9][4], tap t = forward tap 8 - t)    -- the gradient w.r.t. the conv's input
 *   dW[tap][c] += sum_p r[c][p + off(tap)] * du[c][p]                                              -- as orcai_dw_wgrad (Keras layout (3, 3, C, 1))
 * with r = relu_in ? relu(x) : x, or, when bn_mean != NULL, r = relu(BatchNorm(x)) formed on load (x = pre-normalisation tensor, as
 * orcai_dw_wgrad_bn).  epi 0: nothing else.  epi 2 (needs the BatchNorm arguments): dr is the gradient of that BatchNorm's output; its backward
 * sums sum g | sum g * xhat (g = dr gated by the ReLU when bn_relu) are left in `shards` as dbeta[4 CQ] | dgamma[4 CQ] doubles (>= 8 * CQ * 32
 * doubles of scratch) for orcai_bn_bwd_pointwise[_wgrad](sums_ready = 1).  epi 3 (relu_in = 1, no BatchNorm): dr is masked by x > 0.  Only the
 * interior of dr is written.  ORCAI_E_UNSUPPORTED (nothing touched): C > 64, misaligned planes. */
int orcai_dw_bwd_fused(const float* x, const float* du, int B, int C, int H, int W, int relu_in, const float* dw_rev, float* dr, float* dW, int epi, const float* bn_mean,
                       const float* bn_var, const float* bn_gamma, const float* bn_beta, float bn_eps, int bn_relu, double* shards, void* stream);
/* orcai_dw_bwd_fused(epi 2) for block 1's first separable conv when the training forward did not keep the entry conv's pre-normalisation tensor
 * (orcai_conv0_stats + orcai_conv0_affine_bn): the conv input y0 = relu(bn0(conv0(snippet))) is rebuilt per pixel from the snippet's nine taps
 * (w0 [9][16], bias0 [16], bn0's batch statistics) instead of read, and the sums left in `shards` (dbeta[16] | dgamma[16] doubles; >= 32 * 32 doubles
 * of scratch) are bn0's backward sums over dr -- what the first pass of orcai_conv0_bn_bwd_x computes; orcai_conv0_bn_bwd_x_ready is that entry
 * point without its first pass.  resq (optional): the residual branch's gradient w.r.t. y0 at the even pixels (2i, 2j) as planes of 16 channels at
 * the pooled resolution [B][4][ceil(H/2) + 2][padded_width(ceil(W/2))][4] (a plain pointwise pass W_res^T dout): added to dr -- and so part of bn0's
 * sums -- instead of a scatter-add pass over dr afterwards.  k = 3 planes. */
int orcai_dw_bwd_fused_conv0(const float* in, int64_t snippet_stride, const float* du, int B, int H, int W, const float* w0, const float* bias0, const float* dw_rev, float* dr,
                             float* dW, const float* bn_mean, const float* bn_var, const float* bn_gamma, const float* bn_beta, float bn_eps, double* shards, const float* resq,
                             void* stream);
int orcai_conv0_bn_bwd_x_ready(const float* in, int64_t snippet_stride, const float* dy, int B, int H, int W, int ksize, const float* w0, const float* bias, const float* mean,
                               const float* var, const float* gamma, const float* beta, float eps, double* scratch2C, float* dbeta, float* dgamma, float* dW, float* workspace,
                               int64_t workspace_floats, void* stream);
/* Input gradient of Conv2D(16, k, same) -> BatchNormalization (batch statistics) -> ReLU  (architectures.py:164-168; Keras forms it whenever
 * something differentiable sits in front of the model, train.py:201-219 never asks for it):
 *   v0 = conv(in) + bias, xh = (v0 - mean) * rsqrt(var + eps), g = dy where fma(xh, gamma, beta) > 0 else 0,
 *   dv = gamma * rsqrt(var + eps) * (g - dbeta / N - xh * dgamma / N),   N = B * H * W,
 *   dx[b][p] = sum over taps t, channels c of w0[t][c] * dv[c][p - off(t)]   (dv = 0 outside the image).
 * v0, xh, the ReLU decision and dv are formed as orcai_conv0_bn_bwd_x[_ready] forms them, so the dv behind dx is the dv behind dW0.
 * sums2C: dbeta[16] | dgamma[16] as doubles, as orcai_conv0_bn_bwd_x / orcai_dw_bwd_fused_conv0 leave them in scratch2C (still there after
 * orcai_conv0_bn_bwd_x[_ready]).  dy: padded channel-quad planes [B][4][H + 2R][WP][4], 16-byte aligned; only its interior is read.
 * dx: f32 [B][H][W], dense (its own stride H * W whatever snippet_stride is), every element written, nothing accumulated; no atomics, so dx is
 * bit-reproducible.  k = 3: a marching kernel without LDS (csrc/train_trunk.hip conv0_dx_march_kernel); k = 5, 7: LDS tiles.
 * ORCAI_E_BADARG: ksize not in {3, 5, 7}, non-positive sizes, null or misaligned pointers. */
int orcai_conv0_bn_bwd_dx(const float* in, int64_t snippet_stride, const float* dy, int B, int H, int W, int ksize, const float* w0, const float* bias, const float* mean,
                          const float* var, const float* gamma, const float* beta, float eps, const double* sums2C, float* dx, void* stream);
/* The entry conv's two reduction passes on a marching kernel (k = 3; csrc/train_trunk.hip conv0_march_kernel): orcai_conv0_stats_march is
 * orcai_conv0_stats (shards: [32][4][8] sums | sums of squares for orcai_bn_finish_sharded) without tiles, LDS or barriers; orcai_conv0_march(1)
 * (default) lets orcai_conv0_bn_bwd_x_ready run its weight-gradient pass the same way (0: the tile kernel; < 0 queries; returns the previous value). */
int orcai_conv0_stats_march(const float* in, int64_t snippet_stride, int B, int H, int W, const float* w, const float* scale, const float* shift, double* shards, void* stream);
int orcai_conv0_march(int on);
/* dW0[tap][c] += sum in[p + off(tap)] * dv[c][p]  (entry conv weight gradient; `in` is the unpadded snippet view) */
int orcai_conv0_wgrad(const float* in, int64_t snippet_stride, const float* dv, int B, int H, int W, int ksize, float* dW, void* stream);
/* Keras-Reshape layout f32[B][H][W*C] -> padded channel-quad planes (gradient entering the final separable conv) */
int orcai_feat_to_planes(const float* f, int B, int C, int H, int W, int ksize, float* out, void* stream);
/* dx = (y > 0) ? dy : 0 on whole plane buffers (n_floats % 4 == 0) */
int orcai_planes_relu_bwd(const float* dy, const float* y, int64_t n_floats, float* dx, void* stream);

/* Step state in DEVICE memory, so that a whole training step can be captured into a hipGraph and replayed (kernel arguments are baked
 * into a captured graph; what changes from step to step must be read from memory):
 *   counter          uint64[1], the number of optimisation steps applied so far; orcai_counter_advance adds 1 at the end of a step;
 *   orcai_dropout_mask_dev   as orcai_dropout_mask with seed = seed_add + counter[0] * 0xD1B54A32D192ED03;
 *   orcai_adam_step_dev      as orcai_adam_step with step = counter[0] + 1 and the learning rate lr[0] (callbacks change it between steps). */
int orcai_dropout_mask_dev(float* mask, int64_t n, const uint64_t* counter, uint64_t seed_add, float keep, void* stream);
int orcai_adam_step_dev(float* w, const float* g, float* m, float* v, int64_t n, const float* lr, float b1, float b2, float eps, const uint64_t* counter, float gscale,
                        void* stream);
int orcai_counter_advance(uint64_t* counter, void* stream);
/* One clear per training step for every reduction scratch buffer: orcai_scratch_arena zeroes `bytes` (rounded down to 32-KiB slots, at most 1024) at `base`
 * with ONE launch on `stream` and registers the range; until the next call, a launcher whose accumulator argument (the `scratch*` / `shards` pointers of the
 * BatchNorm, pooling and weight-gradient entry points) lies inside a slot that no launcher has taken since skips its own zero-fill launch.  Any other pointer,
 * a slot handed to a second launcher, or no registered arena: the launcher clears its accumulator itself, as before.  The caller hands every accumulating
 * launcher of a step its own slot (orcai_amd/training.py: TrunkTrainer._fresh); base = NULL unregisters.  Host-side state: one stream, one step at a time.
 * orcai_arena_take is the query the launchers use (1 = skip the fill; marks the slot taken). */
int orcai_scratch_arena(void* base, size_t bytes, void* stream);

/* Measurement hook (bench.py): the next call of orcai_bn_bwd_pointwise_wgrad / orcai_h_bn_bwd_pointwise_wgrad records the two HIP events (hipEvent_t handles)
 * on its stream around its MAIN kernel only -- the launcher enqueues two small kernels after it (partial-sum fold, f64 -> f32 gradients), so an event pair
 * around the whole call reads ~35 us above the kernel duration rocprofv3 --kernel-trace lists.  The registration is consumed by that call; NULLs clear it.
 * Host-side state, one thread. */
int orcai_profile_bracket(void* ev_start, void* ev_stop);
/* the events for it, for callers without a HIP binding of their own: timing enabled; elapsed needs both events completed */
int orcai_event_create(void** ev);
int orcai_event_elapsed_ms(void* ev_start, void* ev_stop, float* ms);
int orcai_event_destroy(void* ev);
int orcai_arena_take(const void* p, size_t bytes);

/* A voided step (the f16 path under its static loss scale: Keras' LossScaleOptimizer skips the update when a gradient is not finite).
 *   orcai_step_ok: ok[0] = 1 if every value of g[0, ng) and stats[0, ns) (this step's BatchNorm batch statistics; ns may be 0) is
 *   finite, else 0, and skipped[0] += 1; nothing returns to the host, so the decision stays inside a captured graph.
 *   The *_guarded twins do nothing when ok[0] == 0: weights, Adam moments, moving statistics and the step counter keep their values. */
int orcai_step_ok(const float* g, int64_t ng, const float* stats, int64_t ns, int32_t* ok, int64_t* skipped, void* stream);
/* Data parallel replicas must reach the SAME verdict (the reference's MirroredStrategy applies or skips an update on all replicas together,
 * hpsearch.py:186-205): before the gradient all-reduce, g[0] = NaN when any of this rank's stats[0, ns) is not finite -- the summed bucket is then
 * non-finite on every rank and each rank's orcai_step_ok voids the step.  Nothing is written when all statistics are finite. */
int orcai_poison_if_nonfinite(const float* stats, int64_t ns, float* g, void* stream);
int orcai_adam_step_guarded(float* w, const float* g, float* m, float* v, int64_t n, const float* lr, float b1, float b2, float eps, const uint64_t* counter,
                            float gscale, const int32_t* ok, void* stream);
int orcai_ema_update_guarded(float* moving, const float* batch, int n, float momentum, const int32_t* ok, void* stream);
int orcai_counter_advance_guarded(uint64_t* counter, const int32_t* ok, void* stream);

/* Keras LSTM variables <-> the gate-column order of the recurrence kernels (orcai_lstm_recurrent), on the device, once per training
 * step (replaces the per-step framework index / cat / stack kernels; architectures.py:210-229 define the variables).
 * orcai_pack_lstm: desc int32[n_desc][7] = {src offset in w (floats), dst offset (elements), rows, units, ld_dst, col_off, mode};
 *   mode 0: out32[dst + r*ld_dst + col_off + p] = w[src + r*4u + perm(p)];  mode 1: out16[dst + (col_off + p)*ld_dst + r] = (f16) the same
 *   (transposed, zero-padded copy for orcai_h_gemm_bias_act).  perm(p), p = 32w + 16nt + j: Keras column (2nt + (j>>3))*u + 8w + (j&7).
 * orcai_unpack_lstm_grad: G[r*4u + perm(p)] = src[r*ld_src + col_off + p] + l2g * W[r*4u + perm(p)]   (W may be NULL).
 * orcai_ema_update: moving = moving*momentum + batch*(1 - momentum)  (BatchNormalization moving statistics, one flat buffer). */
int orcai_pack_lstm(const float* w, const int* desc, int n_desc, float* out32, void* out16, void* stream);
int orcai_unpack_lstm_grad(const float* src, int ld_src, int col_off, int rows, int units, float* G, const float* W, float l2g, void* stream);
/* The same for up to 16 (source, destination) pairs in ONE launch -- the 12 of both BiLSTM layers of a training step -- and the value of the L2 penalty over up
 * to 8 slices of the flat weight buffer in one launch (train.py:201-219: kernel_regularizer=l2(0.001) on the LSTM input kernels and Dense-128).  `descs_host`,
 * `off_host`, `n_host` are HOST arrays, read during the call (the descriptors travel by value in the kernel arguments: nothing to keep alive, capturable). */
typedef struct {
  const float* src; /* kernel-order gradient [rows][ld_src] */
  int ld_src, col_off, rows;
  float* G;         /* Keras-layout destination [rows][4 * units] */
  const float* W;   /* Keras-layout weights for the L2 term, or NULL */
  float l2g;
} orcai_unpack_desc;
int orcai_unpack_lstm_grads(const orcai_unpack_desc* descs_host, int n, int units, void* stream);
int orcai_l2_values(const float* base, const int64_t* off_host, const int64_t* n_host, int count, float lambda, double* out, void* stream);
int orcai_ema_update(float* moving, const float* batch, int n, float momentum, void* stream);

/* ------------------------------------------------------------------------------------------
 * f16 path (BASELINE configs[4]: the hyper-parameter sweep's width variants on f16 MFMA; hpsearch.py:186-205 x
 * defaults/default_hps_parameter.json:2-25).  Activations are f16 channel-OCTET planes
 *   [snippet][CO = ceil(C/8)][H + 2R][orcai_padded_width(W, k)][8]   (zero pads, written once by the host),
 * contractions run on v_mfma_f32_16x16x32_f16 with f32 accumulation; weights are f16 COPIES of the f32 master weights in these
 * layouts (orcai_amd/half.py packs them on the host, orcai_h_pack_weights on the device once per training step):
 *   depthwise taps      f16[CO][k*k][8]                      element (o, tap, e) = Keras depthwise kernel [tap/k][tap%k][8o+e][0]
 *   A fragments of W    f16[KG = ceil(Cin/32)][MT = ceil(Cout/16)][64][8]
 *                       element (kg, m, lane, e) = W[cin = 32kg + 8(lane>>4) + e][cout = 16m + (lane&15)], 0 outside W[Cin][Cout]
 *   transposed dense    f16 Wt[N][roundup32(K)] of W[K][N]
 * Pointers to f16 data are void*.  Same conventions as above (device pointers, caller-owned, stream-ordered, capturable).
 * ------------------------------------------------------------------------------------------ */

/* Conv2D(16, k, same)(f32 snippet) * scale + shift [ReLU] -> f16 octet planes of 16 channels (architectures.py:164-168);
 * arguments as orcai_conv0_affine. */
int orcai_h_conv0_affine(const float* in, int64_t snippet_stride, int B, int H, int W, int ksize, const float* w, const float* scale, const float* shift, int relu,
                         void* out, void* stream);
/* The same with the entry BatchNorm + ReLU in the same pass (training forward): v_out = the pre-normalisation conv (as orcai_h_conv0_affine with relu = 0),
 * y_out = relu(BatchNorm(v_out)) formed from the f16 value just stored -- bit-identical to orcai_h_conv0_affine + orcai_h_bn_planes_apply(relu = 1) -- with the
 * batch statistics the caller took from the snippet (orcai_conv0_stats_march + orcai_bn_finish_sharded; architectures.py:164-168). */
int orcai_h_conv0_affine_bn(const float* in, int64_t snippet_stride, int B, int H, int W, int ksize, const float* w, const float* scale, const float* shift,
                            const float* bn_mean, const float* bn_var, const float* bn_gamma, const float* bn_beta, float bn_eps, void* v_out, void* y_out, void* stream);

/* [ReLU] -> depthwise ktap x ktap -> pointwise -> * scale + shift -> [ReLU] on f16 octet planes padded for ksize_planes
 * (architectures.py:174-189, 198-206): orcai_sepconv_planes_u of the f32 path.  out_layout 0: f16 octet planes; 1: f32
 * [B][H][W*Cout] Keras Reshape layout; 2: x-pooled f16 [B][CO][H][roundup4(ceil(W/2))][8]; 3: scatter-add into pixel (2y, 2x) of
 * f16 planes of an (H2, W2) image.  u_out (may be NULL): the depthwise output, f16 octet planes of Cin channels.  Cin, Cout <= 64. */
int orcai_h_sepconv(const void* in, int B, int Cin, int H, int W, int ksize_planes, int ktap, int relu_in, const void* dw, const void* pwf, const float* scale,
                    const float* shift, int Cout, int relu_out, int out_layout, int H2, int W2, void* out, void* u_out, void* stream);

/* MaxPooling2D((3,2), 2, "same")(s) + Conv2D(C, 1, strides 2)(prev) + bias (architectures.py:190-196) on f16 octet planes.
 * xpooled 1: s is the x-pooled tensor of orcai_h_sepconv(out_layout 2); 0: s are planes.  bn_mean..bn_beta (NULL, or all four with
 * xpooled 0): s is the pre-BatchNorm tensor and the pooling runs on BN(s) without materialising it (training forward). */
int orcai_h_pool_res_add(const void* s, const void* prev, int B, int C, int Cp, int H, int W, int ksize, const void* wrf, const float* br, void* out, int xpooled,
                         const float* bn_mean, const float* bn_var, const float* bn_gamma, const float* bn_beta, float bn_eps, void* stream);

/* orcai_h_pool_res_add(xpooled = 1, no BatchNorm) over B windows of one recording, every output row stored into the per-snippet planes that hold
 * it: the f16 twin of orcai_pool_res_add_scatter, with its row semantics (window b's output row r is recording row base + b * img_step + r; stored
 * for r_lo <= r < r_hi, also r < r_lo for a window starting at recording row 0, into rows keep_lo <= y < keep_hi of snippets 0 <= k < nsnip).
 *   out f16[nsnip][ceil(C/8)][Hd + 2*(k/2)][orcai_padded_width(ceil(W/2), k)][8] octet planes (pads untouched), Hd = 2 * period.
 * Bit for bit the values orcai_h_pool_res_add stores for the same window (one kernel body).  ORCAI_E_UNSUPPORTED, before anything is launched: a shape
 * orcai_h_pool_res_add does not take on its x-pooled path (C or Cp > 64, k not 3 / 5 / 7), keep_hi - keep_lo > 2 * period, more than 65535 windows,
 * or a plane / recording-row offset past the kernel's 32-bit indices.  ORCAI_E_BADARG: null or misaligned pointers, non-positive sizes. */
int orcai_h_pool_res_add_scatter(const void* s, const void* prev, int B, int C, int Cp, int H, int W, int ksize, const void* wrf, const float* br, void* out, int Hd,
                                 int nsnip, int period, int base, int img_step, int r_lo, int r_hi, int keep_lo, int keep_hi, void* stream);
/* The same with up to ORCAI_ROW_FAMILIES destination families (orcai_pool_res_add_scatter_families): recording row R goes to row
 * y = R - offset - j * period of image j of every family, 0 <= j < count, keep_lo <= y < keep_hi; out f16[count][ceil(C/8)][Hd + 2*(k/2)][...][8].
 * `fams` is a HOST array, read during the call.  Also ORCAI_E_UNSUPPORTED: more than ORCAI_ROW_FAMILIES families, or a family with
 * keep_hi - keep_lo > 2 * period (a row in more than two of its images). */
typedef struct {
  void* out;
  int Hd, period, offset, count, keep_lo, keep_hi;
} orcai_h_row_family;
int orcai_h_pool_res_add_scatter_families(const void* s, const void* prev, int B, int C, int Cp, int H, int W, int ksize, const void* wrf, const float* br, int base,
                                          int img_step, int r_lo, int r_hi, const orcai_h_row_family* fams /* host */, int n_fams, void* stream);

/* C[M][N] = act(A[M][K] Wt^T + bias) [* scale + shift]: A f32 (converted to f16 on load), Wt f16[N][roundup32(K)], f32 accumulate and
 * output; act 1 = ReLU.  LSTM input projections and Dense-128 (architectures.py:210-237).  K % 4 == 0. */
int orcai_h_gemm_bias_act(const float* A, const void* Wt, const float* bias, const float* scale, const float* shift, float* C, int64_t M, int N, int K, int act,
                          void* stream);

/* f16 path, training: the twins of the f32 training-trunk entry points on f16 octet planes.  Argument lists are IDENTICAL to
 * orcai_bn_planes_stats, orcai_planes_sum, orcai_bn_planes_apply, orcai_bn_bwd_pointwise, orcai_pool_bwd_bn, orcai_outer_reduce,
 * orcai_dw_wgrad, orcai_conv0_bn_bwd, orcai_pack_weights, orcai_feat_to_planes, orcai_planes_relu_bwd (see those for the arithmetic and
 * the reference lines); plane tensors are f16 octet planes, statistics / weight gradients / scratch stay f32 / f64, and matrix operands
 * are f16 A fragments: wtf of orcai_h_bn_bwd_pointwise = fragments of the TRANSPOSED pointwise matrix (row = conv-input channel,
 * k = conv-output channel).  Gradient planes carry the caller's static loss scale; nothing here knows its value.
 * scratch2C: f64[16 * ceil(C/8)] (orcai_h_bn_planes_stats: x 32 accumulator copies).  orcai_h_planes_relu_bwd counts f16 elements (a multiple of 8).
 * orcai_h_pack_weights descriptors {type, src offset (floats), dst offset (halves), C, aux}: 0 / 1 depthwise octets forward / reversed
 * (aux = k*k), 2 A fragments of W[C][aux], 3 A fragments of its transpose, 4 identity fragments of C channels, 5 all-ones taps. */
int orcai_h_bn_planes_stats(const void* v, int B, int C, int H, int W, int ksize, double* scratch2C, float* mean, float* var, void* stream);
int orcai_h_planes_sum(const void* x, int B, int C, int H, int W, int ksize, double* scratchC, float* out, int accumulate, void* stream);
int orcai_h_bn_planes_apply(const void* v, int B, int C, int H, int W, int ksize, const float* mean, const float* var, const float* gamma, const float* beta,
                            float eps, int relu, void* y, void* stream);
int orcai_h_bn_bwd_pointwise(const void* dy, const void* v, int B, int C, int H, int W, int ksize, const float* mean, const float* var, const float* gamma,
                             const float* beta, float eps, int relu, double* scratch2C, int sums_ready, float* dbeta, float* dgamma, const void* wtf, int Cin,
                             void* dv, void* du, void* stream);
/* orcai_h_bn_bwd_pointwise + orcai_h_outer_reduce(u, dv) in one pass (f16 twin of orcai_bn_bwd_pointwise_wgrad; train.py:201-219): dv is formed per pixel,
 * rounded to f16 as the two-launch path stores it, used for du = Wpw dv AND for the pointwise weight gradient dWpw[Cin][C] += sum_pixels u (x) dv, and never
 * written.  u: the conv's stored depthwise output (octet planes of Cin channels); workspace: per-workgroup partial products (>= Cin * C floats; more = more
 * workgroups, up to 1024).  ORCAI_E_UNSUPPORTED (nothing touched) beyond 32 channels on either side: the caller runs the two launches. */
int orcai_h_bn_bwd_pointwise_wgrad(const void* dy, const void* v, const void* u, int B, int C, int H, int W, int ksize, const float* mean, const float* var,
                                   const float* gamma, const float* beta, float eps, int relu, double* scratch2C, int sums_ready, float* dbeta, float* dgamma,
                                   const void* wtf, int Cin, void* du, float* dWpw, float* workspace, int64_t workspace_floats, void* stream);
int orcai_h_pool_bwd_bn(const void* dout, const void* ybn, int B, int C, int H, int W, int ksize, void* dy, const float* bn_gamma, const float* bn_mean,
                        const float* bn_var, float bn_eps, double* bn_sums, void* stream);
/* orcai_h_pool_bwd_bn that also reduces sum(dout) per channel -- the bias gradient of the block's residual conv, dout being the gradient of the block output
 * (f16 twin of orcai_pool_bwd_bn_bias): dout_sums f64[8 * ceil(C/8)] scratch, dbias f32[C] (overwritten; it carries dout's loss scale). */
int orcai_h_pool_bwd_bn_bias(const void* dout, const void* ybn, int B, int C, int H, int W, int ksize, void* dy, const float* bn_gamma, const float* bn_mean,
                             const float* bn_var, float bn_eps, double* bn_sums, double* dout_sums, float* dbias, void* stream);
int orcai_h_outer_reduce(const void* A, int Ca, const void* Bq, int Cb, int B, int H, int W, int ksize, int a_stride2, int Ha, int Wa, float* D, float* workspace,
                         int64_t workspace_floats, void* stream);
int orcai_h_dw_wgrad(const void* x, const void* du, int B, int C, int H, int W, int ksize_planes, int ktap, int relu_in, float* dW, void* stream);
/* orcai_dw_bwd_fused on f16 octet planes (dw_rev: f16 [ceil(C/8)][9][8] reversed taps; dr f16; dW and the sums f32 / f64): with the BatchNorm
 * arguments x is the pre-normalisation tensor and y = f16(relu(BN(x))) is formed on load -- the value orcai_h_bn_planes_apply stored.  shards: >= 16 *
 * ceil(C/8) * 32 doubles; epi 2 leaves dbeta[8 CO] | dgamma[8 CO] there for orcai_h_bn_bwd_pointwise(sums_ready = 1). */
int orcai_h_dw_bwd_fused(const void* x, const void* du, int B, int C, int H, int W, int relu_in, const void* dw_rev, void* dr, float* dW, int epi, const float* bn_mean,
                         const float* bn_var, const float* bn_gamma, const float* bn_beta, float bn_eps, int bn_relu, double* shards, void* stream);
/* orcai_h_dw_bwd_fused(epi 2) with a gradient that lives on the even pixels only added inside the pass (resq: f16 planes of C channels at the pooled
 * resolution [B][ceil(C/8)][ceil(H/2) + 2][padded_width(ceil(W/2))][8]): for block 1's first conv with x = the entry conv's stored v0 the sums left in
 * `shards` are bn0's backward sums over the TOTAL gradient (orcai_h_conv0_bn_bwd_ready = orcai_h_conv0_bn_bwd without its own sums pass), and the
 * residual branch needs no scatter-add pass over dr. */
int orcai_h_dw_bwd_fused_res(const void* x, const void* du, int B, int C, int H, int W, const void* dw_rev, void* dr, float* dW, const float* bn_mean, const float* bn_var,
                             const float* bn_gamma, const float* bn_beta, float bn_eps, int bn_relu, double* shards, const void* resq, void* stream);
int orcai_h_conv0_bn_bwd_ready(const float* in, int64_t snippet_stride, const void* dy, const void* v, int B, int H, int W, int ksize, const float* mean, const float* var,
                               const float* gamma, const float* beta, float eps, double* scratch2C, float* dbeta, float* dgamma, float* dW, void* stream);
int orcai_h_conv0_bn_bwd(const float* in, int64_t snippet_stride, const void* dy, const void* v, int B, int H, int W, int ksize, const float* mean, const float* var,
                         const float* gamma, const float* beta, float eps, double* scratch2C, float* dbeta, float* dgamma, float* dW, void* stream);
int orcai_h_pack_weights(const float* w, const int* desc, int n_desc, void* out, void* stream);
int orcai_h_feat_to_planes(const float* f, int B, int C, int H, int W, int ksize, void* out, void* stream);
int orcai_h_planes_relu_bwd(const void* dy, const void* y, int64_t n_halves, void* dx, void* stream);
/* Dropout between the residual blocks of ResNet1DConv on the f16 path (csrc/half_dropout.hip); both count f16 elements and need 16-byte aligned buffers.
 *   orcai_h_dropout_mask_dev   f16 0/1 mask: element i is element i of orcai_dropout_mask_dev with the same arguments (bit for bit)
 *   orcai_h_mask_scale         y = f16((f32(x) * f32(mask)) * scale), y == x allowed (the f16 twin of orcai_mask_scale) */
int orcai_h_dropout_mask_dev(void* mask, int64_t n, const uint64_t* counter, uint64_t seed_add, float keep, void* stream);
int orcai_h_mask_scale(const void* x, const void* mask, float scale, int64_t n, void* y, void* stream);

/* ------------------------------------------------------------------------------------------
 * PyTorch custom ops (orcai_amd/torch_ops.py; csrc/interop.hip)
 *   orcai_sigmoid_bwd        dz[i] = g[i] * (1 - p[i]) * p[i]: the gradient at the logit of a head's final sigmoid (orcai_dense_sigmoid,
 *                            orcai_conv1d_sigmoid) from an upstream gradient g w.r.t. the probabilities p; the bits of aten::sigmoid_backward(g, p).
 *   orcai_prepare_inference  the inference weights from the flat trainable weights w and BatchNorm moving statistics `stats` on the device:
 *                            desc int32[n_desc][8] = {kind, dst, count, a0, a1, a2, a3, a4} (offsets in floats into w / stats / out);
 *                            kind 0: BatchNorm fold of `count` channels (gamma w[a0], beta w[a1], mean stats[a2], var stats[a3], conv bias w[a4] or
 *                              a4 < 0 for none): scale = gamma / sqrt(var + eps), shift = beta - mean * scale (+ bias * scale) in double, each
 *                              rounded once to float, scale at out[dst], shift at out[dst + roundup(count, 64)];
 *                            kind 1: depthwise kernel (k, k, count, 1) at w[a0], k = a1 -> [ceil(count/4)][k*k][4] at out[dst] (zero pad channels);
 *                            kind 2: copy of `count` floats from w[a0] to out[dst];
 *                            kind 3: orcai_sepconv_dgrad's wts: count = Cout, gamma w[a0], var stats[a1], pointwise kernel [Cin = a3][Cout] at w[a2]:
 *                              out[dst + co * Cin + ci] = gamma[co] / sqrt(var[co] + eps) * pw[ci][co], the product in double, rounded once;
 *                            kind 4: kind 1 with the taps reversed (tap t <- tap k*k - 1 - t);
 *                            kind 5: transpose of the [a1][a2] matrix at w[a0], count = a1 * a2: out[dst + c * a1 + r] = w[a0 + r * a2 + c].
 *                            The LSTM layouts come from orcai_pack_lstm (mode 0) on the same w. */
int orcai_sigmoid_bwd(const float* p, const float* g, int64_t n, float* dz, void* stream);
int orcai_prepare_inference(const float* w, const float* stats, const int* desc, int n_desc, double eps, float* out, void* stream);

/* ------------------------------------------------------------------------------------------
 * Input gradient of the INFERENCE network (orcai_amd/eval_grad.py; csrc/eval_grad.hip): BatchNorm with its moving statistics, i.e. the folded
 * per-channel (scale, shift) of the inference path, no Dropout, no weight gradients.  The reference never differentiates its predict path
 * (predict.py:265-268); this is what Keras forms for the frozen model (architectures.py:162-241, training=False) behind anything trainable.
 * ------------------------------------------------------------------------------------------ */

/* The folded separable conv y = [relu](scale (.) (pw . dw(relu_in ? relu(x) : x)) + shift) of orcai_sepconv_bn run TRANSPOSED, one pass:
 *   gg[co][q] = g[co][q] where y_gate[co][q] > 0 (everywhere when y_gate is NULL: a conv without ReLU behind it), else 0
 *   du[ci][q] = sum_co wts[co][ci] * gg[co][q]                       (0 outside the image; never written to memory)
 *   dr[ci][p] = sum_t dw_rev[ci][t] * du[ci][p + off(t)],  off(t) = (t / k - k/2) rows, (t % k - k/2) columns
 *   dr[ci][p] = 0 where x_gate[ci][p] <= 0                           (x_gate != NULL: the ReLU in front of the conv; epi 3 of orcai_sepconv_planes_epi)
 *   g, y_gate  padded channel-quad planes of Cout channels [B][ceil(Cout/4)][H + 2R][orcai_padded_width(W, k)][4]: the gradient at y and the stored y
 *   x_gate, dr planes of Cin channels: the stored conv input and the gradient w.r.t. it
 *   wts        f32[Cout][Cin] = scale[co] * pw[ci][co]; dw_rev f32[ceil(Cin/4)][k*k][4], tap t = forward tap k*k - 1 - t (orcai_prepare_inference kinds 3, 4)
 * Only the interior of g and the gates is read (their pads may hold anything); only the interior of dr is written, every element of it, nothing
 * accumulated; no atomics: two launches give the same bits.  k = 3 runs the fused kernel (v_mfma_f32_16x16x4_f32 contraction, du rows in an LDS ring);
 * k = 5, 7, Cin or Cout > 64, B > 65535: ORCAI_E_UNSUPPORTED before anything is touched -- the caller composes orcai_planes_relu_bwd,
 * orcai_sepconv_planes(ktap = 1, wts), orcai_sepconv_planes(ktap = k, dw_rev, identity pointwise), orcai_planes_relu_bwd.
 * ORCAI_E_BADARG: null g / wts / dw_rev / dr, planes or taps not 16-byte aligned, non-positive sizes, ksize not in {3, 5, 7}. */
int orcai_sepconv_dgrad(const float* g, const float* y_gate, const float* x_gate, int B, int Cin, int Cout, int H, int W, int ksize, const float* wts,
                        const float* dw_rev, float* dr, void* stream);
/* A folded BatchNorm on a row tensor f32[M][cols], channel = column % C, and its backward (Dense(128, relu) -> BatchNormalization with moving
 * statistics, architectures.py:231-237: the eval-mode forward keeps the ReLU output `ref` in front of the affine map):
 *   orcai_rows_affine           y = [relu](x * scale[c] + shift[c])
 *   orcai_rows_affine_relu_bwd  dx = ref > 0 ? dy * scale[c] : 0   (ref may be NULL: no gate; dx may alias dy) */
int orcai_rows_affine(const float* x, int64_t M, int cols, int C, const float* scale, const float* shift, int relu, float* y, void* stream);
int orcai_rows_affine_relu_bwd(const float* dy, const float* ref, int64_t M, int cols, int C, const float* scale, float* dx, void* stream);

/* ------------------------------------------------------------------------------------------
 * Weight gradients of the INFERENCE network (EvalGrad.backward(wgrad=True); csrc/eval_grad.hip): fine-tuning with BatchNorm frozen on its moving
 * statistics and no Dropout -- what Keras forms for model(x, training=False) with trainable variables (architectures.py:162-241, training=False).
 * The moving statistics get no gradient.  The reductions themselves are the training step's launchers (orcai_outer_reduce, orcai_planes_sum,
 * orcai_dw_wgrad, orcai_conv0_bn_bwd_x[_ready], the head's GEMMs); orcai_sepconv_wgrad_frozen replaces the first three in one pass where it is faster.
 * ------------------------------------------------------------------------------------------ */

/* A layer z = W . u + bias in front of a frozen BatchNorm, y = scale (.) z + shift with inv = 1 / sqrt(var + eps), scale = gamma * inv,
 * shift = beta - mean * scale (architectures.py:162-241, training=False), from the two reductions over snippets and pixels of gg = the gradient at y:
 *   sums[co]    = sum_p gg[co][p]                      (orcai_planes_sum)
 *   G[co][ci]   = sum_p gg[co][p] * u[ci][p]           (orcai_outer_reduce(gg, u); f32[Cout][Cin])
 *   dbeta[co]   = sums[co]
 *   dbias[co]   = scale[co] * sums[co]
 *   dWpw[ci][co] = scale[co] * G[co][ci]               (Keras pointwise layout (1, 1, Cin, Cout))
 *   dgamma[co]  = inv[co] * (sum_ci pw[ci][co] * G[co][ci] + (bias[co] - mean[co]) * sums[co])     (sum_p gg * z = sum_ci pw * G + bias * sums: neither
 *                                                                                                    z nor u is stored, nothing is divided by gamma)
 * pw: the layer's kernel f32[Cin][Cout]; bias may be NULL (none).  G == NULL (the entry conv, whose dgamma / dbeta / dW orcai_conv0_bn_bwd_x[_ready]
 * deliver): only dbias and dbeta are written, pw / mean / dWpw / dgamma are not read or written.  dbias and dbeta may each be NULL (not wanted); no output
 * may alias an input.  Every output element is written (nothing accumulated) by one thread of ONE workgroup, plain f32: bit-reproducible.
 * ORCAI_E_BADARG: null sums / gamma / var, G without pw / mean / dWpw / dgamma, no output at all, channel counts outside 1 .. 4096. */
int orcai_frozen_bn_finish(const float* G, const float* sums, const float* pw, const float* bias, const float* gamma, const float* mean, const float* var, float eps,
                           int Cin, int Cout, float* dWpw, float* dbias, float* dgamma, float* dbeta, void* stream);
/* The three reductions of a folded separable conv's weight gradients (k = 3) in ONE pass over (x, g) -- what compose_wgrad forms with six launches
 * (architectures.py:162-241, training=False; the formulae above):
 *   gg = g where y_gate > 0 (everywhere when y_gate is NULL),  r = relu_in ? relu(x) : x,  u = dw(r) with the FORWARD taps,  du = wts^T gg
 *   G[co][ci] = sum gg[co][p] * u[ci][p]     dbeta[co] = sum gg[co][p]     dWdw[t][ci] = sum r[ci][p + off(t)] * du[ci][p]   (Keras layout (3, 3, Cin, 1))
 *   x: planes of Cin channels; g, y_gate: planes of Cout channels (only interiors are read: pads may hold anything); taps f32[ceil(Cin/4)][9][4], the layout
 *   orcai_sepconv_bn reads (orcai_prepare_inference kind 1); wts f32[Cout][Cin] = scale[co] * pw[ci][co] (kind 3).
 * u and du never reach memory.  Every element of G, dbeta and dWdw is WRITTEN (nothing accumulated).  Each workgroup leaves its partial sums in a slot of
 * `workspace`; a second launch adds the slots in index order: no float atomics, two launches give the same bits.
 * workspace_floats >= min(B * ceil(H/4) * ceil(W/16), 1024) * (Cout*Cin + Cout + 9*Cin); 1024 * 4736 floats serve every supported shape.
 * ORCAI_E_UNSUPPORTED before anything is touched: ksize 5 or 7, Cin or Cout > 64, B > 65535, a smaller workspace -- the caller runs compose_wgrad.
 * ORCAI_E_BADARG: null x / g / taps / wts / G / dbeta / dWdw / workspace, planes or taps not 16-byte aligned, non-positive sizes, ksize not in {3, 5, 7}. */
int orcai_sepconv_wgrad_frozen(const float* x, const float* g, const float* y_gate, int relu_in, int B, int Cin, int Cout, int H, int W, int ksize, const float* taps,
                               const float* wts, float* G, float* dbeta, float* dWdw, float* workspace, int64_t workspace_floats, void* stream);
/* dbeta / dgamma of a frozen BatchNorm on a row tensor f32[M][cols], channel = column % C (Dense(128, relu) -> BatchNormalization with moving statistics,
 * architectures.py:231-237, training=False): dy = the gradient at the BatchNorm's OUTPUT, x = its input (the ReLU output the eval-mode forward keeps),
 *   dbeta[c] = sum dy,   dgamma[c] = rsqrt(var[c] + eps) * sum dy * (x - mean[c]).
 * workspace: 2 * cols floats.  Column sums in a fixed order, no atomics: two launches give the same bits.
 * ORCAI_E_BADARG: a null pointer, non-positive sizes, cols not a multiple of C. */
int orcai_rows_bn_frozen_wgrad(const float* dy, const float* x, int64_t M, int cols, int C, const float* mean, const float* var, float eps, float* dbeta, float* dgamma,
                               float* workspace, void* stream);

/* ------------------------------------------------------------------------------------------
 * The recording-level gradient (orcai_amd/eval_grad.py: RecordingGrad; csrc/eval_grad.hip): the adjoints of the two linear steps around the detector in
 * `orcai predict` -- slicing the spectrogram [T][W] into snippets i = rows [i * shift, i * shift + H) (predict.py:244-261) and the 50 %-overlap average
 * of their predictions (predict.py:276-293, orcai_overlap_average).  Both work on a CHUNK of consecutive snippets i0 .. i0 + nb - 1, so the caller
 * recomputes the detector chunk by chunk.  Gathers, one thread per output element, no atomics: two launches give the same bits.
 * ------------------------------------------------------------------------------------------ */

/* dpred[i - i0][off][l] = dagg[i * step + off][l] / c(i * step + off) for the snippets i0 <= i < i0 + nb of a recording of n snippets:
 *   dagg f32[S][L] the gradient w.r.t. the averaged probabilities; dpred f32[nb][P][L] w.r.t. the chunk's per-snippet predictions;
 *   c(s) = the number of snippets 0 .. n-1 that cover output step s, as orcai_overlap_average counts it (1 or 2 with step = P / 2).
 * Rows of dagg no snippet covers (the forward writes 0 there) are not read.  Every element of dpred is written.
 * ORCAI_E_BADARG: a null pointer, non-positive n / P / L / step / nb, i0 < 0, i0 + nb > n, (n - 1) * step + P > S.
 * ORCAI_E_UNSUPPORTED (nothing launched): nb * P * L needs 2^31 or more workgroups of 256 threads. */
int orcai_overlap_average_bwd(const float* dagg, int n, int P, int L, int step, int64_t S, int i0, int nb, float* dpred, void* stream);
/* dspec[t][w] += sum over the chunk's snippets i (ascending) that cover row t of dx[i - i0][t - i * shift][w], for the rows
 * [i0 * shift, (i0 + nb - 1) * shift + H) of dspec f32[T][W]; dx f32[nb][H][W].  One read-add-write per element of that row range; the other rows are not
 * touched.  The caller zeroes dspec once (orcai_zero_fill) and runs the chunks on one stream: the result does not depend on how the snippets are chunked
 * beyond the order of f32 additions, and is deterministic.  ORCAI_E_BADARG: a null pointer, non-positive nb / H / W / shift, i0 < 0,
 * (i0 + nb - 1) * shift + H > T.  ORCAI_E_UNSUPPORTED (nothing launched): the chunk's row range times W needs 2^31 or more workgroups of 256 threads
 * (use smaller chunks). */
int orcai_snippets_overlap_add(const float* dx, int i0, int nb, int H, int W, int shift, int64_t T, float* dspec, void* stream);
/* Stream-ordered zero fill of `bytes` (a multiple of 4) at the 4-byte aligned p by a KERNEL (csrc/zero_fill.h: the fill every accumulator of this
 * library gets).  For buffers the CALLER owns (RecordingGrad's dspec): like every fill of the library it asks orcai_arena_take first, so a pointer to a
 * fresh slot of a registered orcai_scratch_arena would be counted as taken and left to the arena's own clear -- do not pass memory of that arena.
 * ORCAI_E_BADARG: null or misaligned p, bytes negative or not a multiple of 4. */
int orcai_zero_fill(void* p, int64_t bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Training augmentation behind the dataset (orcai_amd/augment.py holds the specification, plan_ref / apply_ref; csrc/augment.hip): time
 * and frequency masks, an additive level shift and mixing of two snippets of a batch, on a batch x f32[B][H][W] (normalised dB values in [0, 1]) and
 * its labels y f32[B][S][L] (values 0, 1 and -1 = masked), H a multiple of S.  The reference has no augmentation.  Two launches per batch.
 *
 * Draws.  Draw j (0 <= j < ORCAI_AUGMENT_DRAWS) of snippet b is z = finalise(batch_key + 0x9E3779B97F4A7C15 * (b * ORCAI_AUGMENT_DRAWS + j + 1)) in
 * uint64 arithmetic, `finalise` the three lines of splitmix64 that orcai_dropout_mask uses; an integer in [0, n) is ((z >> 32) * n) >> 32, a uniform
 * f32 in [0, 1) is (float)(z >> 40) * 2^-24.  Slots: 0 mix decision, 1 partner, 2 level shift, 3 + 2k / 4 + 2k height / start of time mask k,
 * 19 + 2k / 20 + 2k height / start of frequency mask k (k < 8); slots 35 .. 39 are not used.
 *
 * Plan.  int32 plan[B][ORCAI_AUGMENT_PLAN_WORDS], every word written:
 *   0        partner snippet (b + 1 + int in [0, B - 1)) mod B if uniform < mix_probability and B > 1, else -1 (not mixed)
 *   1        the bits of the f32 shift (u + u - 1) * level_shift, rounded once
 *   2, 3     time_masks, freq_masks
 *   4 + 2k   start of time mask k, 5 + 2k its height: height in [0, time_mask_rows], start in [0, H - height]; 0, 0 for k >= time_masks
 *   20 + 2k  start of frequency mask k, 21 + 2k its width: the same with W and freq_mask_bins
 * ------------------------------------------------------------------------------------------ */
#define ORCAI_AUGMENT_MAX_MASKS 8
#define ORCAI_AUGMENT_DRAWS 40
#define ORCAI_AUGMENT_PLAN_WORDS 36
#define ORCAI_AUGMENT_MAX_H 4096 /* rows of the row-mask image in LDS */
#define ORCAI_AUGMENT_MAX_W 1024 /* bins of the column-mask image in LDS */
#define ORCAI_AUGMENT_LEVEL_SHIFT 1 /* flags of orcai_augment_apply: add the plan's shift and clamp to [0, 1] */
#define ORCAI_AUGMENT_MASK_LABELS 2 /*   a label step whose H / S rows all lie in the union of the time masks becomes -1 */

/* Draws the plan of one batch on the device; batch_key travels by value, so nothing is copied or synchronised.
 * ORCAI_E_BADARG: null plan, non-positive B / H / W, a negative count, time_mask_rows outside [0, H], freq_mask_bins outside [0, W], level_shift or
 * mix_probability outside [0, 1] (NaN included).  ORCAI_E_UNSUPPORTED (nothing launched): more than ORCAI_AUGMENT_MAX_MASKS masks of a kind,
 * H > ORCAI_AUGMENT_MAX_H, W > ORCAI_AUGMENT_MAX_W, B > 65535. */
int orcai_augment_plan(uint64_t batch_key, int B, int H, int W, int time_masks, int time_mask_rows, int freq_masks, int freq_mask_bins, float level_shift,
                       float mix_probability, int32_t* plan, void* stream);
/* Applies a plan, out of place, in one launch (one snippet per blockIdx.y; the workgroup expands the snippet's masks into a row image and a column
 * image in LDS and looks every element up).  Per element of x[b][r][c], in this order:
 *   v = fmaxf(x_in[b], x_in[partner]) if mixed (the louder of the two in the dB domain), else x_in[b];
 *   with ORCAI_AUGMENT_LEVEL_SHIFT: v = fminf(fmaxf(v + shift, 0), 1);
 *   v = mask_value if r lies in a time mask or c in a frequency mask.
 * Labels y_out[b][s][l]: mixed -> 1 if either snippet has 1, else -1 if either has -1, else 0; not mixed -> y_in; with ORCAI_AUGMENT_MASK_LABELS a
 * step whose rows are all masked -> -1 for every label.  A plan with no mix and no masks and flags 0 copies x_in and y_in bit for bit.  Accesses are
 * 16 bytes wide when x_in's and the partner's block and x_out's block are 16-byte aligned and H * W is a multiple of 4, scalar otherwise; any
 * 4-byte alignment is accepted.  Partner and counts read from the plan are clamped to [0, B) and [0, 8]: a damaged plan cannot reach outside x_in.
 * ORCAI_E_BADARG: a null pointer, non-positive B / H / W / S / L, H % S != 0, mask_value not finite, unknown flag bits, x_out overlapping x_in or
 * y_out overlapping y_in.  ORCAI_E_UNSUPPORTED (nothing launched): H > ORCAI_AUGMENT_MAX_H, W > ORCAI_AUGMENT_MAX_W, B > 65535, S * L >= 2^31. */
int orcai_augment_apply(const float* x_in, const float* y_in, const int32_t* plan, float* x_out, float* y_out, int B, int H, int W, int S, int L,
                        float mask_value, int flags, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ORCAI_HIP_H */
