"""float64 restatement of orcai_stft_mel_db's contract (csrc/frontend.hip, include/orcai_hip.h), its error bound and the case tables of
tests/test_mel_ref.py (CPU) and tests/test_mel_gpu.py.  numpy only; the STFT half is tests/stft_ref.py's.

Contract.  S[t][k] = |X|^2 of stft_ref (float64, centred, zero padding, periodic Hann); W = the mel filterbank of orcai_amd/mel.py rounded to f32
(the weights the kernels read) and promoted back to float64; M_ref = S W^T in float64; the kernels write L = 10 log10(max(M, 1e-10)) and leave max M
in the workspace.

Bound, derived (nothing here is fitted to what a kernel produces).  Per bin the STFT kernels deliver an amplitude a_gpu[k] with |a_gpu[k] - a_ref[k]|
<= e = gamma(N) S1[t] (stft_ref.py; S1[t] = sum_n |x_n w_n|), hence for the power the kernel forms from it, before any rounding of the power itself,
|a_gpu^2 - a_ref^2| <= 2 a_ref e + e^2.  With non-negative weights that is the first term below.  The remaining roundings are all RELATIVE to
non-negative quantities, so they are bounded against the band sum itself:
  * |X|^2 = fma(re, re, im * im) in f32: two roundings, 2 u relative per bin (u = 2^-24)   -- a term the issue's formula does not list: the amplitude
    bound of stft_ref.py is stated for the amplitude, and squaring it in f32 rounds again;
  * the weight is f32: W_ref here IS the rounded weight, so nothing (the issue's formula reserves one u for it; kept, as slack);
  * the band sum: one fma per bin in the tuned kernel (n_k roundings on the longest path), or 64 strided partial sums (ceil(n_k / 64) fmas each) and a
    six-level butterfly in the workgroup-per-frame kernel.  Adding a zero is exact, so a term meets at most min(6, n_k - 1) rounded additions in the
    butterfly: 1 + min(6, n_k - 1) <= n_k roundings for n_k <= 64 and ceil(n_k / 64) + 6 <= n_k for n_k >= 65.  n_k on every path, then.
Each rounding scales the partial result by (1 + d), |d| <= u, so the computed sum lies within ((1 + u)^(n_k + 4) - 1) of the sum of the perturbed
terms, and (1 + u)^(n_k + 4) - 1 <= 1.001 (n_k + 4) u for n_k <= 2049.  Altogether

    |M_gpu - M_ref| <= dM = (1 + r) sum_k W[m][k] (2 a_ref[k] e + e^2) + r M_ref,      r = 1.001 (n_k(m) + 4) 2^-24

(the issue states (n_k + 2); the two extra u are the f32 squaring above).  Compared in amplitude, A = sqrt(max(M, 1e-10)), where the clamp has no
singularity and no element is excluded:  |sqrt(max(x, c)) - sqrt(max(y, c))| <= min(|x - y| / sqrt(max(y, c)), sqrt|x - y|), and the logarithm and
the two f32 operations behind it cost rho = 1e-5 relative in amplitude as in stft_ref.py:

    |A_gpu - A_ref| <= min(dM / A_ref, sqrt(dM)) (1 + rho) + rho A_ref,        A_gpu = 10^(L_gpu / 20) in float64.

Test infrastructure: nothing in orcai_amd/ imports this file.
"""

from __future__ import annotations

import numpy as np

import stft_ref as R
from orcai_amd import mel

AMIN_POW = R.AMIN_POW
U = R.U
RHO = R.RHO


def weights_f64(sr, n_fft, n_mels, fmin, fmax, htk, norm) -> np.ndarray:
    """The filterbank as the kernels see it: f32-rounded weights, as float64 [n_mels, 1 + n_fft // 2]."""
    return mel.mel_filterbank(sr, n_fft, n_mels, fmin, fmax, htk, norm).astype(np.float32).astype(np.float64)


def power_ref(x_f32, n_fft: int, hop: int):
    """(P[T, 1 + n_fft // 2] = |X|^2 unclamped, S1[T]) in float64, by tests/stft_ref.py's framing."""
    x = np.asarray(x_f32)
    assert x.dtype == np.float32 and x.ndim == 1
    n, half = x.size, n_fft // 2
    T = R.num_frames(n, n_fft, hop)
    seg = np.zeros((T - 1) * hop + n_fft, dtype=np.float64)
    a, b = max(-half, 0), min((T - 1) * hop - half + n_fft, n)
    seg[a + half : b + half] = x[a:b]
    fr = np.lib.stride_tricks.sliding_window_view(seg, n_fft)[::hop] * R.hann(n_fft)[None, :]
    assert fr.shape[0] == T
    return np.abs(np.fft.rfft(fr, axis=1)) ** 2, np.abs(fr).sum(axis=1)


def mel_bound(P, S1, W, n_fft: int, route: str = "radix2"):
    """(A_ref, M_ref, dM), all [T, n_mels] float64."""
    e = (R.gamma(n_fft, route) * np.asarray(S1))[:, None]
    a = np.sqrt(P)
    M = P @ W.T
    first = (2.0 * a * e + e * e) @ W.T
    n_k = (W > 0).sum(axis=1)
    r = 1.001 * (n_k + 4) * U
    dM = (1.0 + r)[None, :] * first + r[None, :] * M
    return np.sqrt(np.maximum(M, AMIN_POW)), M, dM


def amp_bar(A_ref, dM):
    return np.minimum(dM / A_ref, np.sqrt(dM)) * (1.0 + RHO) + RHO * A_ref


def ratio_from_db(L, A_ref, dM) -> np.ndarray:
    """|A_got - A_ref| / bar per element from the dB values a kernel (or the emulation) wrote; the bar is never zero (A_ref >= 1e-5)."""
    return np.abs(R.db_to_amp(L) - A_ref) / amp_bar(A_ref, dM)


# ------------------------------------------------------------------------------------------------ input families
FAMILIES = ("noise", "impulses", "band_edge_tone", "silence", "full_scale")


def make_input(family: str, n: int, n_fft: int, hop: int, sr: float = 48000.0, edge_hz: float = 0.0) -> np.ndarray:
    """f32[n].  noise / impulses are stft_ref's; band_edge_tone is a sinusoid at edge_hz (a mel point: the edge two triangles share, or the last band's
    upper edge); silence is all zeros (every band at the clamp); full_scale alternates +1 / -1 with a full-scale step (the largest |X| an input allows)."""
    if family in ("noise", "impulses"):
        return R.make_input(family, n, n_fft, hop)
    i = np.arange(n, dtype=np.float64)
    if family == "band_edge_tone":
        x = 0.5 * np.cos(2.0 * np.pi * edge_hz * i / sr)
    elif family == "silence":
        x = np.zeros(n)
    elif family == "full_scale":
        x = np.where(i % 2 == 0, 1.0, -1.0)
        x[n // 2 :] = 1.0
    else:
        raise KeyError(family)
    return x.astype(np.float32)


# ------------------------------------------------------------------------------------------------ case tables
SR = 48000
# (n_fft, hop, n_samples, purpose)
SHAPES = [
    (512, 256, 10000, "40 frames: one interior fast group between two edge groups"),
    (512, 256, 4100, "17 frames: below any interior group"),
    (512, 255, 3000, "odd hop"),
    (128, 64, 64 * 5 + 3, "radix-2 route, smallest"),
    (1024, 256, 256 * 6 + 7, "radix-2 route"),
    (4096, 1024, 1024 * 3 + 11, "radix-2 route, largest"),
]
# (n_mels, fmin, fmax, htk, norm) per n_fft: every band keeps an FFT bin (tests/test_mel_ref.py asserts it for every tuple)
MELS = {
    # 128 bands over 257 bins of 93.75 Hz only fit above a few kHz, where two mel points are more than a bin apart
    512: [(8, 0.0, 24000.0, False, "slaney"), (40, 0.0, 16000.0, True, None), (128, 6000.0, 24000.0, True, "slaney"), (40, 300.0, 20000.0, False, None)],
    128: [(8, 0.0, 24000.0, False, "slaney"), (16, 2000.0, 24000.0, True, None)],
    1024: [(8, 0.0, 16000.0, True, "slaney"), (40, 0.0, 16000.0, False, None), (128, 0.0, 24000.0, False, "slaney")],
    4096: [(40, 0.0, 24000.0, False, "slaney"), (128, 0.0, 24000.0, True, None), (256, 0.0, 24000.0, False, "slaney")],
}


def cases():
    """Every (n_fft, hop, n, n_mels, fmin, fmax, htk, norm) the GPU test runs."""
    return [(N, hop, n, *m) for N, hop, n, _ in SHAPES for m in MELS[N]]


def edge_frequency(n_mels, fmin, fmax, htk) -> float:
    """The mel point shared by the two middle triangles."""
    return float(mel.mel_frequencies(n_mels + 2, fmin, fmax, htk)[n_mels // 2 + 1])


def clip_normalize_ref(L_f32, q_lo: float, q_hi: float, top_db: float = 80.0) -> np.ndarray:
    """The composition behind the raw dB array, in f32 as the kernels do it: ref = max, 80 dB floor, numpy's nearest-rank percentiles, clip, normalise."""
    from orcai_amd.frontend import nearest_rank_index

    L = np.asarray(L_f32, dtype=np.float32)
    srt = np.sort(L, axis=None)
    n = L.size
    lo_raw, hi_raw = srt[nearest_rank_index(n, q_lo)], srt[nearest_rank_index(n, q_hi)]
    ref = L.max()
    floor = np.float32(-top_db)
    v = np.maximum(L - ref, floor)
    p_lo, p_hi = np.maximum(lo_raw - ref, floor), np.maximum(hi_raw - ref, floor)
    v = np.minimum(np.maximum(v, p_lo), p_hi)
    return ((v - p_lo) / (p_hi - p_lo)).astype(np.float32), (ref, p_lo, p_hi)
