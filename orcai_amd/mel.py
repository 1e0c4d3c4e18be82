"""Host side of the mel front end (``orcai_parameter["spectrogram"]["mel"]``): the mel scales, the triangular filterbank, its sparse band
table for ``orcai_stft_mel_db`` (include/orcai_hip.h) and the parameter's validation.  numpy only; nothing here touches the GPU.

The reference has no mel route.  Semantics are librosa's documented defaults (``librosa.filters.mel``, ``librosa.hz_to_mel``): triangles over
``n_mels + 2`` points equally spaced on the mel scale between fmin and fmax, evaluated at the FFT bin frequencies; Slaney's scale (linear at
200/3 Hz per mel below 1 kHz, logarithmic with step ln(6.4)/27 above) unless ``htk``; Slaney's area normalisation 2 / (f[m+2] - f[m]) unless
``norm`` is null.  librosa is not a dependency, so parity with it is unpinned.
"""

from __future__ import annotations

from functools import lru_cache

import numpy as np

N_MELS_MIN, N_MELS_MAX = 8, 256
NFFT_MIN, NFFT_MAX = 128, 4096
MEL_KEYS = ("n_mels", "fmin", "fmax", "htk", "norm")

_F_SP = 200.0 / 3.0
_MIN_LOG_HZ = 1000.0
_MIN_LOG_MEL = 15.0  # hz_to_mel(1000)
_LOGSTEP = np.log(6.4) / 27.0


def hz_to_mel(frequencies, htk: bool = False):
    f = np.asarray(frequencies, dtype=np.float64)
    if htk:
        return (2595.0 * np.log10(1.0 + f / 700.0))[()]
    safe = np.maximum(f, _MIN_LOG_HZ)  # the logarithm's argument where the linear branch is taken anyway
    return np.where(f >= _MIN_LOG_HZ, _MIN_LOG_MEL + np.log(safe / _MIN_LOG_HZ) / _LOGSTEP, f / _F_SP)[()]


def mel_to_hz(mels, htk: bool = False):
    m = np.asarray(mels, dtype=np.float64)
    if htk:
        return (700.0 * (10.0 ** (m / 2595.0) - 1.0))[()]
    return np.where(m >= _MIN_LOG_MEL, _MIN_LOG_HZ * np.exp(_LOGSTEP * (np.maximum(m, _MIN_LOG_MEL) - _MIN_LOG_MEL)), _F_SP * m)[()]


def mel_frequencies(n_points: int, fmin: float, fmax: float, htk: bool = False) -> np.ndarray:
    """n_points frequencies in Hz, equally spaced on the mel scale from fmin to fmax (both included)."""
    return mel_to_hz(np.linspace(hz_to_mel(fmin, htk), hz_to_mel(fmax, htk), int(n_points)), htk)


def mel_filterbank(sampling_rate: float, nfft: int, n_mels: int, fmin: float, fmax: float, htk: bool = False, norm: str | None = "slaney") -> np.ndarray:
    """f64[n_mels, 1 + nfft // 2]: row m is the triangle over mel points m, m + 1, m + 2 at the FFT bin frequencies."""
    if norm not in ("slaney", None):
        raise ValueError(f"spectrogram parameter mel.norm = {norm!r}: \"slaney\" or null")
    fft_f = np.fft.rfftfreq(n=int(nfft), d=1.0 / float(sampling_rate))
    mel_f = mel_frequencies(int(n_mels) + 2, fmin, fmax, htk)
    fdiff = np.diff(mel_f)
    ramps = mel_f[:, None] - fft_f[None, :]
    lower = -ramps[:-2] / fdiff[:-1, None]
    upper = ramps[2:] / fdiff[1:, None]
    W = np.maximum(0.0, np.minimum(lower, upper))
    if norm == "slaney":
        W *= (2.0 / (mel_f[2:] - mel_f[:-2]))[:, None]
    return W


@lru_cache(maxsize=32)
def _band_table(sampling_rate: float, nfft: int, n_mels: int, fmin: float, fmax: float, htk: bool, norm):
    W = mel_filterbank(sampling_rate, nfft, n_mels, fmin, fmax, htk, norm).astype(np.float32)
    lo = np.zeros(n_mels, dtype=np.int32)
    hi = np.zeros(n_mels, dtype=np.int32)
    off = np.zeros(n_mels, dtype=np.int32)
    parts = []
    total = 0
    for m in range(n_mels):
        nz = np.flatnonzero(W[m])
        if nz.size:
            lo[m], hi[m] = nz[0], nz[-1] + 1  # a triangle: everything between its first and last non-zero bin is non-zero
        off[m] = total
        parts.append(W[m, lo[m] : hi[m]])
        total += int(hi[m] - lo[m])
    weights = np.concatenate(parts) if total else np.zeros(0, dtype=np.float32)
    centres = mel_frequencies(n_mels + 2, fmin, fmax, htk)[1:-1].copy()
    for a in (lo, hi, off, weights, centres):
        a.setflags(write=False)
    return {"lo": lo, "hi": hi, "off": off, "weights": weights, "centres": centres}


def band_table(sampling_rate: float, nfft: int, n_mels: int, fmin: float, fmax: float, htk: bool = False, norm: str | None = "slaney") -> dict:
    """The filterbank as orcai_stft_mel_db takes it: {"lo", "hi", "off": int32[n_mels], "weights": f32[n_weights], "centres": f64[n_mels]}.  Band m
    covers the bins [lo[m], hi[m]) -- the ones with a non-zero f32 weight -- and its weights are weights[off[m] : off[m] + hi[m] - lo[m]]; a bin lies
    under at most two triangles, so n_weights <= 2 (1 + nfft // 2).  centres are the triangles' peak frequencies in Hz.  Cached; read-only."""
    return _band_table(float(sampling_rate), int(nfft), int(n_mels), float(fmin), float(fmax), bool(htk), norm)


def dense_from_table(table: dict, nfft: int) -> np.ndarray:
    """f32[n_mels, 1 + nfft // 2] rebuilt from a band table."""
    n_mels = table["lo"].size
    W = np.zeros((n_mels, 1 + nfft // 2), dtype=np.float32)
    for m in range(n_mels):
        n = int(table["hi"][m] - table["lo"][m])
        W[m, table["lo"][m] : table["hi"][m]] = table["weights"][table["off"][m] : table["off"][m] + n]
    return W


def _is_number(v) -> bool:
    return isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, (bool, np.bool_)) and bool(np.isfinite(v))


def mel_config(spectrogram_parameter: dict) -> dict | None:
    """None when the ``mel`` key is absent or null (the linear front end, unchanged).  Otherwise the validated parameter with its defaults filled
    in, {"n_mels", "fmin", "fmax", "htk", "norm"}; ValueError names the offending key, NotImplementedError an nfft the mel route does not take.
    Host arithmetic only: runs before anything is loaded or launched."""
    mel = spectrogram_parameter.get("mel")
    if mel is None:
        return None
    if not isinstance(mel, dict):
        raise ValueError(f"spectrogram parameter mel = {mel!r}: null or a dict with the keys {', '.join(MEL_KEYS)}")
    unknown = sorted(set(mel) - set(MEL_KEYS))
    if unknown:
        raise ValueError(f"spectrogram parameter mel: unknown key(s) {', '.join(map(repr, unknown))}; known: {', '.join(MEL_KEYS)}")
    if "n_mels" not in mel:
        raise ValueError("spectrogram parameter mel.n_mels is required (the number of bands, 8 to 256)")
    n_mels = mel["n_mels"]
    if isinstance(n_mels, (bool, np.bool_)) or not isinstance(n_mels, (int, np.integer)) or not N_MELS_MIN <= int(n_mels) <= N_MELS_MAX:
        raise ValueError(f"spectrogram parameter mel.n_mels = {n_mels!r}: an integer from {N_MELS_MIN} to {N_MELS_MAX}")
    htk = mel.get("htk", False)
    if not isinstance(htk, (bool, np.bool_)):
        raise ValueError(f"spectrogram parameter mel.htk = {htk!r}: true or false")
    norm = mel.get("norm", "slaney")
    if norm is not None and norm != "slaney":
        raise ValueError(f"spectrogram parameter mel.norm = {norm!r}: \"slaney\" or null")
    sr = spectrogram_parameter["sampling_rate"]
    freq_range = spectrogram_parameter.get("freq_range", (0.0, sr / 2.0))
    fmin = mel.get("fmin", freq_range[0])
    fmax = mel.get("fmax", freq_range[1])
    if not _is_number(fmin) or fmin < 0:
        raise ValueError(f"spectrogram parameter mel.fmin = {fmin!r}: a frequency in Hz, 0 <= fmin < fmax")
    if not _is_number(fmax) or fmax > sr / 2.0:
        raise ValueError(f"spectrogram parameter mel.fmax = {fmax!r}: a frequency in Hz, fmin < fmax <= sampling_rate / 2 = {sr / 2.0}")
    if not fmin < fmax:
        raise ValueError(f"spectrogram parameter mel.fmin = {fmin!r} must lie below mel.fmax = {fmax!r}")
    nfft = spectrogram_parameter["nfft"]
    n = int(nfft)
    if n != nfft or n < NFFT_MIN or n > NFFT_MAX or n & (n - 1):
        raise NotImplementedError(f"spectrogram parameter nfft = {nfft!r} with mel: the mel front end implements the powers of two from {NFFT_MIN} to "
                                  f"{NFFT_MAX} (the linear front end runs every size from 2 to 4096)")
    cfg = {"n_mels": int(n_mels), "fmin": float(fmin), "fmax": float(fmax), "htk": bool(htk), "norm": norm}
    t = band_table(sr, n, **cfg)
    empty = np.flatnonzero(t["hi"] == t["lo"])
    if empty.size:
        raise ValueError(f"spectrogram parameter mel.n_mels = {n_mels} with nfft = {n}: band {int(empty[0])} (centre {t['centres'][empty[0]]:.1f} Hz) has no "
                         f"FFT bin under it ({empty.size} empty band(s) at a bin spacing of {sr / n:.2f} Hz); lower n_mels, raise nfft or raise fmin")
    return cfg


def table_for(spectrogram_parameter: dict, cfg: dict) -> dict:
    return band_table(spectrogram_parameter["sampling_rate"], int(spectrogram_parameter["nfft"]), **cfg)
