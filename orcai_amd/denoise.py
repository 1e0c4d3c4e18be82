"""Host side of the per-channel noise floor (``orcai_parameter["spectrogram"]["denoise"]``): the parameter's validation and the numpy specification
of what ``orcai_column_select`` + ``orcai_subtract_columns`` (include/orcai_hip.h) compute.  numpy only; nothing here touches the GPU.

Hydrophone recordings carry stationary narrow-band noise (engine lines, electrical hum, the recorder's own tones) that a global percentile clip cannot
remove: such a line sits at a constant high level in a few channels for the whole file.  The standard remedy is to subtract from every frequency channel
a robust estimate of its own level over the recording -- an order statistic of the channel's referenced dB values, the median by default -- which
amounts to dividing the channel by its median magnitude.  The reference has no such option.  With ``denoise`` set the front end computes

    V = max(dB - ref_db, -top_db)          the referenced dB spectrogram [T, K] (linear route, or the mel bands when ``mel`` is set)
    m[k] = sort(V[:, k])[nearest_rank_index(T, quantile)]
    Y = V - m                              float32, one rounding

and then the exact percentile clip and the normalisation to [0, 1] on Y (``quantiles`` keeps its meaning).  PCEN (orcai_amd/pcen.py) is the adaptive
version of the same idea and already normalises each channel by its own level, so the two keys together are refused.

The gradient w.r.t. the audio is FrontEnd.denoised_spectrogram_backward (orcai_denoised_spectrogram_bwd: the dB backward kernels with m[k] in their clip
gates, p_lo < fl32(V - m[k]) < p_hi, and m held constant like ref_db, p_lo and p_hi); torch_ops.denoised_spectrogram_wrt_pcm and
torch_ops.DenoisedWaveformFrontEnd are built on it.  The plain backward entries and modules do not know the floor and keep refusing a parameter with
``denoise`` set (no_gradient).

``"denoise": {"quantile": 0.5, "segment": 10.0}`` makes the floor time-varying (a passing boat, a gain change, rain: a global median sits between the two
regimes).  The frames are cut into segments of W = segment_rows(segment, sampling_rate, hop) frames, S = max(1, T // W) of them, the last one taking the
remainder (W .. 2 W - 1 frames; a segment longer than the recording is the global floor); every (segment, channel) gets its own order statistic, and the
floor at a frame interpolates linearly between the segment centres (segment_denoise_ref is the definition; orcai_make_segment_denoised_spectrogram the
entry).  Forward only: the gradient entries refuse a parameter with ``segment`` set (no_segment_gradient).
"""

from __future__ import annotations

import numpy as np

DENOISE_DEFAULTS = {"quantile": 0.5}
DENOISE_KEYS = (*DENOISE_DEFAULTS, "segment")  # segment has no default: absent (or null) is the one floor per channel over the whole recording


def _is_number(v) -> bool:
    return isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, (bool, np.bool_)) and bool(np.isfinite(v))


def denoise_config(spectrogram_parameter: dict) -> dict | None:
    """None when the ``denoise`` key is absent or null (the front end, unchanged).  Otherwise the validated parameter with its default filled in,
    {"quantile"} as a float; ValueError names the offending or unknown key, and both keys when ``pcen`` is set as well.  Host arithmetic only: runs
    before anything is loaded or launched."""
    p = spectrogram_parameter.get("denoise")
    if p is None:
        return None
    if not isinstance(p, dict):
        raise ValueError(f"spectrogram parameter denoise = {p!r}: null or a dict with the optional key {', '.join(DENOISE_DEFAULTS)}")
    unknown = sorted(set(p) - set(DENOISE_KEYS), key=repr)
    if unknown:
        # (the text names the keys that have a default, as it always has; segment is described in this module's docstring and in the README)
        raise ValueError(f"spectrogram parameter denoise: unknown key(s) {', '.join(map(repr, unknown))}; known: {', '.join(DENOISE_DEFAULTS)}")
    q = p.get("quantile", DENOISE_DEFAULTS["quantile"])
    if not _is_number(q) or not 0 <= q <= 1:
        raise ValueError(f"spectrogram parameter denoise.quantile = {q!r}: a number in [0, 1] (the fraction of a channel's frames below its noise floor)")
    if spectrogram_parameter.get("pcen") is not None:
        raise ValueError("spectrogram parameter denoise and pcen are both set: PCEN already normalises every channel by its own level; set one of the two to null")
    cfg = {"quantile": float(q)}
    seg = p.get("segment")
    if seg is not None:  # null is absent: the dict stays what it was before the key existed
        if not _is_number(seg) or not seg > 0:
            raise ValueError(f"spectrogram parameter denoise.segment = {seg!r}: a finite number of seconds > 0 (the length of a noise-floor segment), or null")
        cfg["segment"] = float(seg)
    return cfg


def segment_rows(segment: float, sampling_rate, hop) -> int:
    """W, the frames of a noise-floor segment of `segment` seconds: max(1, rint(segment * sampling_rate / hop))."""
    return max(1, int(np.rint(segment * sampling_rate / hop)))


def segment_count(T: int, seg_rows: int) -> int:
    """S = max(1, T // W): segment s < S - 1 is rows [s W, (s + 1) W), the last one [(S - 1) W, T) -- W .. 2 W - 1 rows, or all T when S == 1."""
    return max(1, T // seg_rows)


def no_segment_gradient(spectrogram_parameter: dict, who: str) -> None:
    """The refusal of the denoised gradient entries for a parameter whose denoise.segment is set: they differentiate the global-floor forward."""
    p = spectrogram_parameter.get("denoise")
    if isinstance(p, dict) and p.get("segment") is not None:
        raise NotImplementedError(f"{who}: spectrogram parameter denoise.segment is set, and the time-varying floor is forward only: this gradient holds ONE floor "
                                  "per channel in its clip gates and would differentiate another forward.  Set denoise.segment to null for the gradient of the "
                                  "global floor")


def no_gradient(spectrogram_parameter: dict, who: str) -> None:
    """The refusal of every plain backward entry and differentiable module for a parameter whose ``denoise`` key is set."""
    if spectrogram_parameter.get("denoise") is not None:
        raise NotImplementedError(f"{who}: spectrogram parameter denoise is set, and this entry's forward and gradient are those of the plain front end, whose clip "
                                  "gates do not know the per-channel offset.  FrontEnd.denoised_spectrogram_backward is the gradient of the denoised front end "
                                  "and torch_ops.DenoisedWaveformFrontEnd(spectrogram_parameter, native_rate) its differentiable module; or set denoise to null")


def denoise_ref(V, quantile: float):
    """The numpy specification.  V: float32 [T, K] referenced dB values without NaN.  Returns (Y, m): m[k] the nearest_rank_index(T, quantile)-th
    smallest of column k, Y = V - m in float32."""
    from orcai_amd.frontend import nearest_rank_index

    V = np.asarray(V, dtype=np.float32)
    if V.ndim != 2 or V.shape[0] < 1:
        raise ValueError(f"denoise_ref: V must be [T, K] with T >= 1, got {V.shape}")
    m = np.sort(V, axis=0)[nearest_rank_index(V.shape[0], quantile)]
    return (V - m).astype(np.float32), m


def segment_denoise_ref(V, quantile: float, seg_rows: int):
    """The numpy specification of the time-varying floor (orcai_segment_column_select + orcai_subtract_segment_floor reproduce its bytes).
    V: float32 [T, K] without NaN; seg_rows = W >= 1.  Returns (Y, m): m float32 [S, K], m[s][k] the nearest_rank_index(n_s, quantile)-th smallest of
    column k inside segment s (segment_count: the last segment takes the remainder), and Y = fl32(V - F), F[t] the floors interpolated linearly between
    the segment centres and held constant outside the first and last centre.  Doubled integer coordinates keep the half-integer centres exact: u = 2 t,
    c2_s = 2 s W + n_s - 1; with c2_s <= u < c2_{s+1}, a = float32(float64(u - c2_s) / float64(c2_{s+1} - c2_s)) and
    F = fl32(m[s] + fl32(a * fl32(m[s+1] - m[s]))), every operation rounded on its own.  With S == 1 this is denoise_ref."""
    from orcai_amd.frontend import nearest_rank_index

    V = np.asarray(V, dtype=np.float32)
    W = int(seg_rows)
    if V.ndim != 2 or V.shape[0] < 1 or W < 1:
        raise ValueError(f"segment_denoise_ref: V must be [T, K] with T >= 1 and seg_rows >= 1, got {V.shape} and {seg_rows!r}")
    T = V.shape[0]
    S = segment_count(T, W)
    bounds = [(s * W, (s + 1) * W if s < S - 1 else T) for s in range(S)]
    m = np.stack([np.sort(V[lo:hi], axis=0)[nearest_rank_index(hi - lo, quantile)] for lo, hi in bounds]).astype(np.float32)
    c2 = np.array([2 * lo + (hi - lo) - 1 for lo, hi in bounds], dtype=np.int64)
    u = 2 * np.arange(T, dtype=np.int64)
    F = np.empty_like(V)
    F[u <= c2[0]] = m[0]
    F[u >= c2[-1]] = m[-1]
    mid = np.flatnonzero((u > c2[0]) & (u < c2[-1]))
    if mid.size:
        s = np.searchsorted(c2, u[mid], side="right") - 1  # c2_s <= u < c2_{s+1}
        a = ((u[mid] - c2[s]).astype(np.float64) / (c2[s + 1] - c2[s]).astype(np.float64)).astype(np.float32)
        d = (m[s + 1] - m[s]).astype(np.float32)
        F[mid] = (m[s] + (a[:, None] * d).astype(np.float32)).astype(np.float32)
    return (V - F).astype(np.float32), m
