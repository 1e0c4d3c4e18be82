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
"""

from __future__ import annotations

import numpy as np

DENOISE_DEFAULTS = {"quantile": 0.5}
DENOISE_KEYS = tuple(DENOISE_DEFAULTS)


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
        raise ValueError(f"spectrogram parameter denoise = {p!r}: null or a dict with the optional key {', '.join(DENOISE_KEYS)}")
    unknown = sorted(set(p) - set(DENOISE_KEYS), key=repr)
    if unknown:
        raise ValueError(f"spectrogram parameter denoise: unknown key(s) {', '.join(map(repr, unknown))}; known: {', '.join(DENOISE_KEYS)}")
    q = p.get("quantile", DENOISE_DEFAULTS["quantile"])
    if not _is_number(q) or not 0 <= q <= 1:
        raise ValueError(f"spectrogram parameter denoise.quantile = {q!r}: a number in [0, 1] (the fraction of a channel's frames below its noise floor)")
    if spectrogram_parameter.get("pcen") is not None:
        raise ValueError("spectrogram parameter denoise and pcen are both set: PCEN already normalises every channel by its own level; set one of the two to null")
    return {"quantile": float(q)}


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
