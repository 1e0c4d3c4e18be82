"""Host side of the PCEN front end (``orcai_parameter["spectrogram"]["pcen"]``): the parameter's validation, the smoother's coefficient and the
float64 specification of what ``orcai_pcen`` (include/orcai_hip.h) computes.  numpy only; nothing here touches the GPU.

Per-channel energy normalisation (Wang et al. 2017; Lostanlen et al. 2019): every frequency channel is divided by a smoothed copy of its own recent
energy and root-compressed -- an automatic gain control per channel that suppresses stationary noise.  The reference has no PCEN.  Semantics are
``librosa.pcen``'s documented ones: the first-order IIR smoother with librosa's coefficient b(time_constant) and its steady-state initial condition
M[0] = S[0], ``scale`` = 2**31 as its convention for float audio in [-1, 1].  librosa is not a dependency, so parity with it is unpinned.

With ``mel`` set as well the energies are the mel band powers; without it the magnitudes |X[k]| of the kept bins.  After PCEN the exact percentile
clip and the normalisation to [0, 1] run on the PCEN values (``quantiles`` keeps its meaning; there is no dB reference and no top_db).  The gradient
w.r.t. the audio is ``FrontEnd.pcen_spectrogram_backward`` (``orcai_pcen_spectrogram_bwd``; ``pcen_bwd_ref`` below specifies its reverse-time scan); the
two dB backward methods keep refusing a parameter with ``pcen`` set.
"""

from __future__ import annotations

import numpy as np

CHUNK = 256  # ORCAI_PCEN_CHUNK (include/orcai_hip.h): frames per chunk of the kernel's scan
NFFT_MIN, NFFT_MAX = 32, 4096
PCEN_DEFAULTS = {"time_constant": 0.4, "gain": 0.98, "bias": 2.0, "power": 0.5, "eps": 1e-6, "scale": 2147483648.0}
PCEN_KEYS = tuple(PCEN_DEFAULTS)

# key -> (test, what the refusal says)
_CONSTRAINTS = {
    "time_constant": (lambda v: v > 0, "seconds, > 0"),
    "gain": (lambda v: 0 <= v <= 1, "in [0, 1]"),
    "bias": (lambda v: v >= 0, ">= 0"),
    "power": (lambda v: 0 < v <= 1, "in (0, 1]"),
    "eps": (lambda v: v > 0, "> 0"),
    "scale": (lambda v: v > 0, "> 0"),
}


def _is_number(v) -> bool:
    return isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, (bool, np.bool_)) and bool(np.isfinite(v))


def pcen_config(spectrogram_parameter: dict) -> dict | None:
    """None when the ``pcen`` key is absent or null (the dB front end, unchanged).  Otherwise the validated parameter with its defaults filled in,
    {"time_constant", "gain", "bias", "power", "eps", "scale"} as floats; ValueError names the offending or unknown key, NotImplementedError an
    nfft the PCEN route does not take.  Host arithmetic only: runs before anything is loaded or launched."""
    p = spectrogram_parameter.get("pcen")
    if p is None:
        return None
    if not isinstance(p, dict):
        raise ValueError(f"spectrogram parameter pcen = {p!r}: null or a dict with the optional keys {', '.join(PCEN_KEYS)}")
    unknown = sorted(set(p) - set(PCEN_KEYS), key=repr)
    if unknown:
        raise ValueError(f"spectrogram parameter pcen: unknown key(s) {', '.join(map(repr, unknown))}; known: {', '.join(PCEN_KEYS)}")
    cfg = {}
    for key, default in PCEN_DEFAULTS.items():
        v = p.get(key, default)
        ok, what = _CONSTRAINTS[key]
        if not _is_number(v) or not ok(v):
            raise ValueError(f"spectrogram parameter pcen.{key} = {v!r}: a number {what}")
        cfg[key] = float(v)
    nfft = spectrogram_parameter["nfft"]
    n = int(nfft)
    if n != nfft or n < NFFT_MIN or n > NFFT_MAX or n & (n - 1):
        raise NotImplementedError(f"spectrogram parameter nfft = {nfft!r} with pcen: the PCEN front end implements the powers of two from {NFFT_MIN} to "
                                  f"{NFFT_MAX} (the dB front end runs every size from 2 to 4096)")
    return cfg


def smoother(time_constant: float, sampling_rate: float, hop: int) -> tuple[float, float]:
    """(a, b) of M[t] = a M[t-1] + b S[t]: librosa.pcen's b = (sqrt(1 + 4 t^2) - 1) / (2 t^2) with t the time constant in frames, a = 1 - b."""
    t = float(time_constant) * float(sampling_rate) / float(hop)
    b = (np.sqrt(1.0 + 4.0 * t * t) - 1.0) / (2.0 * t * t)
    return float(1.0 - b), float(b)


def pcen_ref(E, cfg: dict, sampling_rate: float, hop: int) -> np.ndarray:
    """The float64 specification.  E: [T, K] (or [T]) non-negative energies; cfg: pcen_config's dict.  Sequential over time:
        S = scale E,  M[0] = S[0],  M[t] = a M[t-1] + b S[t],  out = (S (eps + M)^-gain + bias)^power - bias^power"""
    S = cfg["scale"] * np.asarray(E, dtype=np.float64)
    a, b = smoother(cfg["time_constant"], sampling_rate, hop)
    M = np.empty_like(S)
    if S.shape[0]:
        M[0] = S[0]
    for t in range(1, S.shape[0]):
        M[t] = a * M[t - 1] + b * S[t]
    return pcen_values(S, M, cfg)


def pcen_bwd_ref(E, g_y, cfg: dict, sampling_rate: float, hop: int) -> np.ndarray:
    """The float64 specification of orcai_pcen_bwd's map g_y -> dE, sequential in time (include/orcai_hip.h).  E: [T, K] (or [T]) non-negative
    energies; g_y = dL/dy of pcen_ref's values y, the same shape -- the clip's gate and its 1 / (p_hi - p_lo) are the caller's, so an element that is
    clipped, or has u = 0, comes with g_y = 0 and contributes exactly nothing (a select).  With S, M, r = (eps + M)^-gain, u = S r + bias of pcen_ref:
        h = g_y power u^(power - 1),  d = h r,  q = -gain d S / (eps + M)
        lam[T-1] = q[T-1],  lam[t] = q[t] + a lam[t+1]
        dE[t] = scale (d[t] + b lam[t]) for t >= 1,  dE[0] = scale (d[0] + lam[0])   (M[0] = S[0]: coefficient 1, not b)"""
    S = cfg["scale"] * np.asarray(E, dtype=np.float64)
    g_y = np.asarray(g_y, dtype=np.float64)
    if g_y.shape != S.shape:
        raise ValueError(f"pcen_bwd_ref: g_y {g_y.shape} and E {S.shape} differ in shape")
    a, b = smoother(cfg["time_constant"], sampling_rate, hop)
    gain, bias, power, eps = cfg["gain"], cfg["bias"], cfg["power"], cfg["eps"]
    T = S.shape[0]
    M = np.empty_like(S)
    if T:
        M[0] = S[0]
    for t in range(1, T):
        M[t] = a * M[t - 1] + b * S[t]
    r = (eps + M) ** (-gain)
    u = S * r + bias
    live = g_y != 0
    h = np.zeros_like(S)
    h[live] = g_y[live] * power * u[live] ** (power - 1.0)
    d = h * r
    q = -gain * d * (S / (eps + M))
    dE = np.empty_like(S)
    lam = np.zeros_like(S[0]) if T else None
    for t in range(T - 1, -1, -1):
        lam = q[t] + a * lam
        dE[t] = cfg["scale"] * (d[t] + (b if t else 1.0) * lam)
    return dE


def pcen_values(S: np.ndarray, M: np.ndarray, cfg: dict) -> np.ndarray:
    """out of pcen_ref from the scaled energies and their smoothed copy (any float dtype; computed in that dtype).  bias^power is subtracted as the
    same power of the same number, so S = 0 gives exactly 0."""
    dt = S.dtype.type
    gain, bias, power, eps = dt(cfg["gain"]), dt(cfg["bias"]), dt(cfg["power"]), dt(cfg["eps"])
    with np.errstate(divide="ignore"):
        return (S * (eps + M) ** (-gain) + bias) ** power - (np.zeros_like(S) + bias) ** power

