"""Shared helpers of tests/test_mel_grad.py and tests/test_mel_grad_gpu.py: the mel front end's forward restated in torch (any float dtype;
float64 is the reference orcai_mel_spectrogram_bwd is checked against), its gradient by autograd with the three statistics detached, the same
gradient by the written formula of include/orcai_hip.h, and the mask of elements whose gate is decided within rounding.

The forward follows include/orcai_hip.h (orcai_make_mel_spectrogram): P of tests/frontend_grad_ref.py's STFT, M = P W^T with W the f32 filterbank
mel.dense_from_table(mel.band_table(...)) promoted to the working dtype, Ldb = 10 log10(max(M, 1e-10)), v = max(Ldb - ref_db, -80),
out = (clip(v, p_lo, p_hi) - p_lo) / (p_hi - p_lo), layout [frame][band].  ref_db is taken over all bands, p_lo / p_hi are numpy's nearest-rank
order statistics.  Recordings, quantiles and the tie width are frontend_grad_ref's.  Test infrastructure: nothing in orcai_amd/ imports this file."""

from __future__ import annotations

import functools
import math

import numpy as np
import torch

import frontend_grad_ref as G
from oracle import frontend_ref as FR
from orcai_amd import mel

SR = G.SR
TOP_DB = G.TOP_DB
QUANTILES = G.QUANTILES
TIE_DB = G.TIE_DB
TIE_SHARE_MAX = 1e-3
AMIN = 1e-10
# (nfft, hop, n_mels, fmin, fmax, htk, norm)
CASES = (
    (512, 256, 64, 0.0, 24000.0, False, "slaney"),     # the documented shape, widest top bands
    (512, 255, 128, 6000.0, 24000.0, False, "slaney"),  # odd hop, narrow bands, bins below fmin get nothing
    (128, 32, 8, 0.0, 24000.0, True, None),            # smallest size, fewest and widest bands, unnormalised weights
    (1024, 512, 40, 0.0, 16000.0, True, None),         # first workgroup-per-run size, bins above fmax get nothing
    (2048, 300, 64, 0.0, 24000.0, False, "slaney"),    # hop does not divide nfft
    (4096, 1000, 64, 0.0, 16000.0, False, "slaney"),   # largest size, LDS at its limit
)


def parameter(case, which: str) -> dict:
    nfft, hop, n_mels, fmin, fmax, htk, norm = case
    return {"sampling_rate": SR, "nfft": nfft, "n_overlap": hop, "freq_range": [fmin, fmax], "quantiles": list(QUANTILES[which]),
            "mel": {"n_mels": n_mels, "fmin": fmin, "fmax": fmax, "htk": htk, "norm": norm}}


def table_of(case) -> dict:
    nfft, _, n_mels, fmin, fmax, htk, norm = case
    return mel.band_table(SR, nfft, n_mels, fmin, fmax, htk, norm)


def dense_weights(case, dtype=torch.float64) -> torch.Tensor:
    """f32 weights [n_mels][1 + nfft/2] as the kernels read them, in dtype."""
    return torch.from_numpy(mel.dense_from_table(table_of(case), case[0])).to(dtype)


def forward(pcm: torch.Tensor, case, quantiles, stats=None):
    """The normalised mel spectrogram [T][n_mels] in pcm's dtype and a dict of intermediate values.  stats = (ref_db, p_lo, p_hi) are computed from the
    data when None; either way they enter the graph as constants (detached)."""
    nfft, hop = case[0], case[1]
    _, _, P = G.stft_power(pcm, nfft, hop)
    M = P @ dense_weights(case, pcm.dtype).T
    db = 10.0 * torch.log10(torch.clamp(M, min=AMIN))
    if stats is None:
        ref_db = (10.0 * torch.log10(torch.clamp(M.max(), min=AMIN))).detach()
    else:
        ref_db = torch.as_tensor(stats[0], dtype=pcm.dtype)
    v = torch.maximum(db - ref_db, torch.as_tensor(-TOP_DB, dtype=pcm.dtype))
    if stats is None:
        flat = torch.sort(v.detach().reshape(-1)).values
        p_lo = flat[FR.nearest_rank_index(flat.numel(), quantiles[0])]
        p_hi = flat[FR.nearest_rank_index(flat.numel(), quantiles[1])]
    else:
        p_lo, p_hi = (torch.as_tensor(s, dtype=pcm.dtype) for s in stats[1:])
    out = (torch.clamp(v, min=p_lo, max=p_hi) - p_lo) / (p_hi - p_lo)
    return out, {"M": M.detach(), "db": db.detach(), "v": v.detach(), "ref_db": float(ref_db), "p_lo": float(p_lo), "p_hi": float(p_hi)}


def tie_mask(aux: dict) -> torch.Tensor:
    """True where a gate of the backward is decided within rounding: v within TIE_DB of p_lo or p_hi, Ldb - ref_db within TIE_DB of the floor, or
    |M - 1e-10| < 1e-12."""
    v, db, M = aux["v"], aux["db"], aux["M"]
    return ((v - aux["p_lo"]).abs() < TIE_DB) | ((v - aux["p_hi"]).abs() < TIE_DB) | ((db - aux["ref_db"] + TOP_DB).abs() < TIE_DB) | ((M - AMIN).abs() < 1e-12)


def build_case(pcm_f32: torch.Tensor, case, quantiles, seed: int) -> dict:
    x64 = pcm_f32.double().requires_grad_()
    out, aux = forward(x64, case, quantiles)
    mask = tie_mask(aux)
    g = torch.randn(out.shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float32)
    g[mask] = 0.0
    (dpcm,) = torch.autograd.grad(out, x64, g.double())
    stats = (aux["ref_db"], aux["p_lo"], aux["p_hi"])
    return {"pcm": pcm_f32, "g": g, "stats": stats, "out64": out.detach(), "dpcm64": dpcm, "tie_share": float(mask.double().mean()), "aux": aux,
            "floored_share": float((aux["db"] - aux["ref_db"] <= -TOP_DB).double().mean())}


@functools.lru_cache(maxsize=None)
def case(which: str, index: int) -> dict:
    """Everything one (recording, CASES[index]) pair needs, computed once in float64 and shared (treat as read-only): pcm f32, g f32 [T][n_mels]
    (standard normal, zero on the tie mask), the float64 statistics, dpcm64 = the float64 gradient, the tie share."""
    c = CASES[index]
    return build_case(torch.from_numpy(G.recording(which).copy()), c, QUANTILES[which], 100000 * index + 1000 * c[2] + c[1] + (0 if which == "a" else 1))


def dpcm_in(dtype, c: dict, mel_case, quantiles) -> torch.Tensor:
    """The same formula evaluated by torch in `dtype` from the case's pcm, g and (float64, rounded) statistics."""
    x = c["pcm"].to(dtype).requires_grad_()
    out, _ = forward(x, mel_case, quantiles, stats=c["stats"])
    (d,) = torch.autograd.grad(out, x, c["g"].to(dtype))
    return d


def f32_error_share(which: str, index: int) -> float:
    """max |dpcm_f32 - dpcm_f64| / max |dpcm_f64|: how far torch's own float32 evaluation is from the float64 one (the yardstick of the GPU bar)."""
    c = case(which, index)
    return float((dpcm_in(torch.float32, c, CASES[index], QUANTILES[which]).double() - c["dpcm64"]).abs().max() / c["dpcm64"].abs().max())


def dpcm_by_formula(c: dict, mel_case) -> torch.Tensor:
    """The definition in include/orcai_hip.h evaluated step by step in float64: gates, dM, dP as a two-term gather (one even and one odd band per bin),
    the inverse transform as an explicit cosine / sine sum, the overlap-add."""
    nfft, hop = mel_case[0], mel_case[1]
    half = nfft // 2
    t = table_of(mel_case)
    ref_db, p_lo, p_hi = c["stats"]
    Re, Im, P = G.stft_power(c["pcm"].double(), nfft, hop)
    W = dense_weights(mel_case)
    M = P @ W.T
    Ldb = 10.0 * torch.log10(torch.clamp(M, min=AMIN))
    v = torch.clamp(Ldb - ref_db, min=-TOP_DB)
    gate = (M > AMIN) & (Ldb - ref_db > -TOP_DB) & (v > p_lo) & (v < p_hi)
    g_L = torch.where(gate, c["g"].double() / (p_hi - p_lo), torch.zeros((), dtype=torch.float64))
    dM = g_L * 10.0 / (math.log(10.0) * torch.where(gate, M, torch.ones((), dtype=torch.float64)))
    e_band, e_w, o_band, o_w = (torch.from_numpy(a) for a in bin_table(t, nfft))
    dP = e_w.double() * dM[:, e_band.long()] + o_w.double() * dM[:, o_band.long()]
    dRe, dIm = 2.0 * Re * dP, 2.0 * Im * dP
    n = torch.arange(nfft, dtype=torch.float64)
    k = torch.arange(half + 1, dtype=torch.float64)
    ang = 2.0 * math.pi * torch.outer(k, n) / nfft
    win = 0.5 - 0.5 * torch.cos(2.0 * math.pi * n / nfft)
    dframe = win * (dRe @ torch.cos(ang) - dIm @ torch.sin(ang))
    N = c["pcm"].numel()
    dpad = torch.zeros(N + nfft + hop, dtype=torch.float64)
    for f in range(dframe.shape[0]):
        dpad[f * hop : f * hop + nfft] += dframe[f]
    return dpad[half : half + N]


def bin_table(table: dict, nfft: int):
    """(even_band, even_weight, odd_band, odd_weight), each [1 + nfft/2]: the one even-numbered and the one odd-numbered band that can cover a bin and
    the bin's weight in it (band 0 / 1 with weight 0 where none does) -- the gather orcai_mel_spectrogram_bwd's kernel builds in LDS, restated."""
    nb = 1 + nfft // 2
    band = [np.zeros(nb, dtype=np.int32), np.ones(nb, dtype=np.int32)]
    w = [np.zeros(nb, dtype=np.float32), np.zeros(nb, dtype=np.float32)]
    for m in range(table["lo"].size):
        lo, hi, off = int(table["lo"][m]), int(table["hi"][m]), int(table["off"][m])
        assert not w[m & 1][lo:hi].any(), f"bands of equal parity overlap at band {m}"
        band[m & 1][lo:hi] = m
        w[m & 1][lo:hi] = table["weights"][off : off + hi - lo]
    return band[0], w[0], band[1], w[1]


def parity_rule_holds(table: dict) -> bool:
    """band_hi[m] <= band_lo[m + 2] for every m (the launcher's condition, over non-empty bands)."""
    lo, hi = table["lo"], table["hi"]
    return bool(np.all(hi[:-2] <= lo[2:]))


def stats_tensor(c: dict, device) -> torch.Tensor:
    return G.stats_tensor(c, device)


if __name__ == "__main__":  # prints the table of constants kept in tests/test_mel_grad_gpu.py
    for w in ("a", "b"):
        for i, mc in enumerate(CASES):
            c = case(w, i)
            print(f'    ("{w}", {i}): {f32_error_share(w, i):.2e},  # {mc[0]} / {mc[1]} / {mc[2]}: tie share {c["tie_share"]:.1e}, floored {c["floored_share"]:.1e}')
