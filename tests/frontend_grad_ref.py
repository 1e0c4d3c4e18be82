"""Shared helpers of tests/test_frontend_grad.py and tests/test_frontend_grad_gpu.py: the seeded test recordings, the front end's forward
restated in torch (any float dtype; float64 is the reference the HIP backward is checked against), its gradient by autograd with the three
statistics detached, and the mask of elements whose gate is decided within rounding.

The forward follows include/orcai_hip.h (orcai_make_spectrogram): centred, zero-padded, periodic-Hann STFT, P = Re^2 + Im^2,
db = 10 log10(max(P, 1e-10)), v = max(db - ref_db, -80), out = (clip(v, p_lo, p_hi) - p_lo) / (p_hi - p_lo) on the leading k_crop bins,
layout [frame][bin].  ref_db is taken over ALL bins, p_lo / p_hi are the order statistics numpy's percentile(method="nearest") picks among the
kept bins (oracle.frontend_ref.nearest_rank_index).  tests/test_frontend_grad.py pins this restatement to oracle.frontend_ref."""

from __future__ import annotations

import functools
import math

import numpy as np
import torch

from oracle import frontend_ref as FR

SR = 48000
TOP_DB = 80.0
N_SAMPLES = 3 * SR + 17
# (nfft, hop) of the kernel test: the tuned forward's size, hop = nfft / 4, a workgroup-per-run size, a hop that does not divide nfft, the smallest size
SIZES = ((512, 256), (256, 64), (1024, 512), (2048, 300), (32, 16))
# Quantiles per input.  (a): orcai-V1's.  (b): 0.2 s of 3 s is digital silence, so 6.7 % of the elements sit on the -80 dB floor; with q_lo = 0.01 the
# lower clip bound WOULD BE that floor and every floored element would tie with p_lo (far more than the 1e-3 of near-ties the tests allow), so (b)
# takes q_lo = 0.10, above the floored share: p_lo is an ordinary value again, and the floor and the P <= 1e-10 gate are still exercised.
QUANTILES = {"a": (0.01, 0.999), "b": (0.10, 0.999)}
TIE_DB = 1e-3  # a gate closer than this (in dB) counts as decided within rounding
TIE_SHARE_MAX = 1e-3


@functools.lru_cache(maxsize=None)
def recording(which: str) -> np.ndarray:
    """(a) white noise of amplitude 0.1 plus two chirps; (b) the same with 0.2 s of digital silence and one loud tone.  f32[3 s * 48 kHz + 17]."""
    rng = np.random.default_rng(20240611)
    t = np.arange(N_SAMPLES, dtype=np.float64) / SR
    y = rng.uniform(-0.1, 0.1, N_SAMPLES)
    y += 0.3 * np.sin(2 * np.pi * (2000.0 * t + 0.5 * (7000.0 / 3.0) * t * t))  # 2 kHz -> 9 kHz
    y += 0.2 * np.sin(2 * np.pi * (12000.0 * t - 0.5 * (7000.0 / 3.0) * t * t))  # 12 kHz -> 5 kHz
    if which == "b":
        tone = (t >= 2.0) & (t < 2.5)
        y[tone] += 0.9 * np.sin(2 * np.pi * 3000.0 * t[tone])
        y[int(1.0 * SR) : int(1.2 * SR)] = 0.0
    elif which != "a":
        raise KeyError(which)
    out = y.astype(np.float32)
    out.setflags(write=False)
    return out


def k_crop_of(nfft: int, freq_hi: float = 16000.0) -> int:
    return FR.crop_indices(FR.fft_frequencies_ref(SR, nfft), [0, freq_hi])[1]


def parameter(nfft: int, hop: int, which: str, freq_hi: float = 16000.0) -> dict:
    return {"sampling_rate": SR, "nfft": nfft, "n_overlap": hop, "freq_range": [0, freq_hi], "quantiles": list(QUANTILES[which])}


def stft_power(pcm: torch.Tensor, nfft: int, hop: int):
    """Re, Im, P of the centred STFT, [T][1 + nfft/2], in pcm's dtype."""
    pad = nfft // 2
    frames = torch.nn.functional.pad(pcm, (pad, pad)).unfold(0, nfft, hop)
    n = torch.arange(nfft, dtype=torch.float64)
    win = (0.5 - 0.5 * torch.cos(2.0 * math.pi * n / nfft)).to(pcm.dtype)
    X = torch.fft.rfft(frames * win, dim=1)
    return X.real, X.imag, X.real**2 + X.imag**2


def forward(pcm: torch.Tensor, nfft: int, hop: int, k_crop: int, quantiles, stats=None):
    """The normalised spectrogram [T][k_crop] in pcm's dtype and a dict of the intermediate values.  stats = (ref_db, p_lo, p_hi) are computed
    from the data when None; either way they enter the graph as constants (detached)."""
    _, _, P = stft_power(pcm, nfft, hop)
    db = 10.0 * torch.log10(torch.clamp(P, min=1e-10))
    if stats is None:
        ref_db = (10.0 * torch.log10(torch.clamp(P.max(), min=1e-10))).detach()
    else:
        ref_db = torch.as_tensor(stats[0], dtype=pcm.dtype)
    floor = torch.as_tensor(-TOP_DB, dtype=pcm.dtype)
    v = torch.maximum(db - ref_db, floor)[:, :k_crop]
    if stats is None:
        flat = torch.sort(v.detach().reshape(-1)).values
        p_lo = flat[FR.nearest_rank_index(flat.numel(), quantiles[0])]
        p_hi = flat[FR.nearest_rank_index(flat.numel(), quantiles[1])]
    else:
        p_lo, p_hi = (torch.as_tensor(s, dtype=pcm.dtype) for s in stats[1:])
    out = (torch.clamp(v, min=p_lo, max=p_hi) - p_lo) / (p_hi - p_lo)
    return out, {"P": P[:, :k_crop].detach(), "db": db[:, :k_crop].detach(), "v": v.detach(), "ref_db": float(ref_db), "p_lo": float(p_lo), "p_hi": float(p_hi)}


def tie_mask(aux: dict) -> torch.Tensor:
    """True where a gate of the backward is decided within rounding: v within TIE_DB of p_lo or p_hi, db - ref_db within TIE_DB of the floor,
    or P within 1 % of 1e-10."""
    v, db, P = aux["v"], aux["db"], aux["P"]
    return ((v - aux["p_lo"]).abs() < TIE_DB) | ((v - aux["p_hi"]).abs() < TIE_DB) | ((db - aux["ref_db"] + TOP_DB).abs() < TIE_DB) | ((P - 1e-10).abs() < 1e-12)


@functools.lru_cache(maxsize=None)
def case(which: str, nfft: int, hop: int) -> dict:
    """Everything one (input, nfft, hop) case needs, computed once in float64 and shared (treat as read-only): pcm f32, g f32 [T][K] (standard
    normal, zero on the tie mask), the float64 statistics, dpcm64 = the float64 gradient, and the tie share."""
    pcm = torch.from_numpy(recording(which).copy())
    k = k_crop_of(nfft)
    x64 = pcm.double().requires_grad_()
    out, aux = forward(x64, nfft, hop, k, QUANTILES[which])
    mask = tie_mask(aux)
    gen = torch.Generator().manual_seed(1000 * nfft + hop + (0 if which == "a" else 1))
    g = torch.randn(out.shape, generator=gen, dtype=torch.float32)
    g[mask] = 0.0
    (dpcm,) = torch.autograd.grad(out, x64, g.double())
    stats = (aux["ref_db"], aux["p_lo"], aux["p_hi"])
    return {"pcm": pcm, "g": g, "k_crop": k, "stats": stats, "out64": out.detach(), "dpcm64": dpcm, "tie_share": float(mask.double().mean()), "aux": aux}


def dpcm_in(dtype, which: str, nfft: int, hop: int) -> torch.Tensor:
    """The same formula evaluated by torch in `dtype` from the case's pcm, g and (float64, rounded) statistics."""
    c = case(which, nfft, hop)
    x = c["pcm"].to(dtype).requires_grad_()
    out, _ = forward(x, nfft, hop, c["k_crop"], QUANTILES[which], stats=c["stats"])
    (d,) = torch.autograd.grad(out, x, c["g"].to(dtype))
    return d


def f32_error_share(which: str, nfft: int, hop: int) -> float:
    """max |dpcm_f32 - dpcm_f64| / max |dpcm_f64|: how far torch's own float32 evaluation is from the float64 one (the yardstick of the GPU bar)."""
    c = case(which, nfft, hop)
    return float((dpcm_in(torch.float32, which, nfft, hop).double() - c["dpcm64"]).abs().max() / c["dpcm64"].abs().max())


def stats_tensor(c: dict, device) -> torch.Tensor:
    """The f32[6] statistics tensor of the C ABI {pmax, ref_db, p_lo, p_hi, sel_lo_raw, sel_hi_raw} from a case's float64 statistics."""
    ref_db, p_lo, p_hi = c["stats"]
    return torch.tensor([10.0 ** (ref_db / 10.0), ref_db, p_lo, p_hi, p_lo + ref_db, p_hi + ref_db], dtype=torch.float32, device=device)


if __name__ == "__main__":  # prints the table of constants kept in tests/test_frontend_grad_gpu.py
    for w in ("a", "b"):
        for nfft, hop in SIZES:
            print(f'    ("{w}", {nfft}, {hop}): {f32_error_share(w, nfft, hop):.2e},  # tie share {case(w, nfft, hop)["tie_share"]:.1e}')
