"""Shared helpers of tests/test_denoise_grad.py and tests/test_denoise_grad_gpu.py: the denoised front end's forward restated in torch (any float
dtype; float64 is the reference orcai_denoised_spectrogram_bwd is checked against), its gradient by autograd with ref_db, the per-channel floor, p_lo
and p_hi detached, the same gradient by the written formula of include/orcai_hip.h, and the mask of elements whose gate is decided within rounding.

The forward follows include/orcai_hip.h (orcai_make_denoised_spectrogram) on top of tests/frontend_grad_ref.py (linear route: P of its STFT, the
leading k_crop bins, ref_db over ALL bins) and tests/mel_grad_ref.py (mel route: M = P W^T, ref_db over the bands):
    v = max(dB - ref_db, -80),  m[k] = sort(v[:, k])[nearest_rank_index(T, quantile)],  y = v - m,  out = (clip(y, p_lo, p_hi) - p_lo) / (p_hi - p_lo)
with p_lo / p_hi numpy's nearest-rank order statistics of y.  m, p_lo and p_hi are detached: constants of the backward, as ref_db is.  Recordings,
quantiles and the tie width are frontend_grad_ref's.  Test infrastructure: nothing in orcai_amd/ imports this file."""

from __future__ import annotations

import functools
import math

import torch

import frontend_grad_ref as G
import mel_grad_ref as M
from oracle import frontend_ref as FR

SR = G.SR
TOP_DB = G.TOP_DB
TIE_DB = G.TIE_DB
TIE_SHARE_MAX = 1e-3
AMIN = 1e-10
# Quantiles of the global clip per recording: frontend_grad_ref's.  (b) keeps q_lo = 0.10 for the reason given there, which the floor does not remove:
# its 6.7 % of floored elements become -80 - m[k] in y, still the lowest values of every channel, so q_lo = 0.01 would put p_lo among them, where each
# channel's floored frames all hold one value.  tests/test_denoise_grad.py asserts the tie share of every case below.
QUANTILES = G.QUANTILES
# name -> (route, recording, denoise quantile).  route: (nfft, hop) linear, or a case of mel_grad_ref (nfft, hop, n_mels, fmin, fmax, htk, norm).
LINEAR = ((512, 256), (2048, 300), (32, 16))  # wave per run; workgroup per run, hop does not divide nfft; the smallest size
MEL = (M.CASES[0], M.CASES[2], M.CASES[5])   # 512 / 256 / 64; 128 / 32 / 8 the smallest; 4096 / 1000 / 64: more than 64 KiB of LDS
CASES = {}
for _r in LINEAR + MEL:
    for _w in ("a", "b"):
        CASES["-".join(map(str, _r[:3])) + "-" + _w] = (_r, _w, 0.5)
CASES["512-256-a-q25"] = (LINEAR[0], "a", 0.25)  # another order statistic: the lower quartile
CASES["512-256-64-b-q25"] = (MEL[0], "b", 0.25)


def is_mel(route) -> bool:
    return len(route) > 2


def channels(route) -> int:
    return route[2] if is_mel(route) else G.k_crop_of(route[0])


def parameter(route, which: str, quantile: float = 0.5) -> dict:
    sp = M.parameter(route, which) if is_mel(route) else G.parameter(route[0], route[1], which)
    return dict(sp, denoise={"quantile": quantile})


def referenced_db(pcm: torch.Tensor, route, ref_db=None):
    """(X, dB, v, ref_db) of the route, [T][K] in pcm's dtype: X the power P of the kept bins (linear) or the band power M (mel), dB = 10 log10(max(X,
    1e-10)), v = max(dB - ref_db, -80); ref_db from the data (all bins / all bands, detached) when None."""
    _, _, P = G.stft_power(pcm, route[0], route[1])
    X = P @ M.dense_weights(route, pcm.dtype).T if is_mel(route) else P
    if ref_db is None:
        ref_db = (10.0 * torch.log10(torch.clamp(X.max(), min=AMIN))).detach()
    else:
        ref_db = torch.as_tensor(ref_db, dtype=pcm.dtype)
    if not is_mel(route):
        X = X[:, : channels(route)]
    db = 10.0 * torch.log10(torch.clamp(X, min=AMIN))
    return X, db, torch.maximum(db - ref_db, torch.as_tensor(-TOP_DB, dtype=pcm.dtype)), ref_db


def denoise_clip(v: torch.Tensor, quantile: float, quantiles, floor=None, bounds=None):
    """(out, y, m, p_lo, p_hi) from the referenced dB values v [T][K]: the per-column order statistic (floor when given), the subtraction, the global
    clip (bounds = (p_lo, p_hi) when given) and the normalisation.  m, p_lo, p_hi are constants of the graph."""
    if floor is None:
        m = torch.sort(v.detach(), dim=0).values[FR.nearest_rank_index(v.shape[0], quantile)]
    else:
        m = torch.as_tensor(floor, dtype=v.dtype)
    y = v - m
    if bounds is None:
        flat = torch.sort(y.detach().reshape(-1)).values
        p_lo = flat[FR.nearest_rank_index(flat.numel(), quantiles[0])]
        p_hi = flat[FR.nearest_rank_index(flat.numel(), quantiles[1])]
    else:
        p_lo, p_hi = (torch.as_tensor(b, dtype=v.dtype) for b in bounds)
    return (torch.clamp(y, min=p_lo, max=p_hi) - p_lo) / (p_hi - p_lo), y, m, p_lo, p_hi


def forward(pcm: torch.Tensor, route, quantile: float, quantiles, stats=None, floor=None):
    """The normalised denoised spectrogram [T][K] in pcm's dtype and a dict of intermediate values.  stats = (ref_db, p_lo, p_hi, m) are computed from
    the data when None -- but for m when floor f64[K] is given (a one-frame recording is its own floor: y = 0, no range) -- and either way they enter
    the graph as constants."""
    X, db, v, ref_db = referenced_db(pcm, route, None if stats is None else stats[0])
    out, y, m, p_lo, p_hi = denoise_clip(v, quantile, quantiles, floor if stats is None else stats[3], None if stats is None else stats[1:3])
    return out, {"X": X.detach(), "db": db.detach(), "v": v.detach(), "y": y.detach(), "m": m.detach(), "ref_db": float(ref_db), "p_lo": float(p_lo),
                 "p_hi": float(p_hi), "pmax": float(10.0 ** (float(ref_db) / 10.0))}


def tie_mask(aux: dict) -> torch.Tensor:
    """frontend_grad_ref's / mel_grad_ref's mask with v replaced by y in the two clip terms: y within TIE_DB of p_lo or p_hi, dB - ref_db within TIE_DB
    of the floor of the dB scale, or |X - 1e-10| < 1e-12."""
    y, db, X = aux["y"], aux["db"], aux["X"]
    return ((y - aux["p_lo"]).abs() < TIE_DB) | ((y - aux["p_hi"]).abs() < TIE_DB) | ((db - aux["ref_db"] + TOP_DB).abs() < TIE_DB) | ((X - AMIN).abs() < 1e-12)


def build_case(pcm_f32: torch.Tensor, route, quantile: float, quantiles, seed: int, floor=None) -> dict:
    x64 = pcm_f32.double().requires_grad_()
    out, aux = forward(x64, route, quantile, quantiles, floor=floor)
    mask = tie_mask(aux)
    g = torch.randn(out.shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float32)
    g[mask] = 0.0
    (dpcm,) = torch.autograd.grad(out, x64, g.double())
    return {"pcm": pcm_f32, "route": route, "quantile": quantile, "g": g, "stats": (aux["ref_db"], aux["p_lo"], aux["p_hi"], aux["m"]), "out64": out.detach(),
            "dpcm64": dpcm, "tie_share": float(mask.double().mean()), "aux": aux,
            "floored_share": float((aux["db"] - aux["ref_db"] <= -TOP_DB).double().mean())}


@functools.lru_cache(maxsize=None)
def case(name: str) -> dict:
    """Everything one of CASES needs, computed once in float64 and shared (treat as read-only): pcm f32, g f32 [T][K] (standard normal, zero on the tie
    mask), the float64 statistics (ref_db, p_lo, p_hi, m[K]), dpcm64 = the float64 gradient, the tie share."""
    route, which, quantile = CASES[name]
    seed = 7000000 + 1000 * route[0] + route[1] + (0 if which == "a" else 1) + (2 if quantile != 0.5 else 0) + (100000 * route[2] if is_mel(route) else 0)
    return build_case(torch.from_numpy(G.recording(which).copy()), route, quantile, QUANTILES[which], seed)


def dpcm_in(dtype, c: dict, g=None, profile=None) -> torch.Tensor:
    """The same formula evaluated by torch in `dtype` from the case's pcm and (float64, rounded) statistics; g and profile replace the case's."""
    x = c["pcm"].to(dtype).requires_grad_()
    ref_db, p_lo, p_hi, m = c["stats"]
    out, _ = forward(x, c["route"], c["quantile"], None, stats=(ref_db, p_lo, p_hi, m if profile is None else profile))
    (d,) = torch.autograd.grad(out, x, (c["g"] if g is None else g).to(dtype))
    return d


def f32_error_share(name: str) -> float:
    """max |dpcm_f32 - dpcm_f64| / max |dpcm_f64|: how far torch's own float32 evaluation is from the float64 one (the yardstick of the GPU bar)."""
    c = case(name)
    return float((dpcm_in(torch.float32, c).double() - c["dpcm64"]).abs().max() / c["dpcm64"].abs().max())


def g_db_by_formula(c: dict) -> torch.Tensor:
    """g_db of include/orcai_hip.h (orcai_denoised_spectrogram_bwd) in float64: the three gates written out, the floor subtracted before the compare."""
    ref_db, p_lo, p_hi, m = c["stats"]
    X, db, v, _ = referenced_db(c["pcm"].double(), c["route"], ref_db)
    y = v - m
    gate = (X > AMIN) & (db - ref_db > -TOP_DB) & (y > p_lo) & (y < p_hi)
    return torch.where(gate, c["g"].double() / (p_hi - p_lo), torch.zeros((), dtype=torch.float64))


def dpcm_by_formula(c: dict) -> torch.Tensor:
    """dpcm from g_db by the chain behind it, which is the plain front end's: dX = g_db 10 / (ln 10 X), then autograd of X alone (the STFT and, on the
    mel route, the filterbank), whose restatements tests/test_frontend_grad.py and tests/test_mel_grad.py pin."""
    x = c["pcm"].double().requires_grad_()
    X, _, _, _ = referenced_db(x, c["route"], c["stats"][0])
    g_db = g_db_by_formula(c)
    dX = g_db * 10.0 / (math.log(10.0) * torch.where(g_db != 0, X.detach(), torch.ones((), dtype=torch.float64)))
    (d,) = torch.autograd.grad(X, x, dX)
    return d


def stats_tensor(c: dict, device, ref_db_slot: float = 0.0) -> torch.Tensor:
    """The f32[6] statistics tensor as orcai_frontend_stats_dev leaves it behind orcai_make_denoised_spectrogram: {pmax, 0, p_lo(y), p_hi(y), the same two
    raw}.  ref_db_slot: what to put where ref_db reads 0 (the backward must never read it)."""
    _, p_lo, p_hi, _ = c["stats"]
    return torch.tensor([c["aux"]["pmax"], ref_db_slot, p_lo, p_hi, p_lo, p_hi], dtype=torch.float32, device=device)


def profile_tensor(c: dict, device) -> torch.Tensor:
    return c["stats"][3].to(torch.float32).to(device)


if __name__ == "__main__":  # prints the table of constants kept in tests/test_denoise_grad_gpu.py
    for name, (route, w, q) in CASES.items():
        c = case(name)
        print(f'    "{name}": {f32_error_share(name):.2e},  # quantile {q}: tie share {c["tie_share"]:.1e}, floored {c["floored_share"]:.1e}')
