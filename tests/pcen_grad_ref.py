"""Shared helpers of tests/test_pcen_grad.py and tests/test_pcen_grad_gpu.py: the PCEN front end's forward restated in torch (any float dtype; float64
is the reference orcai_pcen_spectrogram_bwd is checked against) with PCEN written as the sequential recurrence, its gradient by autograd with the two
statistics given, the mask of elements whose clip gate is decided within rounding, and the inputs and float32 restatement of the scan-alone test.

The forward follows include/orcai_hip.h (orcai_make_pcen_spectrogram): E = |X| of the kept bins (linear route) or the band power P W^T (mel route) of
tests/frontend_grad_ref.py's STFT, S = scale E, M[0] = S[0], M[t] = a M[t-1] + b S[t], y = (S (eps + M)^-gain + bias)^power - bias^power,
out = (clip(y, p_lo, p_hi) - p_lo) / (p_hi - p_lo), layout [frame][channel]; p_lo / p_hi are numpy's nearest-rank order statistics of y and enter the
graph as constants.  Recordings and quantiles are frontend_grad_ref's: 3 s at hop 256 are 563 frames, two full chunks of the scan and a short one.
Test infrastructure: nothing in orcai_amd/ imports this file."""

from __future__ import annotations

import functools

import numpy as np
import torch

import frontend_grad_ref as G
import mel_grad_ref as MG
from oracle import frontend_ref as FR
from orcai_amd import pcen

SR = G.SR
QUANTILES = G.QUANTILES
# A gate closer than this to p_lo or p_hi, relative to max(|y|, bias^power), counts as decided within rounding: more than 11 x the largest error of the
# forward kernels on record (8.72e-6 of the same measure).
TIE_REL = 1e-4
TIE_SHARE_MAX = 1e-3  # the project's cap (frontend_grad_ref, mel_grad_ref)
CFG = pcen.pcen_config({"nfft": 512, "pcen": {}})  # the defaults
# ("lin", nfft, hop) or ("mel", a case of mel_grad_ref): the shapes of the end-to-end test
CASES = (
    ("lin", 512, 256),
    ("lin", 1024, 512),
    ("lin", 2048, 300),
    ("lin", 32, 16),
    ("mel", MG.CASES[0]),  # 512 / 256 / 64
    ("mel", MG.CASES[2]),  # 128 / 32 / 8
    ("mel", MG.CASES[5]),  # 4096 / 1000 / 64
)


def sizes(case) -> tuple[int, int]:
    return (case[1], case[2]) if case[0] == "lin" else (case[1][0], case[1][1])


def label(case) -> str:
    return f"linear {case[1]} / {case[2]}" if case[0] == "lin" else f"mel {case[1][0]} / {case[1][1]} / {case[1][2]}"


def quantiles_of(case, which: str) -> tuple[float, float]:
    """Linear route: frontend_grad_ref's.  Mel route: PCEN of the band powers of these recordings crowds towards 0 -- 1 % and 10 % of the values lie below
    0.0014 and 0.010, and 2e-3 to 5e-3 of all elements would be within the tie width (1.4e-4) of such a lower bound, above the cap -- so the lower
    quantile is 0.30 there (p_lo between 0.06 and 0.2), which still leaves the silence of (b) and the quietest bands clipped."""
    return QUANTILES[which] if case[0] == "lin" else (0.30, QUANTILES[which][1])


def parameter(case, which: str, pcen_parameter: dict | None = None) -> dict:
    sp = G.parameter(case[1], case[2], which) if case[0] == "lin" else MG.parameter(case[1], which)
    sp["quantiles"] = list(quantiles_of(case, which))
    sp["pcen"] = dict(pcen_parameter or {})
    return sp


def energies(pcm: torch.Tensor, case) -> torch.Tensor:
    """E [T][K] in pcm's dtype.  The magnitude's derivative at |X| = 0 is taken as 0 (a select), as the kernel does."""
    nfft, hop = sizes(case)
    _, _, P = G.stft_power(pcm, nfft, hop)
    if case[0] == "mel":
        return P @ MG.dense_weights(case[1], pcm.dtype).T
    P = P[:, : G.k_crop_of(nfft)]
    pos = P > 0
    return torch.where(pos, torch.sqrt(torch.where(pos, P, torch.ones_like(P))), torch.zeros_like(P))


def pcen_torch(E: torch.Tensor, cfg: dict, sampling_rate: float, hop: int) -> torch.Tensor:
    """pcen.pcen_ref in torch, E's dtype, differentiable: the recurrence frame by frame."""
    a, b = pcen.smoother(cfg["time_constant"], sampling_rate, hop)
    S = cfg["scale"] * E
    rows = [S[0]]
    for t in range(1, S.shape[0]):
        rows.append(a * rows[-1] + b * S[t])
    M = torch.stack(rows)
    bias = torch.as_tensor(cfg["bias"], dtype=E.dtype)
    return (S * (cfg["eps"] + M) ** (-cfg["gain"]) + bias) ** cfg["power"] - bias ** cfg["power"]


def forward(pcm: torch.Tensor, case, quantiles, stats=None, cfg: dict = CFG):
    """The normalised PCEN spectrogram [T][K] in pcm's dtype and a dict of intermediate values.  stats = (p_lo, p_hi) are computed from the data when
    None; either way they are constants of the graph."""
    y = pcen_torch(energies(pcm, case), cfg, SR, sizes(case)[1])
    if stats is None:
        flat = torch.sort(y.detach().reshape(-1)).values
        p_lo = flat[FR.nearest_rank_index(flat.numel(), quantiles[0])]
        p_hi = flat[FR.nearest_rank_index(flat.numel(), quantiles[1])]
    else:
        p_lo, p_hi = (torch.as_tensor(s, dtype=pcm.dtype) for s in stats)
    out = (torch.clamp(y, min=p_lo, max=p_hi) - p_lo) / (p_hi - p_lo)
    return out, {"y": y.detach(), "p_lo": float(p_lo), "p_hi": float(p_hi)}


def tie_mask_of(y, p_lo: float, p_hi: float, cfg: dict = CFG):
    """True where the clip's gate is decided within rounding (torch or numpy)."""
    floor = cfg["bias"] ** cfg["power"]
    width = TIE_REL * (abs(y).clip(floor) if isinstance(y, np.ndarray) else y.abs().clamp(min=floor))
    return (abs(y - p_lo) < width) | (abs(y - p_hi) < width)


def build_case(pcm_f32: torch.Tensor, case, quantiles, seed: int, cfg: dict = CFG) -> dict:
    x64 = pcm_f32.double().requires_grad_()
    out, aux = forward(x64, case, quantiles, cfg=cfg)
    mask = tie_mask_of(aux["y"], aux["p_lo"], aux["p_hi"], cfg)
    g = torch.randn(out.shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float32)
    g[mask] = 0.0
    (dpcm,) = torch.autograd.grad(out, x64, g.double())
    return {"pcm": pcm_f32, "g": g, "stats": (aux["p_lo"], aux["p_hi"]), "out64": out.detach(), "dpcm64": dpcm, "tie_share": float(mask.double().mean()), "aux": aux}


@functools.lru_cache(maxsize=None)
def case(which: str, index: int) -> dict:
    """Everything one (recording, CASES[index]) pair needs, computed once in float64 and shared (treat as read-only): pcm f32, g f32 [T][K] (standard
    normal, zero on the tie mask), the float64 statistics, dpcm64 = the float64 gradient, the tie share."""
    return build_case(torch.from_numpy(G.recording(which).copy()), CASES[index], quantiles_of(CASES[index], which), 7000 + 10 * index + (0 if which == "a" else 1))


def dpcm_in(dtype, c: dict, pcen_case, cfg: dict = CFG) -> torch.Tensor:
    """The same chain evaluated by torch in `dtype` from the case's pcm, g and (float64, rounded) statistics."""
    x = c["pcm"].to(dtype).requires_grad_()
    out, _ = forward(x, pcen_case, None, stats=c["stats"], cfg=cfg)
    (d,) = torch.autograd.grad(out, x, c["g"].to(dtype))
    return d


def f32_error_share(c: dict, pcen_case) -> float:
    """max |dpcm_f32 - dpcm_f64| / max |dpcm_f64|: how far torch's own float32 evaluation is from the float64 one (the yardstick of the GPU bar)."""
    return float((dpcm_in(torch.float32, c, pcen_case).double() - c["dpcm64"]).abs().max() / c["dpcm64"].abs().max())


def stats_tensor(c: dict, device) -> torch.Tensor:
    """The f32[6] statistics tensor of the C ABI as a PCEN run leaves it: pmax and ref_db 0, p_lo / p_hi twice."""
    p_lo, p_hi = c["stats"]
    return torch.tensor([0.0, 0.0, p_lo, p_hi, p_lo, p_hi], dtype=torch.float32, device=device)


# ------------------------------------------------------------------------------------------------ the energy backwards alone
ENERGY_CASES = (("lin", 512, 256), ("lin", 2048, 300), ("mel", MG.CASES[0]), ("mel", MG.CASES[4]))  # 512 / 256 and 2048 / 300 on either route


@functools.lru_cache(maxsize=None)
def energy_case(index: int) -> dict:
    """Recording (b), ENERGY_CASES[index]: gE f32 [T][K] standard normal, dpcm64 = the float64 gradient of sum(gE E), and torch's float32 evaluation of it."""
    pc = ENERGY_CASES[index]
    pcm = torch.from_numpy(G.recording("b").copy())
    x64 = pcm.double().requires_grad_()
    E = energies(x64, pc)
    gE = torch.randn(E.shape, generator=torch.Generator().manual_seed(8000 + index), dtype=torch.float32)
    (d64,) = torch.autograd.grad(E, x64, gE.double())
    x32 = pcm.clone().requires_grad_()
    (d32,) = torch.autograd.grad(energies(x32, pc), x32, gE)
    return {"pcm": pcm, "gE": gE, "dpcm64": d64, "f32_share": float((d32.double() - d64).abs().max() / d64.abs().max())}


# ------------------------------------------------------------------------------------------------ the scan alone
SCAN_SHAPES = ((1, 171), (2, 1), (255, 64), (256, 65), (257, 171), (513, 63), (1030, 171), (4501, 8))  # (T, K); 4501 frames are 18 chunks
# name -> (pcen parameter, sampling rate, hop, smallest energy, decades of the columns' scales).  "long": a^256 = 0.58, carries across chunks matter.
# "a0": one frame is 2^26 time constants, for which pcen.smoother returns b = 1 and a = 0 exactly; M = S then, the values span only
# (scale E)^0.02, and columns of different scale would fill the gaps the clip bounds are to sit in -- one scale for all columns there.
SCAN_PARAMETERS = {
    "default": ({}, SR, 256, 0.0, (-6, -2)),
    "long": ({"time_constant": 2.5}, SR, 256, 0.0, (-6, -2)),
    "gain0": ({"gain": 0.0}, SR, 256, 0.0, (-6, -2)),
    "power1": ({"power": 1.0}, SR, 256, 0.0, (-6, -2)),
    "bias0": ({"bias": 0.0}, SR, 256, 1e-3, (-3, -1)),
    "a0": ({"time_constant": 2.0**-26}, 1, 1, 0.0, (-4, -4)),
}


def scan_cfg(name: str) -> tuple[dict, float, int]:
    p, sr, hop = SCAN_PARAMETERS[name][:3]
    return pcen.pcen_config({"nfft": 512, "pcen": p}), sr, hop


def pcen_m(S: np.ndarray, a, b) -> np.ndarray:
    M = np.empty_like(S)
    M[0] = S[0]
    for t in range(1, S.shape[0]):
        M[t] = a * M[t - 1] + b * S[t]
    return M


def pcen_bwd_f32(E, g_y, cfg: dict, sampling_rate: float, hop: int) -> np.ndarray:
    """pcen.pcen_bwd_ref with every operation in float32, sequential over time (it knows nothing of the kernel's chunks): the yardstick of the scan's bar."""
    f = np.float32
    a, b = (f(v) for v in pcen.smoother(cfg["time_constant"], sampling_rate, hop))
    scale, gain, bias, power, eps = (f(cfg[k]) for k in ("scale", "gain", "bias", "power", "eps"))
    S = scale * np.asarray(E, dtype=f)
    g_y = np.asarray(g_y, dtype=f)
    M = pcen_m(S, a, b)
    r = (eps + M) ** (-gain)
    u = S * r + bias
    live = g_y != 0
    h = np.zeros_like(S)
    h[live] = g_y[live] * power * u[live] ** (power - f(1))
    d = h * r
    q = -gain * (d * (S / (eps + M)))
    dE = np.empty_like(S)
    lam = np.zeros_like(S[0])
    for t in range(S.shape[0] - 1, -1, -1):
        lam = q[t] + a * lam
        dE[t] = scale * (d[t] + (b if t else f(1)) * lam)
    assert dE.dtype == f
    return dE


def scan_energies(T: int, K: int, e_min: float, decades, rng) -> np.ndarray:
    """f32 [T][K] = e_min + c[k] v: a scale per column, log-uniform over the given decades, times v from three clusters -- a tenth near zero (half of it
    exact zeros where e_min allows them), eight tenths around 1, a tenth around 6.  The clusters leave gaps in the PCEN values for the two clip bounds
    to sit in, so that about a tenth is clipped at each end and few gates are near-ties."""
    which = rng.uniform(size=(T, K))
    v = np.where(which < 0.1, rng.uniform(0.0, 0.01, (T, K)), np.where(which < 0.9, rng.uniform(0.3, 1.5, (T, K)), rng.uniform(4.0, 8.0, (T, K))))
    if e_min == 0:
        v[which < 0.05] = 0.0
    return (e_min + 10.0 ** rng.uniform(decades[0], decades[1], K) * v).astype(np.float32)


def bound_in_a_gap(flat: np.ndarray, lo: float, hi: float, floor: float) -> float:
    """The midpoint of the relatively widest gap between neighbours of the sorted values flat, among the ranks from lo n to hi n."""
    n = flat.size
    i0 = min(int(lo * n), n - 2)
    i1 = min(max(int(hi * n), i0 + 1), n - 1)
    gaps = (flat[i0 + 1 : i1 + 1] - flat[i0:i1]) / np.maximum(flat[i0 + 1 : i1 + 1], floor)
    i = i0 + int(np.argmax(gaps))
    return float(np.float32(0.5 * (flat[i] + flat[i + 1])))


@functools.lru_cache(maxsize=None)
def scan_case(shape_index: int, name: str) -> dict:
    """E f32 [T][K] (scan_energies), g f32 standard normal and zero on the tie mask, (p_lo, p_hi) in the widest gaps of the float64 PCEN values around
    their 10 % and 90 % ranks (fewer than 8 elements: nothing is clipped), g_y = the gated g / (p_hi - p_lo), dE64 = pcen_bwd_ref and the float32
    restatement's deviation from it as a share of max|dE64|.  Read-only."""
    T, K = SCAN_SHAPES[shape_index]
    cfg, sr, hop = scan_cfg(name)
    rng = np.random.default_rng(500 + 10 * shape_index + sorted(SCAN_PARAMETERS).index(name))
    E = scan_energies(T, K, SCAN_PARAMETERS[name][3], SCAN_PARAMETERS[name][4], rng)
    g = rng.standard_normal((T, K)).astype(np.float32)
    y = pcen.pcen_ref(E, cfg, sr, hop)
    flat = np.sort(y.reshape(-1))
    floor = cfg["bias"] ** cfg["power"]
    if flat.size >= 8:
        p_lo, p_hi = bound_in_a_gap(flat, 0.07, 0.13, floor), bound_in_a_gap(flat, 0.87, 0.93, floor)
    else:
        p_lo, p_hi = -1.0, float(np.float32(flat[-1] + 1.0))
    assert p_hi > p_lo
    mask = tie_mask_of(y, p_lo, p_hi, cfg)
    g[mask] = 0.0
    gate = (y > p_lo) & (y < p_hi)
    g_y = np.where(gate, g.astype(np.float64) / (np.float64(np.float32(p_hi)) - np.float64(np.float32(p_lo))), 0.0)
    dE64 = pcen.pcen_bwd_ref(E, g_y, cfg, sr, hop)
    dE32 = pcen_bwd_f32(E, g_y, cfg, sr, hop)
    top = float(np.abs(dE64).max())
    assert top > 0
    out = {"E": E, "g": g, "stats": (p_lo, p_hi), "dE64": dE64, "tie_share": float(mask.mean()), "clipped": (float((y <= p_lo).mean()), float((y >= p_hi).mean())),
           "f32_share": float(np.abs(dE32.astype(np.float64) - dE64).max() / top), "cfg": cfg, "sr": sr, "hop": hop}
    for v in (E, g, dE64):
        v.setflags(write=False)
    return out


if __name__ == "__main__":  # prints the tables of constants kept in tests/test_pcen_grad_gpu.py
    print("SCAN_F32_DEVIATION = {")
    for name in SCAN_PARAMETERS:
        for i, (T, K) in enumerate(SCAN_SHAPES):
            c = scan_case(i, name)
            print(f'    ("{name}", {i}): {c["f32_share"]:.2e},  # T {T} K {K}: tie share {c["tie_share"]:.1e}, clipped {c["clipped"][0]:.2f} / {c["clipped"][1]:.2f}')
    print("}\nF32_REFERENCE_DEVIATION = {")
    for w in ("a", "b"):
        for i, pc in enumerate(CASES):
            c = case(w, i)
            print(f'    ("{w}", {i}): {f32_error_share(c, pc):.2e},  # {label(pc)}: tie share {c["tie_share"]:.1e}')
    print("}\nENERGY_F32_DEVIATION = {")
    for i, pc in enumerate(ENERGY_CASES):
        print(f"    {i}: {energy_case(i)['f32_share']:.2e},  # {label(pc)}")
    print("}")
