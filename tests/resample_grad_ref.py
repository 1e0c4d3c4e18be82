"""Shared helpers of tests/test_resample_grad.py and tests/test_resample_grad_gpu.py: the cases, the float64 adjoint of the polyphase resampler in
scatter form (the reference orcai_resample_polyphase_bwd is checked against) and the same sum in gather form in float32 (the yardstick of the GPU bar).

The forward, from the header comment of orcai_amd/csrc/resample.hip (h = ntaps / 2):
    out[n] = sum_j x[i0 - h + 1 + j] * table[phase][j],   i0 = floor(n*M/L), phase = (n*M) mod L,   x = 0 outside [0, n_in)
so output n adds g[n] * table[phase][j] to dx[i0 - h + 1 + j] (scatter), and dx[k] collects the outputs n with i0 in [k - h, k + h - 1], which are
n in [ceil((k-h)*L/M), ceil((k+h)*L/M)) clipped to [0, n_out) (gather)."""

from __future__ import annotations

import functools

import numpy as np

from orcai_amd.resample import design_table, output_length, ratio

# (sr_in, sr_out, n_in): what each covers is in the table of tests/test_resample_grad_gpu.py
CASES = (
    (22050, 48000, 1500),  # table of 320 x 128 floats (larger than LDS), L > M
    (44100, 48000, 1500),  # table of 160 x 128 floats
    (44100, 48000, 257),  # a length off the block size
    (96000, 48000, 3000),  # L = 1, 256 taps
    (8000, 48000, 700),  # M = 1, 768 terms per sample
    (48000, 22050, 3000),  # downsampling, 280 taps, table of 147 x 280 floats
    (44100, 48000, 50),  # shorter than one window: every sum is clipped at both ends
    (44100, 48000, 1),
)


def case_id(c) -> str:
    return f"{c[0]}-{c[1]}-{c[2]}"


def adjoint_ref(g: np.ndarray, n_in: int, sr_in: int, sr_out: int) -> np.ndarray:
    """float64 [n_in]: the adjoint of the resampler applied to g [output_length(n_in, sr_in, sr_out)], one output after the other (scatter form)."""
    L, M = ratio(sr_in, sr_out)
    table = design_table(L, M).astype(np.float64)
    ntaps = table.shape[1]
    n_out = output_length(n_in, sr_in, sr_out)
    assert g.shape == (n_out,), (g.shape, n_out)
    g = g.astype(np.float64)
    dx = np.zeros(n_in)
    for n in range(n_out):
        i0, phase = divmod(n * M, L)
        k0 = i0 - ntaps // 2 + 1
        lo, hi = max(k0, 0), min(k0 + ntaps, n_in)
        if lo < hi:
            dx[lo:hi] += g[n] * table[phase, lo - k0 : hi - k0]
    return dx


def gather_range(k: int, n_out: int, L: int, M: int, ntaps: int) -> tuple[int, int]:
    """[lo, hi): the outputs whose window holds input k."""
    h = ntaps // 2
    ceil_div = lambda a: -((-a * L) // M)  # noqa: E731  ceil(a*L/M), negative a included
    return min(max(ceil_div(k - h), 0), n_out), min(max(ceil_div(k + h), 0), n_out)


def adjoint_gather(g: np.ndarray, n_in: int, sr_in: int, sr_out: int, dtype=np.float64) -> np.ndarray:
    """The same sums in gather form: dx[k] over n in gather_range(k) in ascending n.  float64: every term in float64.  float32: the running sum is
    rounded to float32 after every term (the product of two float32 is exact in float64, so this is one rounding per term: a fused multiply-add)."""
    L, M = ratio(sr_in, sr_out)
    table = design_table(L, M)
    ntaps = table.shape[1]
    n_out = output_length(n_in, sr_in, sr_out)
    g32 = g.astype(np.float32)
    dx = np.zeros(n_in, dtype=dtype)
    for k in range(n_in):
        lo, hi = gather_range(k, n_out, L, M, ntaps)
        n = np.arange(lo, hi, dtype=np.int64)
        i0, phase = np.divmod(n * M, L)
        terms = g32[lo:hi].astype(np.float64) * table[phase, k - (i0 - ntaps // 2 + 1)].astype(np.float64)
        if dtype == np.float64:
            dx[k] = terms.sum()
        else:
            acc = np.float32(0.0)
            for t in terms:
                acc = np.float32(np.float64(acc) + t)
            dx[k] = acc
    return dx


@functools.lru_cache(maxsize=None)
def case(sr_in: int, sr_out: int, n_in: int) -> dict:
    """One case, computed once and shared (read-only): x f32[n_in] and g f32[n_out], both uniform(-1, 1) from a seed of the case, and dx64 = adjoint_ref(g)."""
    rng = np.random.default_rng([sr_in, sr_out, n_in])
    n_out = output_length(n_in, sr_in, sr_out)
    x = rng.uniform(-1.0, 1.0, n_in).astype(np.float32)
    g = rng.uniform(-1.0, 1.0, n_out).astype(np.float32)
    dx64 = adjoint_ref(g, n_in, sr_in, sr_out)
    for a in (x, g, dx64):
        a.setflags(write=False)
    L, M = ratio(sr_in, sr_out)
    return {"x": x, "g": g, "dx64": dx64, "n_out": n_out, "L": L, "M": M}


def f32_deviation_share(sr_in: int, sr_out: int, n_in: int) -> float:
    """max |gather in float32 - float64 reference| / max |reference|."""
    c = case(sr_in, sr_out, n_in)
    d32 = adjoint_gather(c["g"], n_in, sr_in, sr_out, dtype=np.float32)
    return float(np.abs(d32.astype(np.float64) - c["dx64"]).max() / np.abs(c["dx64"]).max())


if __name__ == "__main__":  # prints the table of constants kept in tests/test_resample_grad_gpu.py
    for c in CASES:
        ref = case(*c)
        share, top = f32_deviation_share(*c), float(np.abs(ref["dx64"]).max())
        cap = 2e-6 * max(1.0, ref["L"] / ref["M"])
        print(f"    {c}: {share:.2e},  # max|dx| {top:.3f}: bar {8 * share * top:.2e} absolute, cap {cap:.2e}")
