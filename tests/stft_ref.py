"""float64 restatement of orcai_stft_db's contract (csrc/frontend.hip), its error bound, its input families, the launcher's route
choice as a pure function, and the case tables of tests/test_stft_ref.py (CPU) and tests/test_stft_gpu.py.  numpy only.

Contract.  Samples promoted to float64; centred frames with zero padding, s0 = t hop - n_fft // 2, n_frames =
1 + (n - (n_fft & 1)) // hop; periodic Hann 0.5 - 0.5 cos(2 pi n / N); np.fft.rfft.  The kernels write
L[t][k] = 10 log10(max(|X|^2, 1e-10)) for k < k_crop and leave max |X|^2 over ALL 1 + n_fft // 2 bins in the workspace.

Bound, in amplitude.  a = sqrt(max(|X|^2, 1e-10)) has no singularity at the clamp, so every bin of every frame is compared:

    |a_gpu - a_ref| <= gamma(N) S[t] + rho a_ref,      a_gpu = 10^(L_gpu / 20) in float64,  S[t] = sum_n |x_n w_n|

  * gamma(N) = (4 log2 N + 4) 2^-24 for the two f32 FFT kernels: four roundings per radix-2 level (twiddle, complex multiply, add), plus the f32
    window and the window product; every intermediate of a frame's transform is bounded by S[t].  For sizes that are no power of two log2 N is
    rounded up (only the CPU emulation uses that).
  * gamma = 4 2^-24 for the direct float64 transform, whose only f32 roundings are the complex64 store and |X|^2.
  * rho = 1e-5: v_log_f32 and the two f32 operations after it round at |L| < 128 dB, at most 3 2^-17 dB; times ln 10 / 20 that is 2.6e-6
    relative in amplitude, rounded up.
Derived worst-case bars, not measurements; tests/test_stft_ref.py shows an f32 FFT on the CPU staying under a tenth of them.

Test infrastructure: nothing in orcai_amd/ imports this file.
"""

from __future__ import annotations

import math

import numpy as np

AMIN_POW = 1e-10
U = 2.0**-24
RHO = 1e-5
CLAMP_DB_TOL = 3 * 2.0**-17  # how far the dB value of a clamped bin may sit from -100
STFT_BLOCKS = 1536  # persistent workgroups of the 512-point launch (frontend.hip)
NFFT_TUNED = 512
NFFT_MAX = 4096
CHUNK = 4096  # frames per reference chunk

E_BADARG = -1
E_UNSUPPORTED = -2


def num_frames(n_samples: int, n_fft: int, hop: int) -> int:
    return 1 + (n_samples - (n_fft & 1)) // hop


def hann(n_fft: int) -> np.ndarray:
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n_fft) / n_fft)


def stft_ref_chunks(x_f32, n_fft: int, hop: int, chunk: int = CHUNK):
    """Yields (t0, a_ref[f64, frames x (1 + n_fft // 2)], S[f64, frames], max |X|^2 of the chunk) for runs of at most `chunk` frames."""
    x = np.asarray(x_f32)
    assert x.dtype == np.float32 and x.ndim == 1 and chunk <= CHUNK
    n = x.size
    T = num_frames(n, n_fft, hop)
    half = n_fft // 2
    w = hann(n_fft)
    for t0 in range(0, T, chunk):
        t1 = min(t0 + chunk, T)
        lo = t0 * hop - half  # first sample of the chunk's first frame
        hi = (t1 - 1) * hop - half + n_fft
        seg = np.zeros(hi - lo, dtype=np.float64)
        a, b = max(lo, 0), min(hi, n)
        if b > a:
            seg[a - lo : b - lo] = x[a:b]
        fr = np.lib.stride_tricks.sliding_window_view(seg, n_fft)[::hop] * w[None, :]
        assert fr.shape[0] == t1 - t0
        P = np.abs(np.fft.rfft(fr, axis=1)) ** 2
        yield t0, np.sqrt(np.maximum(P, AMIN_POW)), np.abs(fr).sum(axis=1), float(P.max())


def stft_ref(x_f32, n_fft: int, hop: int):
    """(a_ref[T, 1 + n_fft // 2], pmax_ref, S[T]), all float64."""
    parts = list(stft_ref_chunks(x_f32, n_fft, hop))
    return np.concatenate([p[1] for p in parts]), max(p[3] for p in parts), np.concatenate([p[2] for p in parts])


def dft_ref_direct(x_f32, n_fft: int, hop: int):
    """The same contract by a direct O(N^2) float64 DFT with explicit loops over frames and samples: |X|^2 [T, 1 + n_fft // 2]."""
    x = np.asarray(x_f32, dtype=np.float64)
    n, half = x.size, n_fft // 2
    T = num_frames(n, n_fft, hop)
    k = np.arange(half + 1)
    P = np.empty((T, half + 1))
    for t in range(T):
        acc = np.zeros(half + 1, dtype=np.complex128)
        for j in range(n_fft):
            i = t * hop - half + j
            if 0 <= i < n:
                acc += x[i] * (0.5 - 0.5 * math.cos(2.0 * math.pi * j / n_fft)) * np.exp(-2j * np.pi * ((k * j) % n_fft) / n_fft)
        P[t] = acc.real**2 + acc.imag**2
    return P


# ------------------------------------------------------------------------------------------------ bound
def gamma(n_fft: int, route: str) -> float:
    if route == "dft":
        return 4 * U
    return (4 * math.ceil(math.log2(n_fft)) + 4) * U


def db_to_amp(L) -> np.ndarray:
    return 10.0 ** (np.asarray(L, dtype=np.float64) / 20.0)


def amp_ratio(a_got, a_ref, S, g: float) -> np.ndarray:
    """|a_got - a_ref| / (g S[t] + rho a_ref) per element (a_ref >= 1e-5, so the denominator is never zero)."""
    a_ref = np.asarray(a_ref)
    return np.abs(np.asarray(a_got, dtype=np.float64) - a_ref) / (g * np.asarray(S)[:, None] + RHO * a_ref)


def bound_ratio(L_gpu, a_ref, S, g: float) -> np.ndarray:
    """The same from the dB values the kernels write."""
    return amp_ratio(db_to_amp(L_gpu), a_ref, S, g)


# ------------------------------------------------------------------------------------------------ input families
FAMILIES = ("noise", "tones", "tone_floor", "impulses", "ramp", "silence_gap", "tone_above_crop")


def _noise(rng, n):
    return np.clip(np.round(3000.0 * rng.standard_normal(n)), -32767, 32767) / 32768.0


def impulse_positions(n: int, n_fft: int, hop: int):
    cand = [0, 1, hop - 1, hop, n_fft // 2 - 1, n_fft // 2, (n // 2) | 1, n - 1]
    return sorted({s for s in cand if 0 <= s < n})


def make_input(family: str, n: int, n_fft: int, hop: int, seed: int = 0) -> np.ndarray:
    """f32[n]; the float32 array IS the input (the reference promotes it), so every family is exact in f32."""
    rng = np.random.default_rng([seed, FAMILIES.index(family), n, n_fft, hop])
    i = np.arange(n, dtype=np.float64)
    if family == "noise":
        x = _noise(rng, n)
    elif family == "tones":  # exactly on bin 37: bin order, bit reversal
        x = 0.5 * np.cos(2.0 * np.pi * 37.0 * i / n_fft)
    elif family == "tone_floor":  # 100 dB of dynamic range inside a frame
        x = 0.9 * np.cos(2.0 * np.pi * 200.3 * i / n_fft) + 1e-4 * _noise(rng, n)
    elif family == "impulses":
        x = np.zeros(n)
        x[impulse_positions(n, n_fft, hop)] = 1.0
    elif family == "ramp":
        x = _noise(rng, n) * np.geomspace(1e-6, 30.0, n)
    elif family == "silence_gap":
        x = _noise(rng, n)
        a = n // 3
        x[a : a + n_fft + hop + 5] = 0.0
    elif family == "tone_above_crop":  # 20 kHz of 48 kHz: k = 0.42 N, above every small crop
        x = 0.5 * np.cos(2.0 * np.pi * round(0.42 * n_fft) * i / n_fft) + 1e-3 * _noise(rng, n)
    else:
        raise KeyError(family)
    return x.astype(np.float32)


def impulse_frames(n: int, n_fft: int, hop: int):
    """For the impulses family: {t: [window position of every impulse inside frame t]} (frames not listed hold only zeros)."""
    half = n_fft // 2
    T = num_frames(n, n_fft, hop)
    cover: dict = {}
    for s in impulse_positions(n, n_fft, hop):
        # 0 <= s - t hop + half < n_fft
        for t in range(max(0, -(-(s + half - n_fft + 1) // hop)), min(T - 1, (s + half) // hop) + 1):
            cover.setdefault(t, []).append(s - t * hop + half)
    return cover


# ------------------------------------------------------------------------------------------------ the launcher's rules
def stft_route(n_samples: int, n_fft: int, hop: int, k_crop: int, n_frames: int | None = None) -> dict:
    """orcai_stft_db's choices for well-aligned, non-null buffers.  Returns {"rc", "route", "labels", "launches", ...}:
    route in {"refused", "dft", "radix2", "512"}; launches = [(label, g_begin, g_end, workgroups)] for the 512 route; labels = the
    set of code paths the call reaches:
      dft / dft_optin_lds, radix2, odd_hop, mixed_only, fast171 / fast0 (+ "prefetch_trips>=2", ">=3", ">=4"), mixed_head, mixed_tail,
      wave_fast / wave_generic (what the waves of the mixed kernel decide), ragged_wave (a wave whose frames end before its fourth)."""
    if n_frames is None:
        n_frames = num_frames(n_samples, n_fft, hop) if hop > 0 else 1
    r = {"rc": 0, "route": "refused", "labels": set(), "launches": []}
    if n_samples <= 0 or hop <= 0 or k_crop < 1 or n_fft < 2 or k_crop > 1 + n_fft // 2:
        return dict(r, rc=E_BADARG)
    if n_frames != num_frames(n_samples, n_fft, hop):
        return dict(r, rc=E_BADARG)
    if n_fft != NFFT_TUNED:
        if n_fft > NFFT_MAX:
            return dict(r, rc=E_UNSUPPORTED)
        if n_fft < 32 or n_fft & (n_fft - 1):
            lds = 8 * (n_fft + (n_fft & 1) + 2 * n_fft)
            r["route"] = "dft"
            r["labels"] = {"dft_optin_lds" if lds > 48 * 1024 else "dft"}
            r["lds_bytes"] = lds
            return r
        r["route"] = "radix2"
        r["labels"] = {"radix2"}
        return r
    r["route"] = "512"
    n_groups = (n_frames + 15) // 16
    grid = lambda g: min(g, STFT_BLOCKS)
    labels = r["labels"]
    if n_frames % 4:
        labels.add("ragged_wave")
    if hop & 1:
        labels |= {"odd_hop", "wave_generic"}
        r["launches"] = [("odd_hop", 0, n_groups, grid(n_groups))]
        return dict(r, n_groups=n_groups, g_lo=n_groups, g_hi=n_groups)
    g_lo = g_hi = n_groups
    if hop == 256:
        g_lo = 1
        by_samples = ((n_samples - 1024) // 256 - 12) // 16 + 1 if n_samples >= 4096 else 0
        by_frames = (n_frames - 16) // 16 + 1 if n_frames >= 16 else 0
        g_hi = min(by_samples, by_frames, n_groups)
        if g_hi < g_lo:
            g_lo = g_hi = n_groups
    mixed = []
    if g_hi > g_lo:
        fast = "fast171" if k_crop == 171 else "fast0"
        labels.add(fast)
        trips = -(-(g_hi - g_lo) // STFT_BLOCKS)
        for m in (2, 3, 4):
            if trips >= m:
                labels.add(f"prefetch_trips>={m}")
        r["launches"].append((fast, g_lo, g_hi, grid(g_hi - g_lo)))
        r["launches"].append(("mixed_head", 0, g_lo, grid(g_lo)))
        labels.add("mixed_head")
        mixed.append((0, g_lo))
        if g_hi < n_groups:
            r["launches"].append(("mixed_tail", g_hi, n_groups, grid(n_groups - g_hi)))
            labels.add("mixed_tail")
            mixed.append((g_hi, n_groups))
    else:
        r["launches"].append(("mixed_only", 0, n_groups, grid(n_groups)))
        labels.add("mixed_only")
        mixed.append((0, n_groups))
    if hop != 256:
        labels.add("wave_generic")
    else:  # few groups: the head, the tail, or a recording shorter than 8192 samples
        for a, b in mixed:
            for g in range(a, b):
                for wave in range(4):
                    t0w = 16 * g + 4 * wave
                    w0 = t0w * hop - 256
                    ok = w0 >= 0 and w0 % 4 == 0 and w0 + 1280 <= n_samples and t0w + 3 < n_frames
                    labels.add("wave_fast" if ok else "wave_generic")
    return dict(r, n_groups=n_groups, g_lo=g_lo, g_hi=g_hi)


def interior_bounds_check(n_samples: int, n_frames: int, g_lo: int, g_hi: int) -> None:
    """What the FAST_ONLY kernel assumes of every group in [g_lo, g_hi): its four waves read pcm[w0, w0 + 1280) unguarded and write 16 whole frames."""
    for g in {g_lo, g_hi - 1}:
        for wave in range(4):
            w0 = (16 * g + 4 * wave) * 256 - 256
            assert w0 >= 0 and w0 % 4 == 0 and w0 + 1280 <= n_samples, (g, wave, w0, n_samples)
        assert 16 * g + 15 < n_frames


def prefetch_case_n_samples(interior: int = 3 * STFT_BLOCKS + 100) -> int:
    """Smallest n_samples at hop 256 with `interior` interior groups, a ragged last wave and a mixed tail: with 3 x 1536 + 100 groups, 100
    workgroups of the FAST_ONLY launch take four trips of the prefetch loop (two passes of the loop unrolled by two) and the others three."""
    g_hi = 1 + interior
    n = 1024 + (16 * (g_hi - 1) + 12) * 256  # first n with by_samples == g_hi
    while True:
        r = stft_route(n, 512, 256, 171)
        if r["g_hi"] - r["g_lo"] == interior and "mixed_tail" in r["labels"] and "ragged_wave" in r["labels"]:
            return n
        assert r["g_hi"] - r["g_lo"] <= interior
        n += 1


# ------------------------------------------------------------------------------------------------ case tables
# 512-point route: (hop, n_samples).  n_frames mod 16 takes 0, 1 and 15 and n_frames mod 4 != 0 occurs (tests/test_stft_ref.py checks both).
CASES_512 = [
    (256, 1),  # one frame, one sample
    (256, 255),  # shorter than a hop
    (256, 4095),  # 16 frames, one group, no interior
    (256, 8191),  # 32 frames: the last length without an interior group
    (256, 8192),  # 33 frames: the first with one (group 1), ragged tail group
    (256, 12345),  # 49 frames
    (256, 16 * 256 * 3 + 7),  # 49 frames, two interior groups
    (256, 16 * 256 * 3 + 256 * 14 + 9),  # 63 frames: n_frames mod 16 == 15
    (128, 46 * 128 + 5),  # 47 frames
    (300, 32 * 300 + 10),  # 33 frames, even hop that is no multiple of 4
    (255, 30 * 255 + 3),  # 31 frames, odd hop
    (512, 47 * 512 + 100),  # 48 frames, no overlap between frames' halves
    (1000, 17 * 1000 + 500),  # 18 frames, gaps between frames
    (2, 700),  # 351 frames, almost identical neighbours
]
KCROPS_512 = (171, 257)

# other routes: (n_fft, hop, n_samples)
CASES_RADIX2 = [(N, hop, (200 if hop == 77 else 4) * hop + 13) for N in (32, 64, 1024, 4096) for hop in (N // 4, 77, N)]
CASES_DFT = [(N, hop, (60 if hop == 77 else 5) * hop + 3) for N in (2, 16, 500, 675, 4095, 3000) for hop in (max(1, N // 4), 77)]
FAMILIES_OTHER = ("noise", "impulses", "tone_floor")


def kcrops_other(n_fft: int):
    full = 1 + n_fft // 2
    return sorted({1, max(1, (full * 2) // 3), full})


CROPS_INVARIANCE = (1, 16, 17, 170, 171, 172, 256)


def all_labels() -> set:
    """Every label stft_route can return."""
    return {"dft", "dft_optin_lds", "radix2", "odd_hop", "mixed_only", "fast171", "fast0", "mixed_head", "mixed_tail", "wave_fast", "wave_generic",
            "ragged_wave", "prefetch_trips>=2", "prefetch_trips>=3", "prefetch_trips>=4"}
