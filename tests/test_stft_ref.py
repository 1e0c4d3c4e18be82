"""tests/stft_ref.py checked on the CPU: the float64 reference against two independent restatements, the bound against an f32 FFT, the
restated launcher rules against their own invariants, and the case tables of tests/test_stft_gpu.py against the labels the rules return."""

import numpy as np
import pytest

import stft_ref as R


# ------------------------------------------------------------------------------------------------ the reference
@pytest.mark.parametrize("n_fft,hop,n", [(16, 5, 61), (31, 7, 100), (512, 256, 1300)])
def test_reference_equals_direct_dft(n_fft, hop, n):
    x = R.make_input("noise", n, n_fft, hop)
    a, pmax, S = R.stft_ref(x, n_fft, hop)
    P = R.dft_ref_direct(x, n_fft, hop)
    assert a.shape == P.shape == (R.num_frames(n, n_fft, hop), 1 + n_fft // 2)
    live = P > 1e-6  # above the clamp and above cancellation noise: 1e-12 relative holds
    assert live.mean() > 0.9
    assert np.abs(a**2 - P)[live].max() <= 1e-12 * P.max()
    assert np.abs(a[live] - np.sqrt(P[live])).max() <= 1e-12 * np.sqrt(P.max())
    assert abs(pmax - P.max()) <= 1e-12 * P.max()
    w = R.hann(n_fft)
    xp = np.concatenate([np.zeros(n_fft // 2), x.astype(np.float64), np.zeros(n_fft)])
    assert np.allclose(S, [np.abs(xp[t * hop : t * hop + n_fft] * w).sum() for t in range(a.shape[0])], rtol=1e-13, atol=0)


@pytest.mark.parametrize("n_fft,hop,n", [(512, 256, 48000), (1024, 300, 20000), (675, 128, 9000)])
def test_reference_equals_oracle_before_referencing(n_fft, hop, n):
    """oracle.frontend_ref.stft_ref is the complex64 transform calculate_spectrogram_ref references and floors."""
    from oracle import frontend_ref as F

    x = R.make_input("ramp", n, n_fft, hop)
    a, pmax, _ = R.stft_ref(x, n_fft, hop)
    Z = F.stft_ref(x, n_fft, hop).T.astype(np.complex128)  # complex64 storage: 2^-24 relative per component
    assert Z.shape == a.shape
    P = np.maximum(np.abs(Z) ** 2, R.AMIN_POW)
    assert np.abs(np.sqrt(P) - a).max() <= 2.0**-23 * a.max()
    # and to 1e-12 before that storage rounding
    pad = n_fft // 2
    fr = np.lib.stride_tricks.sliding_window_view(np.pad(x, (pad, pad)), n_fft)[::hop]
    Z64 = np.fft.rfft(F.hann_window(n_fft)[None, :] * fr, axis=1)
    assert np.abs(np.sqrt(np.maximum(np.abs(Z64) ** 2, R.AMIN_POW)) - a).max() <= 1e-12 * a.max()
    assert abs((np.abs(Z64) ** 2).max() - pmax) <= 1e-12 * pmax


def test_chunks_are_seamless():
    x = R.make_input("noise", 3000, 64, 16)
    whole = R.stft_ref(x, 64, 16)
    parts = list(R.stft_ref_chunks(x, 64, 16, chunk=37))
    assert [p[0] for p in parts] == list(range(0, 188, 37))
    assert np.array_equal(np.concatenate([p[1] for p in parts]), whole[0]) and max(p[3] for p in parts) == whole[1]
    assert np.array_equal(np.concatenate([p[2] for p in parts]), whole[2])


def test_families_are_f32_and_seeded():
    for fam in R.FAMILIES:
        a, b = R.make_input(fam, 5000, 512, 256), R.make_input(fam, 5000, 512, 256)
        assert a.dtype == np.float32 and a.shape == (5000,) and np.array_equal(a, b) and np.isfinite(a).all()
    x = R.make_input("tone_floor", 5000, 512, 256)
    a, _, _ = R.stft_ref(x, 512, 256)
    mid = a[5:15]
    assert (20 * np.log10(mid.max(axis=1) / mid.min(axis=1)) > 90).all()  # the dynamic range inside one frame
    g = R.make_input("silence_gap", 5000, 512, 256)
    assert (g[5000 // 3 : 5000 // 3 + 512 + 256] == 0).all()
    t = R.make_input("tone_above_crop", 5000, 512, 256)
    a, _, _ = R.stft_ref(t, 512, 256)
    assert (a[3:15].argmax(axis=1) == 215).all()


@pytest.mark.parametrize("n_fft,hop,n", [(512, 256, 12345), (512, 1000, 17500), (64, 77, 2000), (675, 168, 4000)])
def test_impulse_frames_of_the_reference(n_fft, hop, n):
    """Frames that cover one impulse are flat at the window value of its position; frames that cover none are the clamp."""
    x = R.make_input("impulses", n, n_fft, hop)
    a, _, _ = R.stft_ref(x, n_fft, hop)
    cover = R.impulse_frames(n, n_fft, hop)
    w = R.hann(n_fft)
    singles = 0
    for t in range(a.shape[0]):
        if t not in cover:
            assert (a[t] == 1e-5).all()
        elif len(cover[t]) == 1 and w[cover[t][0]] > 1e-4:
            singles += 1
            assert np.abs(a[t] - w[cover[t][0]]).max() <= 1e-12
    assert singles >= 1 and len(cover) < a.shape[0]


# ------------------------------------------------------------------------------------------------ the bound
def _emulate_f32(x, n_fft, hop):
    """The same contract in f32 with torch's FFT: f32 window table, f32 product, f32 transform, f32 |X|^2.  Returns the clamped amplitude (the
    square root taken in float64) and max |X|^2: the emulation is of the transform, the gamma term of the bound.  The rho term belongs to the
    f32 logarithm: one f32 ulp of a dB value near -100 is 7.6e-6 dB = 8.8e-7 in relative amplitude, 0.088 rho by itself."""
    torch = pytest.importorskip("torch")
    half = n_fft // 2
    T = R.num_frames(x.size, n_fft, hop)
    xp = np.concatenate([np.zeros(half, np.float32), x, np.zeros(n_fft, np.float32)])
    fr = np.lib.stride_tricks.sliding_window_view(xp, n_fft)[::hop][:T] * R.hann(n_fft).astype(np.float32)[None, :]
    assert fr.dtype == np.float32
    Z = torch.fft.rfft(torch.from_numpy(np.ascontiguousarray(fr)), dim=1)
    assert Z.dtype == torch.complex64
    P = (Z.real * Z.real + Z.imag * Z.imag).numpy()
    assert P.dtype == np.float32
    return np.sqrt(np.maximum(P.astype(np.float64), R.AMIN_POW)), float(P.max())


@pytest.mark.parametrize("n_fft", [32, 512, 4096, 500, 675])
@pytest.mark.parametrize("family", R.FAMILIES + ("silence",))
def test_f32_emulation_is_far_inside_the_bound(n_fft, family):
    hop = max(1, n_fft // 2 - 3)
    n = 40 * hop + 11
    x = np.zeros(n, np.float32) if family == "silence" else R.make_input(family, n, n_fft, hop)
    a_f32, pmax = _emulate_f32(x, n_fft, hop)
    a, pmax_ref, S = R.stft_ref(x, n_fft, hop)
    g = R.gamma(n_fft, "radix2")
    ratio = R.amp_ratio(a_f32, a, S, g)
    assert ratio.max() <= 0.1, ratio.max()
    assert abs(np.sqrt(pmax) - np.sqrt(pmax_ref)) <= 0.1 * g * S.max() + 1e-30


def test_bound_sees_a_misplaced_frame_and_a_wrong_bin():
    x = R.make_input("noise", 6000, 512, 256)
    a, _, S = R.stft_ref(x, 512, 256)
    L = (20 * np.log10(a)).astype(np.float32)
    g = R.gamma(512, "512")
    assert R.bound_ratio(L, a, S, g).max() <= 0.1
    assert R.bound_ratio(np.roll(L, 1, axis=0), a, S, g).max() > 100
    assert R.bound_ratio(np.roll(L, 1, axis=1), a, S, g).max() > 100
    assert R.bound_ratio(L + np.float32(0.01), a, S, g).max() > 10  # 0.01 dB everywhere


# ------------------------------------------------------------------------------------------------ the launcher's rules
def test_route_interior_groups_are_safe_and_maximal():
    """Every interior group satisfies what the FAST_ONLY kernel assumes; the groups next to the interior do not (the rule is tight)."""
    for n in list(range(1, 200, 37)) + list(range(3900, 21000, 61)) + [8191, 8192, 12288, 12289, R.prefetch_case_n_samples()]:
        r = R.stft_route(n, 512, 256, 171)
        T = R.num_frames(n, 512, 256)
        assert r["n_groups"] == -(-T // 16)
        if "fast171" not in r["labels"]:
            assert r["labels"] >= {"mixed_only"} and r["launches"] == [("mixed_only", 0, r["n_groups"], min(r["n_groups"], R.STFT_BLOCKS))]
            assert n < 8192
            continue
        assert n >= 8192 and r["g_lo"] == 1
        R.interior_bounds_check(n, T, r["g_lo"], r["g_hi"])
        g = r["g_hi"]  # the first group left to the mixed kernel must really break a condition
        assert g == r["n_groups"] or (16 * g + 12) * 256 - 256 + 1280 > n or 16 * g + 15 >= T
        covered = sorted((a, b) for _, a, b, _ in r["launches"])
        assert covered[0][0] == 0 and covered[-1][1] == r["n_groups"] and all(covered[i][1] == covered[i + 1][0] for i in range(len(covered) - 1))
        assert all(0 < wg <= R.STFT_BLOCKS and wg <= b - a for _, a, b, wg in r["launches"])


def test_route_edges():
    assert "mixed_only" in R.stft_route(8191, 512, 256, 171)["labels"]
    r = R.stft_route(8192, 512, 256, 171)
    assert (r["g_lo"], r["g_hi"], r["n_groups"]) == (1, 2, 3) and r["labels"] >= {"fast171", "mixed_head", "mixed_tail", "wave_fast", "wave_generic"}
    assert "fast0" in R.stft_route(8192, 512, 256, 172)["labels"]
    assert R.stft_route(10**6, 512, 128, 171)["labels"] == {"mixed_only", "wave_generic", "ragged_wave"}
    assert R.stft_route(10**6, 512, 255, 171)["labels"] == {"odd_hop", "wave_generic", "ragged_wave"}
    assert R.stft_route(1000, 3000, 100, 5)["labels"] == {"dft_optin_lds"} and R.stft_route(1000, 2047, 100, 5)["labels"] == {"dft"}
    assert R.stft_route(1000, 2048, 100, 5)["labels"] == {"radix2"}
    assert R.stft_route(1000, 16, 100, 5)["route"] == "dft" and R.stft_route(1000, 32, 100, 5)["route"] == "radix2"
    for bad in [(0, 512, 256, 171), (100, 512, 0, 171), (100, 512, 256, 0), (100, 512, 256, 258), (100, 1, 1, 1)]:
        assert R.stft_route(*bad)["rc"] == R.E_BADARG
    assert R.stft_route(100, 512, 256, 171, n_frames=2)["rc"] == R.E_BADARG
    assert R.stft_route(10000, 4097, 256, 171)["rc"] == R.E_UNSUPPORTED and R.stft_route(10000, 4096, 256, 171)["rc"] == 0


def test_prefetch_case_size():
    n = R.prefetch_case_n_samples()
    r = R.stft_route(n, 512, 256, 171)
    assert r["g_hi"] - r["g_lo"] == 3 * R.STFT_BLOCKS + 100
    assert r["labels"] >= {"fast171", "prefetch_trips>=4", "mixed_head", "mixed_tail", "ragged_wave"}
    assert 19.2e6 < n < 19.4e6 and R.num_frames(n, 512, 256) * 171 * 4 < 53e6
    assert R.stft_route(n - 1, 512, 256, 171)["g_hi"] - 1 < 3 * R.STFT_BLOCKS + 100 or "ragged_wave" not in R.stft_route(n - 1, 512, 256, 171)["labels"]
    # three trips for most workgroups, four for the first hundred
    trips = [len(range(1 + b, r["g_hi"], R.STFT_BLOCKS)) for b in range(R.STFT_BLOCKS)]
    assert trips.count(4) == 100 and trips.count(3) == R.STFT_BLOCKS - 100


def test_case_tables_reach_every_label():
    seen = set()
    frames_mod16, ragged = set(), False
    for hop, n in R.CASES_512:
        for k in R.KCROPS_512:
            seen |= R.stft_route(n, 512, hop, k)["labels"]
        T = R.num_frames(n, 512, hop)
        frames_mod16.add(T % 16)
        ragged |= T % 4 != 0
    for N, hop, n in R.CASES_RADIX2 + R.CASES_DFT:
        for k in R.kcrops_other(N):
            r = R.stft_route(n, N, hop, k)
            assert r["rc"] == 0 and 3 <= R.num_frames(n, N, hop) <= 400
            seen |= r["labels"]
    assert {N for N, _, _ in R.CASES_RADIX2} == {32, 64, 1024, 4096} and {N for N, _, _ in R.CASES_DFT} == {2, 16, 500, 675, 4095, 3000}
    assert {R.stft_route(n, N, hop, 1)["labels"].pop() for N, hop, n in R.CASES_DFT if N in (3000, 4095)} == {"dft_optin_lds"}
    seen |= R.stft_route(R.prefetch_case_n_samples(), 512, 256, 171)["labels"]
    assert seen == R.all_labels(), R.all_labels() - seen
    assert frames_mod16 >= {0, 1, 15} and ragged
    # both sides of the first interior group, and the fallback without one
    assert (256, 8191) in R.CASES_512 and (256, 8192) in R.CASES_512
    assert "mixed_only" in R.stft_route(8191, 512, 256, 171)["labels"] and "fast171" in R.stft_route(8192, 512, 256, 171)["labels"]
    assert {h for h, _ in R.CASES_512} >= {256, 128, 300, 255, 512, 1000, 2} and (2, 700) in R.CASES_512
    assert {n for h, n in R.CASES_512 if h == 256} >= {1, 255, 4095, 8191, 8192, 12345, 16 * 256 * 3 + 7}
