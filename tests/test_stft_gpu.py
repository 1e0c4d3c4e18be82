"""orcai_stft_db (csrc/frontend.hip) through the C ABI against the float64 contract of tests/stft_ref.py, on all three routes: the 512-point
kernel in its five instantiations / launch splits, the radix-2 kernel, the direct float64 transform.

Every bin of every frame is compared in amplitude against |a_gpu - a_ref| <= gamma(N) S[t] + rho a_ref (derived in tests/stft_ref.py, not
measured); max |X|^2 against the reference's over all bins; the level-1 histogram through the exact order statistics it leads to; the staged
float4 copy through a guard behind the output that must keep its bits.  Each test prints the largest error-to-bound ratio it saw."""

import ctypes as C

import numpy as np
import pytest

import stft_ref as R

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

GUARD = 64 + 3  # floats behind n_frames * k_crop (odd, so the guard does not end on a float4 boundary)
SENTINEL_BITS = 0x7FC12345  # a NaN payload no kernel produces from finite samples
TOP_DB = 80.0


def to_device(x):
    return torch.tensor(np.asarray(x), device="cuda")  # a copy: the shared reference inputs are read-only


class Harness:
    def __init__(self):
        from orcai_amd import _native as N

        self.N = N
        self.lib = N.lib()
        self.ws = torch.zeros(self.lib.orcai_frontend_workspace_bytes(), dtype=torch.uint8, device="cuda")
        self.wsp = self.ws.data_ptr()
        self.s = N.stream_ptr()

    def buffer(self, count):
        return torch.full((count + GUARD,), SENTINEL_BITS, dtype=torch.int32, device="cuda")

    @staticmethod
    def untouched(buf, start=0):
        return bool((buf[start:] == SENTINEL_BITS).all().item())

    def stats(self):
        st = (C.c_float * 6)()
        assert self.lib.orcai_frontend_stats_host(self.wsp, st, self.s) == 0
        return [np.float32(v) for v in st]

    def stft(self, xd, n_fft, hop, k_crop):
        """reset + orcai_stft_db.  Returns (L f32[T, k_crop] on the host, max |X|^2, the device buffer (int32 view, guard included))."""
        n = xd.numel()
        T = R.num_frames(n, n_fft, hop)
        buf = self.buffer(T * k_crop)
        assert self.lib.orcai_frontend_reset(self.wsp, self.s) == 0
        rc = self.lib.orcai_stft_db(xd.data_ptr(), n, n_fft, hop, T, k_crop, buf.data_ptr(), self.wsp, self.s)
        assert rc == 0, rc
        pmax = self.stats()[0]
        assert self.untouched(buf, T * k_crop), "the guard behind n_frames * k_crop was written"
        body = buf[: T * k_crop]
        assert not bool((body == SENTINEL_BITS).any().item()), "an output element was never written"
        L = body.view(torch.float32).cpu().numpy().reshape(T, k_crop)
        assert np.isfinite(L).all()
        return L, float(pmax), buf

    def select(self, buf, count, r_lo, r_hi):
        """orcai_quantile_select on the device's own values, on the histogram orcai_stft_db left in the workspace."""
        assert self.lib.orcai_quantile_select(buf.data_ptr(), count, r_lo, r_hi, self.wsp, self.s) == 0
        assert self.lib.orcai_frontend_finalize(0, TOP_DB, self.wsp, self.s) == 0
        st = self.stats()
        return st[4], st[5]


@pytest.fixture(scope="module")
def h():
    return Harness()


_REF = {}


def reference(family, n, n_fft, hop):
    """(x, a_ref, pmax_ref, S), computed once per input and shared; nobody writes into it."""
    key = (family, n, n_fft, hop)
    if key not in _REF:
        x = R.make_input(family, n, n_fft, hop)
        a, pmax, S = R.stft_ref(x, n_fft, hop)
        for arr in (x, a, S):
            arr.setflags(write=False)
        _REF[key] = (x, a, pmax, S)
    return _REF[key]


def check_accuracy(h, family, n, n_fft, hop, k_crops, route):
    x, a, pmax_ref, S = reference(family, n, n_fft, hop)
    g = R.gamma(n_fft, route)
    xd = to_device(x)
    worst = 0.0
    for k in k_crops:
        assert R.stft_route(n, n_fft, hop, k)["route"] == route
        L, pmax, _ = h.stft(xd, n_fft, hop, k)
        ratio = R.bound_ratio(L, a[:, :k], S, g)
        worst = max(worst, float(ratio.max()))
        t, b = np.unravel_index(ratio.argmax(), ratio.shape)
        print(f"{route} N={n_fft} hop={hop} n={n} k_crop={k} {family}: ratio {ratio.max():.4f} at frame {t} bin {b}")
        assert ratio.max() <= 1.0, (family, n_fft, hop, n, k, float(ratio.max()), int(t), int(b))
        pm = abs(np.sqrt(pmax) - np.sqrt(pmax_ref)) / (g * S.max() + 1e-300)
        print(f"    sqrt(pmax) error / (gamma max S) = {pm:.4f}")
        assert abs(np.sqrt(pmax) - np.sqrt(pmax_ref)) <= g * S.max(), (pmax, pmax_ref)
        if family == "impulses":
            cover = R.impulse_frames(n, n_fft, hop)
            empty = [t for t in range(L.shape[0]) if t not in cover]
            if empty:  # frames of zeros: exactly the clamp, one bit pattern
                v = L[empty]
                assert np.unique(v.view(np.int32)).size == 1 and abs(float(v.flat[0]) + 100.0) <= R.CLAMP_DB_TOL, np.unique(v)
    return worst


# ------------------------------------------------------------------------------------------------ 1. accuracy, 512-point route
@pytest.mark.parametrize("family", R.FAMILIES)
@pytest.mark.parametrize("hop,n", R.CASES_512)
def test_accuracy_512(h, hop, n, family):
    check_accuracy(h, family, n, 512, hop, R.KCROPS_512, "512")


# ------------------------------------------------------------------------------------------------ 2. accuracy, the other two routes
@pytest.mark.parametrize("family", R.FAMILIES_OTHER)
@pytest.mark.parametrize("n_fft,hop,n", R.CASES_RADIX2)
def test_accuracy_radix2(h, n_fft, hop, n, family):
    check_accuracy(h, family, n, n_fft, hop, R.kcrops_other(n_fft), "radix2")


@pytest.mark.parametrize("family", R.FAMILIES_OTHER)
@pytest.mark.parametrize("n_fft,hop,n", R.CASES_DFT)
def test_accuracy_dft(h, n_fft, hop, n, family):
    check_accuracy(h, family, n, n_fft, hop, R.kcrops_other(n_fft), "dft")


# ------------------------------------------------------------------------------------------------ 3. the prefetch loop's later trips
def test_prefetch_loop_every_frame(h):
    """3 x 1536 + 100 interior groups: a hundred workgroups of the FAST_ONLY launch take four trips through the prefetch loop, the others three;
    head group, ragged tail group.  Every frame against the chunked reference, at k_crop 171 (<true,true,171>) and 172 (<true,true,0>)."""
    n = R.prefetch_case_n_samples()
    r = R.stft_route(n, 512, 256, 171)
    assert r["labels"] >= {"fast171", "prefetch_trips>=4", "mixed_head", "mixed_tail", "ragged_wave"}
    assert "fast0" in R.stft_route(n, 512, 256, 172)["labels"]
    R.interior_bounds_check(n, R.num_frames(n, 512, 256), r["g_lo"], r["g_hi"])
    x = R.make_input("noise", n, 512, 256)
    xd = to_device(x)
    L171, pmax171, _ = h.stft(xd, 512, 256, 171)
    L172, pmax172, _ = h.stft(xd, 512, 256, 172)
    assert pmax171 == pmax172
    g = R.gamma(512, "512")
    worst, pmax_ref, s_max = 0.0, 0.0, 0.0
    for t0, a, S, pm in R.stft_ref_chunks(x, 512, 256):
        t1 = t0 + a.shape[0]
        for L, k in ((L171, 171), (L172, 172)):
            ratio = R.bound_ratio(L[t0:t1], a[:, :k], S, g)
            if ratio.max() > 1.0:
                t, b = np.unravel_index(ratio.argmax(), ratio.shape)
                grp = (t0 + t) // 16
                pytest.fail(f"k_crop {k}: ratio {ratio.max():.3g} at frame {t0 + t} bin {b}: group {grp}, workgroup {(grp - 1) % R.STFT_BLOCKS}, "
                            f"trip {(grp - 1) // R.STFT_BLOCKS}")
            worst = max(worst, float(ratio.max()))
        pmax_ref, s_max = max(pmax_ref, pm), max(s_max, float(S.max()))
    print(f"prefetch case: n_samples {n}, {L171.shape[0]} frames, largest ratio {worst:.4f}")
    assert abs(np.sqrt(pmax171) - np.sqrt(pmax_ref)) <= g * s_max


# ------------------------------------------------------------------------------------------------ 4. crop invariance, bit for bit
@pytest.mark.parametrize("n_fft,hop,n", [(512, 256, 16 * 256 * 3 + 7), (512, 300, 9610), (512, 255, 7653), (1024, 77, 5000), (675, 128, 4000)])
def test_crop_invariance_bitwise(h, n_fft, hop, n):
    x = R.make_input("tone_floor", n, n_fft, hop)
    xd = to_device(x)
    full, pmax_full, _ = h.stft(xd, n_fft, hop, 1 + n_fft // 2)
    for k in R.CROPS_INVARIANCE:
        L, pmax, _ = h.stft(xd, n_fft, hop, k)
        assert np.array_equal(L.view(np.int32), full[:, :k].view(np.int32)), k
        assert pmax == pmax_full, k


# ------------------------------------------------------------------------------------------------ 5. max |X|^2 over all bins
ROUTE_SHAPES = [("512", 512, 256, 12345), ("512", 512, 300, 9610), ("radix2", 1024, 256, 5300), ("dft", 675, 128, 4200)]


@pytest.mark.parametrize("route,n_fft,hop,n", ROUTE_SHAPES)
def test_pmax_comes_from_above_the_crop(h, route, n_fft, hop, n):
    x, a, pmax_ref, S = reference("tone_above_crop", n, n_fft, hop)
    assert R.num_frames(n, n_fft, hop) % 4 != 0 and R.stft_route(n, n_fft, hop, 8)["route"] == route
    assert np.unravel_index(a.argmax(), a.shape)[1] == round(0.42 * n_fft) and a[:, :8].max() < 0.01 * a.max()
    L, pmax, _ = h.stft(to_device(x), n_fft, hop, 8)
    assert abs(np.sqrt(pmax) - np.sqrt(pmax_ref)) <= R.gamma(n_fft, route) * S.max(), (pmax, pmax_ref)
    assert np.sqrt(pmax) > 50 * R.db_to_amp(L).max()  # not the maximum of what was written


@pytest.mark.parametrize("route,n_fft,hop,n", ROUTE_SHAPES)
def test_pmax_from_the_last_ragged_frame(h, route, n_fft, hop, n):
    x = R.make_input("noise", n, n_fft, hop).copy()
    T = R.num_frames(n, n_fft, hop)
    x[(T - 1) * hop :] *= np.float32(16.0)  # from the last frame's centre on: the frame before sees it under the window's tail
    a, pmax_ref, S = R.stft_ref(x, n_fft, hop)
    assert T % 4 != 0 and np.unravel_index(a.argmax(), a.shape)[0] == T - 1 and a[T - 1].max() > 1.5 * a[: T - 1].max()
    L, pmax, _ = h.stft(to_device(x), n_fft, hop, 8)
    assert abs(np.sqrt(pmax) - np.sqrt(pmax_ref)) <= R.gamma(n_fft, route) * S.max(), (pmax, pmax_ref)
    assert R.bound_ratio(L, a[:, :8], S, R.gamma(n_fft, route)).max() <= 1.0


# ------------------------------------------------------------------------------------------------ 6. the histogram counts exactly the values written
@pytest.mark.parametrize("family", ["impulses", "noise"])
@pytest.mark.parametrize("route,n_fft,hop,n,k", [("512", 512, 256, 12345, 171), ("512", 512, 256, 12345, 257), ("512", 512, 256, 4095 + 256, 171),
                                                  ("512", 512, 300, 9610, 171), ("512", 512, 255, 7653, 3), ("radix2", 1024, 256, 5300, 342),
                                                  ("dft", 675, 128, 4200, 225)])
def test_histogram_equals_values_written(h, route, n_fft, hop, n, k, family):
    """Order statistics selected on the histogram orcai_stft_db built equal np.sort of the array it wrote, bit for bit.  n_frames mod 4 != 0: on
    the 512-point route the last wave transforms frames past n_frames (zeros: the clamp value, the smallest there is); counting them shifts
    every rank."""
    from orcai_amd.frontend import nearest_rank_index

    T = R.num_frames(n, n_fft, hop)
    assert T % 4 != 0 and R.stft_route(n, n_fft, hop, k)["route"] == route
    x = R.make_input(family, n, n_fft, hop)
    xd = to_device(x)
    cnt = T * k
    for r_lo, r_hi in [(0, cnt - 1), (cnt // 2, cnt // 2), (nearest_rank_index(cnt, 0.01), nearest_rank_index(cnt, 0.999))]:
        L, _, buf = h.stft(xd, n_fft, hop, k)
        lo, hi = h.select(buf, cnt, r_lo, r_hi)
        srt = np.sort(L, axis=None)
        assert lo.view(np.int32) == srt[r_lo].view(np.int32) and hi.view(np.int32) == srt[r_hi].view(np.int32), (r_lo, r_hi, lo, hi, srt[r_lo], srt[r_hi])
        assert h.untouched(buf, cnt)
    if family == "impulses":
        assert (srt == srt[0]).mean() > 0.3 and srt[-1] > srt[0] + 50  # massive ties at the clamp, and values far above it


# ------------------------------------------------------------------------------------------------ 7. orcai_make_spectrogram is its five steps
@pytest.mark.parametrize("n_fft,hop,n,k", [(512, 256, 12345, 171), (1024, 300, 20011, 342)])
def test_make_spectrogram_is_its_steps(h, n_fft, hop, n, k):
    from orcai_amd.frontend import nearest_rank_index

    x = R.make_input("ramp", n, n_fft, hop)
    xd = to_device(x)
    T = R.num_frames(n, n_fft, hop)
    cnt = T * k
    r_lo, r_hi = nearest_rank_index(cnt, 0.01), nearest_rank_index(cnt, 0.999)
    one = h.buffer(cnt)
    assert h.lib.orcai_make_spectrogram(xd.data_ptr(), n, n_fft, hop, T, k, r_lo, r_hi, TOP_DB, one.data_ptr(), h.wsp, h.s) == 0
    st_one = h.stats()
    _, _, steps = h.stft(xd, n_fft, hop, k)
    assert h.lib.orcai_quantile_select(steps.data_ptr(), cnt, r_lo, r_hi, h.wsp, h.s) == 0
    assert h.lib.orcai_frontend_finalize(1, TOP_DB, h.wsp, h.s) == 0
    assert h.lib.orcai_clip_normalize(steps.data_ptr(), cnt, h.wsp, h.s) == 0
    st_steps = h.stats()
    assert torch.equal(one, steps) and h.untouched(one, cnt)
    assert [v.view(np.int32) for v in st_one] == [v.view(np.int32) for v in st_steps]
    out = one[:cnt].view(torch.float32).cpu().numpy()
    assert out.min() == 0.0 and out.max() == 1.0


# ------------------------------------------------------------------------------------------------ 8. refusals
def test_refusals_leave_everything_untouched(h):
    n, n_fft, hop, k = 5000, 512, 256, 171
    T = R.num_frames(n, n_fft, hop)
    xd = torch.from_numpy(R.make_input("noise", n + 8, n_fft, hop)).cuda()
    buf = h.buffer(T * 300)
    p, o, w = xd.data_ptr(), buf.data_ptr(), h.wsp
    assert p % 16 == 0 and o % 16 == 0
    BAD, UNS = R.E_BADARG, R.E_UNSUPPORTED
    cases = [
        ("n_frames one too many", (p, n, n_fft, hop, T + 1, k, o, w), BAD),
        ("n_frames one too few", (p, n, n_fft, hop, T - 1, k, o, w), BAD),
        ("n_frames of the even-size rule for an odd size", (p, n, 675, 250, 1 + n // 250, k, o, w), BAD),
        ("pcm off 16-byte alignment", (p + 4, n, n_fft, hop, T, k, o, w), BAD),
        ("out_db off 16-byte alignment", (p, n, n_fft, hop, T, k, o + 4, w), BAD),
        ("out_db off 16-byte alignment, radix-2 route", (p, n, 1024, hop, T, k, o + 8, w), BAD),
        ("k_crop 0", (p, n, n_fft, hop, T, 0, o, w), BAD),
        ("k_crop 2 + N/2", (p, n, n_fft, hop, T, 258, o, w), BAD),
        ("k_crop 2 + N/2, direct route", (p, n, 500, hop, T, 252, o, w), BAD),
        ("hop 0", (p, n, n_fft, 0, T, k, o, w), BAD),
        ("negative hop", (p, n, n_fft, -256, T, k, o, w), BAD),
        ("n_fft 1", (p, n, 1, hop, T, 1, o, w), BAD),
        ("n_fft 4097", (p, n, 4097, hop, T, k, o, w), UNS),
        ("n_fft 8192", (p, n, 8192, hop, T, k, o, w), UNS),
        ("no samples", (p, 0, n_fft, hop, 1, k, o, w), BAD),
        ("null pcm", (None, n, n_fft, hop, T, k, o, w), BAD),
        ("null out_db", (p, n, n_fft, hop, T, k, None, w), BAD),
        ("null workspace", (p, n, n_fft, hop, T, k, o, None), BAD),
    ]
    assert h.lib.orcai_frontend_reset(h.wsp, h.s) == 0
    ws_before = h.ws.clone()
    for what, args, want in cases:
        n_a, nfft_a, hop_a, T_a, k_a = args[1:6]
        if args[0] is not None and args[6] is not None and args[7] is not None and args[0] % 16 == 0 and args[6] % 16 == 0:
            assert R.stft_route(n_a, nfft_a, hop_a, k_a, n_frames=T_a)["rc"] == want, what
        assert h.lib.orcai_stft_db(*args, h.s) == want, what
        torch.cuda.synchronize()
        assert h.untouched(buf), what
        assert torch.equal(h.ws, ws_before), what
    assert h.lib.orcai_frontend_reset(None, h.s) == BAD
    assert h.lib.orcai_frontend_stats_host(None, (C.c_float * 6)(), h.s) == BAD
    assert h.lib.orcai_quantile_select(None, 10, 0, 9, h.wsp, h.s) == BAD and h.lib.orcai_quantile_select(o, 10, 0, 10, h.wsp, h.s) == BAD
    assert h.untouched(buf)
