"""The gradient of the denoised front end w.r.t. the audio on the GPU: orcai_denoised_spectrogram_bwd against the float64 reference of
tests/denoise_grad_ref.py on both routes, a zero floor against the plain backward entries bit for bit, the floor in the gate, the launcher's contract and
refusals, and the chain make_spectrogram -> backward on the device, the torch ops, DenoisedWaveformFrontEnd and the detector behind it."""

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import denoise_grad_ref as R  # noqa: E402
import orcai_amd.torch_ops  # noqa: E402, F401  (registers the ops)

# Measured on the CPU for exactly these inputs (tests/denoise_grad_ref.py run as a script prints this table): the reference's formula evaluated by torch
# in float32 -- from the same pcm, g, statistics and profile the kernel gets -- deviates from its float64 evaluation by this share of max|dpcm|.  The bar
# for the kernel is 8 x the value of its case, the bar and the argument of tests/test_frontend_grad_gpu.py and tests/test_mel_grad_gpu.py (the
# f32 evaluation of the same formula is what the hardware can be asked for, 8 covers another legitimate summation order).
F32_REFERENCE_DEVIATION = {
    "512-256-a": 3.34e-06,  # quantile 0.5: tie share 4.2e-05, floored 7.3e-05
    "512-256-b": 4.02e-06,  # quantile 0.5: tie share 5.2e-05, floored 6.4e-02
    "2048-300-a": 2.47e-06,  # quantile 0.5: tie share 9.1e-06, floored 1.2e-04
    "2048-300-b": 3.11e-06,  # quantile 0.5: tie share 3.3e-05, floored 5.6e-02
    "32-16-a": 5.91e-06,  # quantile 0.5: tie share 2.0e-05, floored 1.1e-04
    "32-16-b": 6.55e-06,  # quantile 0.5: tie share 3.0e-05, floored 6.7e-02
    "512-256-64-a": 2.43e-06,  # quantile 0.5: tie share 8.3e-05, floored 0.0e+00
    "512-256-64-b": 1.58e-06,  # quantile 0.5: tie share 8.3e-05, floored 6.4e-02
    "128-32-8-a": 3.33e-06,  # quantile 0.5: tie share 1.1e-04, floored 0.0e+00
    "128-32-8-b": 2.44e-06,  # quantile 0.5: tie share 5.6e-05, floored 6.6e-02
    "4096-1000-64-a": 6.15e-07,  # quantile 0.5: tie share 2.2e-04, floored 0.0e+00
    "4096-1000-64-b": 7.79e-07,  # quantile 0.5: tie share 5.4e-04, floored 4.1e-02
    "512-256-a-q25": 3.21e-06,  # quantile 0.25: tie share 3.1e-05, floored 7.3e-05
    "512-256-64-b-q25": 1.68e-06,  # quantile 0.25: tie share 8.3e-05, floored 6.4e-02
}
LIN0, MEL0 = R.LINEAR[0], R.MEL[0]
SP_LIN, SP_MEL = R.parameter(LIN0, "a"), R.parameter(MEL0, "a")
LIN_ARGS = (48000, 512, 256, 16000.0, 0, 0.0, 0.0, False, True, 0.5, 0.01, 0.999)
MEL_ARGS = (48000, 512, 256, 0.0, 64, 0.0, 24000.0, False, True, 0.5, 0.01, 0.999)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(torch.int32), b.view(torch.int32))


def _fe():
    from orcai_amd.frontend import get_frontend

    return get_frontend()


def _weights(route):
    t = R.M.table_of(route)
    return t, torch.from_numpy(t["weights"].copy()).cuda()


def _bwd(pcm, n_fft, hop, n_frames, k, g, stats, profile, dpcm, table=None, weights=None, n_samples=None, n_weights=None, lo=None, hi=None, top_db=80.0):
    """The C entry point itself (return code, no exception).  A tensor argument may be None (a null) or an int (a raw address); table: a band table (host
    arrays) selects the mel route, lo / hi override its arrays."""
    from orcai_amd import _native as N

    p = lambda t: 0 if t is None else (t if isinstance(t, int) else N.ptr(t))  # noqa: E731
    keep = None
    bands = (0, 0, 0)
    if table is not None:
        keep = [np.ascontiguousarray(a, dtype=np.int32) for a in (table["lo"] if lo is None else lo, table["hi"] if hi is None else hi, table["off"])]
        bands = tuple(a.ctypes.data for a in keep)
    n = pcm.numel() if n_samples is None else n_samples
    nw = (0 if weights is None else weights.numel()) if n_weights is None else n_weights
    return N.lib().orcai_denoised_spectrogram_bwd(p(pcm), n, n_fft, hop, n_frames, k, *bands, p(weights), nw, p(g), p(stats), p(profile), top_db, p(dpcm),
                                                  N.stream_ptr())


# ------------------------------------------------------------------------------------------------------------------ 1. the kernel against the definition
@pytest.mark.parametrize("name", list(R.CASES))
def test_kernel_against_the_float64_reference(name):
    """Measured on an MI355X: the kernel's error is 0.6 - 1.6 x the torch-float32 deviation of its case (the printed line).  The statistics tensor carries a poisoned ref_db slot: the backward takes
    ref_db from pmax and never reads it."""
    c = R.case(name)
    route, which, quantile = R.CASES[name]
    dpcm = _fe().denoised_spectrogram_backward(c["pcm"].cuda(), c["g"].cuda(), R.stats_tensor(c, "cuda", ref_db_slot=float("nan")), R.profile_tensor(c, "cuda"),
                                               R.parameter(route, which, quantile))
    ref = c["dpcm64"]
    share = float((dpcm.cpu().double() - ref).abs().max() / ref.abs().max())
    dev = F32_REFERENCE_DEVIATION[name]
    print(f"{name}: kernel error {share:.2e} of max|dpcm|; torch f32 {dev:.2e}; bar {8 * dev:.2e}")
    assert torch.isfinite(dpcm).all()
    assert share <= 8 * dev, (share, dev)


# ------------------------------------------------------------------------------------------------------------------ 2. a zero floor is the plain backward
@pytest.mark.parametrize("route", [R.LINEAR[0], R.LINEAR[1], R.MEL[0]], ids=lambda r: "-".join(map(str, r[:3])))
def test_a_zero_floor_is_the_plain_backward_bit_for_bit(route):
    """The statistics of the PLAIN forward (its ref_db in slot 1, which the plain entry reads and the new one recomputes from pmax) and profile = 0:
    ref_db from pmax and the unchanged arithmetic behind the gate at once."""
    fe = _fe()
    for which in ("a", "b"):
        sp = {k: v for k, v in R.parameter(route, which).items() if k != "denoise"}
        pcm = torch.from_numpy(R.G.recording(which).copy()).cuda()
        spec, stats = fe.make_spectrogram(pcm, sp, return_stats=True)
        T, K = spec.shape
        g = torch.randn((T, K), device="cuda", generator=torch.Generator("cuda").manual_seed(11))
        want = fe.backward(pcm, g, stats, sp)
        dpcm = torch.full_like(pcm, float("nan"))
        table, w = _weights(route) if R.is_mel(route) else (None, None)
        assert _bwd(pcm, route[0], route[1], T, K, g, stats, torch.zeros(K, device="cuda"), dpcm, table, w) == 0
        assert float(want.abs().max()) > 0 and same_bits(dpcm, want), (route, which)


# ------------------------------------------------------------------------------------------------------------------ 3. the floor enters the gate
@pytest.mark.parametrize("name, k", [("512-256-a", 40), ("512-256-64-a", 20), ("512-256-64-a", 21)])
def test_the_floor_enters_the_gate_of_its_own_channel_only(name, k):
    """g is 1 on channel k (0 where that channel's gate is decided within rounding, as everywhere in these files) and 0 elsewhere."""
    c = R.case(name)
    route, which, quantile = R.CASES[name]
    sp = R.parameter(route, which, quantile)
    g = torch.zeros_like(c["g"])
    g[:, k] = 1.0
    g[R.tie_mask(c["aux"])] = 0.0
    assert float(g.sum()) > 0.9 * g.shape[0]
    ref = R.dpcm_in(torch.float64, c, g=g)
    fe = _fe()
    pcm, stats, profile = c["pcm"].cuda(), R.stats_tensor(c, "cuda"), R.profile_tensor(c, "cuda")
    dpcm = fe.denoised_spectrogram_backward(pcm, g.cuda(), stats, profile, sp)
    share = float((dpcm.cpu().double() - ref).abs().max() / ref.abs().max())
    print(f"{name} channel {k}: kernel error {share:.2e} of max|dpcm|")
    assert float(ref.abs().max()) > 0 and share <= 1e-4
    up = profile.clone()
    up[k] += 200.0  # y = v - m[k] - 200 < -200 < p_lo for every frame of the channel
    assert c["stats"][1] > -200.0
    assert not fe.denoised_spectrogram_backward(pcm, g.cuda(), stats, up, sp).any()
    other = profile + 200.0
    other[k] = profile[k]
    assert same_bits(fe.denoised_spectrogram_backward(pcm, g.cuda(), stats, other, sp), dpcm)


# ------------------------------------------------------------------------------------------------------------------ 4. the launcher
def test_two_launches_give_identical_bits_and_every_element_is_written():
    for name in ("512-256-b", "2048-300-b", "512-256-64-b", "4096-1000-64-b"):  # wave per run, workgroup per run, on both routes; more than 64 KiB of LDS
        c = R.case(name)
        route = c["route"]
        pcm, stats, profile = c["pcm"].cuda(), R.stats_tensor(c, "cuda"), R.profile_tensor(c, "cuda")
        table, w = _weights(route) if R.is_mel(route) else (None, None)
        T, K = c["g"].shape
        g = torch.randn((T, K), device="cuda", generator=torch.Generator("cuda").manual_seed(3))
        outs = []
        for _ in range(2):
            dpcm = torch.full((pcm.numel(),), float("nan"), device="cuda")
            assert _bwd(pcm, route[0], route[1], T, K, g, stats, profile, dpcm, table, w) == 0
            outs.append(dpcm)
        assert torch.isfinite(outs[0]).all() and float(outs[0].abs().max()) > 0, name
        assert same_bits(outs[0], outs[1]), name


@pytest.mark.parametrize("route", [LIN0, MEL0], ids=["linear", "mel"])
def test_a_recording_shorter_than_one_window(route):
    """100 samples, one frame of 512.  One frame is its own floor (y = 0, no range), so the profile is a given ramp instead; the bounds are the order
    statistics of the resulting y.  The bar is 8 x the float32 deviation of this very case."""
    pcm = torch.from_numpy(R.G.recording("a")[:100].copy())
    K = R.channels(route)
    c = R.build_case(pcm, route, 0.5, (0.01, 0.999), seed=9, floor=torch.linspace(-50.0, -20.0, K, dtype=torch.float64))
    ref = c["dpcm64"]
    dev = float((R.dpcm_in(torch.float32, c).double() - ref).abs().max() / ref.abs().max())
    dpcm = _fe().denoised_spectrogram_backward(pcm.cuda(), c["g"].cuda(), R.stats_tensor(c, "cuda"), R.profile_tensor(c, "cuda"), R.parameter(route, "a"))
    share = float((dpcm.cpu().double() - ref).abs().max() / ref.abs().max())
    print(f"100 samples, {len(route) > 2 and 'mel' or 'linear'}: kernel error {share:.2e} of max|dpcm|; torch f32 {dev:.2e}")
    assert c["out64"].shape == (1, K) and dpcm.shape == (100,) and float(ref.abs().max()) > 0 and share <= 8 * dev, (share, dev)


def test_refusals_leave_dpcm_untouched():
    from orcai_amd import _native as N

    pcm = torch.from_numpy(R.G.recording("a")[:4000].copy()).cuda()
    n = pcm.numel()
    table, w = _weights(MEL0)
    T = 1 + n // 256
    g = torch.zeros((T + 1, 171), device="cuda")
    stats = torch.tensor([1.0, 0.0, -30.0, 25.0, -30.0, 25.0], device="cuda")
    profile = torch.full((172,), -40.0, device="cuda")
    lin = dict(pcm=pcm, n_fft=512, hop=256, n_frames=T, k=171, g=g, stats=stats, profile=profile)
    mel = dict(lin, k=64, table=table, weights=w)
    for a in (lin, mel):
        ok = torch.full((n,), float("nan"), device="cuda")
        assert _bwd(dpcm=ok, **a) == 0 and torch.isfinite(ok).all()
    dpcm = torch.full((n,), float("nan"), device="cuda")

    def refused(want, what, base, **change):
        assert _bwd(dpcm=dpcm, **dict(base, **change)) == want, what
        assert torch.isnan(dpcm).all(), what

    for name, base in (("linear", lin), ("mel", mel)):
        for missing in ("pcm", "g", "stats", "profile"):  # null device pointers (a null dpcm has nothing to leave untouched: checked below)
            refused(N.E_BADARG, (name, missing), base, **{missing: None}, n_samples=n)
        assert _bwd(dpcm=None, **base) == N.E_BADARG
        for odd in ("g", "stats", "profile"):  # not 4-byte aligned
            refused(N.E_BADARG, (name, odd, "misaligned"), base, **{odd: N.ptr(base[odd]) + 2})
        assert _bwd(dpcm=N.ptr(dpcm) + 2, **base) == N.E_BADARG and torch.isnan(dpcm).all()
        refused(N.E_BADARG, (name, "n_samples 0"), base, n_samples=0)
        refused(N.E_BADARG, (name, "hop 0"), base, hop=0)
        refused(N.E_BADARG, (name, "n_frames + 1"), base, n_frames=T + 1)
        for nfft in (500, 16, 8192):
            refused(N.E_UNSUPPORTED, (name, nfft), base, n_fft=nfft, hop=250, n_frames=1 + n // 250, k=8)
    refused(N.E_BADARG, "k 0", lin, k=0)
    refused(N.E_BADARG, "k past 1 + n_fft / 2", lin, k=258)
    refused(N.E_UNSUPPORTED, "mel at n_fft 64", mel, n_fft=64, hop=250, n_frames=1 + n // 250)
    refused(N.E_BADARG, "n_mels 7", mel, k=7)
    refused(N.E_BADARG, "null weights", mel, weights=None, n_weights=w.numel())
    refused(N.E_BADARG, "misaligned pcm on the mel route", mel, pcm=pcm[1:], n_frames=1 + (n - 1) // 256)
    hi = table["hi"].copy()
    hi[63] = 258
    refused(N.E_BADARG, "band past 1 + n_fft / 2", mel, hi=hi)
    lo = table["lo"].copy()
    assert table["hi"][0] <= table["lo"][2]
    lo[2] = table["hi"][0] - 1  # band 2 now starts under band 0: two even bands share a bin
    hi2 = table["hi"].copy()
    hi2[2] -= 1
    refused(N.E_UNSUPPORTED, "bands 0 and 2 overlap", mel, lo=lo, hi=hi2)

    fe = _fe()
    g, profile = g[:T], profile[:171]
    with pytest.raises(ValueError, match=r"grad must be a float32 CUDA tensor \[16, 171\] \(nfft = 512, hop = 256"):
        fe.denoised_spectrogram_backward(pcm, g[:-1], stats, profile, SP_LIN)
    with pytest.raises(ValueError, match=r"stats must be the float32 CUDA tensor \[6\]"):
        fe.denoised_spectrogram_backward(pcm, g, stats[:5], profile, SP_LIN)
    with pytest.raises(ValueError, match=r"profile must be the float32 CUDA tensor \[171\]"):
        fe.denoised_spectrogram_backward(pcm, g, stats, profile[:-1], SP_LIN)
    with pytest.raises(ValueError, match=r"nfft = 512, n_mels = 64.*profile must be the float32 CUDA tensor \[64\]"):
        fe.denoised_spectrogram_backward(pcm, g[:, :64].contiguous(), stats, profile, SP_MEL)
    with pytest.raises(ValueError, match="profile"):
        fe.denoised_spectrogram_backward(pcm, g, stats, profile.double(), SP_LIN)
    lib = N.lib()
    assert lib.orcai_denoised_spectrogram_bwd_occupancy(512, 0) >= 2 and lib.orcai_denoised_spectrogram_bwd_occupancy(512, 64) >= 2
    assert lib.orcai_denoised_spectrogram_bwd_occupancy(4096, 0) >= 1
    assert lib.orcai_denoised_spectrogram_bwd_occupancy(500, 0) == -1 and lib.orcai_denoised_spectrogram_bwd_occupancy(64, 64) == -1
    for nfft, n_mels in ((512, 64), (2048, 64)):  # the same launch plan and a kernel of the same footprint: as many workgroups per compute unit as the plain twin
        assert lib.orcai_denoised_spectrogram_bwd_occupancy(nfft, n_mels) == lib.orcai_mel_spectrogram_bwd_occupancy(nfft, n_mels)


# ------------------------------------------------------------------------------------------------------------------ 5. end to end
@pytest.mark.parametrize("sp, args", [(SP_LIN, LIN_ARGS), (SP_MEL, MEL_ARGS)], ids=["linear", "mel"])
def test_forward_then_backward_on_the_device_is_the_ops_gradient(sp, args):
    fe = _fe()
    pcm1 = torch.from_numpy(R.G.recording("a")[: 48000 + 17].copy()).cuda()
    pcm2 = torch.from_numpy(R.G.recording("b")[40000:100000].copy()).cuda()
    want = fe.make_spectrogram(pcm1, sp)
    assert same_bits(torch.ops.orcai.denoised_spectrogram(pcm1, *args), want)
    with torch.no_grad():
        assert same_bits(torch.ops.orcai.denoised_spectrogram_wrt_pcm(pcm1, *args), want)
    x1, x2 = pcm1.clone().requires_grad_(), pcm2.clone().requires_grad_()
    s1 = torch.ops.orcai.denoised_spectrogram_wrt_pcm(x1, *args)
    s2 = torch.ops.orcai.denoised_spectrogram_wrt_pcm(x2, *args)  # another recording overwrites the front end's workspace and scratch before s1's backward
    assert same_bits(s1.detach(), want) and s1.requires_grad
    g = torch.randn(s1.shape, device="cuda", generator=torch.Generator("cuda").manual_seed(1))
    (d1,) = torch.autograd.grad(s1, x1, g)
    spec1, st1, prof1 = fe.make_spectrogram(pcm1, sp, return_stats=True, return_profile=True)  # device tensors, handed on as they are
    assert same_bits(spec1, want)
    assert same_bits(d1, fe.denoised_spectrogram_backward(pcm1, g, st1, prof1, sp))
    assert torch.isfinite(d1).all() and float(d1.abs().max()) > 0
    (d2,) = torch.autograd.grad(s2.sum(), x2)
    _, st2, prof2 = fe.make_spectrogram(pcm2, sp, return_stats=True, return_profile=True)
    assert same_bits(d2, fe.denoised_spectrogram_backward(pcm2, torch.ones_like(s2), st2, prof2, sp))
    with pytest.raises(NotImplementedError, match="denoised_spectrogram_wrt_pcm"):  # the plain op stays forward only and says where the gradient is
        torch.ops.orcai.denoised_spectrogram(x1, *args).sum().backward()
    with pytest.raises(NotImplementedError, match="denoise"):  # and FrontEnd.backward keeps refusing
        fe.backward(pcm1, g, st1, sp)


def test_opcheck_and_compile_of_the_new_ops():
    from torch.library import opcheck

    pcm = torch.from_numpy(R.G.recording("a")[:24000].copy()).cuda()
    opcheck(torch.ops.orcai.denoised_spectrogram.default, (pcm, *MEL_ARGS))
    opcheck(torch.ops.orcai.denoised_spectrogram_wrt_pcm.default, (pcm, *LIN_ARGS))
    opcheck(torch.ops.orcai.denoised_spectrogram_wrt_pcm.default, (pcm.clone().requires_grad_(), *LIN_ARGS))
    opcheck(torch.ops.orcai.denoised_spectrogram_with_stats.default, (pcm, *LIN_ARGS))
    spec, stats, profile = torch.ops.orcai.denoised_spectrogram_with_stats(pcm, *LIN_ARGS)
    opcheck(torch.ops.orcai.denoised_spectrogram_backward.default, (torch.ones_like(spec), pcm, stats, profile, *LIN_ARGS[:-2]))

    def f(x):
        return (torch.ops.orcai.denoised_spectrogram_wrt_pcm(x, *LIN_ARGS) ** 2).sum()

    x, xc = pcm.clone().requires_grad_(), pcm.clone().requires_grad_()
    loss = f(x)
    loss.backward()
    loss_c = torch.compile(f, backend="aot_eager", fullgraph=True)(xc)  # fullgraph: a graph break is an error
    loss_c.backward()
    assert same_bits(loss_c.detach(), loss.detach()) and same_bits(xc.grad, x.grad) and float(x.grad.abs().max()) > 0


def test_waveform_gradient_through_the_detector():
    """pcm at 96 kHz -> DenoisedWaveformFrontEnd (resample, denoised_spectrogram_wrt_pcm on 64 mel bands) -> snippets -> OrcaiModule(input_grad="eval")
    -> scalar loss -> backward: pcm.grad has the native length, is finite, non-zero and, bit for bit, the chain composed by hand (the construction of
    tests/test_mel_grad_gpu.py's test of the same name, with its model)."""
    from orcai_amd.architectures import ResNet1DConv
    from orcai_amd.resample import resample_device
    from orcai_amd.torch_ops import DenoisedWaveformFrontEnd, OrcaiModule

    H, W, B = 64, 64, 2
    model = ResNet1DConv((H, W, 1), 4, [12, 20], 3, dropout_rate=0.0, seed=4)
    m = OrcaiModule(model, input_grad="eval").cuda().eval()
    front = DenoisedWaveformFrontEnd(SP_MEL, 96000)
    rng = np.random.default_rng(7)
    t = np.arange(96000) / 96000.0
    pcm0 = torch.from_numpy((0.1 * rng.uniform(-1, 1, t.size) + 0.3 * np.sin(2 * np.pi * (3000.0 * t + 4000.0 * t * t))).astype(np.float32)).cuda()
    pcm = pcm0.clone().requires_grad_()
    spec = front(pcm)
    assert spec.shape[1] == W and spec.shape[0] >= B * H
    x = spec[: B * H].view(B, H, W)
    x.retain_grad()
    loss = (m(x) ** 2).sum()
    loss.backward()
    assert pcm.grad.shape == pcm0.shape and torch.isfinite(pcm.grad).all() and float(pcm.grad.abs().max()) > 0
    fe = _fe()
    at_rate = resample_device(pcm0, 96000, 48000)
    spec0, st, prof = fe.make_spectrogram(at_rate, SP_MEL, return_stats=True, return_profile=True)
    assert same_bits(spec0, spec.detach())
    gspec = torch.zeros_like(spec0)
    gspec[: B * H] = x.grad.view(B * H, W)
    d_rate = fe.denoised_spectrogram_backward(at_rate, gspec, st, prof, SP_MEL)
    assert same_bits(pcm.grad, torch.ops.orcai.resample_backward(d_rate, pcm0.numel(), 96000, 48000))
    # the linear route's module at the native rate, on its own
    lin = DenoisedWaveformFrontEnd(SP_LIN, 96000)
    p2 = pcm0.clone().requires_grad_()
    (lin(p2) ** 2).sum().backward()
    assert p2.grad.shape == pcm0.shape and torch.isfinite(p2.grad).all() and float(p2.grad.abs().max()) > 0
