"""The gradient of the mel front end w.r.t. the audio on the GPU: orcai_mel_spectrogram_bwd against the float64 reference of tests/mel_grad_ref.py, the
launcher's contract and refusals, the torch ops (mel_spectrogram_wrt_pcm and the two functional ops underneath) and the chain native-rate pcm ->
waveform_front_end -> snippets -> OrcaiModule(input_grad="eval") -> loss differentiated down to the waveform."""

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import mel_grad_ref as R  # noqa: E402
import orcai_amd.torch_ops  # noqa: E402, F401  (registers the ops)

# Measured on the CPU for exactly these inputs (tests/mel_grad_ref.py run as a script prints this table): the reference's formula evaluated by torch in
# float32 -- from the same pcm, g and statistics the kernel gets -- deviates from its float64 evaluation by this share of max|dpcm|.  The bar for the
# kernel is 8 x the value of its case (the f32 evaluation of the same formula is what the hardware can be asked for, 8 covers another
# legitimate summation order).  Key: (recording, index into R.CASES).
F32_REFERENCE_DEVIATION = {
    ("a", 0): 1.70e-06,  # 512 / 256 / 64: tie share 1.1e-04, floored 0.0e+00
    ("a", 1): 1.17e-06,  # 512 / 255 / 128: tie share 4.1e-05, floored 0.0e+00
    ("a", 2): 1.20e-06,  # 128 / 32 / 8: tie share 5.6e-05, floored 0.0e+00
    ("a", 3): 1.04e-06,  # 1024 / 512 / 40: tie share 1.8e-04, floored 0.0e+00
    ("a", 4): 5.20e-07,  # 2048 / 300 / 64: tie share 6.5e-05, floored 0.0e+00
    ("a", 5): 4.80e-07,  # 4096 / 1000 / 64: tie share 2.2e-04, floored 0.0e+00
    ("b", 0): 1.56e-06,  # 512 / 256 / 64: tie share 8.3e-05, floored 6.4e-02
    ("b", 1): 1.47e-06,  # 512 / 255 / 128: tie share 2.8e-05, floored 6.2e-02
    ("b", 2): 9.44e-07,  # 128 / 32 / 8: tie share 1.7e-04, floored 6.6e-02
    ("b", 3): 8.53e-07,  # 1024 / 512 / 40: tie share 1.8e-04, floored 6.0e-02
    ("b", 4): 8.14e-07,  # 2048 / 300 / 64: tie share 2.3e-04, floored 5.4e-02
    ("b", 5): 1.13e-06,  # 4096 / 1000 / 64: tie share 5.4e-04, floored 4.1e-02
}
MEL0 = R.CASES[0]
SP = R.parameter(MEL0, "a")
ARGS = (48000, 512, 256, 64, 0.0, 24000.0, False, True, 0.01, 0.999)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(torch.int32), b.view(torch.int32))


def _fe():
    from orcai_amd.frontend import get_frontend

    return get_frontend()


def _bwd(pcm, n_fft, hop, n_frames, table, weights, g, stats, dpcm, n_samples=None, n_mels=None, n_weights=None, lo=None, hi=None, off=None, top_db=80.0):
    """The C entry point itself (return code, no exception).  table: a band table (host arrays); lo / hi / off override its arrays, 0 passes a null."""
    from orcai_amd import _native as N

    p = lambda t: 0 if t is None else N.ptr(t)  # noqa: E731
    h = lambda o, a: 0 if o is None and a is None else (o if o is not None else a).ctypes.data  # noqa: E731
    keep = [np.ascontiguousarray(a, dtype=np.int32) if a is not None else None for a in (lo, hi, off)]
    n = pcm.numel() if n_samples is None else n_samples
    return N.lib().orcai_mel_spectrogram_bwd(p(pcm), n, n_fft, hop, n_frames, table["lo"].size if n_mels is None else n_mels,
                                             h(keep[0], table.get("lo")), h(keep[1], table.get("hi")), h(keep[2], table.get("off")), p(weights),
                                             (0 if weights is None else weights.numel()) if n_weights is None else n_weights, p(g), p(stats), top_db, p(dpcm),
                                             N.stream_ptr())


# ------------------------------------------------------------------------------------------------------------------ 1. the kernel against the definition
@pytest.mark.parametrize("which", ["a", "b"])
@pytest.mark.parametrize("index", range(len(R.CASES)))
def test_kernel_against_the_float64_reference(which, index):
    """Measured on an MI355X: the kernel's error is 0.7 - 1.5 x the torch-float32 deviation of its case (the printed line)."""
    c = R.case(which, index)
    mc = R.CASES[index]
    dpcm = _fe().mel_spectrogram_backward(c["pcm"].cuda(), c["g"].cuda(), R.stats_tensor(c, "cuda"), R.parameter(mc, which))
    ref = c["dpcm64"]
    share = float((dpcm.cpu().double() - ref).abs().max() / ref.abs().max())
    dev = F32_REFERENCE_DEVIATION[(which, index)]
    print(f"({which}) nfft {mc[0]} hop {mc[1]} n_mels {mc[2]}: kernel error {share:.2e} of max|dpcm|; torch f32 {dev:.2e}; bar {8 * dev:.2e}")
    assert torch.isfinite(dpcm).all()
    assert share <= 8 * dev, (share, dev)


# ------------------------------------------------------------------------------------------------------------------ 2. the launcher
def test_two_launches_give_identical_bits_and_every_element_is_written():
    for index in (0, 4, 5):  # 512 / 256: wave per run; 2048 / 300: workgroup per run; 4096 / 1000: more than 64 KiB of LDS
        mc = R.CASES[index]
        c = R.case("b", index)
        pcm, stats = c["pcm"].cuda(), R.stats_tensor(c, "cuda")
        t = R.table_of(mc)
        w = torch.from_numpy(t["weights"].copy()).cuda()
        T = 1 + pcm.numel() // mc[1]
        g = torch.randn((T, mc[2]), device="cuda", generator=torch.Generator("cuda").manual_seed(3))
        outs = []
        for _ in range(2):
            dpcm = torch.full((pcm.numel(),), float("nan"), device="cuda")
            assert _bwd(pcm, mc[0], mc[1], T, t, w, g, stats, dpcm) == 0
            outs.append(dpcm)
        assert torch.isfinite(outs[0]).all() and float(outs[0].abs().max()) > 0, mc
        assert same_bits(outs[0], outs[1]), mc


def test_a_recording_shorter_than_one_window():
    """100 samples, one frame of 512 (all but 100 of its samples are padding).  The bar is 8 x the float32 deviation of this very case."""
    pcm = torch.from_numpy(R.G.recording("a")[:100].copy())
    c = R.build_case(pcm, MEL0, (0.01, 0.999), seed=9)
    ref = c["dpcm64"]
    dev = float((R.dpcm_in(torch.float32, c, MEL0, None).double() - ref).abs().max() / ref.abs().max())
    dpcm = _fe().mel_spectrogram_backward(pcm.cuda(), c["g"].cuda(), R.stats_tensor(c, "cuda"), SP)
    share = float((dpcm.cpu().double() - ref).abs().max() / ref.abs().max())
    print(f"100 samples: kernel error {share:.2e} of max|dpcm|; torch f32 {dev:.2e}")
    assert c["out64"].shape == (1, 64) and dpcm.shape == (100,) and float(ref.abs().max()) > 0 and share <= 8 * dev, (share, dev)


def test_one_band_of_one_frame_reaches_only_that_frames_window():
    """g zero but for (frame 20, band m): dpcm is zero outside [20 hop - nfft/2, 20 hop + nfft/2), and inside it equals the float64 gradient of that
    single element -- a gather that read another band's dM (zero here) would return zeros, one that read this dM for another band's bins a wrong shape."""
    nfft, hop = MEL0[0], MEL0[1]
    c = R.case("a", 0)
    pcm = c["pcm"][:20000].contiguous()
    stats = c["stats"]
    for m in (0, 31, 62, 63):  # first, an odd, an even and the last band
        x = pcm.double().requires_grad_()
        out, aux = R.forward(x, MEL0, None, stats=stats)
        assert stats[1] + 1.0 < float(aux["v"][20, m]) < stats[2] - 1.0, (m, float(aux["v"][20, m]))  # the element's gates are open, away from ties
        g = torch.zeros(out.shape)
        g[20, m] = 1.0
        (ref,) = torch.autograd.grad(out, x, g.double())
        dpcm = _fe().mel_spectrogram_backward(pcm.cuda(), g.cuda(), R.stats_tensor(c, "cuda"), SP).cpu()
        a, b = 20 * hop - nfft // 2, 20 * hop + nfft // 2
        assert not dpcm[:a].any() and not dpcm[b:].any(), m
        assert float(ref.abs().max()) > 0 and float((dpcm.double() - ref).abs().max() / ref.abs().max()) <= 1e-4, m


# ------------------------------------------------------------------------------------------------------------------ 3. refusals
def test_refusals_leave_dpcm_untouched():
    from orcai_amd import _native as N

    pcm = torch.from_numpy(R.G.recording("a")[:4000].copy()).cuda()
    n = pcm.numel()
    t = R.table_of(MEL0)
    w = torch.from_numpy(t["weights"].copy()).cuda()
    T = 1 + n // 256
    g = torch.zeros((T + 1, 64), device="cuda")
    stats = torch.tensor([1.0, 0.0, -60.0, -5.0, -60.0, -5.0], device="cuda")
    ok = torch.full((n,), float("nan"), device="cuda")
    assert _bwd(pcm, 512, 256, T, t, w, g, stats, ok) == 0 and torch.isfinite(ok).all()
    dpcm = torch.full((n,), float("nan"), device="cuda")

    def refused(want, what, *a, **k):
        assert _bwd(*a, **k) == want, what
        assert torch.isnan(dpcm).all(), what

    for missing in ("pcm", "w", "g", "stats"):  # null device pointers (a null dpcm has nothing to leave untouched: checked below)
        a = dict(pcm=pcm, w=w, g=g, stats=stats)
        a[missing] = None
        refused(N.E_BADARG, missing, a["pcm"], 512, 256, T, t, a["w"], a["g"], a["stats"], dpcm, n_samples=n, n_weights=w.numel())
    assert _bwd(pcm, 512, 256, T, t, w, g, stats, None) == N.E_BADARG
    for missing in ("lo", "hi", "off"):  # null host arrays
        refused(N.E_BADARG, missing, pcm, 512, 256, T, {k: v for k, v in t.items() if k != missing}, w, g, stats, dpcm, n_mels=64)
    refused(N.E_BADARG, "n_samples 0", pcm, 512, 256, T, t, w, g, stats, dpcm, n_samples=0)
    refused(N.E_BADARG, "hop 0", pcm, 512, 0, T, t, w, g, stats, dpcm)
    refused(N.E_BADARG, "n_frames + 1", pcm, 512, 256, T + 1, t, w, g, stats, dpcm)
    refused(N.E_BADARG, "n_mels 7", pcm, 512, 256, T, t, w, g, stats, dpcm, n_mels=7)
    big = {k: np.resize(t[k], 257) for k in ("lo", "hi", "off")}
    refused(N.E_BADARG, "n_mels 257", pcm, 512, 256, T, big, w, g, stats, dpcm, n_mels=257)
    hi = t["hi"].copy()
    hi[63] = 258
    refused(N.E_BADARG, "band past 1 + n_fft / 2", pcm, 512, 256, T, t, w, g, stats, dpcm, hi=hi)
    off = t["off"].copy()
    off[63] = w.numel() - 1
    refused(N.E_BADARG, "offset past n_weights", pcm, 512, 256, T, t, w, g, stats, dpcm, off=off)
    refused(N.E_BADARG, "n_weights 0", pcm, 512, 256, T, t, w, g, stats, dpcm, n_weights=0)
    refused(N.E_BADARG, "misaligned pcm", pcm[1:], 512, 256, 1 + (n - 1) // 256, t, w, g, stats, dpcm)
    for nfft in (500, 64, 8192):
        refused(N.E_UNSUPPORTED, nfft, pcm, nfft, 250, 1 + n // 250, t, w, g, stats, dpcm)
    lo = t["lo"].copy()
    assert t["hi"][0] <= t["lo"][2]
    lo[2] = t["hi"][0] - 1  # band 2 now starts under band 0: two even bands share a bin (its weights run one short of the band: still inside the array)
    hi2 = t["hi"].copy()
    hi2[2] -= 1
    refused(N.E_UNSUPPORTED, "bands 0 and 2 overlap", pcm, 512, 256, T, t, w, g, stats, dpcm, lo=lo, hi=hi2)
    fe = _fe()
    with pytest.raises(ValueError, match="nfft = 512, n_mels = 64"):
        fe.mel_spectrogram_backward(pcm, g[:-2], stats, SP)
    with pytest.raises(NotImplementedError, match="nfft"):
        fe.mel_spectrogram_backward(pcm, g, stats, dict(SP, nfft=500))
    with pytest.raises(ValueError, match="mel"):
        fe.mel_spectrogram_backward(pcm, g, stats, {k: v for k, v in SP.items() if k != "mel"})
    with pytest.raises(NotImplementedError, match="mel_spectrogram_backward"):
        fe.spectrogram_backward(pcm, g, stats, SP)
    assert N.lib().orcai_mel_spectrogram_bwd_occupancy(512, 64) >= 2 and N.lib().orcai_mel_spectrogram_bwd_occupancy(4096, 256) >= 1
    assert N.lib().orcai_mel_spectrogram_bwd_occupancy(500, 64) == -1


# ------------------------------------------------------------------------------------------------------------------ 4. the ops
def test_op_forward_bits_gradient_bits_and_stats_survive_another_recording():
    fe = _fe()
    pcm1 = torch.from_numpy(R.G.recording("a")[:48000 + 17].copy()).cuda()
    pcm2 = torch.from_numpy(R.G.recording("b")[40000:100000].copy()).cuda()
    want = torch.ops.orcai.mel_spectrogram(pcm1, *ARGS)
    with torch.no_grad():
        assert same_bits(torch.ops.orcai.mel_spectrogram_wrt_pcm(pcm1, *ARGS), want)
    x1, x2 = pcm1.clone().requires_grad_(), pcm2.clone().requires_grad_()
    s1 = torch.ops.orcai.mel_spectrogram_wrt_pcm(x1, *ARGS)
    s2 = torch.ops.orcai.mel_spectrogram_wrt_pcm(x2, *ARGS)  # another recording overwrites the front end's workspace before s1's backward
    assert same_bits(s1.detach(), want) and s1.requires_grad
    g = torch.randn(s1.shape, device="cuda", generator=torch.Generator("cuda").manual_seed(1))
    (d1,) = torch.autograd.grad(s1, x1, g)
    spec1, st1 = fe.make_spectrogram(pcm1, SP, return_stats=True)
    assert same_bits(spec1, want)
    assert same_bits(d1, fe.mel_spectrogram_backward(pcm1, g, st1, SP))
    assert torch.isfinite(d1).all() and float(d1.abs().max()) > 0
    (d2,) = torch.autograd.grad(s2.sum(), x2)
    assert same_bits(d2, fe.mel_spectrogram_backward(pcm2, torch.ones_like(s2), fe.make_spectrogram(pcm2, SP, return_stats=True)[1], SP))
    with pytest.raises(RuntimeError):  # orcai::mel_spectrogram itself keeps having no autograd
        torch.ops.orcai.mel_spectrogram(x1, *ARGS).sum().backward()


def test_opcheck_new_ops():
    from torch.library import opcheck

    pcm = torch.from_numpy(R.G.recording("a")[:24000].copy()).cuda()
    opcheck(torch.ops.orcai.mel_spectrogram_wrt_pcm.default, (pcm, *ARGS))
    opcheck(torch.ops.orcai.mel_spectrogram_wrt_pcm.default, (pcm.clone().requires_grad_(), *ARGS))
    opcheck(torch.ops.orcai.mel_spectrogram_with_stats.default, (pcm, *ARGS))
    spec, stats = torch.ops.orcai.mel_spectrogram_with_stats(pcm, *ARGS)
    opcheck(torch.ops.orcai.mel_spectrogram_backward.default, (torch.ones_like(spec), pcm, stats, *ARGS[:8]))


# ------------------------------------------------------------------------------------------------------------------ 5. end to end
def test_waveform_gradient_through_the_detector():
    """pcm at 96 kHz -> waveform_front_end (resample, mel_spectrogram_wrt_pcm) -> snippets -> OrcaiModule(input_grad="eval") of input width n_mels ->
    scalar loss -> backward: pcm.grad is finite, non-zero and, bit for bit, the chain composed by hand -- resample_backward of mel_spectrogram_backward of
    the snippet gradients scattered back onto the spectrogram (the construction of tests/test_frontend_grad_gpu.py's test of the same name)."""
    from orcai_amd.architectures import ResNet1DConv
    from orcai_amd.resample import resample_device
    from orcai_amd.torch_ops import MelWaveformFrontEnd, OrcaiModule, waveform_front_end

    H, W, B = 64, 64, 2
    model = ResNet1DConv((H, W, 1), 4, [12, 20], 3, dropout_rate=0.0, seed=4)
    m = OrcaiModule(model, input_grad="eval").cuda().eval()
    front = waveform_front_end(SP, 96000)
    assert type(front) is MelWaveformFrontEnd
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
    assert torch.isfinite(pcm.grad).all() and float(pcm.grad.abs().max()) > 0
    fe = _fe()
    at_rate = resample_device(pcm0, 96000, 48000)
    spec0, st = fe.make_spectrogram(at_rate, SP, return_stats=True)
    assert same_bits(spec0, spec.detach())
    gspec = torch.zeros_like(spec0)
    gspec[: B * H] = x.grad.view(B * H, W)
    d_rate = fe.mel_spectrogram_backward(at_rate, gspec, st, SP)
    assert same_bits(pcm.grad, torch.ops.orcai.resample_backward(d_rate, pcm0.numel(), 96000, 48000))
