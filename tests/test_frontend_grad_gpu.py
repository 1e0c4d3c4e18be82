"""The gradient of the spectrogram front end w.r.t. the audio on the GPU: orcai_spectrogram_bwd against the float64 reference of
tests/frontend_grad_ref.py, the launcher's contract, the torch ops (spectrogram_wrt_pcm and the two functional ops underneath) and the chain
pcm -> spectrogram -> snippets -> OrcaiModule(input_grad=True) -> loss differentiated down to the waveform."""

import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import frontend_grad_ref as R  # noqa: E402
import orcai_amd.torch_ops  # noqa: E402, F401  (registers the ops)

# Measured on the CPU for exactly these inputs (tests/frontend_grad_ref.py run as a script prints this table): the reference's formula evaluated
# by torch in float32 -- from the same pcm, g and statistics the kernel gets -- deviates from its float64 evaluation by this share of max|dpcm|.
# The error is dominated by the 1 / P factor of bins whose power is small by cancellation, not by the transform.  The bar for the kernel is 8 x
# the value of its case (the margin tests/test_input_grad_gpu.py uses for another summation order in f32).
F32_REFERENCE_DEVIATION = {
    ("a", 512, 256): 4.07e-06,
    ("a", 256, 64): 3.37e-06,
    ("a", 1024, 512): 2.26e-06,
    ("a", 2048, 300): 2.62e-06,
    ("a", 32, 16): 4.22e-06,
    ("b", 512, 256): 3.35e-06,
    ("b", 256, 64): 2.77e-06,
    ("b", 1024, 512): 3.53e-06,
    ("b", 2048, 300): 2.59e-06,
    ("b", 32, 16): 2.74e-06,
}
ARGS = (48000, 512, 256, 16000.0, 0.01, 0.999)
SP = {"sampling_rate": 48000, "nfft": 512, "n_overlap": 256, "freq_range": [0, 16000.0], "quantiles": [0.01, 0.999]}


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(torch.int32), b.view(torch.int32))


def _fe():
    from orcai_amd.frontend import get_frontend

    return get_frontend()


def _bwd(pcm, n_fft, hop, n_frames, k_crop, g, stats, dpcm, n_samples=None, top_db=80.0):
    """The C entry point itself (return code, no exception)."""
    from orcai_amd import _native as N

    p = lambda t: 0 if t is None else N.ptr(t)  # noqa: E731
    n = pcm.numel() if n_samples is None else n_samples
    return N.lib().orcai_spectrogram_bwd(p(pcm), n, n_fft, hop, n_frames, k_crop, p(g), p(stats), top_db, p(dpcm), N.stream_ptr())


# ------------------------------------------------------------------------------------------------------------------ 1. the kernel against the definition
@pytest.mark.parametrize("which", ["a", "b"])
@pytest.mark.parametrize("nfft,hop", R.SIZES)
def test_kernel_against_the_float64_reference(which, nfft, hop):
    c = R.case(which, nfft, hop)
    pcm, g = c["pcm"].cuda(), c["g"].cuda()
    dpcm = _fe().spectrogram_backward(pcm, g, R.stats_tensor(c, "cuda"), R.parameter(nfft, hop, which))
    ref = c["dpcm64"]
    share = float((dpcm.cpu().double() - ref).abs().max() / ref.abs().max())
    dev = F32_REFERENCE_DEVIATION[(which, nfft, hop)]
    print(f"({which}) nfft {nfft} hop {hop}: kernel error {share:.2e} of max|dpcm|; torch f32 {dev:.2e}; bar {8 * dev:.2e}")
    assert torch.isfinite(dpcm).all()
    assert share <= 8 * dev, (share, dev)


# ------------------------------------------------------------------------------------------------------------------ 2. the launcher
def test_two_launches_give_identical_bits_and_every_element_is_written():
    c = R.case("b", 512, 256)  # (its statistics are realistic for the other sizes too: most gates are open)
    for nfft, hop in ((512, 256), (2048, 300), (4096, 1000)):  # wave per run; workgroup per run; the largest size, 64 KiB of LDS
        pcm = c["pcm"].cuda()
        k = R.k_crop_of(nfft)
        T = 1 + pcm.numel() // hop
        g = torch.randn((T, k), device="cuda", generator=torch.Generator("cuda").manual_seed(3))
        stats = R.stats_tensor(c, "cuda")
        outs = []
        for _ in range(2):
            dpcm = torch.full((pcm.numel(),), float("nan"), device="cuda")
            assert _bwd(pcm, nfft, hop, T, k, g, stats, dpcm) == 0
            outs.append(dpcm)
        assert torch.isfinite(outs[0]).all() and float(outs[0].abs().max()) > 0, (nfft, hop)
        assert same_bits(outs[0], outs[1]), (nfft, hop)


def test_a_recording_shorter_than_one_window():
    """100 samples, one frame of 512 (all but 100 of its samples are padding).  The bar is 8 x the float32 deviation of this very case."""
    nfft, hop, k = 512, 256, 171
    pcm = torch.from_numpy(R.recording("a")[:100].copy())
    x = pcm.double().requires_grad_()
    out, aux = R.forward(x, nfft, hop, k, (0.01, 0.999))
    g = torch.randn(out.shape, generator=torch.Generator().manual_seed(9))
    g[R.tie_mask(aux)] = 0.0
    (ref,) = torch.autograd.grad(out, x, g.double())
    stats = (aux["ref_db"], aux["p_lo"], aux["p_hi"])
    x32 = pcm.clone().requires_grad_()
    (d32,) = torch.autograd.grad(R.forward(x32, nfft, hop, k, None, stats=stats)[0], x32, g)
    dev = float((d32.double() - ref).abs().max() / ref.abs().max())
    dpcm = _fe().spectrogram_backward(pcm.cuda(), g.cuda(), R.stats_tensor({"stats": stats}, "cuda"), SP)
    share = float((dpcm.cpu().double() - ref).abs().max() / ref.abs().max())
    print(f"100 samples: kernel error {share:.2e} of max|dpcm|; torch f32 {dev:.2e}")
    assert out.shape == (1, k) and dpcm.shape == (100,) and share <= 8 * dev, (share, dev)


def test_argument_errors_and_unsupported_sizes():
    from orcai_amd import _native as N

    pcm = torch.from_numpy(R.recording("a")[:4000].copy()).cuda()
    n = pcm.numel()
    g = torch.zeros((1 + n // 256, 171), device="cuda")
    stats = torch.tensor([1.0, 0.0, -60.0, -5.0, -60.0, -5.0], device="cuda")
    dpcm = torch.zeros(n, device="cuda")
    T = 1 + n // 256
    assert _bwd(pcm, 512, 256, T, 171, g, stats, dpcm) == 0
    for missing in ("pcm", "g", "stats", "dpcm"):  # null pointers
        a = dict(pcm=pcm, g=g, stats=stats, dpcm=dpcm)
        a[missing] = None
        assert _bwd(a["pcm"], 512, 256, T, 171, a["g"], a["stats"], a["dpcm"], n_samples=n) == N.E_BADARG, missing
    assert _bwd(pcm, 512, 256, T, 171, g, stats, dpcm, n_samples=0) == N.E_BADARG
    assert _bwd(pcm, 512, 0, T, 171, g, stats, dpcm) == N.E_BADARG
    assert _bwd(pcm, 512, 256, T + 1, 171, g, stats, dpcm) == N.E_BADARG  # not librosa's frame count
    assert _bwd(pcm, 512, 256, T, 0, g, stats, dpcm) == N.E_BADARG
    assert _bwd(pcm, 512, 256, T, 258, g, stats, dpcm) == N.E_BADARG  # more bins than 1 + n_fft / 2
    for nfft in (500, 16, 8192, 48):
        assert _bwd(pcm, nfft, 250, 1 + n // 250, 8, g, stats, dpcm) == N.E_UNSUPPORTED, nfft
    fe = _fe()
    sp500 = dict(SP, nfft=500, n_overlap=250)
    spec, st = fe.make_spectrogram(pcm, sp500, return_stats=True)  # the forward still runs the size the backward refuses
    assert spec.shape[0] == 1 + n // 250 and torch.isfinite(spec).all()
    with pytest.raises(NotImplementedError, match="nfft = 500"):
        fe.spectrogram_backward(pcm, torch.zeros_like(spec), st, sp500)
    with pytest.raises(ValueError, match="nfft = 512"):
        fe.spectrogram_backward(pcm, g[:-1], stats, SP)


def test_stats_on_the_device_are_the_hosts():
    fe = _fe()
    pcm = torch.from_numpy(R.recording("b")[:48000].copy()).cuda()
    spec, st = fe.make_spectrogram(pcm, SP, return_stats=True)
    host = fe.stats()
    assert [float(v) for v in st.cpu()] == [host[k] for k in ("pmax", "ref_db", "p_lo", "p_hi", "sel_lo_raw", "sel_hi_raw")]
    assert same_bits(spec, fe.make_spectrogram(pcm, SP))


# ------------------------------------------------------------------------------------------------------------------ 3. the op
def test_op_forward_bits_gradient_bits_and_stats_survive_another_recording():
    fe = _fe()
    pcm1 = torch.from_numpy(R.recording("a")[:48000 + 17].copy()).cuda()
    pcm2 = torch.from_numpy(R.recording("b")[40000:100000].copy()).cuda()
    want = torch.ops.orcai.spectrogram(pcm1, *ARGS)
    with torch.no_grad():
        assert same_bits(torch.ops.orcai.spectrogram_wrt_pcm(pcm1, *ARGS), want)
    x1, x2 = pcm1.clone().requires_grad_(), pcm2.clone().requires_grad_()
    s1 = torch.ops.orcai.spectrogram_wrt_pcm(x1, *ARGS)
    s2 = torch.ops.orcai.spectrogram_wrt_pcm(x2, *ARGS)  # another recording overwrites the front end's workspace before s1's backward
    assert same_bits(s1.detach(), want) and s1.requires_grad
    g = torch.randn(s1.shape, device="cuda", generator=torch.Generator("cuda").manual_seed(1))
    (d1,) = torch.autograd.grad(s1, x1, g)
    spec1, st1 = fe.make_spectrogram(pcm1, SP, return_stats=True)
    assert same_bits(spec1, want)
    assert same_bits(d1, fe.spectrogram_backward(pcm1, g, st1, SP))
    assert torch.isfinite(d1).all() and float(d1.abs().max()) > 0
    (d2,) = torch.autograd.grad(s2.sum(), x2)
    assert same_bits(d2, fe.spectrogram_backward(pcm2, torch.ones_like(s2), fe.make_spectrogram(pcm2, SP, return_stats=True)[1], SP))


def test_opcheck_new_ops():
    from torch.library import opcheck

    pcm = torch.from_numpy(R.recording("a")[:24000].copy()).cuda()
    opcheck(torch.ops.orcai.spectrogram_wrt_pcm.default, (pcm, *ARGS))
    opcheck(torch.ops.orcai.spectrogram_wrt_pcm.default, (pcm.clone().requires_grad_(), *ARGS))
    opcheck(torch.ops.orcai.spectrogram_with_stats.default, (pcm, *ARGS))
    spec, stats = torch.ops.orcai.spectrogram_with_stats(pcm, *ARGS)
    opcheck(torch.ops.orcai.spectrogram_backward.default, (torch.ones_like(spec), pcm, stats, *ARGS[:4]))


# ------------------------------------------------------------------------------------------------------------------ 4. end to end
def test_waveform_gradient_through_the_detector():
    """pcm -> spectrogram_wrt_pcm -> snippets -> OrcaiModule(input_grad=True).train() -> scalar loss -> backward: pcm.grad is finite, non-zero
    and equals spectrogram_backward of the snippet gradients scattered back onto the spectrogram; the same chain through torch.compile
    (aot_eager, the ops called with the seed the module draws first) gives the same bits.  ResNet1DConv: its backward is bit-reproducible."""
    from orcai_amd.architectures import ResNet1DConv
    from orcai_amd.torch_ops import OrcaiModule

    H, W, B = 64, 171, 2
    model = ResNet1DConv((H, W, 1), 4, [12, 20], 3, dropout_rate=0.0, seed=4)
    pcm0 = torch.from_numpy(R.recording("a")[:48000].copy()).cuda()

    m = OrcaiModule(model, seed=2, input_grad=True).cuda().train()
    for p in m.parameters():
        p.requires_grad_(False)
    pcm = pcm0.clone().requires_grad_()
    spec = torch.ops.orcai.spectrogram_wrt_pcm(pcm, *ARGS)
    x = spec[: B * H].view(B, H, W)
    x.retain_grad()
    loss = (m(x) ** 2).sum()
    loss.backward()
    assert torch.isfinite(pcm.grad).all() and float(pcm.grad.abs().max()) > 0
    fe = _fe()
    gspec = torch.zeros_like(spec)
    gspec[: B * H] = x.grad.view(B * H, W)
    assert same_bits(pcm.grad, fe.spectrogram_backward(pcm0, gspec, fe.make_spectrogram(pcm0, SP, return_stats=True)[1], SP))

    m2 = OrcaiModule(model, seed=2, input_grad=True).cuda().train()
    ws, cfg = [w.detach() for w in m2.weights_list()], m2.config

    def f(p, st):
        s = torch.ops.orcai.spectrogram_wrt_pcm(p, *ARGS)
        y = torch.ops.orcai.forward_wrt_input(s[: B * H].view(B, H, W), ws, st, cfg, True, 2 * 1000003)
        return (y**2).sum()

    pc = pcm0.clone().requires_grad_()
    loss_c = torch.compile(f, backend="aot_eager")(pc, m2.stats_list())
    loss_c.backward()
    assert same_bits(loss_c.detach(), loss.detach())
    assert same_bits(pc.grad, pcm.grad)
