"""The gradient of the PCEN front end, the parts that need no GPU: pcen.pcen_bwd_ref (the float64 specification of orcai_pcen_bwd's map g_y -> dE)
against torch's float64 autograd of the sequential recurrence and against the dot-product identity, the share of near-tie elements in every case the GPU
tests use, and the refusals that stay (their messages now name the new entry points)."""

import inspect

import numpy as np
import pytest

import pcen_grad_ref as R
from orcai_amd import pcen

torch = pytest.importorskip("torch")

# name -> (pcen parameter, sampling rate, hop, smallest energy)
PARAMETERS = {k: R.SCAN_PARAMETERS[k] for k in ("default", "gain0", "power1", "bias0", "a0")}


def _inputs(T, name, K=5):
    p, sr, hop, e_min = PARAMETERS[name][:4]
    cfg = pcen.pcen_config({"nfft": 512, "pcen": p})
    rng = np.random.default_rng(1000 * T + len(name))
    E = 10.0 ** rng.uniform(np.log10(e_min) if e_min > 0 else -9, 0, (T, K))
    if e_min == 0:
        E[rng.uniform(size=(T, K)) < 0.1] = 0.0
    return cfg, sr, hop, E, rng.standard_normal((T, K))


@pytest.mark.parametrize("name", list(PARAMETERS))
@pytest.mark.parametrize("T", [1, 2, 5, 300])
def test_pcen_bwd_ref_is_the_gradient_of_the_recurrence(T, name):
    cfg, sr, hop, E, g_y = _inputs(T, name)
    if name == "a0":
        assert pcen.smoother(cfg["time_constant"], sr, hop) == (0.0, 1.0)
    # u = 0 (bias = 0 and S = 0) never comes with a gradient: y = 0 is always clipped (include/orcai_hip.h)
    assert name != "bias0" or E.min() >= 1e-3
    if cfg["bias"] == 0.0:
        g_y[E == 0] = 0.0
    x = torch.from_numpy(E).requires_grad_()
    y = R.pcen_torch(x, cfg, sr, hop)
    assert np.allclose(y.detach().numpy(), pcen.pcen_ref(E, cfg, sr, hop), rtol=1e-12, atol=1e-12)  # (y is a difference: small values carry the rounding of bias^power)
    (want,) = torch.autograd.grad(y, x, torch.from_numpy(g_y))
    got = pcen.pcen_bwd_ref(E, g_y, cfg, sr, hop)
    assert got.shape == E.shape and got.dtype == np.float64
    assert np.abs(got - want.numpy()).max() <= 1e-10 * np.abs(want.numpy()).max()


@pytest.mark.parametrize("name", list(PARAMETERS))
def test_dot_product_identity(name):
    """<J v, g> = <v, J^T g>: J v is torch's Jacobian-vector product of the float64 forward (E > 0 here, so the forward is smooth along every direction)."""
    cfg, sr, hop, E, g = _inputs(40, name)
    E = np.maximum(E, 1e-3)
    v = np.random.default_rng(3).standard_normal(E.shape)
    x = torch.from_numpy(E).requires_grad_()
    _, jv = torch.autograd.functional.jvp(lambda e: R.pcen_torch(e, cfg, sr, hop), x, torch.from_numpy(v))
    lhs = float((jv.numpy() * g).sum())
    rhs = float((v * pcen.pcen_bwd_ref(E, g, cfg, sr, hop)).sum())
    assert abs(lhs - rhs) <= 1e-10 * max(abs(lhs), abs(rhs))


def test_pcen_bwd_ref_shapes():
    cfg = R.CFG
    assert pcen.pcen_bwd_ref(np.zeros((0, 3)), np.zeros((0, 3)), cfg, 48000, 256).shape == (0, 3)
    one = pcen.pcen_bwd_ref(np.array([0.5, 0.25]), np.array([1.0, 0.0]), cfg, 48000, 256)  # [T]: one channel
    two = pcen.pcen_bwd_ref(np.array([[0.5], [0.25]]), np.array([[1.0], [0.0]]), cfg, 48000, 256)
    assert one.shape == (2,) and np.array_equal(one, two[:, 0])
    with pytest.raises(ValueError, match="shape"):
        pcen.pcen_bwd_ref(np.zeros((2, 3)), np.zeros((3, 2)), cfg, 48000, 256)


def test_a_clipped_frame_still_receives_the_later_frames_gradient():
    """g_y only at the last frame: every earlier frame has d = q = 0 and dE = scale b a^(T-1-t) q[T-1] all the same; frame 0 takes coefficient 1."""
    cfg = R.CFG
    a, b = pcen.smoother(cfg["time_constant"], 48000, 256)
    E = np.full((6, 1), 1e-4)
    g_y = np.zeros((6, 1))
    g_y[5] = 1.0
    dE = pcen.pcen_bwd_ref(E, g_y, cfg, 48000, 256)[:, 0]
    assert (dE[:5] < 0).all()  # a louder past raises M and lowers the last frame's value
    assert np.allclose(dE[2:5] / dE[1:4], 1.0 / a, rtol=1e-12)
    assert np.isclose(dE[0] / dE[1], a / b, rtol=1e-12)


@pytest.mark.parametrize("which", ["a", "b"])
@pytest.mark.parametrize("index", range(len(R.CASES)))
def test_tie_share_of_the_end_to_end_cases(which, index):
    c = R.case(which, index)
    print(f"({which}) {R.label(R.CASES[index])}: tie share {c['tie_share']:.2e}")
    assert c["tie_share"] <= R.TIE_SHARE_MAX
    assert c["stats"][1] > c["stats"][0] >= 0.0 and float(c["dpcm64"].abs().max()) > 0


@pytest.mark.parametrize("name", list(R.SCAN_PARAMETERS))
def test_tie_share_of_the_scan_cases(name):
    for i, (T, K) in enumerate(R.SCAN_SHAPES):
        c = R.scan_case(i, name)
        print(f"{name} T {T} K {K}: tie share {c['tie_share']:.2e}, clipped {c['clipped'][0]:.2f} / {c['clipped'][1]:.2f}")
        assert c["tie_share"] <= R.TIE_SHARE_MAX or T * K < 2000, (T, K)  # below 2000 elements one tie is already more than 5e-4
        assert T * K < 2000 or (0.05 < c["clipped"][0] < 0.2 and 0.05 < c["clipped"][1] < 0.2), (T, K, c["clipped"])


def test_the_pinned_refusals_name_the_new_entry_points():
    """The four refusals tests/test_pcen_gpu.py pins keep raising; what they say now points at the gradient's own names (the methods' by string: raising
    them for real needs the GPU and is what that file does; the forward-only ops' by a backward on fake tensors)."""
    from torch._subclasses.fake_tensor import FakeTensorMode

    from orcai_amd import frontend, torch_ops

    assert "FrontEnd.pcen_spectrogram_backward" in inspect.getsource(frontend.FrontEnd._no_pcen_gradient)
    for method in (frontend.FrontEnd.spectrogram_backward, frontend.FrontEnd.mel_spectrogram_backward):
        assert "_no_pcen_gradient" in inspect.getsource(method)
    route = (48000, 512, 256, 16000.0, 0, 0.0, 0.0, False, True)
    for base, tail in (("pcen_spectrogram", (0.4, 0.98, 2.0, 0.5, 1e-6, 2.0**31)), ("denoised_spectrogram", (0.5,))):  # the two forward-only ops, for real
        with FakeTensorMode():
            x = torch.empty(4113, requires_grad=True)
            y = getattr(torch.ops.orcai, base)(x, *route, *tail, 0.01, 0.999)
            with pytest.raises(NotImplementedError, match=f"orcai::{base}_wrt_pcm"):
                torch.autograd.grad(y.sum(), x)
    sp = {"sampling_rate": 48000, "nfft": 512, "n_overlap": 256, "freq_range": [0, 16000], "quantiles": [0.01, 0.999], "pcen": {}}
    for make in (torch_ops.waveform_front_end, torch_ops.WaveformFrontEnd, torch_ops.MelWaveformFrontEnd):
        with pytest.raises(NotImplementedError, match="PcenWaveformFrontEnd"):
            make(dict(sp, mel={"n_mels": 64}) if make is torch_ops.MelWaveformFrontEnd else sp, 96000)
    front = torch_ops.PcenWaveformFrontEnd(sp, 96000)  # host arithmetic only
    assert front.route[:2] == (16000.0, 0) and front.pcen == tuple(pcen.PCEN_DEFAULTS[k] for k in pcen.PCEN_KEYS)
    assert torch_ops.PcenWaveformFrontEnd(dict(sp, mel={"n_mels": 64}), 96000).route[1] == 64
    with pytest.raises(ValueError, match="pcen is absent"):
        torch_ops.PcenWaveformFrontEnd({k: v for k, v in sp.items() if k != "pcen"}, 96000)


def test_fake_implementations_give_the_shapes():
    from torch._subclasses.fake_tensor import FakeTensorMode

    import orcai_amd.torch_ops  # noqa: F401  (registers the ops)

    lin = (48000, 512, 256, 16000.0, 0, 0.0, 0.0, False, True, 0.4, 0.98, 2.0, 0.5, 1e-6, 2.0**31, 0.01, 0.999)
    with FakeTensorMode():
        pcm = torch.empty(20000)
        spec = torch.ops.orcai.pcen_spectrogram_wrt_pcm(pcm, *lin)
        spec2, stats = torch.ops.orcai.pcen_spectrogram_with_stats(pcm, *lin)
        d = torch.ops.orcai.pcen_spectrogram_backward(spec, pcm, stats, *lin[:-2])
    assert tuple(spec.shape) == tuple(spec2.shape) == (79, 171) and tuple(stats.shape) == (6,) and tuple(d.shape) == (20000,)
