"""The gradient of the denoised front end w.r.t. the audio, everything that needs no GPU: the float64 restatement of tests/denoise_grad_ref.py against
denoise.denoise_ref and the oracle's clip, the tie share of every case the GPU file uses, autograd of the restatement against the written formula of
include/orcai_hip.h, FrontEnd.denoised_spectrogram_backward's refusals, the ops' schemas and fake implementations, and the new C symbols."""

import inspect

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import denoise_grad_ref as R  # noqa: E402
from oracle import frontend_ref as FR  # noqa: E402
from orcai_amd import denoise, frontend  # noqa: E402

LIN = {"sampling_rate": 48000, "nfft": 512, "n_overlap": 256, "freq_range": [0, 16000], "quantiles": [0.01, 0.999]}
MEL = dict(LIN, mel={"n_mels": 64, "fmin": 0.0, "fmax": 24000.0, "htk": False, "norm": "slaney"})
LIN_ARGS = (48000, 512, 256, 16000.0, 0, 0.0, 0.0, False, True, 0.5, 0.01, 0.999)
MEL_ARGS = (48000, 512, 256, 0.0, 64, 0.0, 24000.0, False, True, 0.25, 0.01, 0.999)


def _frontend_without_gpu():
    fe = frontend.FrontEnd.__new__(frontend.FrontEnd)  # host arithmetic only: neither the library nor a device
    fe._mel_tables = {}
    return fe


# ---------------------------------------------------------------------------------------------------------------- 1. the restatement
@pytest.mark.parametrize("T, K, quantile, quantiles", [(37, 5, 0.5, (0.01, 0.999)), (64, 3, 0.25, (0.1, 0.9)), (1, 4, 0.5, (0.0, 1.0)), (200, 17, 1.0, (0.05, 0.95))])
def test_restatement_is_denoise_ref_and_the_oracles_clip(T, K, quantile, quantiles):
    """denoise_clip on f32-valued data in float64 against the numpy specification: m and Y of denoise.denoise_ref, then the clip and normalisation
    oracle.frontend_ref.preprocess_spectrogram_ref applies (np.percentile(method="nearest") of the flat values, clip, min-max)."""
    rng = np.random.default_rng(T * 100 + K)
    V = np.maximum(rng.normal(-40.0, 15.0, (T, K)), -80.0).astype(np.float32)
    Y, m = denoise.denoise_ref(V, quantile)
    out, y, m64, p_lo, p_hi = R.denoise_clip(torch.from_numpy(V).double(), quantile, quantiles)
    assert np.array_equal(m64.numpy().astype(np.float32), m)
    assert np.array_equal(y.numpy().astype(np.float32), Y)  # the float64 difference of two f32 values, rounded once: the f32 subtraction
    lo, hi = (np.sort(Y.reshape(-1))[FR.nearest_rank_index(Y.size, q)] for q in quantiles)
    assert lo == np.float32(float(p_lo)) and hi == np.float32(float(p_hi))
    if hi > lo:
        want = (np.clip(Y, lo, hi) - lo) / (hi - lo)  # the oracle's clip and min-max on the f32 values
        # Y and the bounds are the float64 ones rounded to f32: half an ulp of 160 dB (7.6e-6) each, three of them, over a range of more than 10 dB
        assert hi - lo > 10.0 and np.allclose(out.numpy(), want, rtol=0, atol=3e-6)
    a = np.percentile(Y, [100 * quantiles[0], 100 * quantiles[1]], method="nearest")
    assert (a[0], a[1]) == (lo, hi)  # what the oracle's preprocess step picks for the same data


# ---------------------------------------------------------------------------------------------------------------- 2. the condition of the GPU cases
@pytest.mark.parametrize("name", list(R.CASES))
def test_tie_share_of_every_gpu_case(name):
    """The GPU bar compares gradients with the near-tie elements' g zeroed; that is a statement about the kernel only while such elements are rare.
    Recording (b) keeps frontend_grad_ref's q_lo = 0.10 (see R.QUANTILES); with it no case needs another denoise quantile."""
    c = R.case(name)
    print(f"{name}: tie share {c['tie_share']:.2e}, floored {c['floored_share']:.2e}, p_lo {c['stats'][1]:.3f}, p_hi {c['stats'][2]:.3f}")
    assert c["tie_share"] <= R.TIE_SHARE_MAX, name
    assert c["stats"][2] > c["stats"][1] and float(c["dpcm64"].abs().max()) > 0
    if R.CASES[name][1] == "b":
        assert c["floored_share"] > 0.03  # the dB floor and the X <= 1e-10 gate are exercised
    m = c["stats"][3]
    assert m.shape == (R.channels(c["route"]),) and float(m.max()) <= 0.0 and float(m.min()) >= -80.0 and float(m.max() - m.min()) > 1.0  # a real profile


# ---------------------------------------------------------------------------------------------------------------- 3. autograd == the written formula
@pytest.mark.parametrize("name", ["512-256-a", "32-16-b", "128-32-8-b", "512-256-64-b-q25"])
def test_autograd_of_the_restatement_is_the_closed_formula(name):
    c = R.case(name)
    d = R.dpcm_by_formula(c)
    scale = float(c["dpcm64"].abs().max())
    assert float((d - c["dpcm64"]).abs().max()) <= 1e-12 * scale
    g_db = R.g_db_by_formula(c)
    assert 0.5 < float((g_db != 0).double().mean()) < 1.0  # most gates open, some closed
    # the floor is IN the gate: the plain gate (v against the same bounds) would decide otherwise on a good share of the elements
    ref_db, p_lo, p_hi, m = c["stats"]
    v = c["aux"]["v"]
    assert float((((v > p_lo) & (v < p_hi)) != ((v - m > p_lo) & (v - m < p_hi))).double().mean()) > 0.05


def test_the_floor_is_a_constant_of_the_backward():
    """With everything but one column's g zero, raising that column's floor until y < p_lo closes every gate: the float64 gradient is exactly zero,
    and the other columns' floors do not enter."""
    c = R.case("512-256-a")
    k = 40
    g = torch.zeros_like(c["g"])
    g[:, k] = 1.0
    m = c["stats"][3]
    assert float(R.dpcm_in(torch.float64, c, g=g).abs().max()) > 0
    up = m.clone()
    up[k] += 200.0
    assert not R.dpcm_in(torch.float64, c, g=g, profile=up).any()
    other = m.clone()
    other[k + 1] += 200.0
    assert torch.equal(R.dpcm_in(torch.float64, c, g=g, profile=other), R.dpcm_in(torch.float64, c, g=g))


# ---------------------------------------------------------------------------------------------------------------- 4. the Python entry's refusals
def test_denoised_spectrogram_backward_refusals():
    """Reached without a GPU: the parameter is judged before any tensor is looked at.  (The shape refusals need CUDA tensors -- a CPU pcm is the first
    thing refused -- and are in tests/test_denoise_grad_gpu.py.)"""
    fe = _frontend_without_gpu()
    x = torch.zeros(4000)
    for sp in (LIN, MEL, dict(LIN, denoise=None)):
        with pytest.raises(ValueError, match="denoise is absent.*spectrogram_backward.*mel_spectrogram_backward"):
            fe.denoised_spectrogram_backward(x, x, x, x, sp)
    with pytest.raises(ValueError, match="denoise and pcen"):
        fe.denoised_spectrogram_backward(x, x, x, x, dict(LIN, denoise={}, pcen={}))
    with pytest.raises(NotImplementedError, match="nfft = 500.*gradient"):
        fe.denoised_spectrogram_backward(x, x, x, x, dict(LIN, denoise={}, nfft=500, n_overlap=250))
    with pytest.raises(NotImplementedError, match="nfft"):  # the mel route's own sizes (mel.mel_config)
        fe.denoised_spectrogram_backward(x, x, x, x, dict(MEL, denoise={}, nfft=64))
    with pytest.raises(ValueError, match="quantile"):
        fe.denoised_spectrogram_backward(x, x, x, x, dict(LIN, denoise={"quantile": 2}))
    with pytest.raises(ValueError, match="hop"):
        fe.denoised_spectrogram_backward(x, x, x, x, dict(LIN, denoise={}, n_overlap=0))
    with pytest.raises(TypeError, match="CUDA"):
        fe.denoised_spectrogram_backward(x, x, x, x, dict(LIN, denoise={}))
    assert "self._backward(" in inspect.getsource(frontend.FrontEnd.denoised_spectrogram_backward)
    src = inspect.getsource(frontend.FrontEnd._backward)  # the body it shares with FrontEnd.backward holds the tensors' refusals
    for what in ("grad must be a float32 CUDA tensor", "stats must be the float32 CUDA tensor [6]", "profile must be the float32 CUDA tensor"):
        assert what in src


def test_the_plain_entries_keep_refusing_and_name_the_new_ones():
    from orcai_amd import torch_ops

    fe = _frontend_without_gpu()
    x = torch.zeros(4000)
    sp = dict(LIN, denoise={})
    for call in (fe.backward, fe.spectrogram_backward, fe.mel_spectrogram_backward, fe.pcen_spectrogram_backward):
        with pytest.raises(NotImplementedError, match="FrontEnd.denoised_spectrogram_backward.*DenoisedWaveformFrontEnd"):
            call(x, x, x, sp)
    for make in (torch_ops.waveform_front_end, torch_ops.WaveformFrontEnd, torch_ops.MelWaveformFrontEnd, torch_ops.PcenWaveformFrontEnd):
        with pytest.raises(NotImplementedError, match="DenoisedWaveformFrontEnd"):
            make(sp, 96000)
    front = torch_ops.DenoisedWaveformFrontEnd(sp, 96000)  # host arithmetic only
    assert front.route[:2] == (16000.0, 0) and front.quantile == 0.5 and "denoise.quantile=0.5" in front.extra_repr()
    front = torch_ops.DenoisedWaveformFrontEnd(dict(MEL, denoise={"quantile": 0.25}), 96000)
    assert front.route[1] == 64 and front._args == (0.0, 64, 0.0, 24000.0, False, True, 0.25)
    with pytest.raises(ValueError, match="denoise is absent"):
        torch_ops.DenoisedWaveformFrontEnd(LIN, 96000)
    with pytest.raises(ValueError, match="denoise and pcen"):
        torch_ops.DenoisedWaveformFrontEnd(dict(sp, pcen={}), 96000)
    with pytest.raises(NotImplementedError, match="nfft = 500"):
        torch_ops.DenoisedWaveformFrontEnd(dict(sp, nfft=500), 96000)


# ---------------------------------------------------------------------------------------------------------------- 5. the ops
def test_op_schemas():
    import orcai_amd.torch_ops  # noqa: F401  (registers the ops)

    arguments = ("SymInt sampling_rate, SymInt nfft, SymInt hop, float freq_hi, SymInt n_mels, float fmin, float fmax, bool htk, bool slaney_norm, "
                 "float quantile")
    for name in ("denoised_spectrogram", "denoised_spectrogram_wrt_pcm"):
        assert str(getattr(torch.ops.orcai, name).default._schema) == f"orcai::{name}(Tensor pcm, {arguments}, float q_lo, float q_hi) -> Tensor"
    assert (str(torch.ops.orcai.denoised_spectrogram_with_stats.default._schema)
            == f"orcai::denoised_spectrogram_with_stats(Tensor pcm, {arguments}, float q_lo, float q_hi) -> (Tensor, Tensor, Tensor)")
    assert (str(torch.ops.orcai.denoised_spectrogram_backward.default._schema)
            == f"orcai::denoised_spectrogram_backward(Tensor grad, Tensor pcm, Tensor stats, Tensor profile, {arguments}) -> Tensor")
    for name in ("denoised_spectrogram", "denoised_spectrogram_wrt_pcm", "denoised_spectrogram_with_stats", "denoised_spectrogram_backward"):
        assert not getattr(torch.ops.orcai, name).default._schema.is_mutable


def test_fake_implementations_give_the_shapes():
    from torch._subclasses.fake_tensor import FakeTensorMode

    import orcai_amd.torch_ops  # noqa: F401

    with FakeTensorMode():
        pcm = torch.empty(20000)
        for args, K in ((LIN_ARGS, 171), (MEL_ARGS, 64)):
            spec0 = torch.ops.orcai.denoised_spectrogram(pcm, *args)
            spec = torch.ops.orcai.denoised_spectrogram_wrt_pcm(pcm, *args)
            spec2, stats, profile = torch.ops.orcai.denoised_spectrogram_with_stats(pcm, *args)
            d = torch.ops.orcai.denoised_spectrogram_backward(spec, pcm, stats, profile, *args[:-2])
            assert tuple(spec0.shape) == tuple(spec.shape) == tuple(spec2.shape) == (79, K)
            assert tuple(stats.shape) == (6,) and tuple(profile.shape) == (K,) and tuple(d.shape) == (20000,)
            assert d.dtype == spec.dtype == torch.float32


def test_the_parameter_the_ops_build_is_the_modules():
    from orcai_amd import torch_ops

    assert torch_ops._denoised_parameter(*LIN_ARGS) == dict(LIN, freq_range=[0, 16000.0], denoise={"quantile": 0.5})
    assert torch_ops._denoised_parameter(*MEL_ARGS) == dict(MEL, freq_range=[0.0, 24000.0], denoise={"quantile": 0.25})
    assert denoise.denoise_config(torch_ops._denoised_parameter(*MEL_ARGS)) == {"quantile": 0.25}
    with pytest.raises(NotImplementedError, match="nfft = 500"):  # refused before the forward runs, as spectrogram_wrt_pcm does
        torch_ops._denoised_gradient_sizes(48000, 500, 250, 16000.0, 0, 0.0, 0.0, False, True, 0.5, 0.01, 0.999)


# ---------------------------------------------------------------------------------------------------------------- 6. the C ABI
def test_the_new_symbols_are_declared_listed_and_exported():
    from pathlib import Path

    from orcai_amd import _native as N

    header = (Path(__file__).resolve().parent.parent / "include" / "orcai_hip.h").read_text()
    for name in ("orcai_denoised_spectrogram_bwd", "orcai_denoised_spectrogram_bwd_occupancy"):
        assert f"int {name}(" in header and name in N._SIGNATURES and name in N.exported_symbols()
        assert getattr(N.lib(), name) is not None
    assert len(N._SIGNATURES["orcai_denoised_spectrogram_bwd"][1]) == 17
    assert "Forward only: no gradient exists" not in header and "HELD CONSTANT" in header.split("orcai_make_denoised_spectrogram(")[1]
