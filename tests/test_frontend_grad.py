"""The gradient of the spectrogram front end w.r.t. the audio, without a GPU: the float64 torch reference (tests/frontend_grad_ref.py) pinned
to oracle.frontend_ref and to the written definition, the cap on elements whose gate is decided within rounding, the new ops' schemas and
fake shapes, a torch.compile trace of forward and backward on fake tensors, and the new C symbols."""

import math
import re
from pathlib import Path

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import frontend_grad_ref as R  # noqa: E402
from oracle import frontend_ref as FR  # noqa: E402
from orcai_amd import _native as N  # noqa: E402
from orcai_amd import torch_ops as O  # noqa: E402, F401  (registers the ops)

ROOT = Path(__file__).resolve().parent.parent
ARGS = (48000, 512, 256, 16000.0, 0.01, 0.999)


# ---------------------------------------------------------------------------------------------------------------- the reference
@pytest.mark.parametrize("which", ["a", "b"])
@pytest.mark.parametrize("nfft,hop", [(512, 256), (2048, 300)])
def test_reference_forward_is_the_oracles(which, nfft, hop):
    """The float64 restatement against oracle.frontend_ref on the test recordings.  The STFT is compared where the oracle still holds float64
    values: it rounds numpy's float64 rfft to complex64, so the restatement must lie within that one rounding (2^-24 relative per component)
    of it.  The normalised output is float32 arithmetic in the oracle (three roundings of dB values below 128, ulp 7.6e-6 dB, over a clip range
    of more than 10 dB, in the value and in both bounds: < 1e-5), so 1e-5 absolute on values in [0, 1]."""
    y = R.recording(which)
    re_, im_, _ = R.stft_power(torch.from_numpy(y.copy()).double(), nfft, hop)
    S = FR.stft_ref(y, nfft, hop).T.astype(np.complex128)
    mine = re_.numpy() + 1j * im_.numpy()
    assert mine.shape == S.shape
    bound = 2.0**-24 * 1.001 * (np.abs(S.real) + np.abs(S.imag)) + 1e-12
    assert (np.abs(mine - S) <= bound).all(), float(np.abs(mine - S).max())
    c = R.case(which, nfft, hop)
    sp = R.parameter(nfft, hop, which)
    want = FR.make_spectrogram_ref(y, {"spectrogram": sp})[0]
    assert want.shape == tuple(c["out64"].shape) == (1 + len(y) // hop, c["k_crop"])
    err = float(np.abs(c["out64"].numpy() - want.astype(np.float64)).max())
    print(f"{which} {nfft}/{hop}: max |out64 - oracle| = {err:.2e}")
    assert err <= 1e-5


def test_reference_gradient_is_the_written_definition():
    """autograd through the restated forward (statistics detached) against the four formulas of include/orcai_hip.h evaluated literally in
    float64, on a short recording with a hop that does not divide the transform size."""
    nfft, hop, k = 32, 12, 11
    pcm = torch.from_numpy(R.recording("b")[47600:48100].copy()).double()  # runs into the digital silence
    x = pcm.clone().requires_grad_()
    out, aux = R.forward(x, nfft, hop, k, (0.3, 0.9))
    gen = torch.Generator().manual_seed(5)
    g = torch.randn(out.shape, generator=gen, dtype=torch.float64)
    g[R.tie_mask(aux)] = 0.0
    (auto,) = torch.autograd.grad(out, x, g)
    re_, im_, P = (t.detach()[:, :k] for t in R.stft_power(pcm, nfft, hop))
    db = 10.0 * torch.log10(torch.clamp(P, min=1e-10))
    v = torch.clamp(db - aux["ref_db"], min=-R.TOP_DB)
    open_ = (P > 1e-10) & (db - aux["ref_db"] > -R.TOP_DB) & (v > aux["p_lo"]) & (v < aux["p_hi"])
    assert 0.2 < float(open_.double().mean()) < 0.95 and bool((P <= 1e-10).any())  # every kind of gate occurs
    g_db = torch.where(open_, g / (aux["p_hi"] - aux["p_lo"]), torch.zeros_like(g))
    dP = g_db * 10.0 / (math.log(10.0) * torch.where(open_, P, torch.ones_like(P)))
    dRe, dIm = 2.0 * re_ * dP, 2.0 * im_ * dP
    n = torch.arange(nfft, dtype=torch.float64)
    ang = 2.0 * math.pi * torch.arange(k, dtype=torch.float64)[:, None] * n[None, :] / nfft
    w = 0.5 - 0.5 * torch.cos(2.0 * math.pi * n / nfft)
    dframe = w * (dRe @ torch.cos(ang) - dIm @ torch.sin(ang))
    want = torch.zeros(pcm.numel() + nfft, dtype=torch.float64)
    for t in range(dframe.shape[0]):
        want[t * hop : t * hop + nfft] += dframe[t]
    want = want[nfft // 2 : nfft // 2 + pcm.numel()]
    assert float((auto - want).abs().max()) <= 1e-11 * float(want.abs().max())


@pytest.mark.parametrize("which", ["a", "b"])
def test_share_of_elements_decided_within_rounding_is_capped(which):
    for nfft, hop in R.SIZES:
        c = R.case(which, nfft, hop)
        assert c["tie_share"] <= R.TIE_SHARE_MAX, (which, nfft, hop, c["tie_share"])
        assert float((c["g"] == 0).double().mean()) == c["tie_share"]  # nothing else was zeroed
        assert torch.isfinite(c["dpcm64"]).all() and float(c["dpcm64"].abs().max()) > 0
    b = R.case("b", 512, 256)["aux"]
    if which == "b":  # the input does exercise the P <= 1e-10 gate and the -80 dB floor, and p_lo is above the floor
        assert bool((b["P"] <= 1e-10).any()) and bool(((b["P"] > 1e-10) & (b["db"] - b["ref_db"] < -R.TOP_DB)).any()) and b["p_lo"] > -R.TOP_DB + 1.0


# ---------------------------------------------------------------------------------------------------------------- ops and ABI
def test_new_ops_are_registered_and_spectrogram_is_unchanged():
    ops = torch.ops.orcai
    assert str(ops.spectrogram.default._schema) == (
        "orcai::spectrogram(Tensor pcm, SymInt sampling_rate, SymInt nfft, SymInt hop, float freq_hi, float q_lo, float q_hi) -> Tensor")
    assert str(ops.spectrogram_wrt_pcm.default._schema) == (
        "orcai::spectrogram_wrt_pcm(Tensor pcm, SymInt sampling_rate, SymInt nfft, SymInt hop, float freq_hi, float q_lo, float q_hi) -> Tensor")
    assert str(ops.spectrogram_with_stats.default._schema) == (
        "orcai::spectrogram_with_stats(Tensor pcm, SymInt sampling_rate, SymInt nfft, SymInt hop, float freq_hi, float q_lo, float q_hi) -> (Tensor, Tensor)")
    assert str(ops.spectrogram_backward.default._schema) == (
        "orcai::spectrogram_backward(Tensor grad, Tensor pcm, Tensor stats, SymInt sampling_rate, SymInt nfft, SymInt hop, float freq_hi) -> Tensor")


@pytest.mark.parametrize("n,nfft,hop,sr,fhi,K", [(48000 * 3 + 17, 512, 256, 48000, 16000, 171), (1001, 256, 100, 22050, 5000, 59), (5, 512, 256, 48000, 16000, 171),
                                                (333, 2048, 300, 48000, 16000, 683)])
def test_fake_shapes(n, nfft, hop, sr, fhi, K):
    """Meta shapes of the three ops, with recordings shorter than one window (n < nfft) and odd lengths."""
    pcm = torch.empty(n, device="meta")
    T = 1 + n // hop
    y = torch.ops.orcai.spectrogram_wrt_pcm(pcm, sr, nfft, hop, fhi, 0.01, 0.999)
    assert y.shape == (T, K) and y.dtype == torch.float32 and y.device.type == "meta"
    assert y.shape == torch.ops.orcai.spectrogram(pcm, sr, nfft, hop, fhi, 0.01, 0.999).shape
    spec, stats = torch.ops.orcai.spectrogram_with_stats(pcm, sr, nfft, hop, fhi, 0.01, 0.999)
    assert spec.shape == (T, K) and stats.shape == (6,) and stats.dtype == torch.float32
    d = torch.ops.orcai.spectrogram_backward(torch.empty((T, K), device="meta"), pcm, stats, sr, nfft, hop, fhi)
    assert d.shape == (n,) and d.dtype == torch.float32 and d.device.type == "meta"


def test_unsupported_transform_sizes_are_named():
    from orcai_amd.frontend import FrontEnd

    for nfft in (32, 64, 512, 4096):
        FrontEnd._check_nfft_backward(nfft)
    for nfft in (500, 16, 255, 8192):
        with pytest.raises(NotImplementedError, match=f"nfft = {nfft}"):
            FrontEnd._check_nfft_backward(nfft)
    with pytest.raises(NotImplementedError, match="nfft = 500"):  # refused before the forward is launched (no device is touched)
        torch.ops.orcai.spectrogram_wrt_pcm(torch.zeros(4000, requires_grad=True), 48000, 500, 250, 16000.0, 0.01, 0.999)


def test_c_entry_points_are_declared_and_bound():
    header = (ROOT / "include" / "orcai_hip.h").read_text()
    for name, nargs in (("orcai_spectrogram_bwd", 11), ("orcai_frontend_stats_dev", 3)):
        assert name in N.exported_symbols()
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", header)
        assert m is not None, name
        assert len([a for a in m.group(1).split(",")]) == nargs == len(N._SIGNATURES[name][1])
    args = [a.strip() for a in re.search(r"\bint\s+orcai_spectrogram_bwd\s*\(([^)]*)\)\s*;", header).group(1).split(",")]
    assert args[0] == "const float* pcm" and args[6] == "const float* gout" and args[7] == "const float* stats_dev" and args[9] == "float* dpcm"
    assert "HELD CONSTANT" in header  # the definition's central caveat is in the header comment
    assert getattr(N.lib(), "orcai_spectrogram_bwd") is not None and getattr(N.lib(), "orcai_frontend_stats_dev") is not None


def test_compile_traces_forward_and_backward_on_fake_tensors():
    """torch.compile(backend = aot_eager's machinery, fullgraph=True) of gain -> spectrogram_wrt_pcm -> loss with the gain requiring grad:
    AOTAutograd traces the forward AND the backward w.r.t. the audio on fake tensors through the op's Autograd kernel and the fake
    implementations of the two functional ops underneath.  No device exists here, so the partition function writes down the joint graph and
    stops (the pattern of tests/test_input_grad.py); running the compiled function is the GPU file's part."""
    import torch._dynamo
    from torch._functorch.aot_autograd import aot_module_simplified

    seen = {}

    class Traced(Exception):
        pass

    def f(pcm, gain):
        spec = torch.ops.orcai.spectrogram_wrt_pcm(pcm * gain, *ARGS)
        return (spec * spec).sum()

    def partition(joint, joint_inputs, **kwargs):
        seen["targets"] = [str(n.target) for n in joint.graph.nodes if n.op == "call_function"]
        outs = joint.graph.find_nodes(op="output")[0].args[0]
        flat = [v for group in outs for v in (group if isinstance(group, (list, tuple)) else [group])]
        seen["out"] = [tuple(int(d) for d in v.meta["val"].shape) for v in flat if hasattr(v, "meta") and "val" in v.meta]
        raise Traced

    def backend(gm, example_inputs):
        return aot_module_simplified(gm, example_inputs, fw_compiler=lambda g, i: g, partition_fn=partition)

    torch._dynamo.reset()
    pcm = torch.zeros(48000 + 17)
    gain = torch.ones((), requires_grad=True)
    with pytest.raises(Exception) as err:
        torch.compile(f, backend=backend, fullgraph=True)(pcm, gain)
    assert "targets" in seen, err.value
    assert any("orcai.spectrogram_with_stats.default" in t for t in seen["targets"]), seen["targets"]
    assert any("orcai.spectrogram_backward.default" in t for t in seen["targets"]), seen["targets"]
    assert () in seen["out"], seen["out"]
