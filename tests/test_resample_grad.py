"""The gradient of the resampler without a GPU: the float64 reference of tests/resample_grad_ref.py is the adjoint of oracle.resample_ref, the gather
range the kernel walks reproduces the scatter form, and the two torch ops (orcai::resample, orcai::resample_backward) and WaveformFrontEnd are
registered with their schemas, fake shapes and refusals."""

import re
from pathlib import Path

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import resample_grad_ref as R  # noqa: E402
from orcai_amd import torch_ops as O  # noqa: E402
from orcai_amd.resample import design_table, output_length, ratio  # noqa: E402

SP = {"sampling_rate": 48000, "nfft": 512, "n_overlap": 256, "freq_range": [0, 16000], "quantiles": [0.01, 0.999]}


# ------------------------------------------------------------------------------------------------------------------ the reference
@pytest.mark.parametrize("c", R.CASES, ids=R.case_id)
def test_reference_is_the_adjoint_of_the_oracle_resampler(c):
    """<A x, g> = <x, A^T g> in float64, A = oracle.resample_ref.resample_ref (which rounds its result to float32: A x is recomputed here in float64
    from the float32 taps it uses, and pinned to the oracle's output first)."""
    from oracle.resample_ref import resample_ref

    sr_in, sr_out, n_in = c
    ref = R.case(*c)
    x, g = ref["x"].astype(np.float64), ref["g"].astype(np.float64)
    y32 = resample_ref(ref["x"], sr_in, sr_out)
    L, M = ref["L"], ref["M"]
    table = design_table(L, M).astype(np.float64)
    ntaps = table.shape[1]
    xp = np.concatenate([np.zeros(ntaps), x, np.zeros(ntaps)])
    y = np.empty(ref["n_out"])
    for n in range(ref["n_out"]):
        i0, phase = divmod(n * M, L)
        k0 = i0 - ntaps // 2 + 1 + ntaps
        y[n] = xp[k0 : k0 + ntaps] @ table[phase]
    assert y32.shape == y.shape and np.abs(y32 - y).max() <= 1e-6 * max(1.0, np.abs(y).max())  # the oracle's A, up to its float32 rounding
    lhs, rhs = float(y @ g), float(x @ ref["dx64"])
    bound = 1e-9 * float(np.linalg.norm(y) * np.linalg.norm(g))
    print(f"{R.case_id(c)}: <Ax, g> - <x, A^T g> = {lhs - rhs:.2e}, bound {bound:.2e}")
    assert abs(lhs - rhs) <= bound


@pytest.mark.parametrize("c", R.CASES, ids=R.case_id)
def test_gather_range_reproduces_the_scatter_form(c):
    """Summing dx[k] over n in [ceil((k-h)L/M), ceil((k+h)L/M)) clipped to [0, n_out) gives the scatter form; the neighbours on either side of the
    range do not hold k in their window (the range is complete and tight)."""
    sr_in, sr_out, n_in = c
    ref = R.case(*c)
    L, M, n_out = ref["L"], ref["M"], ref["n_out"]
    ntaps = design_table(L, M).shape[1]
    gathered = R.adjoint_gather(ref["g"], n_in, sr_in, sr_out)
    assert np.abs(gathered - ref["dx64"]).max() <= 1e-13 * max(1.0, np.abs(ref["dx64"]).max())
    holds = lambda n, k: 0 <= k - ((n * M) // L - ntaps // 2 + 1) < ntaps  # noqa: E731
    for k in {0, 1, n_in // 2, n_in - 1}:
        lo, hi = R.gather_range(k, n_out, L, M, ntaps)
        assert all(holds(n, k) for n in range(lo, hi))
        assert (lo == 0 or not holds(lo - 1, k)) and (hi == n_out or not holds(hi, k)), (k, lo, hi)


def test_cases_cover_what_they_are_meant_to():
    shapes = {(si, so): (ratio(si, so), design_table(*ratio(si, so)).shape) for si, so, _ in R.CASES}
    assert shapes[(22050, 48000)] == ((320, 147), (320, 128)) and shapes[(48000, 22050)] == ((147, 320), (147, 280))
    assert shapes[(96000, 48000)] == ((1, 2), (1, 256)) and shapes[(8000, 48000)] == ((6, 1), (6, 128))
    assert shapes[(44100, 48000)] == ((160, 147), (160, 128))


# ------------------------------------------------------------------------------------------------------------------ C ABI
def test_header_declares_the_backward_next_to_the_forward():
    from orcai_amd import _native as N

    header = (Path(__file__).resolve().parent.parent / "include" / "orcai_hip.h").read_text()
    protos = {name: [a.strip() for a in args.split(",")] for name, args in re.findall(r"\bint\s+(orcai_resample_polyphase\w*)\s*\(([^)]*)\)\s*;", header)}
    assert set(protos) == {"orcai_resample_polyphase", "orcai_resample_polyphase_bwd"}
    bwd = protos["orcai_resample_polyphase_bwd"]
    assert bwd == ["const float* dout", "int64_t n_out", "float* dx", "int64_t n_in", "int L", "int M", "const float* table", "int ntaps", "void* stream"]
    assert len(N._SIGNATURES["orcai_resample_polyphase_bwd"][1]) == len(bwd)
    assert getattr(N.lib(), "orcai_resample_polyphase_bwd") is not None


# ------------------------------------------------------------------------------------------------------------------ ops
def test_ops_are_registered_with_their_schemas():
    ops = torch.ops.orcai
    assert str(ops.resample.default._schema) == "orcai::resample(Tensor pcm, SymInt sr_in, SymInt sr_out) -> Tensor"
    assert str(ops.resample_backward.default._schema) == "orcai::resample_backward(Tensor grad, SymInt n_in, SymInt sr_in, SymInt sr_out) -> Tensor"


@pytest.mark.parametrize("c", R.CASES + ((22050, 48000, 79380000), (48000, 48000, 1234)), ids=R.case_id)
def test_fake_shapes(c):
    sr_in, sr_out, n_in = c
    n_out = output_length(n_in, sr_in, sr_out)
    y = torch.ops.orcai.resample(torch.empty(n_in, device="meta"), sr_in, sr_out)
    assert y.shape == (n_out,) and y.dtype == torch.float32 and y.device.type == "meta"
    dx = torch.ops.orcai.resample_backward(torch.empty(n_out, device="meta"), n_in, sr_in, sr_out)
    assert dx.shape == (n_in,) and dx.dtype == torch.float32
    if sr_in == sr_out:
        assert n_out == n_in


def test_eager_ops_refuse_cpu_tensors():
    with pytest.raises(ValueError, match="pcm must be a 1-d f32 cuda tensor"):
        torch.ops.orcai.resample(torch.zeros(100), 22050, 48000)
    with pytest.raises(ValueError, match="grad must be a 1-d f32 cuda tensor"):
        torch.ops.orcai.resample_backward(torch.zeros(218), 100, 22050, 48000)
    with pytest.raises(ValueError, match="pcm"):
        O.WaveformFrontEnd(SP, 22050)(torch.zeros(1000))


def test_waveform_front_end_fake_shape_and_parameters():
    m = O.WaveformFrontEnd(SP, 22050)
    assert (m.native_rate, m.sampling_rate, m.nfft, m.hop, m.freq_hi, m.q_lo, m.q_hi) == (22050, 48000, 512, 256, 16000.0, 0.01, 0.999)
    assert list(m.parameters()) == [] and "22050 Hz -> 48000 Hz" in repr(m)
    n = 30000
    y = m(torch.empty(n, device="meta"))
    assert y.shape == (1 + output_length(n, 22050, 48000) // 256, 171)
    assert O.WaveformFrontEnd(SP, 48000)(torch.empty(n, device="meta")).shape == (1 + n // 256, 171)
    with pytest.raises(ValueError, match="freq_range"):
        O.WaveformFrontEnd(dict(SP, freq_range=[1000, 16000]), 22050)


def test_compile_traces_the_module_forward_and_backward_on_fake_tensors():
    """torch.compile(fullgraph=True) of gain -> WaveformFrontEnd -> loss with the gain requiring grad: AOTAutograd traces the forward AND the backward
    w.r.t. the audio at its native rate on fake tensors, through the Autograd kernels of orcai::resample and orcai::spectrogram_wrt_pcm and the fake
    implementations of the functional ops underneath.  No device exists here, so the partition function writes down the joint graph and stops (the
    pattern of tests/test_frontend_grad.py); running the compiled module is the GPU file's part.  With backend="eager" (no AOTAutograd) Dynamo alone
    traces the module without a graph break, up to the first real kernel, which refuses the CPU tensor by name."""
    import torch._dynamo
    from torch._functorch.aot_autograd import aot_module_simplified

    m = O.WaveformFrontEnd(SP, 22050)
    seen = {}

    class Traced(Exception):
        pass

    def f(pcm, gain):
        return (m(pcm * gain) ** 2).sum()

    def partition(joint, joint_inputs, **kwargs):
        seen["targets"] = [str(n.target) for n in joint.graph.nodes if n.op == "call_function"]
        outs = joint.graph.find_nodes(op="output")[0].args[0]
        flat = [v for group in outs for v in (group if isinstance(group, (list, tuple)) else [group])]
        seen["out"] = [tuple(int(d) for d in v.meta["val"].shape) for v in flat if hasattr(v, "meta") and "val" in v.meta]
        raise Traced

    def backend(gm, example_inputs):
        return aot_module_simplified(gm, example_inputs, fw_compiler=lambda g, i: g, partition_fn=partition)

    torch._dynamo.reset()
    pcm = torch.zeros(30000)
    gain = torch.ones((), requires_grad=True)
    with pytest.raises(Exception) as err:
        torch.compile(f, backend=backend, fullgraph=True)(pcm, gain)
    assert "targets" in seen, err.value
    for op in ("orcai.resample.default", "orcai.resample_backward.default", "orcai.spectrogram_with_stats.default", "orcai.spectrogram_backward.default"):
        assert any(op in t for t in seen["targets"]), (op, seen["targets"])
    assert () in seen["out"], seen["out"]

    graphs = []

    def eager_backend(gm, example_inputs):
        graphs.append([str(n.target) for n in gm.graph.nodes if n.op == "call_function"])
        return gm.forward

    torch._dynamo.reset()
    with pytest.raises(ValueError, match="pcm must be a 1-d f32 cuda tensor"):  # one graph, traced on fake tensors; running it needs the GPU
        torch.compile(m, backend=eager_backend, fullgraph=True)(pcm)
    assert len(graphs) == 1 and any("resample" in t for t in graphs[0]) and any("spectrogram_wrt_pcm" in t for t in graphs[0]), graphs
    torch._dynamo.reset()
