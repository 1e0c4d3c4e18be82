"""The whole-recording gradient without a GPU: the C-ABI tie of the new symbols, the schemas and fake shapes of the new ops, their refusals, and the
snippet geometry RecordingGrad and the two adjoint launchers share with the forward (predict.py:244-293)."""

import pytest

torch = pytest.importorskip("torch")

from orcai_amd import torch_ops as O  # noqa: E402
from orcai_amd.architectures import ResNet1DConv, ResNetLSTM  # noqa: E402

NEW_SYMBOLS = {"orcai_overlap_average_bwd": 10, "orcai_snippets_overlap_add": 9, "orcai_zero_fill": 3}
SMALL = ((32, 12, 1), 3, [10, 20], 3, 0.0)  # H 32, shift 16, tpo 4, P 8, step 4


def _models():
    return [ResNetLSTM(*SMALL, 64), ResNet1DConv(*SMALL)]


def _vars(model, device="meta"):
    spec = model.variable_spec()
    return [torch.empty(s, device=device) for _, s, _, t in spec if t], [torch.empty(s, device=device) for _, s, _, t in spec if not t]


def test_new_symbols_in_header_table_and_library():
    import test_capi_symbols as S
    from orcai_amd import _native as N

    proto = S.header_prototypes()
    lib = N.lib()
    for name, nargs in NEW_SYMBOLS.items():
        assert name in proto and name in N._SIGNATURES, name
        assert len(proto[name][1]) == len(N._SIGNATURES[name][1]) == nargs, name
        assert getattr(lib, name) is not None


def test_new_ops_are_registered_with_their_schemas():
    ops = torch.ops.orcai
    fwd = "(Tensor spec, Tensor[] weights, Tensor[] stats, str config, SymInt chunk) -> Tensor"
    bwd = "(Tensor grad, Tensor spec, Tensor[] weights, Tensor[] stats, str config, SymInt chunk) -> "
    assert str(ops.detect_recording.default._schema) == "orcai::detect_recording" + fwd
    assert str(ops.detect_recording_wrt_params.default._schema) == "orcai::detect_recording_wrt_params" + fwd
    assert str(ops.detect_recording_bwd.default._schema) == "orcai::detect_recording_bwd" + bwd + "Tensor"
    assert str(ops.detect_recording_bwd_params.default._schema) == "orcai::detect_recording_bwd_params" + bwd + "(Tensor, Tensor)"
    # the op the recording-level forward runs keeps its schema, and no backward
    assert str(ops.predict_spectrogram.default._schema) == "orcai::predict_spectrogram(Tensor spec, Tensor[] weights, Tensor[] stats, str config) -> Tensor"


@pytest.mark.parametrize("T", [32, 101, 112])
def test_fake_shapes(T):
    for model in _models():
        w, s = _vars(model)
        cfg = O.model_config(model)
        spec = torch.empty((T, 12), device="meta")
        for op in (torch.ops.orcai.detect_recording, torch.ops.orcai.detect_recording_wrt_params):
            avg = op(spec, w, s, cfg, 64)
            assert avg.shape == (T // 4, 3) and avg.dtype == torch.float32 and avg.device.type == "meta"
        g = torch.empty((T // 4, 3), device="meta")
        dspec = torch.ops.orcai.detect_recording_bwd(g, spec, w, s, cfg, 2)
        assert dspec.shape == (T, 12) and dspec.dtype == torch.float32
        dspec, dw = torch.ops.orcai.detect_recording_bwd_params(g, spec, w, s, cfg, 2)
        assert dspec.shape == (T, 12) and dw.shape == (model.layout().n_w,) and dw.dtype == torch.float32


def test_cpu_tensors_are_refused():
    model = _models()[0]
    w, s = _vars(model, device="cpu")
    cfg = O.model_config(model)
    spec = torch.zeros((48, 12))
    for op in (torch.ops.orcai.detect_recording, torch.ops.orcai.detect_recording_wrt_params):
        with pytest.raises(ValueError, match="cuda"):
            op(spec, w, s, cfg, 64)
    with pytest.raises(ValueError, match="cuda"):
        torch.ops.orcai.detect_recording_bwd(torch.zeros((12, 3)), spec, w, s, cfg, 64)
    with pytest.raises(ValueError, match="cuda"):
        torch.ops.orcai.detect_recording_bwd_params(torch.zeros((12, 3)), spec, w, s, cfg, 64)
    with pytest.raises(ValueError, match=r"spec must be f32 \[T, 12\]"):
        torch.ops.orcai.detect_recording(torch.zeros((48, 13)), w, s, cfg, 64)


def test_f16_models_are_refused():
    from orcai_amd.eval_grad import RecordingGrad

    half = ResNetLSTM(*SMALL, 64, precision="f16")
    with pytest.raises(NotImplementedError, match="precision"):
        RecordingGrad(half)
    with pytest.raises(NotImplementedError, match="f16"):
        O.OrcaiModule(half, input_grad="eval")
    with pytest.raises(ValueError, match="chunk"):
        RecordingGrad(_models()[0], chunk=0)


def test_module_refuses_a_spec_gradient_it_was_not_built_for():
    m = O.OrcaiModule(_models()[0])
    with pytest.raises(NotImplementedError, match="input_grad='eval'"):
        m.detect_recording(torch.zeros((48, 12), requires_grad=True))


@pytest.mark.parametrize("T,n,rows,S", [(31, 0, (0, 0), 7), (32, 1, (0, 32), 8), (47, 1, (0, 32), 11), (48, 2, (0, 48), 12), (101, 5, (0, 96), 25)])
def test_geometry(T, n, rows, S):
    """The number of snippets and the spectrogram rows they cover, as the forward counts them (compute_aggregated_predictions, aggregate_predictions_device)."""
    from orcai_amd.eval_grad import RecordingGrad, recording_geometry

    g = recording_geometry(32, 2, T)
    assert (g["n"], g["rows"], g["S"]) == (n, rows, S)
    assert (g["H"], g["shift"], g["tpo"], g["P"], g["step"]) == (32, 16, 4, 8, 4)
    assert g["n"] == max((T - 32) // 16 + 1, 0)  # predict.py:244
    if n:
        assert (n - 1) * g["step"] + g["P"] <= S and rows[1] <= T < rows[1] + g["shift"]
    for model in _models():
        assert RecordingGrad(model, chunk=2).geometry(T) == g
