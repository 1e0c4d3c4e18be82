"""The orcai torch custom ops without a GPU: registration, schemas, fake (meta) shapes, the OrcaiModule parameter layout, f16 refusal."""

import json

import pytest

torch = pytest.importorskip("torch")

from orcai_amd import torch_ops as O  # noqa: E402
from orcai_amd.architectures import ResNet1DConv, ResNetLSTM  # noqa: E402

V1 = dict(input_shape=(736, 171, 1), num_labels=7, filters=[30, 40, 50, 60], kernel_size=3, lstm_units=128)


def _vars(model, device="meta"):
    spec = model.variable_spec()
    w = [torch.empty(s, device=device) for _, s, _, t in spec if t]
    s = [torch.empty(s, device=device) for _, s, _, t in spec if not t]
    return w, s


def test_ops_are_registered_with_their_schemas():
    ops = torch.ops.orcai
    assert str(ops.spectrogram.default._schema) == (
        "orcai::spectrogram(Tensor pcm, SymInt sampling_rate, SymInt nfft, SymInt hop, float freq_hi, float q_lo, float q_hi) -> Tensor")
    assert str(ops.forward.default._schema) == (
        "orcai::forward(Tensor x, Tensor[] weights, Tensor(a!)[] stats, str config, bool training, SymInt dropout_seed) -> Tensor")
    assert str(ops.predict_spectrogram.default._schema) == (
        "orcai::predict_spectrogram(Tensor spec, Tensor[] weights, Tensor[] stats, str config) -> Tensor")


@pytest.mark.parametrize(
    "model,B,out",
    [
        (ResNetLSTM(**V1), 3, (3, 46, 7)),
        (ResNetLSTM((64, 40, 1), 4, [12, 20], 5, lstm_units=64), 2, (2, 16, 4)),
        (ResNet1DConv((48, 21, 1), 5, [12, 30, 40], 7), 2, (2, 6, 5)),
    ],
)
def test_forward_fake_shapes(model, B, out):
    H, W = model.input_hw
    w, s = _vars(model)
    cfg = O.model_config(model)
    for training in (False, True):
        y = torch.ops.orcai.forward(torch.empty((B, H, W), device="meta"), w, s, cfg, training, 0)
        assert y.shape == out and y.dtype == torch.float32 and y.device.type == "meta"
    assert model.output_shape[1:] == out[1:]


def test_predict_spectrogram_fake_shapes():
    model = ResNetLSTM(**V1)
    w, s = _vars(model)
    cfg = O.model_config(model)
    for T, n in ((736, 1), (735, 0), (368 * 7 + 736, 8), (100, 0)):
        y = torch.ops.orcai.predict_spectrogram(torch.empty((T, 171), device="meta"), w, s, cfg)
        assert y.shape == (n, 46, 7), (T, y.shape)


@pytest.mark.parametrize("n,nfft,hop,sr,fhi,K", [(48000 * 3 + 17, 512, 256, 48000, 16000, 171), (1000, 255, 100, 22050, 5000, 58), (5, 512, 256, 48000, 16000, 171)])
def test_spectrogram_fake_shapes(n, nfft, hop, sr, fhi, K):
    y = torch.ops.orcai.spectrogram(torch.empty(n, device="meta"), sr, nfft, hop, fhi, 0.01, 0.999)
    assert y.shape == (1 + (n - (nfft & 1)) // hop, K) and y.dtype == torch.float32


def test_fake_shapes_with_symbolic_lengths():
    """Under a FakeTensorMode with a ShapeEnv, T and n are expressions of the input's length (what torch.compile's dynamic shapes see)."""
    from torch._subclasses.fake_tensor import FakeTensorMode
    from torch.fx.experimental.symbolic_shapes import ShapeEnv

    model = ResNetLSTM(**V1)
    cfg = O.model_config(model)
    from torch.fx.experimental.symbolic_shapes import DimDynamic, StatelessSymbolicContext

    mode = FakeTensorMode(shape_env=ShapeEnv())
    pcm = mode.from_tensor(torch.empty(48000 * 20), symbolic_context=StatelessSymbolicContext(dynamic_sizes=[DimDynamic.DYNAMIC]))
    with mode:
        w = [torch.empty(s) for _, s, _, t in model.variable_spec() if t]
        st = [torch.empty(s) for _, s, _, t in model.variable_spec() if not t]
        spec = torch.ops.orcai.spectrogram(pcm, 48000, 512, 256, 16000.0, 0.01, 0.999)
        out = torch.ops.orcai.predict_spectrogram(spec, w, st, cfg)
    assert isinstance(spec.shape[0], torch.SymInt) and isinstance(out.shape[0], torch.SymInt)
    assert int(spec.shape[0].node.hint) == 1 + 48000 * 20 // 256
    assert int(out.shape[0].node.hint) == (1 + 48000 * 20 // 256 - 736) // 368 + 1


def test_backward_op_fake_shape():
    model = ResNet1DConv((48, 21, 1), 5, [12, 30, 40], 3)
    n = sum(int(torch.Size(s).numel()) for _, s, _, t in model.variable_spec() if t)
    g = torch.ops.orcai.forward_backward(torch.empty((2, 6, 5), device="meta"), torch.empty((2, 6, 5), device="meta"), O.model_config(model))
    assert g.shape == (n,)


@pytest.mark.parametrize("model", [ResNetLSTM((64, 40, 1), 4, [12, 20], 5, lstm_units=64, seed=1), ResNet1DConv((48, 21, 1), 5, [12, 30], 3, seed=1)])
def test_module_parameters_follow_variable_spec(model):
    m = O.OrcaiModule(model)
    spec = model.variable_spec()
    assert [(n, tuple(p.shape)) for n, p in m.named_parameters()] == [(O.param_name(n), tuple(s)) for n, s, _, t in spec if t]
    assert [(n, tuple(b.shape)) for n, b in m.named_buffers()] == [(O.param_name(n), tuple(s)) for n, s, _, t in spec if not t]
    assert all("/" not in n for n, _ in m.named_parameters())
    assert O.param_name("b1/sep_a/depthwise") == "b1__sep_a__depthwise"
    for n, _, _, _ in spec:  # the values are the model's
        assert torch.equal(m.get_parameter(O.param_name(n)) if n in m._trainable else m.get_buffer(O.param_name(n)), torch.from_numpy(model.weights[n]))
    cfg = json.loads(m.config)
    assert cfg["architecture"] == model.architecture and cfg["filters"] == model.filters


def test_module_to_model_writes_the_state_back():
    model = ResNetLSTM((64, 40, 1), 4, [12, 20], 3, lstm_units=32, seed=3)
    m = O.OrcaiModule(model)
    with torch.no_grad():
        m.get_parameter("dense2__bias").add_(1.0)
        m.get_buffer("bn_f__var").mul_(2.0)
    back = m.to_model()
    assert back is model
    assert (model.weights["dense2/bias"] == 1.0).all() and (model.weights["bn_f/var"] == 2.0).all()


def test_module_from_a_model_directory(tmp_path):
    import shutil
    from pathlib import Path

    src = Path(O.__file__).parent / "models" / "orcai-V1"
    d = tmp_path / "orcai-V1"
    shutil.copytree(src, d)
    model = ResNetLSTM(**V1, seed=2)
    model.save(d / "orcai-v1.keras")
    m = O.OrcaiModule(d)
    assert torch.equal(m.get_parameter("dense2__kernel"), torch.from_numpy(model.weights["dense2/kernel"]))


def test_f16_models_are_refused():
    with pytest.raises(NotImplementedError, match="f16"):
        O.OrcaiModule(ResNetLSTM((64, 40, 1), 4, [12, 20], 3, lstm_units=32, precision="f16"))
    with pytest.raises(NotImplementedError, match="f16"):
        O.model_config(ResNet1DConv((48, 21, 1), 5, [12, 30], 3, precision="f16"))
    cfg = json.loads(O.model_config(ResNetLSTM((64, 40, 1), 4, [12, 20], 3, lstm_units=32)))
    cfg["precision"] = "f16"
    model = ResNetLSTM((64, 40, 1), 4, [12, 20], 3, lstm_units=32)
    w, s = _vars(model)
    with pytest.raises(NotImplementedError, match="f16"):
        torch.ops.orcai.forward(torch.empty((1, 64, 40), device="meta"), w, s, json.dumps(cfg), False, 0)


def test_eager_ops_refuse_cpu_tensors():
    model = ResNetLSTM((64, 40, 1), 4, [12, 20], 3, lstm_units=32)
    w, s = _vars(model, device="cpu")
    with pytest.raises(ValueError, match="cuda"):
        torch.ops.orcai.forward(torch.zeros((1, 64, 40)), w, s, O.model_config(model), False, 0)
