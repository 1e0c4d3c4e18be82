"""The eval-mode input gradient without a GPU: the float64 oracle against oracle.model_ref, the schemas and fake shapes of the new ops (also under a
symbolic batch), the OrcaiModule(input_grad="eval") switch, the C-ABI tie of the new symbols, and the compile trace on fake tensors."""

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import eval_grad_ref as R  # noqa: E402
from oracle import model_ref as M  # noqa: E402
from orcai_amd import torch_ops as O  # noqa: E402
from orcai_amd.architectures import ResNet1DConv, ResNetLSTM  # noqa: E402

NEW_SYMBOLS = ("orcai_sepconv_dgrad", "orcai_rows_affine", "orcai_rows_affine_relu_bwd")


def _vars(model, device="meta"):
    spec = model.variable_spec()
    return [torch.empty(s, device=device) for _, s, _, t in spec if t], [torch.empty(s, device=device) for _, s, _, t in spec if not t]


@pytest.mark.parametrize("name,cfg,B,conv1d,seed", R.E2E_CASES, ids=[c[0] for c in R.E2E_CASES])
def test_oracle_probabilities_equal_model_ref(name, cfg, B, conv1d, seed):
    """tests/eval_grad_ref.forward_eval in float64 against oracle.model_ref.forward_ref / forward_ref_1dconv(dtype=float64): 1e-12."""
    p, x, _ = R.e2e_inputs(cfg, B, conv1d, seed)
    got = R.forward_eval(p, torch.tensor(x, dtype=torch.float64), conv1d).numpy()
    ref = (M.forward_ref_1dconv if conv1d else M.forward_ref)(p, x, dtype=torch.float64)
    assert got.shape == ref.shape and float(np.abs(got - ref).max()) <= 1e-12


def test_new_ops_are_registered_with_their_schemas():
    ops = torch.ops.orcai
    assert str(ops.detect_wrt_input.default._schema) == "orcai::detect_wrt_input(Tensor x, Tensor[] weights, Tensor[] stats, str config) -> Tensor"
    assert str(ops.detect_with_saved.default._schema) == "orcai::detect_with_saved(Tensor x, Tensor[] weights, Tensor[] stats, str config) -> (Tensor, Tensor)"
    assert str(ops.detect_backward.default._schema) == (
        "orcai::detect_backward(Tensor grad, Tensor saved, Tensor[] weights, Tensor[] stats, str config) -> Tensor")
    # the existing ops keep theirs
    assert str(ops.forward_wrt_input.default._schema) == (
        "orcai::forward_wrt_input(Tensor x, Tensor[] weights, Tensor(a!)[] stats, str config, bool training, SymInt dropout_seed) -> Tensor")


@pytest.mark.parametrize(
    "model,B,out",
    [
        (ResNetLSTM((736, 171, 1), 7, [30, 40, 50, 60], 3, lstm_units=128), 3, (3, 46, 7)),
        (ResNetLSTM((64, 40, 1), 4, [12, 20], 5, lstm_units=64), 2, (2, 16, 4)),
        (ResNet1DConv((48, 21, 1), 5, [12, 30, 40], 7), 2, (2, 6, 5)),
    ],
)
def test_fake_shapes(model, B, out):
    from orcai_amd.eval_grad import saved_layout

    H, W = model.input_hw
    w, s = _vars(model)
    cfg = O.model_config(model)
    x = torch.empty((B, H, W), device="meta")
    y = torch.ops.orcai.detect_wrt_input(x, w, s, cfg)
    assert y.shape == out and y.dtype == torch.float32 and y.device.type == "meta"
    probs, saved = torch.ops.orcai.detect_with_saved(x, w, s, cfg)
    layout, per = saved_layout(model)
    assert probs.shape == out and saved.shape == (B * per,) and saved.dtype == torch.float32
    assert per == sum(int(np.prod(shape)) for _, _, shape in layout) and all(off % 4 == 0 for n, off, _ in layout if n != "x")  # 16-byte aligned (the snippets need not be)
    assert [n for n, _, _ in layout][0] == "y0" and [n for n, _, _ in layout][-2:] == ["probs", "x"]
    dx = torch.ops.orcai.detect_backward(torch.empty(out, device="meta"), saved, w, s, cfg)
    assert dx.shape == (B, H, W) and dx.dtype == torch.float32


def test_fake_shapes_with_a_symbolic_batch():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from torch.fx.experimental.symbolic_shapes import DimDynamic, ShapeEnv, StatelessSymbolicContext

    from orcai_amd.eval_grad import saved_layout

    model = ResNetLSTM((64, 40, 1), 4, [12, 20], 3, lstm_units=64)
    cfg = O.model_config(model)
    mode = FakeTensorMode(shape_env=ShapeEnv())
    x = mode.from_tensor(torch.empty((5, 64, 40)), symbolic_context=StatelessSymbolicContext(dynamic_sizes=[DimDynamic.DYNAMIC, DimDynamic.STATIC, DimDynamic.STATIC]))
    with mode:
        w = [torch.empty(s) for _, s, _, t in model.variable_spec() if t]
        st = [torch.empty(s) for _, s, _, t in model.variable_spec() if not t]
        probs, saved = torch.ops.orcai.detect_with_saved(x, w, st, cfg)
        dx = torch.ops.orcai.detect_backward(torch.empty_like(probs), saved, w, st, cfg)
    assert isinstance(probs.shape[0], torch.SymInt) and isinstance(saved.shape[0], torch.SymInt) and isinstance(dx.shape[0], torch.SymInt)
    assert int(saved.shape[0].node.hint) == 5 * saved_layout(model)[1] and int(dx.shape[0].node.hint) == 5 and tuple(dx.shape[1:]) == (64, 40)


def test_module_switch_selects_the_op(monkeypatch):
    """input_grad="eval": orcai::detect_wrt_input in .eval(), orcai::forward_wrt_input in .train(); True / False are unchanged."""
    model = ResNetLSTM((64, 40, 1), 4, [12, 20], 3, lstm_units=32, seed=1)
    calls = []

    class Spy:
        def __init__(self, name):
            self.name = name

        def __call__(self, x, *a):
            calls.append((self.name, len(a)))
            return x

    class Ops:
        forward, forward_wrt_input, detect_wrt_input = Spy("forward"), Spy("forward_wrt_input"), Spy("detect_wrt_input")

    class Namespace:
        orcai = Ops

    monkeypatch.setattr(O.torch, "ops", Namespace)
    x = torch.zeros((1, 64, 40))
    for flag, mode, want in (("eval", "eval", "detect_wrt_input"), ("eval", "train", "forward_wrt_input"), (True, "eval", "forward_wrt_input"), (True, "train", "forward_wrt_input"),
                             (False, "eval", "forward"), (False, "train", "forward")):
        m = O.OrcaiModule(model, input_grad=flag)
        getattr(m, mode)()
        calls.clear()
        m(x)
        assert [c[0] for c in calls] == [want], (flag, mode, calls)
        assert calls[0][1] == (3 if want == "detect_wrt_input" else 5)
    m = O.OrcaiModule(model, input_grad="eval").train()
    m(x), m(x)
    assert m.dropout_draws == 2
    m.eval()(x)
    assert m.dropout_draws == 2  # the eval-mode op draws nothing
    with pytest.raises(ValueError, match="input_grad"):
        O.OrcaiModule(model, input_grad="always")


def test_new_symbols_in_header_table_and_library():
    import test_capi_symbols as S
    from orcai_amd import _native as N

    proto = S.header_prototypes()
    lib = N.lib()
    for name in NEW_SYMBOLS:
        assert name in proto and name in N._SIGNATURES, name
        assert len(proto[name][1]) == len(N._SIGNATURES[name][1]), name
        assert getattr(lib, name) is not None
    assert len(proto["orcai_sepconv_dgrad"][1]) == 13


def test_f16_models_are_refused():
    from orcai_amd.eval_grad import EvalGrad

    half = ResNetLSTM((64, 40, 1), 4, [12, 20], 3, lstm_units=32, precision="f16")
    with pytest.raises(NotImplementedError, match="precision"):
        EvalGrad(half)
    with pytest.raises(NotImplementedError, match="f16"):
        O.OrcaiModule(half, input_grad="eval")


def test_eager_op_refuses_cpu_tensors():
    model = ResNetLSTM((64, 40, 1), 4, [12, 20], 3, lstm_units=32)
    w, s = _vars(model, device="cpu")
    with pytest.raises(ValueError, match="cuda"):
        torch.ops.orcai.detect_wrt_input(torch.zeros((1, 64, 40)), w, s, O.model_config(model))


def test_compile_traces_forward_and_backward_on_fake_tensors():
    """torch.compile(backend = aot_eager's machinery, fullgraph=True) of gain -> detect_wrt_input -> loss with the gain requiring grad: AOTAutograd
    traces the forward AND the backward w.r.t. the snippets on fake tensors through the op's Autograd kernel and the fake implementations of the two
    functional ops underneath.  No device exists here, so the partition function writes down the joint graph and stops (the pattern of
    tests/test_frontend_grad.py); running the compiled function is the GPU file's part."""
    import torch._dynamo
    from torch._functorch.aot_autograd import aot_module_simplified

    model = ResNet1DConv((48, 21, 1), 5, [12, 30], 3, seed=1)
    cfg = O.model_config(model)
    w, st = _vars(model, device="cpu")
    seen = {}

    class Traced(Exception):
        pass

    def f(x, gain):
        return (torch.ops.orcai.detect_wrt_input(x * gain, w, st, cfg) ** 2).sum()

    def partition(joint, joint_inputs, **kwargs):
        seen["targets"] = [str(n.target) for n in joint.graph.nodes if n.op == "call_function"]
        outs = joint.graph.find_nodes(op="output")[0].args[0]
        flat = [v for group in outs for v in (group if isinstance(group, (list, tuple)) else [group])]
        seen["out"] = [tuple(int(d) for d in v.meta["val"].shape) for v in flat if hasattr(v, "meta") and "val" in v.meta]
        raise Traced

    def backend(gm, example_inputs):
        return aot_module_simplified(gm, example_inputs, fw_compiler=lambda g, i: g, partition_fn=partition)

    torch._dynamo.reset()
    x = torch.zeros((2, 48, 21))
    gain = torch.ones(21, requires_grad=True)
    with pytest.raises(Exception) as err:
        torch.compile(f, backend=backend, fullgraph=True)(x, gain)
    assert "targets" in seen, err.value
    assert any("orcai.detect_with_saved.default" in t for t in seen["targets"]), seen["targets"]
    assert any("orcai.detect_backward.default" in t for t in seen["targets"]), seen["targets"]
    assert () in seen["out"] and (21,) in seen["out"], seen["out"]
