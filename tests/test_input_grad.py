"""The input gradient without a GPU: the two new ops' schemas and fake shapes, the C entry point in the header and the ctypes table, and a
torch.compile trace of forward_wrt_input differentiated w.r.t. x on fake tensors."""

import re
from pathlib import Path

import pytest

torch = pytest.importorskip("torch")

from orcai_amd import _native as N  # noqa: E402
from orcai_amd import torch_ops as O  # noqa: E402
from orcai_amd.architectures import ResNet1DConv, ResNetLSTM  # noqa: E402

ROOT = Path(__file__).resolve().parent.parent
V1 = dict(input_shape=(736, 171, 1), num_labels=7, filters=[30, 40, 50, 60], kernel_size=3, lstm_units=128)
MODELS = [
    (lambda: ResNetLSTM(**V1), 3, (3, 46, 7)),
    (lambda: ResNetLSTM((64, 40, 1), 4, [12, 20], 5, lstm_units=64), 2, (2, 16, 4)),
    (lambda: ResNet1DConv((48, 21, 1), 5, [12, 30, 40], 7), 2, (2, 6, 5)),
]


def _vars(model, device="meta"):
    spec = model.variable_spec()
    return [torch.empty(s, device=device) for _, s, _, t in spec if t], [torch.empty(s, device=device) for _, s, _, t in spec if not t]


def test_new_ops_are_registered_with_their_schemas():
    ops = torch.ops.orcai
    assert str(ops.forward_wrt_input.default._schema) == (
        "orcai::forward_wrt_input(Tensor x, Tensor[] weights, Tensor(a!)[] stats, str config, bool training, SymInt dropout_seed) -> Tensor")
    assert str(ops.forward_wrt_input_backward.default._schema) == (
        "orcai::forward_wrt_input_backward(Tensor grad, Tensor probs, str config) -> (Tensor, Tensor)")


def test_c_entry_point_is_declared_and_bound():
    assert "orcai_conv0_bn_bwd_dx" in N.exported_symbols()
    header = (ROOT / "include" / "orcai_hip.h").read_text()
    m = re.search(r"\bint\s+orcai_conv0_bn_bwd_dx\s*\(([^)]*)\)\s*;", header)
    assert m is not None
    args = [a.strip() for a in m.group(1).split(",")]
    assert len(args) == 17 and args[1] == "int64_t snippet_stride" and args[-3] == "const double* sums2C" and args[-2] == "float* dx"
    ret, argtypes = N._SIGNATURES["orcai_conv0_bn_bwd_dx"]
    assert len(argtypes) == 17


@pytest.mark.parametrize("make,B,out", MODELS)
def test_forward_wrt_input_fake_shapes(make, B, out):
    model = make()
    H, W = model.input_hw
    w, s = _vars(model)
    cfg = O.model_config(model)
    for training in (False, True):
        y = torch.ops.orcai.forward_wrt_input(torch.empty((B, H, W), device="meta"), w, s, cfg, training, 0)
        assert y.shape == out and y.dtype == torch.float32 and y.device.type == "meta"
    n = sum(int(torch.Size(t.shape).numel()) for t in w)
    flat, dx = torch.ops.orcai.forward_wrt_input_backward(torch.empty(out, device="meta"), torch.empty(out, device="meta"), cfg)
    assert flat.shape == (n,) and flat.dtype == torch.float32
    assert dx.shape == (B, H, W) and dx.dtype == torch.float32 and dx.device.type == "meta"
    assert flat.shape == torch.ops.orcai.forward_backward(torch.empty(out, device="meta"), torch.empty(out, device="meta"), cfg).shape


def test_fake_shapes_with_a_symbolic_batch():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from torch.fx.experimental.symbolic_shapes import DimDynamic, ShapeEnv, StatelessSymbolicContext

    model = ResNetLSTM((64, 40, 1), 4, [12, 20], 5, lstm_units=64)
    cfg = O.model_config(model)
    mode = FakeTensorMode(shape_env=ShapeEnv())
    x = mode.from_tensor(torch.empty((5, 64, 40)), symbolic_context=StatelessSymbolicContext(dynamic_sizes=[DimDynamic.DYNAMIC, DimDynamic.STATIC, DimDynamic.STATIC]))
    with mode:
        w = [torch.empty(s) for _, s, _, t in model.variable_spec() if t]
        st = [torch.empty(s) for _, s, _, t in model.variable_spec() if not t]
        y = torch.ops.orcai.forward_wrt_input(x, w, st, cfg, True, 0)
        flat, dx = torch.ops.orcai.forward_wrt_input_backward(torch.empty_like(y), y, cfg)
    assert isinstance(y.shape[0], torch.SymInt) and int(y.shape[0].node.hint) == 5 and tuple(y.shape[1:]) == (16, 4)
    assert isinstance(dx.shape[0], torch.SymInt) and int(dx.shape[0].node.hint) == 5 and tuple(dx.shape[1:]) == (64, 40)
    assert flat.shape == (sum(int(torch.Size(t.shape).numel()) for t in w),)


def test_module_input_grad_switch_selects_the_op():
    model = ResNetLSTM((64, 40, 1), 4, [12, 20], 3, lstm_units=32, seed=3)
    assert O.OrcaiModule(model).input_grad is False and O.OrcaiModule(model, input_grad=True).input_grad is True
    m = O.OrcaiModule(model, seed=2, input_grad=True).to("meta")
    with torch.no_grad():
        y = m(torch.empty((2, 64, 40), device="meta"))
    assert y.shape == (2, 16, 4)


def test_compile_traces_the_input_gradient_on_fake_tensors():
    """torch.compile(fullgraph=True) of a function that runs forward_wrt_input(training=True) behind a learnable gain, with the gain requiring
    grad, so that AOTAutograd traces forward AND backward w.r.t. x on fake tensors through the op's Autograd kernel and the fake implementations
    of both ops.  No device exists here, so the compiled function is never run: the backend is aot_eager's (aot_module_simplified with no
    compilers) with a partition function that writes down the joint graph and stops.  What is shown: no graph break, the joint graph calls
    orcai::forward_wrt_input and orcai::forward_wrt_input_backward and yields a gradient of the gain's shape (which exists only through dL/dx).
    Running the compiled function, and torch.autograd.grad inside it, is the GPU file's part."""
    import torch._dynamo
    from torch._functorch.aot_autograd import aot_module_simplified

    model = ResNetLSTM((64, 40, 1), 4, [12, 20], 3, lstm_units=32, seed=3)
    cfg = O.model_config(model)
    w, st = _vars(model, device="cpu")
    seen = {}

    class Traced(Exception):
        pass

    def f(x, gain):
        y = torch.ops.orcai.forward_wrt_input(x * gain, w, st, cfg, True, 5)
        return (y * y).sum()

    def partition(joint, joint_inputs, **kwargs):
        # (an op that mutates an argument -- the moving statistics -- appears as auto_functionalized(op, ...): the op is the node's first argument)
        seen["targets"] = [str(n.target) + " " + (str(n.args[0]) if n.args else "") for n in joint.graph.nodes if n.op == "call_function"]
        outs = joint.graph.find_nodes(op="output")[0].args[0]
        flat = [v for group in outs for v in (group if isinstance(group, (list, tuple)) else [group])]
        seen["out"] = [tuple(int(d) for d in v.meta["val"].shape) for v in flat if hasattr(v, "meta") and "val" in v.meta]
        raise Traced

    def backend(gm, example_inputs):
        return aot_module_simplified(gm, example_inputs, fw_compiler=lambda g, i: g, partition_fn=partition)

    torch._dynamo.reset()
    x = torch.zeros((2, 64, 40))
    gain = torch.ones((40,), requires_grad=True)
    with pytest.raises(Exception) as err:
        torch.compile(f, backend=backend, fullgraph=True)(x, gain)
    assert "targets" in seen, err.value
    assert any("orcai.forward_wrt_input.default" in t for t in seen["targets"]), seen["targets"]
    assert any("orcai.forward_wrt_input_backward.default" in t for t in seen["targets"]), seen["targets"]
    assert (40,) in seen["out"], seen["out"]
