"""Frozen-BatchNorm fine-tuning without a GPU: the G identity behind orcai_frozen_bn_finish against float64 autograd, the float64 oracle of the whole
network's weight gradients against its own f32 run (the calibration of the GPU bar), and the surface of the new ops (fake shapes, refusals, C ABI)."""

from pathlib import Path

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import eval_grad_ref as R  # noqa: E402
import frozen_grad_ref as FR  # noqa: E402
from orcai_amd import torch_ops as O  # noqa: E402
from orcai_amd.architectures import BN_EPS, ResNet1DConv, ResNetLSTM  # noqa: E402

NEW_SYMBOLS = ("orcai_sepconv_wgrad_frozen", "orcai_frozen_bn_finish", "orcai_rows_bn_frozen_wgrad")
GPU_BAR = 5e-4  # of max|ref| per variable: tests/test_frozen_grad_gpu.py, the rule of test_eval_grad_gpu.py for dx

# torch-CPU f32 autograd of frozen_grad_ref.weight_gradients against its float64 run at the seeds of eval_grad_ref.E2E_CASES: the worst variable of each
# case, as a share of that variable's max|ref| (and dx) -- all far inside a quarter of the GPU bar (1.25e-4), so no ReLU / pooling decision differs
# between the precisions at these seeds, for the weight gradients as for dx:
#   k3      dense2/bias         1.67e-6   (dx 6.7e-7)
#   k5      b1/sep_b/bias       5.65e-6   (dx 1.8e-6)
#   wide    b2/sep_b/depthwise  1.56e-6   (dx 9.8e-7)
#   k7      b2/bn_a/gamma       1.51e-6   (dx 5.3e-7)
#   conv1d  b1/sep_a/depthwise  1.31e-6   (dx 2.8e-7)


def test_g_identity_reproduces_autograd():
    """One small folded layer y = relu(scale (.) (pw . u + bias) + shift) in float64: dWpw, dbias, dgamma, dbeta from G = sum gg (x) u and sum gg alone
    (the formulae of include/orcai_hip.h: no z, no division by gamma) equal autograd's."""
    rng = np.random.default_rng(3)
    B, Cin, Cout, H, W = 2, 5, 7, 6, 4
    t = lambda *s: torch.tensor(rng.standard_normal(s))  # noqa: E731
    u, r = t(B, Cin, H, W), t(B, Cout, H, W)
    pw, bias, gamma, beta = (v.requires_grad_() for v in (t(Cin, Cout), t(Cout), t(Cout), t(Cout)))
    mean, var = t(Cout), torch.tensor(rng.uniform(0.5, 2.0, Cout))
    inv = torch.rsqrt(var + BN_EPS)
    z = torch.einsum("io,bihw->bohw", pw, u) + bias.view(1, -1, 1, 1)
    y = torch.relu((gamma * inv).view(1, -1, 1, 1) * z + (beta - mean * gamma * inv).view(1, -1, 1, 1))
    (y * r).sum().backward()
    gg = torch.where(y.detach() > 0, r, torch.zeros_like(r))
    G, sums = torch.einsum("bohw,bihw->oi", gg, u), gg.sum(dim=(0, 2, 3))
    scale = (gamma * inv).detach()
    pwd, biasd = pw.detach(), bias.detach()
    want = {"dWpw": (scale.view(-1, 1) * G).t(), "dbias": scale * sums, "dbeta": sums, "dgamma": inv * ((pwd.t() * G).sum(dim=1) + (biasd - mean) * sums)}
    got = {"dWpw": pw.grad, "dbias": bias.grad, "dbeta": beta.grad, "dgamma": gamma.grad}
    for k in want:
        assert FR.share(want[k].numpy(), got[k].numpy()) <= 1e-13, k


@pytest.mark.parametrize("name,cfg,B,conv1d,seed", R.E2E_CASES, ids=[c[0] for c in R.E2E_CASES])
def test_oracle_f32_stays_within_a_quarter_of_the_gpu_bar(name, cfg, B, conv1d, seed):
    """The oracle is eval_grad_ref's network (same probabilities, same dx), covers every trainable variable, and its f32 run stays within a quarter of the
    GPU bar of its float64 run for every variable (the table above)."""
    p, x, r = R.e2e_inputs(cfg, B, conv1d, seed)
    probs, g64, dx64 = FR.weight_gradients(p, x, r, conv1d, torch.float64)
    ref_probs, ref_dx = R.input_gradient(p, x, r, conv1d, torch.float64)
    assert np.abs(probs - ref_probs).max() <= 1e-12 and FR.share(dx64, ref_dx) <= 1e-10
    model = (ResNet1DConv(cfg["input_shape"], cfg["num_labels"], list(cfg["filters"]), cfg["kernel_size"]) if conv1d else
             ResNetLSTM(cfg["input_shape"], cfg["num_labels"], list(cfg["filters"]), cfg["kernel_size"], lstm_units=cfg["lstm_units"]))
    lay = model.layout()
    assert set(g64) == set(lay.w_names) and all(g64[n].shape == lay.w[n][2] for n in lay.w_names)
    assert all(np.abs(v).max() > 0 for v in g64.values())  # every variable, the separable convs' biases included, has a gradient in eval mode
    _, g32, dx32 = FR.weight_gradients(p, x, r, conv1d, torch.float32)
    shares = {k: FR.share(g32[k], g64[k]) for k in g64}
    worst = max(shares, key=shares.get)
    print(f"{name}: worst variable {worst} {shares[worst]:.2e} of max|ref|; dx {FR.share(dx32, dx64):.2e}")
    assert shares[worst] <= GPU_BAR / 4, (worst, shares[worst])


def test_wgrad_formula_calibration():
    """The f32 evaluation of the kernel formulae at the seeds of WGRAD_CASES deviates from float64 by no more than the shares written next to the cases
    (the GPU bar is 4 x the worst of them)."""
    for Cin, Cout, H, W in FR.WGRAD_CASES:
        case = FR.wgrad_case(Cin, Cout, H, W)
        for yg, ri in FR.WGRAD_MODES:
            ref, got = FR.wgrad_formula(case, torch.float64, yg, ri), FR.wgrad_formula(case, torch.float32, yg, ri)
            for key, a, b in zip(("G", "dbeta", "dWdw"), got, ref):
                assert a.shape == b.shape and FR.share(a.numpy(), b.numpy()) <= 1.5 * FR.F32_REFERENCE_DEVIATION[key], (Cin, Cout, H, W, yg, ri, key)
    assert ref[0].shape == (Cout, Cin) and ref[1].shape == (Cout,) and ref[2].shape == (3, 3, Cin, 1)


def _vars(model, device="meta"):
    spec = model.variable_spec()
    return [torch.empty(s, device=device) for _, s, _, t in spec if t], [torch.empty(s, device=device) for _, s, _, t in spec if not t]


@pytest.mark.parametrize(
    "model,B,out",
    [
        (ResNetLSTM((736, 171, 1), 7, [30, 40, 50, 60], 3, lstm_units=128), 3, (3, 46, 7)),
        (ResNetLSTM((64, 40, 1), 4, [12, 20], 5, lstm_units=64), 2, (2, 16, 4)),
        (ResNet1DConv((48, 21, 1), 5, [12, 30, 40], 7), 2, (2, 6, 5)),
    ],
)
def test_fake_shapes(model, B, out):
    H, W = model.input_hw
    w, s = _vars(model)
    cfg = O.model_config(model)
    x = torch.empty((B, H, W), device="meta")
    y = torch.ops.orcai.detect_wrt_params(x, w, s, cfg)
    assert y.shape == out and y.dtype == torch.float32 and y.device.type == "meta"
    probs, saved = torch.ops.orcai.detect_with_saved(x, w, s, cfg)
    dx, flat = torch.ops.orcai.detect_backward_params(torch.empty(out, device="meta"), saved, w, s, cfg)
    assert dx.shape == (B, H, W) and dx.dtype == torch.float32
    assert flat.shape == (model.layout().n_w,) and flat.dtype == torch.float32
    assert [tuple(g.shape) for g in model.layout().split_w(flat)] == [tuple(t.shape) for t in w]  # the inverse of _Engine.flat's direction


def test_schemas():
    assert str(torch.ops.orcai.detect_wrt_params.default._schema) == "orcai::detect_wrt_params(Tensor x, Tensor[] weights, Tensor[] stats, str config) -> Tensor"
    assert str(torch.ops.orcai.detect_backward_params.default._schema) == (
        "orcai::detect_backward_params(Tensor grad, Tensor saved, Tensor[] weights, Tensor[] stats, str config) -> (Tensor, Tensor)")
    # the existing op keeps its contract: no weight gradient
    assert "never a weight gradient" in O.detect_wrt_input.__doc__


def test_module_switch_and_refusals():
    model = ResNetLSTM((64, 40, 1), 4, [12, 20], 3, lstm_units=32, seed=1)
    with pytest.raises(ValueError, match="frozen_bn"):
        O.OrcaiModule(model, frozen_bn=True, input_grad=True)
    m = O.OrcaiModule(model, frozen_bn=True)
    assert m.frozen_bn and m.input_grad == "eval" and O.OrcaiModule(model, frozen_bn=True, input_grad="eval").input_grad == "eval"
    assert not O.OrcaiModule(model).frozen_bn
    x = torch.zeros((1, 64, 40))
    for mode in (m.train(), m.eval()):  # both run the eval-mode op: on the CPU its check names the missing GPU, and no Dropout seed is drawn
        with pytest.raises(ValueError, match="cuda"):
            mode(x)
    assert m.dropout_draws == 0
    half = ResNetLSTM((32, 12, 1), 3, [10, 20], 3, 0.0, 64, precision="f16")
    with pytest.raises(NotImplementedError, match="f16"):
        O.OrcaiModule(half, frozen_bn=True)
    from orcai_amd.eval_grad import EvalGrad

    with pytest.raises(NotImplementedError, match="precision"):
        EvalGrad(half)


def test_backward_signature_and_c_abi():
    import inspect

    from orcai_amd import _native as N
    from orcai_amd.eval_grad import EvalGrad, compose_wgrad

    sig = inspect.signature(EvalGrad.backward)
    assert sig.parameters["wgrad"].default is False and callable(compose_wgrad)
    header = (Path(__file__).resolve().parent.parent / "include" / "orcai_hip.h").read_text()
    for name in NEW_SYMBOLS:
        assert name in N._SIGNATURES and name in header


def test_compile_traces_forward_and_backward_on_fake_tensors():
    """AOTAutograd traces module -> loss with the PARAMETERS requiring grad on fake tensors: the joint graph holds orcai::detect_with_saved and
    orcai::detect_backward_params, and its outputs include one gradient per weight (the pattern of tests/test_eval_grad.py)."""
    import torch._dynamo
    from torch._functorch.aot_autograd import aot_module_simplified

    model = ResNet1DConv((48, 21, 1), 5, [12, 30], 3, seed=1)
    cfg = O.model_config(model)
    w = [torch.zeros(s, requires_grad=True) for _, s, _, t in model.variable_spec() if t]
    st = [torch.ones(s) for _, s, _, t in model.variable_spec() if not t]
    seen = {}

    class Traced(Exception):
        pass

    def f(x, *ws):
        return (torch.ops.orcai.detect_wrt_params(x, list(ws), st, cfg) ** 2).sum()

    def partition(joint, joint_inputs, **kwargs):
        seen["targets"] = [str(n.target) for n in joint.graph.nodes if n.op == "call_function"]
        raise Traced

    def backend(gm, example_inputs):
        return aot_module_simplified(gm, example_inputs, fw_compiler=lambda g, i: g, partition_fn=partition)

    torch._dynamo.reset()
    with pytest.raises(Exception) as e:
        torch.compile(f, backend=backend, fullgraph=True)(torch.zeros((2, 48, 21)), *w)
    assert isinstance(e.value, Traced) or isinstance(e.value.__cause__, Traced) or "Traced" in repr(e.value), repr(e.value)
    assert any("detect_with_saved" in t for t in seen["targets"]) and any("detect_backward_params" in t for t in seen["targets"]), seen["targets"]
