"""The eval-mode input gradient on the GPU: orcai_sepconv_dgrad alone against its formula in float64, EvalGrad end to end against float64
autograd of the eval-mode oracle (tests/eval_grad_ref.py), the launch record, and what the feature is for: a frozen detector that stays frozen."""

import math

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import eval_grad_ref as R  # noqa: E402
from recording_lib import RecordingLib  # noqa: E402

# Measured on the CPU for exactly the inputs of R.KERNEL_CASES (B = 2; all three gate modes): the header's formula evaluated by torch in f32 deviates
# from its float64 evaluation by at most this share of max|dr| -- k 3: 2.415e-7 (64 -> 64 at 24 x 22, no gates), k 5: 1.989e-7, k 7: 2.449e-7.
# The bar for the kernel is 8 x the worst value of its k: 1.93e-6, 1.59e-6, 1.96e-6 of max|dr|.
F32_REFERENCE_DEVIATION = {3: 2.415e-7, 5: 1.989e-7, 7: 2.449e-7}
KERNEL_BAR = {k: 8 * v for k, v in F32_REFERENCE_DEVIATION.items()}
MODES = ("both", "y", "none")


def _bits(a):
    return a.contiguous().view(torch.int32)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _case_tensors(case, pad_value=0.0):
    k = case["k"]
    return dict(g=_dev(R.to_planes(case["g"], k, pad_value)), y=_dev(R.to_planes(case["y"], k, pad_value)), x=_dev(R.to_planes(case["x"], k, pad_value)),
                wts=_dev(case["wts"]), taps=_dev(R.taps_layout(case["taps"], k)))


def _run(case, t, mode, composed=False):
    """dr planes (pre-zeroed) of one launch of orcai_sepconv_dgrad -- for k = 5 / 7, where the launcher refuses, or with composed=True, of the
    composition of existing launchers EvalGrad falls back to."""
    from orcai_amd import _native as N
    from orcai_amd.eval_grad import compose_dgrad

    B, Cout, H, W = case["g"].shape
    Cin, k = case["x"].shape[1], case["k"]
    y = t["y"] if mode != "none" else None
    x = t["x"] if mode == "both" else None
    dr = torch.zeros_like(t["x"])
    lib, st = N.lib(), N.stream_ptr()
    rc = N.E_UNSUPPORTED
    if not composed:
        rc = lib.orcai_sepconv_dgrad(t["g"].data_ptr(), None if y is None else y.data_ptr(), None if x is None else x.data_ptr(), B, Cin, Cout, H, W, k, t["wts"].data_ptr(),
                                     t["taps"].data_ptr(), dr.data_ptr(), st)
        assert rc == (0 if k == 3 else N.E_UNSUPPORTED), rc
    if rc == N.E_UNSUPPORTED:
        assert not bool(dr.any())  # a refusal touches nothing
        compose_dgrad(lib, t["g"].clone(), y, x, B, Cin, Cout, H, W, k, t["wts"], t["taps"], dr, torch.zeros_like(t["x"]), st)
    torch.cuda.synchronize()
    return dr


@pytest.mark.parametrize("Cin,Cout,H,W,k", R.KERNEL_CASES, ids=[f"{c[0]}to{c[1]}_{c[2]}x{c[3]}_k{c[4]}" for c in R.KERNEL_CASES])
def test_kernel_matches_its_formula(Cin, Cout, H, W, k):
    """orcai_sepconv_dgrad against the header's formula in float64 on the host, with both gates, y_gate only and none.  Bar: KERNEL_BAR (8 x the deviation
    of the formula evaluated in f32 by torch on the CPU).  Also: bit-identical between two launches and with every pad of g and the gates filled with
    3e30, the pads of a pre-zeroed dr still zero, and the fused result within the same bar of the composition of existing launchers."""
    case = R.kernel_case(Cin, Cout, H, W, k)
    t = _case_tensors(case)
    hot = _case_tensors(case, pad_value=3.0e30)
    for mode in MODES:
        ref = R.formula(case, mode, torch.float64).numpy()
        scale = float(np.abs(ref).max())
        dr = _run(case, t, mode)
        got, pads = R.from_planes(dr.cpu().numpy(), Cin, H, W, k)
        err = float(np.abs(got.astype(np.float64) - ref).max()) / scale
        print(f"{Cin}->{Cout} {H}x{W} k {k} gates {mode}: kernel {err:.2e} of max|dr| = {scale:.3e}; bar {KERNEL_BAR[k]:.2e}")
        assert np.isfinite(got).all() and err <= KERNEL_BAR[k], (mode, err, KERNEL_BAR[k])
        assert not pads.any()  # only the interior is written
        assert torch.equal(_bits(dr), _bits(_run(case, t, mode)))
        if k == 3:
            assert torch.equal(_bits(dr), _bits(_run(case, hot, mode)))  # pad contents do not matter
            comp, _ = R.from_planes(_run(case, t, mode, composed=True).cpu().numpy(), Cin, H, W, k)
            dev = float(np.abs(comp.astype(np.float64) - got).max()) / scale
            print(f"    fused vs composition: {dev:.2e}")
            assert dev <= KERNEL_BAR[k], (mode, dev)


def test_kernel_refuses_bad_arguments():
    from orcai_amd import _native as N

    a = torch.zeros(1 << 16, device="cuda")
    dr = torch.zeros(1 << 16, device="cuda")
    lib, st, p = N.lib(), N.stream_ptr(), a.data_ptr()
    call = lambda g, y, x, B, Cin, Cout, H, W, k, wts, taps, out: lib.orcai_sepconv_dgrad(g, y, x, B, Cin, Cout, H, W, k, wts, taps, out, st)  # noqa: E731
    assert call(None, p, p, 2, 8, 8, 6, 5, 3, p, p, dr.data_ptr()) == N.E_BADARG
    assert call(p, p, p, 2, 8, 8, 6, 5, 3, None, p, dr.data_ptr()) == N.E_BADARG
    assert call(p, p, p, 2, 8, 8, 6, 5, 3, p, None, dr.data_ptr()) == N.E_BADARG
    assert call(p, p, p, 2, 8, 8, 6, 5, 3, p, p, None) == N.E_BADARG
    assert call(p + 4, p, p, 2, 8, 8, 6, 5, 3, p, p, dr.data_ptr()) == N.E_BADARG  # misaligned planes
    assert call(p, p + 8, p, 2, 8, 8, 6, 5, 3, p, p, dr.data_ptr()) == N.E_BADARG
    assert call(p, p, p, 2, 8, 8, 6, 5, 3, p, p, dr.data_ptr() + 4) == N.E_BADARG
    for B, Cin, Cout, H, W, k in ((0, 8, 8, 6, 5, 3), (2, 0, 8, 6, 5, 3), (2, 8, -1, 6, 5, 3), (2, 8, 8, 0, 5, 3), (2, 8, 8, 6, 0, 3), (2, 8, 8, 6, 5, 4), (2, 8, 8, 6, 5, 9),
                                  (2, 8, 8, 6, 5, 1)):
        assert call(p, p, p, B, Cin, Cout, H, W, k, p, p, dr.data_ptr()) == N.E_BADARG, (B, Cin, Cout, H, W, k)
    assert call(p, p, p, 2, 8, 8, 6, 5, 5, p, p, dr.data_ptr()) == N.E_UNSUPPORTED
    assert call(p, p, p, 2, 68, 8, 6, 5, 3, p, p, dr.data_ptr()) == N.E_UNSUPPORTED
    torch.cuda.synchronize()
    assert not bool(dr.any())


# ------------------------------------------------------------------------------------------------------------------ end to end
_CACHE = {}


def _e2e(name):
    """One forward + backward of EvalGrad for an R.E2E_CASES entry (with the launch record) and the float64 reference, computed once and shared."""
    if name in _CACHE:
        return _CACHE[name]
    from orcai_amd.architectures import ResNet1DConv, ResNetLSTM
    from orcai_amd.eval_grad import EvalGrad

    _, cfg, B, conv1d, seed = next(c for c in R.E2E_CASES if c[0] == name)
    p, x, r = R.e2e_inputs(cfg, B, conv1d, seed)
    if conv1d:
        model = ResNet1DConv(cfg["input_shape"], cfg["num_labels"], list(cfg["filters"]), cfg["kernel_size"], 0.0)
    else:
        model = ResNetLSTM(cfg["input_shape"], cfg["num_labels"], list(cfg["filters"]), cfg["kernel_size"], 0.5, cfg["lstm_units"])  # a Dropout rate the eval path must ignore
    model.set_weights_dict(p)
    eg = EvalGrad(model)
    eg.lib = RecordingLib(eg._lib())
    xd = _dev(x[..., 0])
    probs, saved = eg.forward(xd)
    dx = eg.backward(_dev(r), saved)
    torch.cuda.synchronize()
    rec, eg.lib = eg.lib, eg.lib._lib
    ref_probs, ref_dx = R.input_gradient(p, x, r, conv1d, torch.float64)
    _CACHE[name] = dict(model=model, eg=eg, x=xd, r=_dev(r), probs=probs, saved=saved, dx=dx, rec=rec, ref_probs=ref_probs, ref_dx=ref_dx, cfg=cfg, B=B)
    return _CACHE[name]


@pytest.mark.parametrize("name", [c[0] for c in R.E2E_CASES])
def test_input_gradient_vs_float64_autograd(name):
    """EvalGrad.forward + backward, loss sum(probs * r), against float64 autograd of the eval-mode oracle: max|dx - ref| <= 5e-4 max|ref| (the project's
    gradient bar).  The forward: trunk features bit-identical to trunk_device's, probabilities within 5e-6 of orcai::forward(training=False) (whether
    they are equal is printed) and of the float64 oracle."""
    from orcai_amd.torch_ops import OrcaiModule

    c = _e2e(name)
    got = c["dx"].cpu().numpy().astype(np.float64)
    scale = float(np.abs(c["ref_dx"]).max())
    err = float(np.abs(got - c["ref_dx"]).max()) / scale
    model, B = c["model"], c["B"]
    H, W = model.input_hw
    T, wd, _ = model.stage_shapes()[-1]
    feat = torch.empty((B, T, wd * 36), device="cuda")
    model.trunk_device(c["x"].view(-1), H * W, B, feat, keep={})
    mod = OrcaiModule(model).cuda().eval()
    with torch.no_grad():
        fwd = mod(c["x"])
    dprobs = float((c["probs"] - fwd).abs().max())
    dref = float(np.abs(c["probs"].cpu().numpy().astype(np.float64) - c["ref_probs"]).max())
    print(f"{name}: max|dx - ref| / max|ref| = {err:.2e} (max|ref| {scale:.2e}); probs vs orcai::forward(eval) {dprobs:.1e} (equal: {torch.equal(c['probs'], fwd)}), vs float64 {dref:.1e}")
    assert np.isfinite(got).all() and err <= 5e-4, err
    assert torch.equal(_bits(c["eg"].views(c["saved"])["feat"]), _bits(feat))
    assert dprobs <= 5e-6 and dref <= 5e-6, (dprobs, dref)


@pytest.mark.parametrize("name", ["k3", "wide", "conv1d"])
def test_launch_record(name):
    """k = 3: every separable conv's backward is ONE accepted orcai_sepconv_dgrad, and no weight-gradient or statistics launcher runs."""
    c = _e2e(name)
    rec = c["rec"]
    assert rec.rcs("orcai_sepconv_dgrad") == [0] * (2 * len(c["model"].filters) + 1)
    names = {n for n, _, _ in rec.calls}
    banned = ("orcai_outer_reduce", "orcai_dw_wgrad", "orcai_dw_bwd_fused", "orcai_bn_bwd_pointwise", "orcai_bn_planes_stats", "orcai_conv0_stats")
    assert not [n for n in names if n.startswith(banned)], sorted(names)
    assert rec.rcs("orcai_conv0_bn_bwd_dx") == [0] and rec.rcs("orcai_pool_bwd") == [0] * len(c["model"].filters)


def test_routing_of_large_wide_layers():
    """Beyond 32 input channels EvalGrad asks the fused kernel only for small launches (the orcai-V1 shapes where it measured slower take the
    composition: DESIGN 4.7); up to 32 channels, and for k = 5 / 7 (where the launcher itself refuses), it always asks."""
    from orcai_amd.architectures import ResNetLSTM
    from orcai_amd.eval_grad import EvalGrad

    v1 = EvalGrad(ResNetLSTM((736, 171, 1), 7, [30, 40, 50, 60], 3, 0.5, 128))
    assert v1.fused(64, 16, 736, 171) and v1.fused(64, 30, 736, 171) and v1.fused(64, 30, 368, 86)
    assert not v1.fused(64, 40, 368, 86) and not v1.fused(64, 60, 92, 22) and not v1.fused(64, 60, 46, 11)
    assert v1.fused(2, 60, 46, 11) and v1.fused(1, 40, 92, 43)
    assert EvalGrad(ResNetLSTM((48, 21, 1), 7, [12, 30, 40], 7, 0.0, 64)).fused(4096, 40, 48, 21)


def test_composed_path_for_k5_and_k7():
    for name in ("k5", "k7"):
        rec = _e2e(name)["rec"]
        n = 2 * len(_e2e(name)["model"].filters) + 1
        assert rec.rcs("orcai_sepconv_dgrad") == [-2] * n  # refused before anything was touched; compose_dgrad ran instead


# ------------------------------------------------------------------------------------------------------------------ the point of the feature
def _module(name="k3"):
    from orcai_amd.torch_ops import OrcaiModule

    c = _e2e(name)
    return c, OrcaiModule(c["model"], input_grad="eval").cuda().eval()


def test_frozen_detector_stays_frozen_and_is_reproducible():
    c, m = _module()
    before = {n: t.detach().clone() for n, t in list(m.named_parameters()) + list(m.named_buffers())}
    grads = []
    for _ in range(2):
        x = c["x"].clone().requires_grad_()
        (m(x) * c["r"]).sum().backward()
        grads.append(x.grad)
    for n, t in list(m.named_parameters()) + list(m.named_buffers()):
        assert torch.equal(_bits(t.detach()), _bits(before[n])), n
    assert all(p.grad is None for p in m.parameters())
    assert torch.equal(_bits(grads[0]), _bits(grads[1]))
    assert torch.equal(_bits(grads[0]), _bits(c["dx"]))  # the op is EvalGrad
    assert m.dropout_draws == 0


def test_two_forwards_alive_at_once():
    c, m = _module()
    xa = c["x"].clone().requires_grad_()
    xb = (c["x"] * 0.5 + 0.1).requires_grad_()
    ya, yb = m(xa), m(xb)  # both graphs alive
    (yb * c["r"]).sum().backward()
    (ya * c["r"]).sum().backward()
    assert torch.equal(_bits(xa.grad), _bits(c["dx"]))
    xb2 = xb.detach().clone().requires_grad_()
    (m(xb2) * c["r"]).sum().backward()
    assert torch.equal(_bits(xb.grad), _bits(xb2.grad)) and not torch.equal(xa.grad, xb.grad)


def test_new_weights_reach_evalgrad_without_invalidate():
    """set_weights_dict on the model an EvalGrad(params=None) already ran on, and no invalidate(): the next forward and backward are, bit for bit,
    those of an EvalGrad built after the change -- never the old network's."""
    from orcai_amd.architectures import ResNetLSTM
    from orcai_amd.eval_grad import EvalGrad

    c = _e2e("k3")
    cfg = c["cfg"]
    make = lambda seed: ResNetLSTM(cfg["input_shape"], cfg["num_labels"], list(cfg["filters"]), cfg["kernel_size"], 0.5, cfg["lstm_units"], seed=seed)  # noqa: E731
    model = make(1)
    eg = EvalGrad(model)
    old, _ = eg.forward(c["x"])
    model.set_weights_dict(make(2).weights)
    probs, saved = eg.forward(c["x"])
    dx = eg.backward(c["r"], saved)
    fresh = EvalGrad(model)
    want, want_saved = fresh.forward(c["x"])
    assert not torch.equal(want, old)  # the two networks differ on this input
    assert torch.equal(_bits(probs), _bits(want))
    assert torch.equal(_bits(dx), _bits(fresh.backward(c["r"], want_saved)))
    eg.invalidate()  # still there, still harmless
    assert torch.equal(_bits(eg.forward(c["x"])[0]), _bits(want))


def test_saliency_helper():
    from orcai_amd.eval_grad import saliency

    c, m = _module()
    x = c["x"].clone().requires_grad_()
    m(x)[:, :, 1].sum().backward()
    assert torch.equal(_bits(saliency(c["model"], c["x"], label=1)), _bits(x.grad))
    x = c["x"].clone().requires_grad_()
    m(x).sum().backward()
    assert torch.equal(_bits(saliency(c["model"], c["x"])), _bits(x.grad))


def test_learnable_gain_in_front_of_the_eval_mode_detector_learns():
    """Ten steps of gradient descent on a per-frequency gain in front of OrcaiModule(input_grad="eval").eval(): the loss, a deterministic function of
    the gain, is lower at the end (step 0.02 along the gradient normalised by its largest component, as in test_input_grad_gpu)."""
    import test_torch_ops_gpu as G

    c, m = _module()
    model = c["model"]
    H, W = model.input_hw
    gen = torch.Generator(device="cuda").manual_seed(4)
    x = torch.rand((c["B"], H, W), device="cuda", generator=gen)
    y = G._labels(model, c["B"], 3)
    gain = torch.ones(W, device="cuda", requires_grad=True)
    losses = []
    for _ in range(10):
        q = m(x * gain).clamp(1e-7, 1 - 1e-7)
        mask = (y != -1.0).float()
        loss = (-(y * q.log() + (1 - y) * (1 - q).log()) * mask).sum() / mask.sum()
        (dg,) = torch.autograd.grad(loss, gain)
        losses.append(float(loss.detach()))
        with torch.no_grad():
            gain -= 0.02 * dg / dg.abs().max()
    print("gain training (eval mode):", [f"{v:.5f}" for v in losses])
    assert all(math.isfinite(v) for v in losses) and losses[-1] < losses[0], losses


def test_compiled_equals_eager():
    c, m = _module("conv1d")
    ws, st, cfg = [w.detach() for w in m.weights_list()], m.stats_list(), m.config
    W = c["model"].input_hw[1]

    def f(x, gain):
        y = torch.ops.orcai.detect_wrt_input(x * gain, ws, st, cfg)
        return (y * y).sum()

    res = []
    for fn in (f, torch.compile(f, backend="aot_eager", fullgraph=True)):
        gain = torch.linspace(0.5, 1.5, W, device="cuda").requires_grad_()
        loss = fn(c["x"], gain)
        loss.backward()
        res.append((loss.detach(), gain.grad))
    assert torch.equal(_bits(res[0][0]), _bits(res[1][0])) and torch.equal(_bits(res[0][1]), _bits(res[1][1]))


def test_opcheck():
    from torch.library import opcheck

    c, m = _module()
    ws, st, cfg = [w.detach().clone() for w in m.weights_list()], [s.clone() for s in m.stats_list()], m.config
    x = c["x"]
    opcheck(torch.ops.orcai.detect_wrt_input.default, (x, ws, st, cfg))
    opcheck(torch.ops.orcai.detect_wrt_input.default, (x.clone().requires_grad_(), ws, st, cfg))
    opcheck(torch.ops.orcai.detect_with_saved.default, (x, ws, st, cfg))
    probs, saved = torch.ops.orcai.detect_with_saved(x, ws, st, cfg)
    opcheck(torch.ops.orcai.detect_backward.default, (torch.ones_like(probs), saved, ws, st, cfg))


def test_f16_and_misuse():
    from orcai_amd.architectures import ResNetLSTM
    from orcai_amd.eval_grad import EvalGrad
    from orcai_amd.torch_ops import OrcaiModule

    half = ResNetLSTM((32, 12, 1), 3, [10, 20], 3, 0.0, 64, precision="f16")
    with pytest.raises(NotImplementedError, match="precision"):
        EvalGrad(half)
    with pytest.raises(NotImplementedError, match="f16"):
        OrcaiModule(half, input_grad="eval")
    c, m = _module()
    with pytest.raises(ValueError, match="saved must be"):
        c["eg"].backward(c["r"], c["saved"][:-1])
    with pytest.raises(ValueError, match="dprobs must be"):
        c["eg"].backward(c["r"][:1], c["saved"])
    # the existing eval-mode refusals stay
    plain = OrcaiModule(c["model"], input_grad=True).cuda().eval()
    out = plain(c["x"].clone().requires_grad_())
    with pytest.raises(RuntimeError, match="training=False"):
        out.sum().backward()
