"""The gradient w.r.t. the input snippets on the GPU: orcai_conv0_bn_bwd_dx alone against its formula in float64, the whole training step
against float64 autograd (oracle.train_ref with x requiring grad), the benchmarked shape on the branches the GPU took and against the
free-running oracle, and the torch ops (forward_wrt_input / OrcaiModule(input_grad=True))."""

import math

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from oracle import model_ref as M  # noqa: E402
from oracle import train_ref as T  # noqa: E402
from recording_lib import RecordingLib  # noqa: E402

EPS = 1e-3  # BatchNormalization epsilon of the layers (Keras default), the value the trainer passes

# ------------------------------------------------------------------------------------------------------------------ 1. the kernel alone
KERNEL_SHAPES = [(32, 12), (48, 21), (16, 120), (37, 171), (736, 171)]
# Measured on the CPU for exactly these inputs (every shape, B = 2): the formula below evaluated by torch in f32 deviates from its float64
# evaluation by at most this share of max|dx| (the summation order over the 16 k^2 products differs; the worst case of each k is the
# 37 x 171 or the 736 x 171 shape).  The bar for the kernel is 8 x the worst value of its k.
F32_REFERENCE_DEVIATION = {3: 4.64e-7, 5: 7.09e-7, 7: 1.05e-6}
KERNEL_BAR = {k: 8 * v for k, v in F32_REFERENCE_DEVIATION.items()}


def _padded_width(W, k):
    return (W + k // 2 + 3) & ~3


def _formula(x, dy, w0, bias, mean, var, gamma, beta, dbeta, dgamma, k, dtype):
    """dx of the header's formula by torch on the host in `dtype`.  x [B][H][W], dy [B][16][H][W], w0 Keras (k, k, 1, 16)."""
    c = lambda a: torch.as_tensor(np.asarray(a), dtype=dtype)  # noqa: E731
    x, dy, bias, mean, var, gamma, beta, dbeta, dgamma = (c(a) for a in (x, dy, bias, mean, var, gamma, beta, dbeta, dgamma))
    wt = c(w0).permute(3, 2, 0, 1).contiguous()
    B, H, W = x.shape
    n = B * H * W
    bc = lambda a: a.view(1, 16, 1, 1)  # noqa: E731
    v0 = torch.nn.functional.conv2d(x[:, None], wt, bias, padding=k // 2)
    inv = torch.rsqrt(bc(var) + EPS)
    xh = (v0 - bc(mean)) * inv
    g = torch.where(xh * bc(gamma) + bc(beta) > 0, dy, torch.zeros_like(dy))
    dv = bc(gamma) * inv * (g - bc(dbeta) / n - xh * bc(dgamma) / n)
    return torch.nn.functional.conv_transpose2d(dv, wt, padding=k // 2)[:, 0]


def kernel_case(H, W, k, B=2, seed=0):
    """Seeded inputs of one kernel case (host arrays).  mean / var are the batch statistics of v0 (f32), the sums are those of bn0's backward in
    float64.  dy is zero wherever the ReLU input lies within 1e-3 of zero, so that no f32 / f64 rounding decides a branch."""
    rng = np.random.default_rng(1000 * k + H + W + seed)
    x = rng.random((B, H, W), dtype=np.float32)
    w0 = (rng.standard_normal((k, k, 1, 16)) / k).astype(np.float32)
    bias = (0.1 * rng.standard_normal(16)).astype(np.float32)
    gamma = (1.0 + 0.2 * rng.standard_normal(16)).astype(np.float32)
    beta = (0.2 * rng.standard_normal(16)).astype(np.float32)
    wt = torch.tensor(w0, dtype=torch.float64).permute(3, 2, 0, 1).contiguous()
    v0 = torch.nn.functional.conv2d(torch.tensor(x, dtype=torch.float64)[:, None], wt, torch.tensor(bias, dtype=torch.float64), padding=k // 2)
    mean = v0.mean(dim=(0, 2, 3)).numpy().astype(np.float32)
    var = v0.var(dim=(0, 2, 3), unbiased=False).numpy().astype(np.float32)
    xh = (v0.numpy() - mean.astype(np.float64).reshape(1, 16, 1, 1)) / np.sqrt(var.astype(np.float64).reshape(1, 16, 1, 1) + EPS)
    z = xh * gamma.astype(np.float64).reshape(1, 16, 1, 1) + beta.astype(np.float64).reshape(1, 16, 1, 1)
    dy = rng.standard_normal((B, 16, H, W)).astype(np.float32)
    dy[np.abs(z) < 1e-3] = 0.0
    g = np.where(z > 0, dy.astype(np.float64), 0.0)
    dbeta, dgamma = g.sum(axis=(0, 2, 3)), (g * xh).sum(axis=(0, 2, 3))
    return dict(x=x, dy=dy, w0=w0, bias=bias, mean=mean, var=var, gamma=gamma, beta=beta, dbeta=dbeta, dgamma=dgamma, k=k)


def _planes(dy, k, pad_value=0.0):
    """[B][16][H][W] -> padded channel-quad planes [B][4][H + 2R][WP][4] with the pads filled with pad_value."""
    B, C, H, W = dy.shape
    R, WP = k // 2, _padded_width(W, k)
    out = np.full((B, 16, H + 2 * R, WP), pad_value, dtype=np.float32)
    out[:, :, R : R + H, :W] = dy
    return np.ascontiguousarray(out.reshape(B, 4, 4, H + 2 * R, WP).transpose(0, 1, 3, 4, 2))


def _launch(case, src, stride, planes, B, H, W):
    from orcai_amd import _native as N

    dev = lambda a, dt=torch.float32: torch.as_tensor(np.asarray(a), dtype=dt).cuda()  # noqa: E731
    t = {n: dev(case[n]) for n in ("bias", "mean", "var", "gamma", "beta")}
    w0 = dev(case["w0"]).contiguous()
    sums = dev(np.concatenate([case["dbeta"], case["dgamma"]]), torch.float64)
    dx = torch.full((B, H, W), float("nan"), device="cuda")
    rc = N.lib().orcai_conv0_bn_bwd_dx(src.data_ptr(), stride, planes.data_ptr(), B, H, W, case["k"], w0.data_ptr(), t["bias"].data_ptr(), t["mean"].data_ptr(),
                                       t["var"].data_ptr(), t["gamma"].data_ptr(), t["beta"].data_ptr(), EPS, sums.data_ptr(), dx.data_ptr(), N.stream_ptr())
    assert rc == 0, rc
    torch.cuda.synchronize()
    return dx


@pytest.mark.parametrize("k", [3, 5, 7])
@pytest.mark.parametrize("H,W", KERNEL_SHAPES)
def test_kernel_matches_its_formula(H, W, k):
    """orcai_conv0_bn_bwd_dx against the header's formula in float64 on the host, from the same in, dy, statistics and sums.  Bar: 8 x the
    deviation of the same formula evaluated in f32 by torch on the CPU from its float64 evaluation on these inputs, measured per kernel size
    over the five shapes: 4.64e-7 (k 3), 7.09e-7 (k 5), 1.05e-6 (k 7) of max|dx|, so the bars are 3.7e-6, 5.7e-6 and 8.4e-6 of max|dx|.  Also: bit-identical between two
    launches, with the pads of dy filled with large finite values, and for the 50 %-overlap view of the snippets."""
    B = 2
    case = kernel_case(H, W, k, B)
    args = {n: case[n] for n in ("w0", "bias", "mean", "var", "gamma", "beta", "dbeta", "dgamma", "k")}
    ref = _formula(case["x"], case["dy"], dtype=torch.float64, **args).numpy()
    f32 = _formula(case["x"], case["dy"], dtype=torch.float32, **args).numpy().astype(np.float64)
    scale = float(np.abs(ref).max())
    src = torch.from_numpy(case["x"]).cuda()
    planes = torch.from_numpy(_planes(case["dy"], k)).cuda()
    dx = _launch(case, src, H * W, planes, B, H, W)
    err = float(np.abs(dx.cpu().numpy().astype(np.float64) - ref).max()) / scale
    print(f"k {k} {H}x{W}: kernel {err:.2e}, torch-CPU f32 {float(np.abs(f32 - ref).max()) / scale:.2e} of max|dx| = {scale:.3e}; bar {KERNEL_BAR[k]:.2e}")
    assert bool(torch.isfinite(dx).all())
    assert err <= KERNEL_BAR[k], (err, KERNEL_BAR[k])
    bits = lambda a: a.contiguous().view(torch.int32)  # noqa: E731
    assert torch.equal(bits(dx), bits(_launch(case, src, H * W, planes, B, H, W)))  # (a)
    assert torch.equal(bits(dx), bits(_launch(case, src, H * W, torch.from_numpy(_planes(case["dy"], k, pad_value=3.0e30)).cuda(), B, H, W)))  # (b)
    if H % 2 == 0:  # (c) snippets that overlap by half: snippet b starts (H / 2) * W floats after snippet b - 1
        rec = torch.from_numpy(np.random.default_rng(k).random(((B + 1) * (H // 2), W), dtype=np.float32)).cuda()
        copied = torch.stack([rec[b * (H // 2) : b * (H // 2) + H] for b in range(B)]).contiguous()
        c2 = dict(case)
        assert torch.equal(bits(_launch(c2, rec, (H // 2) * W, planes, B, H, W)), bits(_launch(c2, copied, H * W, planes, B, H, W)))


def test_kernel_refuses_bad_arguments():
    from orcai_amd import _native as N

    case = kernel_case(16, 12, 3)
    a = torch.zeros(4096, device="cuda")
    s = torch.zeros(32, dtype=torch.float64, device="cuda")
    p = [a.data_ptr()] * 6
    lib = N.lib()
    for B, H, W, k in ((2, 16, 12, 4), (2, 16, 12, 9), (0, 16, 12, 3), (2, 0, 12, 3), (2, 16, -1, 3)):
        assert lib.orcai_conv0_bn_bwd_dx(a.data_ptr(), H * W, a.data_ptr(), B, H, W, k, *p, EPS, s.data_ptr(), a.data_ptr(), N.stream_ptr()) == N.E_BADARG
    assert case["k"] == 3


# ------------------------------------------------------------------------------------------------------------------ 2. the whole step
def _inputs(cfg, B, seed, rate):
    """The inputs tests/test_train_full_gpu.py::_run draws for (cfg, B, seed)."""
    p = M.calibrated_params(seed=seed, **cfg)
    rng = np.random.default_rng(seed)
    for k in p:
        if k.endswith(("gamma", "beta")):
            p[k] = (p[k] + 0.2 * rng.standard_normal(p[k].shape)).astype(np.float32)
    H, W, _ = cfg["input_shape"]
    steps = H // 2 ** len(cfg["filters"])
    L, u = cfg["num_labels"], cfg["lstm_units"]
    x = rng.random((B, H, W, 1), dtype=np.float32)
    y = (rng.random((B, steps, L)) > 0.5).astype(np.float32)
    y[0, :, 0] = -1.0
    masks = {k: (rng.random((B, steps, d)) > rate).astype(np.float32) for k, d in (("drop1", 2 * u), ("drop2", 2 * u), ("drop3", 128))}
    return p, x, y, masks


def _oracle_dx(p_np, x, y, masks_np, rate, forced_np=None, conv1d=False):
    """dL/dx of the float64 oracle: oracle.train_ref's forward with x requiring grad (masked BCE + L2 for ResNetLSTM, masked BCE for ResNet1DConv)."""
    dt = torch.float64
    p = {k: torch.tensor(np.asarray(v), dtype=dt) for k, v in p_np.items()}
    n_blocks = sum(1 for k in p if k.endswith("/res/kernel"))
    masks = None if masks_np is None else {k: torch.tensor(v, dtype=dt) for k, v in masks_np.items()}
    xt = torch.tensor(x, dtype=dt, requires_grad=True)
    if conv1d:
        probs, _ = T.forward_train_1dconv(p, xt, masks, rate, n_blocks)
    else:
        forced = None if forced_np is None else {k: torch.tensor(np.asarray(v), dtype=torch.int64 if k.startswith("pool/") else dt) for k, v in forced_np.items()}
        probs, _ = T.forward_train(p, xt, masks, rate, n_blocks, forced)
    T.masked_bce(torch.tensor(y, dtype=dt), probs).backward()  # (the L2 term does not depend on x)
    return xt.grad.numpy()[..., 0]


def _lstm_step(cfg, B, seed, rate=0.5, with_dx=True, record=False):
    from orcai_amd.architectures import ResNetLSTM
    from orcai_amd.training import Trainer

    p, x, y, masks = _inputs(cfg, B, seed, rate)
    H, W, _ = cfg["input_shape"]
    model = ResNetLSTM(cfg["input_shape"], cfg["num_labels"], list(cfg["filters"]), cfg["kernel_size"], rate, cfg["lstm_units"])
    model.set_weights_dict(p)
    tr = Trainer(model, learning_rate=1e-3)
    if record:
        tr.trunk.lib = RecordingLib(tr.trunk.lib)
    dx = torch.full((B, H, W), float("nan"), device="cuda") if with_dx else None
    xd = torch.from_numpy(np.ascontiguousarray(x[..., 0])).cuda().view(-1)
    out = tr.forward_backward(xd, H * W, B, torch.from_numpy(y).cuda(), masks={k: torch.from_numpy(v).cuda() for k, v in masks.items()}, dx=dx)
    tr._test_inputs = (p, x, y, masks, rate)
    return tr, out, dx


def _same_weight_gradients(a, b):
    """The existing bar of test_gradients_match_the_trainer: 1e-5 of each tensor's max-abs (float atomics reorder)."""
    for n, (o, k, _) in a.P.offsets.items():
        ga, gb = a.P.g[o : o + k], b.P.g[o : o + k]
        scale = float(gb.abs().max())
        assert float((ga - gb).abs().max()) <= 1e-5 * scale, n


STEP_CONFIGS = [
    (dict(input_shape=(32, 12, 1), filters=(10, 20), kernel_size=3, lstm_units=64, num_labels=3), 3),
    (dict(input_shape=(32, 16, 1), filters=(10, 20), kernel_size=5, lstm_units=64, num_labels=2), 2),
    (dict(input_shape=(16, 120, 1), filters=(20, 24), kernel_size=3, lstm_units=64, num_labels=3), 2),
    (dict(input_shape=(48, 21, 1), filters=(12, 30, 40), kernel_size=7, lstm_units=64, num_labels=7), 2),
]


@pytest.mark.parametrize("cfg,B", STEP_CONFIGS, ids=["k3", "k5", "wide", "k7"])
def test_step_input_gradient_vs_autograd(cfg, B):
    """ResNetLSTM, Dropout 0.5 with explicit masks, seed 5, free-running float64 oracle: max|dx - ref| <= 5e-4 max|ref| (the project's gradient
    bar without its floor); the weight gradients of the step with dx equal those of a step without it to 1e-5 of each tensor's max."""
    tr, out, dx = _lstm_step(cfg, B, seed=5)
    p, x, y, masks, rate = tr._test_inputs
    ref = _oracle_dx(p, x, y, masks, rate)
    got = dx.cpu().numpy().astype(np.float64)
    scale = float(np.abs(ref).max())
    err = float(np.abs(got - ref).max()) / scale
    print(f"k {cfg['kernel_size']} {cfg['input_shape'][:2]}: max|dx - ref| / max|ref| = {err:.2e}, max|ref| = {scale:.2e}")
    assert np.isfinite(got).all() and err <= 5e-4, err
    other, _, _ = _lstm_step(cfg, B, seed=5, with_dx=False)
    _same_weight_gradients(tr, other)


def test_step_input_gradient_resnet1dconv():
    """ResNet1DConv (rate 0), seed 6, the inputs of test_resnet_1dconv_training_step_vs_autograd: the same bar."""
    from orcai_amd.architectures import FINAL_FILTERS, ResNet1DConv
    from orcai_amd.training import Trainer

    cfg = dict(input_shape=(48, 21, 1), filters=(12, 30, 40), kernel_size=3, lstm_units=64, num_labels=5)
    p = M.calibrated_params(seed=6, **cfg)
    p = {k: v for k, v in p.items() if not k.startswith(("lstm", "dense", "bn_d"))}
    rng = np.random.default_rng(6)
    for k in p:
        if k.endswith(("gamma", "beta")):
            p[k] = (p[k] + 0.2 * rng.standard_normal(p[k].shape)).astype(np.float32)
    L = cfg["num_labels"]
    p["conv1d/kernel"] = (0.1 * rng.standard_normal((FINAL_FILTERS, FINAL_FILTERS, L))).astype(np.float32)
    p["conv1d/bias"] = (0.1 * rng.standard_normal(L)).astype(np.float32)
    B, (H, W, _) = 3, cfg["input_shape"]
    x = rng.random((B, H, W, 1), dtype=np.float32)
    y = (rng.random((B, H // 8, L)) > 0.5).astype(np.float32)
    y[1, :, 2] = -1.0
    ref = _oracle_dx(p, x, y, None, 0.0, conv1d=True)
    grads = []
    for with_dx in (True, False):
        model = ResNet1DConv(cfg["input_shape"], L, list(cfg["filters"]), 3, 0.0)
        model.set_weights_dict(p)
        tr = Trainer(model, learning_rate=1e-3)
        dx = torch.full((B, H, W), float("nan"), device="cuda") if with_dx else None
        tr.forward_backward(torch.from_numpy(np.ascontiguousarray(x[..., 0])).cuda().view(-1), H * W, B, torch.from_numpy(y).cuda(), masks=None, dx=dx)
        grads.append((tr, dx))
    got = grads[0][1].cpu().numpy().astype(np.float64)
    scale = float(np.abs(ref).max())
    err = float(np.abs(got - ref).max()) / scale
    print(f"ResNet1DConv: max|dx - ref| / max|ref| = {err:.2e}, max|ref| = {scale:.2e}")
    assert err <= 5e-4, err
    _same_weight_gradients(grads[0][0], grads[1][0])


def test_trainer_refuses_a_wrong_dx():
    from orcai_amd.architectures import ResNetLSTM
    from orcai_amd.training import Trainer

    cfg, B = STEP_CONFIGS[0]
    tr, _, _ = _lstm_step(cfg, B, seed=5, with_dx=False)
    H, W, _ = cfg["input_shape"]
    x = torch.rand(B * H * W, device="cuda")
    y = torch.zeros((B, 8, 3), device="cuda")
    for bad in (torch.empty((B, H, W + 1), device="cuda"), torch.empty((B, H, W), device="cuda", dtype=torch.float64), torch.empty((B, H, W)),
                torch.empty((B, W, H), device="cuda").transpose(1, 2)):
        with pytest.raises(ValueError, match="dx must be"):
            tr.forward_backward(x, H * W, B, y, masks=None, dx=bad)
    tr.forward_backward(x, H * W, B, y, masks=None)  # nothing was left open
    half = Trainer(ResNetLSTM(cfg["input_shape"], 3, [10, 20], 3, 0.0, 64, precision="f16"), learning_rate=1e-3)
    with pytest.raises(NotImplementedError, match="f16"):
        half.forward_backward(x, H * W, B, y, masks=None, dx=torch.empty((B, H, W), device="cuda"))


# ------------------------------------------------------------------------------------------------------------------ 3. the benchmarked shape
# Measured on the MI355X: branch-matched max|dx - ref| / max|ref| = 9.45e-7 (max|ref| 1.01e-2); torch-CPU f32 on its own branches: 0.9e-6 .. 1.2e-6.
# 4 x the measured value is far below the 5e-4 the project accepts for this step's gradients, so 4 x it is the bar.
V1_MATCHED_BAR = 4 * 9.45e-7
def test_input_gradient_at_the_benchmarked_shape(monkeypatch):
    """orcai-V1 (736 x 171, 30/40/50/60, k 3, 128 units, dropout 0.5 with fixed masks), B = 2, the inputs of _run(cfg, 2, seed=11).
    (a) the launch record: orcai_conv0_bn_bwd_dx once with rc 0 when dx is given, never without; the launch sequence the existing test pins holds
    with dx.  (b) against the float64 oracle on the branches the GPU took (forced masks built by test_train_full_gpu._branch_matched_reference,
    imported): max|dx - ref| <= 3.8e-6 max|ref| (measured 9.45e-7; V1_MATCHED_BAR).  (c) against the free-running oracle: the share of pixels off by more than 5e-4 max|ref| is at
    most 1e-2 (torch-CPU f32 itself: 2.65e-3 at this seed; measured here 6.4e-5, worst pixel 5.8e-3 of max); share and worst pixel are printed."""
    import test_train_full_gpu as full

    cfg = dict(input_shape=(736, 171, 1), filters=(30, 40, 50, 60), kernel_size=3, lstm_units=128, num_labels=7)
    tr, out, dx = _lstm_step(cfg, 2, seed=11, record=True)
    rec = tr.trunk.lib
    tr.trunk.lib = rec._lib
    assert rec.rcs("orcai_conv0_bn_bwd_dx") == [0]
    assert rec.rcs("orcai_sepconv_planes_stats") == [0] * 4 and rec.rcs("orcai_sepconv_planes_stats_bn") == [0] * 4
    assert rec.rcs("orcai_conv0_stats_march") == [0] and rec.rcs("orcai_dw_bwd_fused_conv0") == [0] and rec.rcs("orcai_conv0_bn_bwd_x_ready") == [0]
    assert not rec.rcs("orcai_conv0_bn_bwd_x") and not rec.rcs("orcai_bn_planes_apply") and not rec.rcs("orcai_dw_wgrad") and not rec.rcs("orcai_dw_wgrad_bn")
    assert rec.rcs("orcai_dw_bwd_fused") == [0] * 8 and rec.rcs("orcai_pool_bwd_bn_bias") == [0] * 4
    names = [n for n, _, _ in rec.calls]
    assert names.index("orcai_conv0_bn_bwd_dx") == names.index("orcai_conv0_bn_bwd_x_ready") + 1  # directly after the entry conv's weight gradient
    p, x, y, masks, rate = tr._test_inputs
    got = dx.cpu().numpy().astype(np.float64)
    free = _oracle_dx(p, x, y, masks, rate)
    captured = {}
    monkeypatch.setattr(full.T, "loss_and_grads", lambda *a, forced_np=None, **kw: captured.setdefault("forced", forced_np))
    full._branch_matched_reference(tr)  # builds `forced` from the tensors the forward stored; the patched oracle call only hands it over
    monkeypatch.undo()
    matched = _oracle_dx(p, x, y, masks, rate, forced_np=captured["forced"])
    scale = float(np.abs(matched).max())
    err = float(np.abs(got - matched).max()) / scale
    fscale = float(np.abs(free).max())
    d = np.abs(got - free) / fscale
    share, worst = float((d > 5e-4).mean()), float(d.max())
    print(f"orcai-V1 dx: branch-matched max|dx - ref| / max|ref| = {err:.2e} (max|ref| {scale:.2e}); free-running: share of pixels beyond 5e-4 = {share:.2e}, worst pixel {worst:.2e}")
    assert err <= V1_MATCHED_BAR, err
    assert share <= 1e-2, (share, worst)
    other, _, _ = _lstm_step(cfg, 2, seed=11, with_dx=False, record=True)
    assert other.trunk.lib.rcs("orcai_conv0_bn_bwd_dx") == [] and other.trunk.lib.rcs("orcai_conv0_bn_bwd_x_ready") == [0]
    assert [n for n, _, _ in other.trunk.lib.calls] == [n for n in names if n != "orcai_conv0_bn_bwd_dx"]
    _same_weight_gradients(tr, other)


# ------------------------------------------------------------------------------------------------------------------ 4. the ops
def _ops_helpers():
    import test_torch_ops_gpu as G

    return G


# Two runs of ONE path differ for ResNetLSTM: its head's backward accumulates with float atomics, so the gradient entering the trunk -- and with it
# dr1 and dx -- moves in its last bits from run to run.  Measured with two fresh Trainers on the same inputs and the same upstream gradient
# (three runs each): dr1 differs by 2.0e-7 .. 2.7e-7 and dx by 2.5e-7 .. 4.85e-7 of their max-abs for lstm_k3 (rate 0 and 0.5) and lstm_k5,
# while for ResNet1DConv (no atomics upstream of dr1) dr1 and dx are bit-identical.  Bit-for-bit equality of the op and the trainer is
# therefore asserted where the trainer equals itself bit for bit (ResNet1DConv: k = 3, the marching kernel); for ResNetLSTM the bar is
# 8 x the trainer's own worst run-to-run spread, 3.9e-6 of max|dx|.
TRAINER_RUN_TO_RUN = 4.85e-7


@pytest.mark.parametrize("idx,rate", [(0, 0.5), (1, 0.0), (2, 0.0), (3, 0.0)], ids=["lstm_k3", "lstm_k5", "lstm_k7", "conv1d_k3"])
def test_op_input_gradient_equals_the_trainer(idx, rate):
    """torch.autograd.grad of a torch-written loss through forward_wrt_input w.r.t. x against Trainer.backward_from_probs(..., dx=...): bit for
    bit for ResNet1DConv, within 8 x the trainer's own run-to-run spread for ResNetLSTM (see TRAINER_RUN_TO_RUN); w.r.t. the weights it
    matches the trainer's fused loss as in test_gradients_match_the_trainer."""
    from orcai_amd.torch_ops import OrcaiModule, model_config
    from orcai_amd.training import Trainer

    G = _ops_helpers()
    name, cfg, B = G.SMALL[idx]
    model = G.make(cfg, rate=rate)
    m = OrcaiModule(model, input_grad=True).cuda()
    H, W = model.input_hw
    x = torch.rand((B, H, W), device="cuda")
    y = G._labels(model, B, 2)
    xr = x.clone().requires_grad_()
    probs = torch.ops.orcai.forward_wrt_input(xr, m.weights_list(), m.stats_list(), model_config(model), True, 7)
    grads = torch.autograd.grad(G._torch_loss(model, m, probs, y), [xr] + list(m.parameters()))
    # the trainer, split at the probabilities, from the same upstream gradient
    tr = Trainer(G.make(cfg, rate=rate), learning_rate=1e-3, seed=7)
    p2 = tr.forward_train(x.reshape(-1), H * W, B)
    assert G.same_bits(p2, probs.detach())
    leaf = p2.detach().clone().requires_grad_()
    m2 = OrcaiModule(G.make(cfg, rate=rate)).cuda()
    (dprobs,) = torch.autograd.grad(G._torch_loss(model, m2, leaf, y), leaf)
    dx = torch.empty((B, H, W), device="cuda")
    tr.backward_from_probs(dprobs, p2, dx=dx)
    scale = float(dx.abs().max())
    dev = float((grads[0] - dx).abs().max()) / scale
    print(f"{name}: op vs trainer max|ddx| / max|dx| = {dev:.2e}")
    assert scale > 0
    if "lstm_units" in cfg:
        assert dev <= 8 * TRAINER_RUN_TO_RUN, dev
    else:
        assert G.same_bits(grads[0], dx)
    full, _ = G._trainer_step(G.make(cfg, rate=rate), x, y, seed=7)
    for (n, _), g in zip(m.named_parameters(), grads[1:]):
        ref = full.P.G(n.replace("__", "/"))
        scale = float(ref.abs().max())
        assert float((g - ref).abs().max()) <= 1e-5 * scale, n


def test_input_gradient_with_frozen_weights_and_misuse():
    from orcai_amd.torch_ops import OrcaiModule

    G = _ops_helpers()
    name, cfg, B = G.SMALL[0]
    model = G.make(cfg)
    m = OrcaiModule(model, input_grad=True).cuda().train().requires_grad_(False)
    H, W = model.input_hw
    x = torch.rand((B, H, W), device="cuda", requires_grad=True)
    m(x).sum().backward()
    assert x.grad is not None and x.grad.shape == x.shape and float(x.grad.abs().max()) > 0 and all(p.grad is None for p in m.parameters())
    # the old op keeps its refusal, also through the module
    plain = OrcaiModule(model).cuda().train()
    with pytest.raises(NotImplementedError, match="no gradient w.r.t. its input"):
        plain(x)
    # one open step, across the two ops
    first = m(x)
    with pytest.raises(RuntimeError, match="not been backpropagated"):
        plain(x.detach())
    first.sum().backward()
    second = plain(x.detach())
    with pytest.raises(RuntimeError, match="not been backpropagated"):
        m(x)
    second.sum().backward()
    # eval mode has no backward, for the input neither
    out = m.eval()(x)
    with pytest.raises(RuntimeError, match="training=False"):
        out.sum().backward()


def test_opcheck_new_ops():
    from torch.library import opcheck

    from orcai_amd.torch_ops import OrcaiModule, model_config

    G = _ops_helpers()
    name, cfg, B = G.SMALL[0]
    model = G.make(cfg)
    m = OrcaiModule(model).cuda()
    H, W = model.input_hw
    c = model_config(model)
    x = torch.rand((B, H, W), device="cuda")
    ws = [w.detach().clone() for w in m.weights_list()]
    stats = lambda: [s.clone() for s in m.stats_list()]  # noqa: E731
    opcheck(torch.ops.orcai.forward_wrt_input.default, (x, ws, stats(), c, False, 0))
    # the same split as test_torch_ops_gpu.test_opcheck: the schema and fake-tensor checks keep two real results alive at once, which with
    # tensors that require grad is the misuse the op refuses; they run without grad, the autograd registration check with x requiring it
    opcheck(torch.ops.orcai.forward_wrt_input.default, (x.clone().requires_grad_(), ws, stats(), c, True, 3), test_utils=("test_autograd_registration",))
    opcheck(torch.ops.orcai.forward_wrt_input.default, (x, ws, stats(), c, True, 3), test_utils=("test_schema", "test_faketensor"))
    # the backward op consumes the open step (one real call per check), and opcheck hands it copies of its arguments: the op accepts
    # probabilities EQUAL to the open step's
    for util in ("test_schema", "test_faketensor", "test_autograd_registration"):
        with torch.no_grad():
            probs = torch.ops.orcai.forward_wrt_input(x, ws, stats(), c, True, 3)
        opcheck(torch.ops.orcai.forward_wrt_input_backward.default, (torch.ones_like(probs), probs, c), test_utils=(util,))


def test_learnable_gain_in_front_of_a_frozen_detector_learns():
    """Ten steps of gradient descent on a per-frequency gain in front of a frozen OrcaiModule(input_grad=True), Dropout rate 0, one fixed batch:
    the loss is a deterministic function of the gain.  The step is 0.02 along the gradient normalised by its largest component (each gain
    moves by at most 2 % per step); with it the float64 oracle's loss falls at every one of ten steps for this configuration and these weights
    on a batch drawn the same way (0.733 -> 0.664)."""
    from orcai_amd.torch_ops import OrcaiModule

    G = _ops_helpers()
    name, cfg, B = G.SMALL[0]
    model = G.make(cfg)
    net = OrcaiModule(model, input_grad=True).cuda().train().requires_grad_(False)
    H, W = model.input_hw
    g = torch.Generator(device="cuda").manual_seed(4)
    x = torch.rand((B, H, W), device="cuda", generator=g)
    y = G._labels(model, B, 3)
    gain = torch.ones(W, device="cuda", requires_grad=True)
    losses = []
    for _ in range(10):
        q = net(x * gain).clamp(1e-7, 1 - 1e-7)
        mask = (y != -1.0).float()
        loss = (-(y * q.log() + (1 - y) * (1 - q).log()) * mask).sum() / mask.sum()
        (dg,) = torch.autograd.grad(loss, gain)
        losses.append(float(loss.detach()))
        with torch.no_grad():
            gain -= 0.02 * dg / dg.abs().max()
    print("gain training:", [f"{v:.5f}" for v in losses])
    assert all(math.isfinite(v) for v in losses) and losses[-1] < losses[0], losses


def test_compiled_input_gradient_equals_eager():
    """torch.compile(backend="aot_eager", fullgraph=True) of forward_wrt_input(training=True) behind a gain, run on the device: loss and the
    gain's gradient (which exists only through dL/dx) equal eager bit for bit (ResNet1DConv: its backward is bit-reproducible, see
    TRAINER_RUN_TO_RUN)."""
    from orcai_amd.torch_ops import OrcaiModule

    G = _ops_helpers()
    name, cfg, B = G.SMALL[3]
    model = G.make(cfg)
    net = OrcaiModule(model).cuda()
    H, W = model.input_hw
    ws, st, c = [w.detach() for w in net.weights_list()], net.stats_list(), net.config
    x = torch.rand((B, H, W), device="cuda")

    def f(x, gain, stats):
        y = torch.ops.orcai.forward_wrt_input(x * gain, ws, stats, c, True, 5)
        return (y * y).sum()

    res = []
    for fn in (f, torch.compile(f, backend="aot_eager", fullgraph=True)):
        gain = torch.linspace(0.5, 1.5, W, device="cuda").requires_grad_()
        loss = fn(x, gain, [s.clone() for s in st])
        loss.backward()
        res.append((loss.detach(), gain.grad))
    assert G.same_bits(res[0][0], res[1][0]) and G.same_bits(res[0][1], res[1][1])
