"""GPU parity of one full training step (forward in training mode, masked BCE + L2, backward through the whole ResNetLSTM)
against torch autograd on the CPU oracle in float64, for small hyper-parameter variants, and of an Adam step.

Tolerance: every gradient tensor max|delta| <= 5e-4 * max(1e-3, max|ref|): fp32 kernels (float atomics in the weight-gradient
reductions) vs fp64 autograd; the bias gradients of convs that feed a BatchNorm are mathematically zero (BN removes the mean)
and are compared on an absolute scale instead."""

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from oracle import model_ref as M  # noqa: E402
from oracle import train_ref as T  # noqa: E402
from recording_lib import RecordingLib  # noqa: E402


def _run(cfg, B, seed, rate=0.5, record=False, dx=None, negate_odd_gamma=False):
    from orcai_amd.architectures import ResNetLSTM
    from orcai_amd.training import Trainer

    p = M.calibrated_params(seed=seed, **cfg)
    rng = np.random.default_rng(seed)
    for k in p:
        if k.endswith(("gamma", "beta")):
            p[k] = (p[k] + 0.2 * rng.standard_normal(p[k].shape)).astype(np.float32)
    if negate_odd_gamma:  # gamma < 0 on every odd channel of every BatchNorm: the pooling tails take the window minimum there, the backward its arg-min
        for k in p:
            if k.endswith("gamma"):
                p[k][1::2] *= -1.0
    H, W, _ = cfg["input_shape"]
    steps = H // 2 ** len(cfg["filters"])
    L, u = cfg["num_labels"], cfg["lstm_units"]
    x = rng.random((B, H, W, 1), dtype=np.float32)
    y = (rng.random((B, steps, L)) > 0.5).astype(np.float32)
    y[0, :, 0] = -1.0
    masks = {k: (rng.random((B, steps, d)) > rate).astype(np.float32) for k, d in (("drop1", 2 * u), ("drop2", 2 * u), ("drop3", 128))}
    ref = T.loss_and_grads(p, x, y, masks, rate)
    model = ResNetLSTM(cfg["input_shape"], L, list(cfg["filters"]), cfg["kernel_size"], rate, u)
    model.set_weights_dict(p)
    tr = Trainer(model, learning_rate=1e-3)
    if record:
        tr.trunk.lib = RecordingLib(tr.trunk.lib)
    xd = torch.from_numpy(np.ascontiguousarray(x[..., 0])).cuda().view(-1)
    extra = {} if dx is None else {"dx": dx}
    out = tr.forward_backward(xd, H * W, B, torch.from_numpy(y).cuda(), masks={k: torch.from_numpy(v).cuda() for k, v in masks.items()}, **extra)
    tr._test_inputs = (p, x, y, masks, rate)
    return ref, tr, out, p


@pytest.mark.parametrize(
    "cfg,B,negate_odd_gamma",
    [
        (dict(input_shape=(32, 12, 1), filters=(10, 20), kernel_size=3, lstm_units=64, num_labels=3), 3, False),
        (dict(input_shape=(48, 21, 1), filters=(12, 30, 40), kernel_size=3, lstm_units=64, num_labels=7), 2, False),
        (dict(input_shape=(32, 16, 1), filters=(10, 20), kernel_size=5, lstm_units=64, num_labels=2), 2, False),
        # a first block wide enough for the strip-tile kernels (BatchNorm statistics reduced in the separable convs' epilogue)
        (dict(input_shape=(16, 120, 1), filters=(20, 24), kernel_size=3, lstm_units=64, num_labels=3), 2, False),
        # B * 8 = 320 rows in the head's weight-gradient GEMMs: split-K, its zero fill meeting the Trainer's pre-cleared accumulator arena
        (dict(input_shape=(32, 12, 1), filters=(10, 20), kernel_size=3, lstm_units=64, num_labels=3), 40, False),
        # gamma < 0 on every odd channel: the forward pools the window minimum there and the backward routes to its arg-min
        (dict(input_shape=(48, 21, 1), filters=(12, 30, 40), kernel_size=3, lstm_units=64, num_labels=7), 2, True),
    ],
    ids=["cfg0-3", "cfg1-2", "cfg2-2", "cfg3-2", "cfg4-40", "negative_gamma"],  # the earlier cases keep their ids
)
def test_full_step_gradients_vs_autograd(cfg, B, negate_odd_gamma):
    ref, tr, out, p = _run(cfg, B, seed=5, negate_odd_gamma=negate_odd_gamma)
    if negate_odd_gamma:
        assert all((p[f"b{i}/bn_b/gamma"][1::2] < 0).all() for i in (1, 2, 3))
    _check_step(ref, tr, out)


def _from_quad_planes(t, C, H, W, ksize):
    """[B][CQ][H+2R][WP][4] padded channel-quad planes -> [B][C][H][W] float64."""
    R = ksize // 2
    Bq, CQ, HP, WP, _ = t.shape
    return t.permute(0, 1, 4, 2, 3).reshape(Bq, CQ * 4, HP, WP)[:, :C, R : R + H, :W].double().cpu().numpy()


def _branch_matched_reference(tr):
    """The float64 oracle's loss and gradients on the piecewise-linear branch the GPU's f32 forward took.  At 736 x 171 a handful of the 2e8
    ReLU inputs / pooling candidates of a step lie within f32 rounding of zero / of each other; f32 arithmetic (this path, and torch-CPU f32
    autograd alike) then takes the other branch than float64, and ONE such flip reroutes one element's gradient and moves a weight gradient
    by ~1 / sqrt(pixels) of its size (tools/debug_v1_grads.py: three flips explain every deviation of f32 CPU autograd from float64 at this
    shape, and with them forced the two agree to 2e-5).  The branches are read from the tensors the forward stored: ReLU masks from y0, the
    block outputs, bn_f's and dense1's rectified tensors; bn_a's from y_a, materialised here by the orcai_bn_planes_apply launch whose value
    the on-load BatchNorm of the fused kernels reproduces bit for bit (tests/test_train_fused_gpu.py); pooling selections from v_b
    (first maximal element of sign(gamma) * v in window scan order, the kernels' rule)."""
    p, x, y, masks, rate = tr._test_inputs
    return T.loss_and_grads(p, x, y, masks, rate, forced_np=_forced_branches(tr))


def _forced_branches(tr):
    """The ReLU masks and pooling selections of the step `tr` just ran, in the form oracle.train_ref takes as `forced_np`."""
    from oracle.model_ref import same_pad

    p, x, y, masks, rate = tr._test_inputs
    m, k = tr.model, tr.model.kernel_size
    buf, shapes = tr.trunk.buf, m.stage_shapes()
    B = x.shape[0]
    H, W = m.input_hw
    forced = {}
    y0 = _from_quad_planes(buf["y0"], 16, H, W, k)
    forced["relu/bn0"] = forced["relu/b1/in"] = (y0 > 0).astype(np.float64)
    cprev = 16
    for i, c in enumerate(m.filters, start=1):
        h, w, _ = shapes[i - 1]
        if i > 1:
            forced[f"relu/b{i}/in"] = (_from_quad_planes(buf[f"prev{i - 1}"], cprev, h, w, k) > 0).astype(np.float64)
        tr.trunk._bn_apply(buf[f"va{i}"], f"b{i}/bn_a", c, h, w, 1, buf[f"ya{i}"])  # y_a as the kernels formed it on load
        forced[f"relu/b{i}/bn_a"] = (_from_quad_planes(buf[f"ya{i}"], c, h, w, k) > 0).astype(np.float64)
        sgn = np.where(tr.P.W(f"b{i}/bn_b/gamma").cpu().numpy() < 0, -1.0, 1.0)
        sv = _from_quad_planes(buf[f"vb{i}"], c, h, w, k) * sgn[None, :, None, None]
        _, pt, pb = same_pad(h, 3, 2)
        _, pl, pr = same_pad(w, 2, 2)
        svp = np.pad(sv, ((0, 0), (0, 0), (pt, pb), (pl, pr)), constant_values=-np.inf)
        ho, wo = shapes[i][0], shapes[i][1]
        win = np.stack([svp[:, :, dy : dy + 2 * ho : 2, dx : dx + 2 * wo : 2] for dy in range(3) for dx in range(2)], axis=-1)
        forced[f"pool/b{i}"] = np.argmax(win, axis=-1)
        cprev = c
    hc = tr.head.cache
    hl, wl, _ = shapes[-1]
    forced["relu/bn_f"] = (hc["x1"].cpu().numpy().reshape(B, hl, wl, -1).transpose(0, 3, 1, 2) > 0).astype(np.float64)
    forced["relu/dense1"] = (hc["pre1"].cpu().numpy() > 0).astype(np.float64)
    return forced


def _check_step(ref, tr, out):
    acc = out["acc"].cpu().numpy()
    assert np.abs(out["probs"].cpu().numpy() - ref["probs"]).max() <= 5e-6
    assert abs(acc[0] / acc[1] - ref["bce"]) <= 2e-6 * max(1.0, abs(ref["bce"]))
    assert abs(acc[0] / acc[1] + acc[3] - ref["loss"]) <= 2e-6 * max(1.0, abs(ref["loss"]))
    bad = {}
    for name, g in ref["grads"].items():
        got = tr.P.G(name).cpu().numpy()
        zero_mean_bias = name.endswith("/bias") and not name.startswith(("dense2", "lstm", "dense1")) and "res" not in name
        scale = max(1e-3, float(np.abs(g).max())) if not zero_mean_bias else 1.0
        err = float(np.abs(got - g).max()) / scale
        if err > (5e-4 if not zero_mean_bias else 1e-4):
            bad[name] = (err, float(np.abs(g).max()))
    assert not bad, bad
    tr.trunk.update_moving_stats()
    tr.head.update_moving_stats()
    for k, v in ref["new_stats"].items():
        assert np.abs(tr.P.stats[k].cpu().numpy() - v).max() <= 2e-5 * max(1.0, float(np.abs(v).max())), k


def test_full_step_gradients_at_the_benchmarked_shape():
    """The shape bench.py times (BASELINE configs[3]: orcai-V1, 736 x 171, filters 30/40/50/60, k 3, 128 units, dropout 0.5 with fixed
    masks) at B = 2 against float64 autograd, at the bars of the small shapes -- AND a record of which launchers produced the gradients:
    the C launchers pick kernels by shape and answer ORCAI_E_UNSUPPORTED where training.py silently falls back, so this test fails when
    one of the fused passes the benchmark line is made of refuses the benchmarked shape (reference train.py:155-219,
    architectures.py:162-270).  The float64 oracle runs on the branches the f32 forward took (_branch_matched_reference); against the
    free-running oracle the gradients differ by 1e-3 .. 6e-3 -- exactly as torch-CPU f32 autograd does -- which is printed, not asserted."""
    from orcai_amd import _native as N

    cfg = dict(input_shape=(736, 171, 1), filters=(30, 40, 50, 60), kernel_size=3, lstm_units=128, num_labels=7)
    ref, tr, out, p = _run(cfg, 2, seed=11, record=True)
    rec = tr.trunk.lib
    tr.trunk.lib = rec._lib  # (the launches below are the test's own)
    free = {n: float(np.abs(tr.P.G(n).cpu().numpy() - g).max()) / max(1e-3, float(np.abs(g).max())) for n, g in ref["grads"].items()}
    matched = _branch_matched_reference(tr)
    worst = sorted(free.items(), key=lambda kv: -kv[1])[:3]
    print(f"orcai-V1 step vs the free-running float64 oracle: worst {[(n, f'{v:.1e}') for n, v in worst]} (branch flips within f32 rounding: see _branch_matched_reference)")
    assert np.abs(out["probs"].cpu().numpy() - ref["probs"]).max() <= 5e-6  # the forward itself agrees with the free-running oracle
    _check_step(matched, tr, out)
    names = sorted({n for n, _, _ in rec.calls})
    print("launchers of the orcai-V1 training step:", {n: (len(rec.rcs(n)), sum(rc == N.E_UNSUPPORTED for rc in rec.rcs(n))) for n in names})
    # every k = 3 separable conv of the forward on the LDS-tile kernels with the statistics epilogue; the second conv of every block with bn_a on load
    assert rec.rcs("orcai_sepconv_planes_stats") == [0] * 4 and rec.rcs("orcai_sepconv_planes_stats_bn") == [0] * 4
    # the entry conv in two marching passes, its backward with bn0's sums taken inside block 1's marching depthwise backward
    assert rec.rcs("orcai_conv0_stats_march") == [0] and rec.rcs("orcai_dw_bwd_fused_conv0") == [0] and rec.rcs("orcai_conv0_bn_bwd_x_ready") == [0]
    assert not rec.rcs("orcai_conv0_bn_bwd_x") and not rec.rcs("orcai_bn_planes_apply") and not rec.rcs("orcai_dw_wgrad") and not rec.rcs("orcai_dw_wgrad_bn")
    # the marching depthwise backward for the other eight separable convs (sep_f, 2 x blocks 4..2, b1/sep_b)
    assert rec.rcs("orcai_dw_bwd_fused") == [0] * 8
    # BatchNorm backward + du + pointwise weight gradient in one pass on block 1 (the top symbol of the benchmark's profile); wider blocks refuse
    blk1 = [rc for n, rc, a in rec.calls if n == "orcai_bn_bwd_pointwise_wgrad" and (a[5], a[6]) == (736, 171)]
    assert blk1 == [0, 0], blk1
    assert rec.rcs("orcai_pool_bwd_bn_bias") == [0] * 4


WIDE_KERNEL_CONFIGS = [
    # stage widths 171 / 86 / 43: four, two and one 60-column window per row at k = 5; one and two 16-channel output tiles
    (dict(input_shape=(16, 171, 1), filters=(12, 30), kernel_size=5, lstm_units=64, num_labels=3), 2),
    # k = 7 at the sweep's width: row pitch 176, 58 valid columns per 64-pixel window
    (dict(input_shape=(16, 171, 1), filters=(20, 24), kernel_size=7, lstm_units=64, num_labels=3), 2),
    # widths 130 / 65 / 33 / 17 at k = 7, two / three / four output tiles, a final stage of 3 rows
    (dict(input_shape=(24, 130, 1), filters=(30, 40, 50), kernel_size=7, lstm_units=64, num_labels=7), 2),
    # one very wide block, a ragged channel quad (17 = 4 * 4 + 1)
    (dict(input_shape=(8, 300, 1), filters=(17,), kernel_size=5, lstm_units=64, num_labels=2), 3),
]


@pytest.mark.parametrize("cfg,B", WIDE_KERNEL_CONFIGS, ids=["k5_171", "k7_171", "k7_130x3", "k5_300"])
def test_full_step_gradients_wide_kernels(cfg, B):
    """Kernel sizes 5 and 7 -- which the hyper-parameter sweep trains at 736 x 171 (defaults/default_hps_parameter.json) -- on planes
    wider than one 64-pixel window, where the separate launchers TrunkTrainer falls back to for k != 3 need several windows per row:
    window tails, windows crossing a row edge with a 2 / 3 pixel halo, the last window hanging over the row pitch.  Checked as
    test_full_step_gradients_at_the_benchmarked_shape is: probabilities against the free-running float64 oracle, everything else against
    the oracle on the branches the f32 forward took, at _check_step's bars; the free-running deviation is printed.  The launcher record
    shows that the fall-back launchers, and none of the k = 3 marching entry points, produced the result.  For the two (16, 171) shapes
    the step also returns the input gradient, held to test_step_input_gradient_vs_autograd's bar (5e-4 of max|ref|) against the
    free-running oracle's (as that test does) and the branch-matched oracle's."""
    from orcai_amd import _native as N
    from test_input_grad_gpu import _oracle_dx

    H, W, _ = cfg["input_shape"]
    with_dx = (H, W) == (16, 171)
    dx = torch.full((B, H, W), float("nan"), device="cuda") if with_dx else None
    ref, tr, out, p = _run(cfg, B, seed=5, record=True, dx=dx)
    rec = tr.trunk.lib
    tr.trunk.lib = rec._lib  # (the launches below are the test's own)
    free = {n: float(np.abs(tr.P.G(n).cpu().numpy() - g).max()) / max(1e-3, float(np.abs(g).max())) for n, g in ref["grads"].items()}
    worst = sorted(free.items(), key=lambda kv: -kv[1])[:3]
    print(f"k = {cfg['kernel_size']} {cfg['input_shape'][:2]} {cfg['filters']} step vs the free-running float64 oracle: worst {[(n, f'{v:.1e}') for n, v in worst]}")
    names = sorted({n for n, _, _ in rec.calls})
    print("launchers of the training step:", {n: (len(rec.rcs(n)), sum(rc == N.E_UNSUPPORTED for rc in rec.rcs(n))) for n in names})
    matched = _branch_matched_reference(tr)
    assert np.abs(out["probs"].cpu().numpy() - ref["probs"]).max() <= 5e-6  # the forward itself agrees with the free-running oracle
    _check_step(matched, tr, out)
    for name in ("orcai_dw_wgrad", "orcai_sepconv_planes_u", "orcai_bn_planes_stats", "orcai_bn_planes_apply", "orcai_outer_reduce", "orcai_pool_bwd_bn_bias",
                 "orcai_conv0_bn_bwd_x"):
        assert rec.rcs(name) and not any(rec.rcs(name)), (name, rec.rcs(name))
    marching = [n for n in names if n.startswith(("orcai_dw_bwd_fused", "orcai_sepconv_planes_stats")) or n == "orcai_conv0_stats_march"]
    assert not [n for n in marching if 0 in rec.rcs(n)], marching
    if with_dx:
        _, x, y, masks, rate = tr._test_inputs
        free_dx = _oracle_dx(p, x, y, masks, rate)
        want = _oracle_dx(p, x, y, masks, rate, forced_np=_forced_branches(tr))
        got = dx.cpu().numpy().astype(np.float64)
        scale = float(np.abs(want).max())
        err = float(np.abs(got - want).max()) / scale
        free_err = float(np.abs(got - free_dx).max()) / float(np.abs(free_dx).max())
        print(f"k {cfg['kernel_size']} {cfg['input_shape'][:2]}: max|dx - ref| / max|ref| = {err:.2e} (free-running oracle: {free_err:.2e}), max|ref| = {scale:.2e}")
        assert np.isfinite(got).all() and err <= 5e-4 and free_err <= 5e-4, (err, free_err)  # no branch flip at these shapes: the free-running oracle, as in the cited test, holds too


def test_training_reduces_loss_and_roundtrips_weights():
    from orcai_amd.architectures import ResNetLSTM
    from orcai_amd.training import Trainer

    cfg = dict(input_shape=(32, 12, 1), filters=(10, 20), kernel_size=3, lstm_units=64, num_labels=3)
    rng = np.random.default_rng(0)
    model = ResNetLSTM(cfg["input_shape"], 3, [10, 20], 3, 0.0, 64, seed=1)
    tr = Trainer(model, learning_rate=3e-3)
    x = rng.random((8, 32, 12), dtype=np.float32)
    y = (x.reshape(8, 8, 4, 12).mean(axis=(2, 3), keepdims=False)[:, :, None] > 0.5).astype(np.float32).repeat(3, axis=2)
    xd, yd = torch.from_numpy(x).cuda().view(-1), torch.from_numpy(y).cuda()
    losses = []
    for _ in range(30):
        out = tr.train_step(xd, 32 * 12, 8, yd)
        a = out["acc"].cpu().numpy()
        losses.append(a[0] / a[1])
    assert np.isfinite(losses).all() and losses[-1] < 0.7 * losses[0], losses[::5]
    tr.P.to_model(model)
    assert np.isfinite(model.predict(x[..., None])).all()


def _planes_mask_from_nchw(mask, ksize):
    """[B][C][H][W] 0/1 mask -> the padded channel-quad plane layout [B][CQ][H+2R][WP][4] the trunk kernels use."""
    B, C, H, W = mask.shape
    R = ksize // 2
    WP = (W + R + 3) & ~3
    CQ = (C + 3) // 4
    out = np.zeros((B, CQ * 4, H + 2 * R, WP), dtype=np.float32)
    out[:, :C, R : R + H, :W] = mask
    return np.ascontiguousarray(out.reshape(B, CQ, 4, H + 2 * R, WP).transpose(0, 1, 3, 4, 2))


@pytest.mark.parametrize("rate", [0.0, 0.4])
def test_resnet_1dconv_training_step_vs_autograd(rate):
    """SURVEY 8f row 1, training: ResNet1DConv (Dropout after every block -- the residual branch reads the un-dropped tensor --
    and after BN_f, frequency mean, Conv1D head) forward + masked BCE + full backward against torch autograd (float64)."""
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
    steps = H // 8
    x = rng.random((B, H, W, 1), dtype=np.float32)
    y = (rng.random((B, steps, L)) > 0.5).astype(np.float32)
    y[1, :, 2] = -1.0
    model = ResNet1DConv(cfg["input_shape"], L, list(cfg["filters"]), 3, rate)
    model.set_weights_dict(p)
    shapes = model.stage_shapes()
    masks_np, masks_dev = None, None
    if rate > 0:
        masks_np = {f"block{i}": (rng.random((B, shapes[i][2], shapes[i][0], shapes[i][1])) > rate).astype(np.float32) for i in range(1, 4)}
        masks_np["final"] = (rng.random((B, FINAL_FILTERS, shapes[-1][0], shapes[-1][1])) > rate).astype(np.float32)
        masks_dev = {k: torch.from_numpy(_planes_mask_from_nchw(v, 3)).cuda() for k, v in masks_np.items() if k != "final"}
        # after BN_f the tensor is in the Keras Reshape layout [B][T][W*36]: feature = x*36 + c
        masks_dev["final"] = torch.from_numpy(np.ascontiguousarray(masks_np["final"].transpose(0, 2, 3, 1).reshape(B, shapes[-1][0], -1))).cuda()
    ref = T.loss_and_grads_1dconv(p, x, y, masks_np, rate)
    tr = Trainer(model, learning_rate=1e-3)
    out = tr.forward_backward(torch.from_numpy(np.ascontiguousarray(x[..., 0])).cuda().view(-1), H * W, B, torch.from_numpy(y).cuda(), masks=masks_dev)
    acc = out["acc"].cpu().numpy()
    assert np.abs(out["probs"].cpu().numpy() - ref["probs"]).max() <= 5e-6
    assert abs(acc[0] / acc[1] - ref["loss"]) <= 2e-6 * max(1.0, abs(ref["loss"])) and acc[3] == 0.0
    bad = {}
    for name, g in ref["grads"].items():
        got = tr.P.G(name).cpu().numpy()
        zero_mean_bias = name.endswith("/bias") and "res" not in name and not name.startswith("conv1d")
        scale = max(1e-3, float(np.abs(g).max())) if not zero_mean_bias else 1.0
        err = float(np.abs(got - g).max()) / scale
        if err > (5e-4 if not zero_mean_bias else 1e-4):
            bad[name] = err
    assert not bad, bad
    # Adam + moving statistics run for this architecture as well
    tr.apply()
    assert bool(torch.isfinite(tr.P.w).all())


def test_multi_step_trajectory_matches_oracle():
    """Four optimisation steps (forward in training mode, backward, Keras-3 Adam, BN moving statistics) on the GPU against the same
    four steps done with the CPU oracle (autograd gradients + adam_step_ref): weights, Adam slots and moving statistics stay together.
    Zero-mean bias gradients are float noise in the oracle and exactly 0 here; Adam turns noise into O(lr) steps, so those biases
    (which BatchNorm makes irrelevant to the function) are excluded from the weight comparison."""
    from orcai_amd.architectures import ResNetLSTM
    from orcai_amd.training import Trainer

    cfg = dict(input_shape=(32, 12, 1), filters=(10, 20), kernel_size=3, lstm_units=64, num_labels=3)
    p = M.calibrated_params(seed=3, **cfg)
    rng = np.random.default_rng(3)
    B, lr = 4, 1e-3
    xs = [rng.random((B, 32, 12, 1), dtype=np.float32) for _ in range(4)]
    ys = [(rng.random((B, 8, 3)) > 0.5).astype(np.float32) for _ in range(4)]
    model = ResNetLSTM(cfg["input_shape"], 3, [10, 20], 3, 0.0, 64)
    model.set_weights_dict(p)
    tr = Trainer(model, learning_rate=lr)
    w = {k: np.asarray(v, dtype=np.float64) for k, v in p.items()}
    m = {k: np.zeros_like(v) for k, v in w.items() if T.is_trainable(k)}
    v2 = {k: np.zeros_like(v) for k, v in w.items() if T.is_trainable(k)}
    for step in range(4):
        ref = T.loss_and_grads(w, xs[step], ys[step], None, 0.0)
        for k, g in ref["grads"].items():
            w[k], m[k], v2[k] = T.adam_step_ref(w[k], g, m[k], v2[k], step + 1, lr)
        for k, s in ref["new_stats"].items():
            w[k] = s
        out = tr.train_step(torch.from_numpy(np.ascontiguousarray(xs[step][..., 0])).cuda().view(-1), 32 * 12, B, torch.from_numpy(ys[step]).cuda())
        acc = out["acc"].cpu().numpy()
        assert abs(acc[0] / acc[1] + acc[3] - ref["loss"]) <= 1e-4 * max(1.0, abs(ref["loss"])), (step, acc, ref["loss"])
    tr.P.to_model(model)
    worst = {}
    for k, want in w.items():
        zero_mean_bias = k.endswith("/bias") and not k.startswith(("dense2", "lstm", "dense1")) and "res" not in k
        if zero_mean_bias:
            continue
        got = model.weights[k].astype(np.float64)
        err = float(np.abs(got - want).max()) / max(1e-2, float(np.abs(want).max()))
        if err > 2e-3:  # four Adam steps of size lr = 1e-3 each: a sign flip of a near-zero gradient moves a weight by up to 2 lr
            worst[k] = err
    assert not worst, worst


def test_training_step_replays_as_one_hip_graph_with_epilogue_stats():
    """The whole step (dropout masks, forward with the BatchNorm statistics in the conv epilogues, loss, backward, Adam, BatchNorm moving
    statistics, step counter) captured once as a hipGraph and replayed: the per-step state lives in device memory (Trainer.counter,
    lr_dev), so replays draw fresh dropout masks, advance Adam's bias correction and honour a learning-rate change made between replays.
    (1) Step by step: before every step the eager trainer's state is copied into the graph trainer; one step each on the same batch must
    give the same loss and batch statistics and the same gradients up to the float-atomic reordering that two EAGER steps show as well --
    a replay that computes anything else than the eager step fails here at the replay where it happens, unamplified (a 24-step
    trajectory of this dropout network amplifies 1e-7 to 1e-2 between two eager runs too: tools/debug_graph_divergence.py).
    (2) Trajectories on a network small enough to stay together: eager and graph trainers from the same seed, both learn."""
    from orcai_amd.architectures import ResNetLSTM
    from orcai_amd.training import Trainer

    def state_to(src, dst):
        dst.P.w.copy_(src.P.w); dst.P.m.copy_(src.P.m); dst.P.v.copy_(src.P.v); dst.P.stats_flat.copy_(src.P.stats_flat)
        dst.P.batch_flat.copy_(src.P.batch_flat); dst.counter.copy_(src.counter)
        dst.step_count, dst.lr = src.step_count, src.lr

    # (1) a shape that reaches the strip-tile kernel with the statistics epilogue (two strips of 62 columns) and the flat-range one
    rng = np.random.default_rng(1)
    B, H, W = 4, 64, 171
    xs = [torch.from_numpy(rng.random((B, H, W), dtype=np.float32)).cuda().view(-1) for _ in range(3)]
    ys = [torch.from_numpy((rng.random((B, 16, 3)) > 0.5).astype(np.float32)).cuda() for _ in range(3)]
    E, G = (Trainer(ResNetLSTM((H, W, 1), 3, [30, 40], 3, 0.3, 64, seed=1), learning_rate=3e-3, seed=5) for _ in range(2))

    class CaptureRecordingLib(RecordingLib):  # also notes per call whether the stream was being captured (the first call runs eager warm-up steps too)
        def __init__(self, lib):
            super().__init__(lib)
            self.capturing = []

        def __getattr__(self, name):
            call = super().__getattr__(name)

            def noted(*args):
                self.capturing.append(torch.cuda.is_current_stream_capturing())
                return call(*args)

            return noted

    rec = G.trunk.lib = CaptureRecordingLib(G.trunk.lib)
    masks_seen = []
    for step in range(12):
        if step == 6:
            E.lr = 1e-3
        state_to(E, G)
        w_before = E.P.w.clone()
        oe = E.train_step(xs[step % 3], H * W, B, ys[step % 3])
        ge, be = E.P.g.clone(), E.P.batch_flat.clone()
        og = G.train_step_graphed(xs[step % 3], H * W, B, ys[step % 3])
        ae, ag = oe["acc"].cpu().numpy(), og["acc"].cpu().numpy()
        assert abs(ae[0] / ae[1] - ag[0] / ag[1]) <= 1e-6 and ae[1] == ag[1], (step, ae, ag)
        assert float((be - G.P.batch_flat).abs().max()) <= 1e-6 * float(be.abs().max()), step
        for n, (o, k, _) in E.P.offsets.items():
            a, b = ge[o : o + k], G.P.g[o : o + k]
            assert float((a - b).abs().max()) <= 2e-5 * max(float(a.abs().max()), 1e-6), (step, n)
        # the replayed Adam used the eager one's bias correction and learning rate: same update from the same state
        assert float((E.P.w - G.P.w).abs().max()) <= 2e-5, step
        assert float((E.P.w - w_before).abs().max()) > 0
        assert int(E.counter.item()) == int(G.counter.item()) == step + 1 and G.step_count == step + 1
        masks_seen.append(float(og["probs"].sum()))
    assert len(set(np.round(masks_seen, 5))) > 6  # replays are not repeating one frozen step
    # the captured step holds the separable convs with the BatchNorm statistics in their epilogue
    captured = [(n, rc) for (n, rc, _), cap in zip(rec.calls, rec.capturing) if cap]
    assert any(n in ("orcai_sepconv_planes_stats", "orcai_sepconv_planes_stats_bn") and rc == 0 for n, rc in captured), captured

    # (2) free-running: eager and graph trainers from the same seed (the capture's warm-up steps leave no trace in the trainer's state).  The
    # first steps agree to float-atomic noise; later ones are only required to learn -- whether a 24-step trajectory of a dropout network
    # under Adam stays within 1e-7 or wanders off by 1e-2 is decided by the reordering noise alone (two EAGER trainers do both:
    # profiles/r03_graph_divergence.log), so trajectory equality is not a property a test can hold a replay to; (1) is.
    x = rng.random((4, 8, 32, 12), dtype=np.float32)
    y = (x.reshape(4, 8, 8, 4, 12).mean(axis=(3, 4))[..., None] > 0.5).astype(np.float32).repeat(3, axis=3)
    xs = [torch.from_numpy(x[b]).cuda().view(-1) for b in range(4)]
    ys = [torch.from_numpy(y[b]).cuda() for b in range(4)]
    runs = {}
    for mode in ("eager", "graph"):
        tr = Trainer(ResNetLSTM((32, 12, 1), 3, [10, 20], 3, 0.3, 64, seed=1), learning_rate=3e-3, seed=5)
        losses = []
        for step in range(24):
            if step == 12:
                tr.lr = 1e-3  # ReduceLROnPlateau-style change between steps: read from device memory by the replayed Adam
            out = tr.train_step(xs[step % 4], 32 * 12, 8, ys[step % 4]) if mode == "eager" else tr.train_step_graphed(xs[step % 4], 32 * 12, 8, ys[step % 4])
            a = out["acc"].cpu().numpy()
            losses.append(a[0] / a[1])
        runs[mode] = (np.array(losses), int(tr.counter.item()), tr.step_count)
    le, lg = runs["eager"][0], runs["graph"][0]
    assert runs["eager"][1] == runs["graph"][1] == 24 and runs["graph"][2] == 24  # no trace of the warm-up steps
    assert np.abs(le - lg)[:4].max() <= 1e-5, np.abs(le - lg)
    assert np.isfinite(lg).all() and lg[-4:].mean() < 0.95 * lg[:4].mean() and le[-4:].mean() < 0.95 * le[:4].mean()
    assert len(set(np.round(lg[:8], 6))) > 4
