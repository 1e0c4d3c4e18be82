"""ResNet1DConv on the f16 path: the f16 Dropout kernels against their f32 twins and numpy, the inference forward against the fp32 oracle
and the f32 path, one training step against float64 autograd (free-running and branch-matched), a 200-step trajectory against f32
training, a replayed-graph fit loop against eager steps, and the workflows (hyperparameter search, train, reload, predict, `orcai test`)."""

import json
from pathlib import Path

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from oracle import model_ref as M  # noqa: E402
from oracle import train_ref as T  # noqa: E402
from recording_lib import RecordingLib  # noqa: E402

ROOT = Path(__file__).resolve().parent.parent
HPS = json.loads((ROOT / "orcai_amd" / "defaults" / "default_hps_parameter.json").read_text())


def _planes(x, G, ksize, dtype):
    """[B][C][H][W] (numpy or torch) -> the padded plane layout [B][ceil(C/G)][H + 2R][WP][G] of the trunk kernels (G = 4: f32 quads, 8: f16 octets)."""
    x = torch.as_tensor(np.asarray(x) if not torch.is_tensor(x) else x)
    B, C, H, W = x.shape
    R = ksize // 2
    WP = (W + R + 3) & ~3
    CG = (C + G - 1) // G
    out = torch.zeros((B, CG * G, H + 2 * R, WP), dtype=dtype, device=x.device)
    out[:, :C, R : R + H, :W] = x.to(dtype)
    return out.reshape(B, CG, G, H + 2 * R, WP).permute(0, 1, 3, 4, 2).contiguous()


def _from_octets(p, C, H, W, ksize):
    B, CO, HP, WP, _ = p.shape
    R = ksize // 2
    return p.float().permute(0, 1, 4, 2, 3).reshape(B, CO * 8, HP, WP)[:, :C, R : R + H, :W].cpu().numpy().astype(np.float64)


# ---------------------------------------------------------------------------------------------------------------------------------
# 1, 2: the two kernels
@pytest.mark.parametrize("n", [8 * 4099, 8 * 4099 + 5, 3])
def test_h_dropout_mask_is_the_f32_mask_bit_for_bit(n):
    from orcai_amd import _native as N

    lib, st = N.lib(), N.stream_ptr()
    keep, seed = 0.6, 0x1234567
    counter = torch.tensor([7], dtype=torch.int64, device="cuda")
    m16 = torch.full((n + 8,), 5.0, dtype=torch.float16, device="cuda")  # 8 sentinels past the end
    m32 = torch.empty(n, dtype=torch.float32, device="cuda")
    N.check(lib.orcai_h_dropout_mask_dev(m16.data_ptr(), n, counter.data_ptr(), seed, keep, st), "h_dropout_mask_dev")
    N.check(lib.orcai_dropout_mask_dev(m32.data_ptr(), n, counter.data_ptr(), seed, keep, st), "dropout_mask_dev")
    assert torch.equal(m16[:n].float(), m32)
    assert bool((m16[n:] == 5.0).all())  # nothing written past n
    counter.fill_(8)
    other = torch.empty(n, dtype=torch.float16, device="cuda")
    N.check(lib.orcai_h_dropout_mask_dev(other.data_ptr(), n, counter.data_ptr(), seed, keep, st), "h_dropout_mask_dev")
    if n > 64:
        assert not torch.equal(other, m16[:n])  # the step counter moves the draw
        frac = float(m16[:n].float().mean())
        assert abs(frac - keep) <= 5.0 * np.sqrt(keep * (1 - keep) / n), frac  # 5 sigma of a binomial
    assert set(torch.unique(other.float()).tolist()) <= {0.0, 1.0}


def test_h_dropout_mask_keep_fraction_over_a_block_one_mask():
    from orcai_amd import _native as N

    n = 64 * 2 * 739 * 176 * 8 // 16  # a sixteenth of block 1's octet planes at batch 64
    m = torch.empty(n, dtype=torch.float16, device="cuda")
    counter = torch.tensor([0], dtype=torch.int64, device="cuda")
    N.check(N.lib().orcai_h_dropout_mask_dev(m.data_ptr(), n, counter.data_ptr(), 99, 0.5, N.stream_ptr()), "h_dropout_mask_dev")
    frac = float(m.float().mean())
    assert abs(frac - 0.5) <= 5.0 * np.sqrt(0.25 / n), frac


@pytest.mark.parametrize("n", [8 * 1000, 8 * 1000 + 3, 5])
def test_h_mask_scale_matches_numpy_exactly(n):
    from orcai_amd import _native as N

    lib, st = N.lib(), N.stream_ptr()
    rng = np.random.default_rng(n)
    x = (rng.standard_normal(n) * 30.0).astype(np.float16)
    x[:3] = [65504.0, -0.0, 6e-8]  # the f16 extremes: largest finite, signed zero, subnormal
    m = (rng.random(n) > 0.4).astype(np.float16)
    scale = np.float32(1.0 / (1.0 - 0.4))
    want = ((x.astype(np.float32) * m.astype(np.float32)) * scale).astype(np.float16)
    xd, md = torch.from_numpy(x).cuda(), torch.from_numpy(m).cuda()
    y = torch.full((n + 8,), 7.0, dtype=torch.float16, device="cuda")
    N.check(lib.orcai_h_mask_scale(xd.data_ptr(), md.data_ptr(), float(scale), n, y.data_ptr(), st), "h_mask_scale")
    got = y[:n].cpu().numpy()
    assert np.array_equal(got.view(np.uint16), want.view(np.uint16))
    assert bool((y[n:] == 7.0).all())
    N.check(lib.orcai_h_mask_scale(xd.data_ptr(), md.data_ptr(), float(scale), n, xd.data_ptr(), st), "h_mask_scale")  # in place
    assert np.array_equal(xd.cpu().numpy().view(np.uint16), want.view(np.uint16))


def test_h_mask_scale_leaves_plane_pads_zero():
    from orcai_amd import _native as N

    rng = np.random.default_rng(3)
    x = _planes(rng.standard_normal((3, 13, 9, 14)), 8, 3, torch.float16).cuda()
    ones = torch.ones_like(x)  # a mask drawn over the whole buffer keeps pad positions too
    y = torch.empty_like(x)
    N.check(N.lib().orcai_h_mask_scale(x.data_ptr(), ones.data_ptr(), 2.0, x.numel(), y.data_ptr(), N.stream_ptr()), "h_mask_scale")
    full = y.float().permute(0, 1, 4, 2, 3).reshape(3, 16, 11, 16)
    pads = full.clone()
    pads[:, :13, 1:10, :14] = 0
    assert not bool(pads.any())
    assert torch.equal(full[:, :13, 1:10, :14], 2.0 * x.float().permute(0, 1, 4, 2, 3).reshape(3, 16, 11, 16)[:, :13, 1:10, :14])


# ---------------------------------------------------------------------------------------------------------------------------------
# 3: inference
def _conv1d_params(cfg, seed):
    from orcai_amd.architectures import FINAL_FILTERS

    p = M.calibrated_params(seed=seed, calib_batch=1, **cfg)
    p = {k: v for k, v in p.items() if not k.startswith(("lstm", "dense", "bn_d"))}
    rng = np.random.default_rng(seed)
    L = cfg["num_labels"]
    p["conv1d/kernel"] = (0.1 * rng.standard_normal((FINAL_FILTERS, FINAL_FILTERS, L))).astype(np.float32)
    p["conv1d/bias"] = (0.1 * rng.standard_normal(L)).astype(np.float32)
    return p


@pytest.mark.parametrize(
    "shape,filters,k,L",
    [((736, 171), tuple(HPS["filters"]["set3"]), 3, 7), ((48, 21), (12, 30, 40), 5, 1), ((32, 19), (10, 20), 7, 64), ((64, 45), (16, 24, 44), 3, 64)],
)
def test_half_conv1d_forward_vs_oracle_and_f32(shape, filters, k, L):
    from orcai_amd.architectures import ResNet1DConv

    cfg = dict(input_shape=(*shape, 1), num_labels=L, filters=filters, kernel_size=k, lstm_units=64)
    p = _conv1d_params(cfg, seed=11)
    model = ResNet1DConv(cfg["input_shape"], L, list(filters), k, 0.0, precision="f16")
    model.set_weights_dict(p)
    B = 3
    x = np.random.default_rng(6).random((B, *shape, 1), dtype=np.float32)
    got = model.predict(x, batch_size=B)
    assert model._half_engine is not None and "lstm1/Wt" not in model._half_engine._dev  # the f16 engine ran and packed no LSTM weights
    ref = M.forward_ref_1dconv(p, x)
    model.precision = "f32"
    f32 = model.predict(x, batch_size=B)
    model.precision = "f16"
    e_ref, e_32 = float(np.abs(got - ref).max()), float(np.abs(got - f32).max())
    print(f"f16 ResNet1DConv {shape} {filters} k={k} L={L}: max|dp| vs the fp32 oracle {e_ref:.2e}, vs the f32 path {e_32:.2e}")
    assert got.shape == ref.shape and e_ref <= 5e-3 and e_32 <= 5e-3
    # keep= hook: feat and freq_mean of the head
    keep = {}
    xd = torch.from_numpy(np.ascontiguousarray(x[..., 0])).cuda()
    out = torch.empty((B, model.out_steps, L), dtype=torch.float32, device="cuda")
    model.forward_device(xd.view(-1), shape[0] * shape[1], B, out, chunk=B, keep=keep)
    assert {"feat", "freq_mean"} <= set(keep) and keep["freq_mean"].shape == (B, model.out_steps, 36)
    wl = model.stage_shapes()[-1][1]
    assert torch.allclose(keep["freq_mean"], keep["feat"].view(B, model.out_steps, wl, 36).mean(dim=2), rtol=1e-5, atol=1e-6)
    assert np.allclose(out.cpu().numpy(), got, rtol=0, atol=1e-6)


def test_half_conv1d_predict_spectrogram():
    from orcai_amd.architectures import ResNet1DConv

    cfg = dict(input_shape=(64, 45, 1), num_labels=5, filters=(12, 30, 44), kernel_size=3, lstm_units=64)
    p = _conv1d_params(cfg, seed=2)
    model = ResNet1DConv(cfg["input_shape"], 5, [12, 30, 44], 3, 0.0, precision="f16")
    model.set_weights_dict(p)
    spec = np.random.default_rng(4).random((64 * 9 + 17, 45), dtype=np.float32)
    got = model.predict_spectrogram(torch.from_numpy(spec).cuda(), chunk=4).cpu().numpy()
    n = (spec.shape[0] - 64) // 32 + 1
    snippets = np.stack([spec[i * 32 : i * 32 + 64] for i in range(n)])[..., None]
    ref = M.forward_ref_1dconv(p, snippets)
    assert got.shape == ref.shape == (n, 8, 5)
    assert float(np.abs(got - ref).max()) <= 5e-3


# ---------------------------------------------------------------------------------------------------------------------------------
# 4: one training step against float64 autograd
def _forward_train_1dconv(p, x_nhwc, masks, rate, n_blocks, forced):
    """oracle.train_ref.forward_train_1dconv with the branch hooks of oracle.train_ref.forward_train: forced = {"record": {}} records the
    ReLU masks / pooling selections the float64 forward takes; forced = {key: branch} makes it take the given ones."""
    new_stats = {}
    keep = 1.0 - rate
    x = x_nhwc.permute(0, 3, 1, 2)
    x = T._relu(T._bn_train(T._conv_same(x, p["conv0/kernel"], p["conv0/bias"], 1), p, "bn0", new_stats), forced, "relu/bn0")
    prev = x
    for b in range(1, n_blocks + 1):
        x = T._relu(x, forced, f"relu/b{b}/in")
        x = T._relu(T._bn_train(T._sepconv(x, p, f"b{b}/sep_a"), p, f"b{b}/bn_a", new_stats), forced, f"relu/b{b}/bn_a")
        x = T._bn_train(T._sepconv(x, p, f"b{b}/sep_b"), p, f"b{b}/bn_b", new_stats)
        x = T._maxpool_same(x, forced=forced, key=f"pool/b{b}")
        x = x + T._conv_same(prev, p[f"b{b}/res/kernel"], p[f"b{b}/res/bias"], 2)
        prev = x
        if masks is not None:
            x = x * masks[f"block{b}"] / keep
    x = T._relu(T._bn_train(T._sepconv(x, p, "sep_f"), p, "bn_f", new_stats), forced, "relu/bn_f")
    if masks is not None:
        x = x * masks["final"] / keep
    x = x.mean(dim=3).permute(0, 2, 1)
    w = p["conv1d/kernel"]
    K = w.shape[0]
    xp = torch.nn.functional.pad(x.permute(0, 2, 1), ((K - 1) // 2, K // 2))
    y = torch.nn.functional.conv1d(xp, w.permute(2, 1, 0).contiguous(), p["conv1d/bias"])
    return torch.sigmoid(y.permute(0, 2, 1))


def _loss_and_grads(params_np, x, y, masks_np, rate, forced_np):
    p = {k: torch.tensor(np.asarray(v), dtype=torch.float64, requires_grad=T.is_trainable(k)) for k, v in params_np.items()}
    n_blocks = sum(1 for k in p if k.endswith("/res/kernel"))
    masks = None if masks_np is None else {k: torch.tensor(v, dtype=torch.float64) for k, v in masks_np.items()}
    forced = {k: (v if k == "record" else torch.tensor(np.asarray(v), dtype=torch.int64) if k.startswith("pool/") else torch.tensor(np.asarray(v), dtype=torch.float64))
              for k, v in forced_np.items()}
    probs = _forward_train_1dconv(p, torch.tensor(x, dtype=torch.float64), masks, rate, n_blocks, forced)
    bce = T.masked_bce(torch.tensor(y, dtype=torch.float64), probs)
    bce.backward()
    out = {"loss": float(bce.detach()), "probs": probs.detach().numpy(), "grads": {k: v.grad.numpy() for k, v in p.items() if v.requires_grad}}
    if "record" in forced:
        out["record"] = {k: v.numpy() for k, v in forced["record"].items()}
    return out


def _f16_branches(tr, cfg, B, rate):
    """The ReLU masks and pooling selections the f16 forward took, read back from the tensors it stored (see tests/test_half_gpu.py)."""
    from oracle.model_ref import same_pad
    from orcai_amd.architectures import BN_EPS

    k = cfg["kernel_size"]
    H, W, _ = cfg["input_shape"]
    buf, shapes = tr.trunk.buf, tr.model.stage_shapes()
    forced = {}
    y0 = _from_octets(buf["y0"], 16, H, W, k)
    forced["relu/bn0"] = forced["relu/b1/in"] = (y0 > 0).astype(np.float64)
    cprev = 16
    for i, c in enumerate(cfg["filters"], start=1):
        h, w, _ = shapes[i - 1]
        if i > 1:  # sep_a of block i reads relu(Dropout(prev_{i-1}))
            src = f"prevd{i - 1}" if rate > 0 else f"prev{i - 1}"
            forced[f"relu/b{i}/in"] = (_from_octets(buf[src], cprev, h, w, k) > 0).astype(np.float64)
        if tr.trunk.on_load.get(i):
            tr.trunk._bn_apply(buf[f"va{i}"], f"b{i}/bn_a", c, h, w, 1, buf[f"ya{i}"])
        forced[f"relu/b{i}/bn_a"] = (_from_octets(buf[f"ya{i}"], c, h, w, k) > 0).astype(np.float64)
        sgn = np.where(tr.P.W(f"b{i}/bn_b/gamma").cpu().numpy() < 0, -1.0, 1.0)
        sv = _from_octets(buf[f"vb{i}"], c, h, w, k) * sgn[None, :, None, None]
        _, pt, pb = same_pad(h, 3, 2)
        _, pl, pr = same_pad(w, 2, 2)
        svp = np.pad(sv, ((0, 0), (0, 0), (pt, pb), (pl, pr)), constant_values=-np.inf)
        ho, wo = shapes[i][0], shapes[i][1]
        win = np.stack([svp[:, :, dy : dy + 2 * ho : 2, dx : dx + 2 * wo : 2] for dy in range(3) for dx in range(2)], axis=-1)
        forced[f"pool/b{i}"] = np.argmax(win, axis=-1)
        cprev = c
    # BN_f + ReLU of the head (f32): its pre-ReLU value from the stored f32 features and this step's batch statistics
    hc = tr.head.cache
    hl, wl, _ = shapes[-1]
    fv = hc["featv"].cpu().numpy().astype(np.float64).reshape(B, hl, wl, 36)
    mean, var = hc["f_mean"].cpu().numpy().astype(np.float64), hc["f_var"].cpu().numpy().astype(np.float64)
    g, b = tr.P.W("bn_f/gamma").cpu().numpy().astype(np.float64), tr.P.W("bn_f/beta").cpu().numpy().astype(np.float64)
    pre = (fv - mean) / np.sqrt(var + BN_EPS) * g + b
    forced["relu/bn_f"] = (pre.transpose(0, 3, 1, 2) > 0).astype(np.float64)
    return forced


def _step_setup(cfg, B, seed, rate, precision):
    from orcai_amd.architectures import FINAL_FILTERS, ResNet1DConv
    from orcai_amd.training import Trainer

    p = _conv1d_params(cfg, seed)
    rng = np.random.default_rng(seed)
    for key in p:
        if key.endswith(("gamma", "beta")):
            p[key] = (p[key] + 0.2 * rng.standard_normal(p[key].shape)).astype(np.float32)
    H, W, _ = cfg["input_shape"]
    L, k = cfg["num_labels"], cfg["kernel_size"]
    nb = len(cfg["filters"])
    steps = H // 2**nb
    x = rng.random((B, H, W, 1), dtype=np.float32)
    y = (rng.random((B, steps, L)) > 0.5).astype(np.float32)
    y[1, :, 0] = -1.0
    model = ResNet1DConv(cfg["input_shape"], L, list(cfg["filters"]), k, rate, precision=precision)
    model.set_weights_dict(p)
    shapes = model.stage_shapes()
    masks_np, masks_dev = None, None
    if rate > 0:
        G, dt = (8, torch.float16) if precision == "f16" else (4, torch.float32)
        masks_np = {f"block{i}": (rng.random((B, shapes[i][2], shapes[i][0], shapes[i][1])) > rate).astype(np.float32) for i in range(1, nb + 1)}
        masks_np["final"] = (rng.random((B, FINAL_FILTERS, shapes[-1][0], shapes[-1][1])) > rate).astype(np.float32)
        masks_dev = {key: _planes(v, G, k, dt).cuda() for key, v in masks_np.items() if key != "final"}
        masks_dev["final"] = torch.from_numpy(np.ascontiguousarray(masks_np["final"].transpose(0, 2, 3, 1).reshape(B, shapes[-1][0], -1))).cuda()
    tr = Trainer(model, learning_rate=1e-3)
    out = tr.forward_backward(torch.from_numpy(np.ascontiguousarray(x[..., 0])).cuda().view(-1), H * W, B, torch.from_numpy(y).cuda(), masks=masks_dev)
    return p, x, y, masks_np, tr, out


@pytest.mark.parametrize("rate", [0.0, 0.4])
@pytest.mark.parametrize(
    "cfg,B",
    [
        (dict(input_shape=(48, 21, 1), filters=(12, 30, 40), kernel_size=3, lstm_units=64, num_labels=5), 3),
        (dict(input_shape=(64, 61, 1), filters=(30, 40, 50, 60), kernel_size=3, lstm_units=64, num_labels=7), 2),
    ],
)
def test_half_conv1d_training_step_vs_autograd(cfg, B, rate):
    """Forward in training mode (block Dropout, final Dropout) + masked BCE + backward on the f16 path against float64 autograd, held to the bars of
    tests/test_half_gpu.py's _check_half_step: probabilities 5e-3, loss 5e-3 relative, every gradient / grad_scale within relative L2 2e-2 of the
    float64 gradient of the branch the f16 forward took and at cosine >= 0.9 to the free-running one.  The branches where the f16 forward and the
    free-running float64 forward part are counted and bounded, so that forcing the oracle cannot hide a systematically wrong mask."""
    p, x, y, masks_np, tr, out = _step_setup(cfg, B, seed=6, rate=rate, precision="f16")
    assert tr.half and tr.trunk.buf["y0"].dtype == torch.float16
    free = _loss_and_grads(p, x, y, masks_np, rate, {"record": {}})
    forced = _f16_branches(tr, cfg, B, rate)
    matched = _loss_and_grads(p, x, y, masks_np, rate, forced)
    # branch disagreements between the f16 forward and the free-running float64 one: f16 rounding flips the ~1 % of values within 2^-11 of a ReLU
    # threshold or of a window's runner-up (at most 0.17 % of a ReLU's and 0.28 % of a pooling's elements at these shapes); a wrong mask or a wrong
    # Dropout layout would flip a large share
    flips = {key: float((forced[key] != free["record"][key]).mean()) for key in forced}
    print("f16 branches that differ from the free-running float64 forward:", {key: f"{v:.2%}" for key, v in flips.items()})
    assert all(v <= 0.01 for key, v in flips.items() if key.startswith("relu/")), flips
    assert all(v <= 0.02 for key, v in flips.items() if key.startswith("pool/")), flips
    acc = out["acc"].cpu().numpy()
    probs = out["probs"].cpu().numpy()
    dp_free, dp_matched = float(np.abs(probs - free["probs"]).max()), float(np.abs(probs - matched["probs"]).max())
    print(f"f16 ResNet1DConv step rate {rate}: max|dp| {dp_free:.1e} (free-running), {dp_matched:.1e} (branch-matched)")
    assert dp_free <= 5e-3 and dp_matched <= 5e-3
    assert abs(acc[0] / acc[1] - free["loss"]) <= 5e-3 * max(1.0, abs(free["loss"])) and acc[3] == 0.0
    relm, cos, bad = {}, {}, {}
    for name, g in free["grads"].items():
        got = tr.P.G(name).cpu().numpy().astype(np.float64) / tr.grad_scale
        assert np.isfinite(got).all(), name
        if name.endswith("/bias") and "res" not in name and not name.startswith("conv1d"):
            assert np.abs(got).max() <= 1e-3, name  # a bias in front of a BatchNorm has zero gradient
            continue
        gm = matched["grads"][name]
        relm[name] = float(np.linalg.norm(got - gm)) / max(float(np.linalg.norm(gm)), 1e-12)
        cos[name] = float((got * g).sum() / max(np.linalg.norm(got) * np.linalg.norm(g), 1e-30))
        if relm[name] > 2e-2 or cos[name] < 0.9:
            bad[name] = (relm[name], cos[name])
    top = sorted(relm.items(), key=lambda kv: -kv[1])[:3]
    print(f"  gradients: relative L2 vs branch-matched median {np.median(list(relm.values())):.1e}, worst {[(n, f'{v:.1e}') for n, v in top]}; "
          f"min cosine vs free-running {min(cos.values()):.4f}")
    assert not bad, bad
    # the conv1d / bn_f gradients carry the loss scale like the trunk's (Adam divides the whole buffer by it)
    assert relm["conv1d/kernel"] <= 2e-2 and relm["bn_f/gamma"] <= 2e-2
    tr.apply()
    assert int(tr.skipped.item()) == 0 and bool(torch.isfinite(tr.P.w).all())


def test_half_conv1d_step_launchers_with_dropout():
    """Which launchers the f16 ResNet1DConv step ran: the f16 mask twin at every Dropout site (forward after each block, backward into sep_f and
    into every later block's sep_a input), never the f32 kernel on octet planes, and block 1's fused entry backward with the masks present."""
    cfg = dict(input_shape=(48, 21, 1), filters=(12, 30, 40), kernel_size=3, lstm_units=64, num_labels=5)
    from orcai_amd.architectures import ResNet1DConv
    from orcai_amd.training import Trainer

    model = ResNet1DConv(cfg["input_shape"], 5, [12, 30, 40], 3, 0.4, seed=2, precision="f16")
    tr = Trainer(model, learning_rate=1e-3, seed=3)
    rec = RecordingLib(tr.trunk.lib)
    tr.trunk.lib = rec
    x = torch.rand((3, 48, 21), device="cuda")
    y = (torch.rand((3, 6, 5), device="cuda") > 0.5).float()
    out = tr.forward_backward(x.view(-1), 48 * 21, 3, y)  # masks drawn by the trainer (f16 octet planes)
    tr.trunk.lib = rec._lib
    assert rec.rcs("orcai_h_mask_scale") == [0] * (3 + 1 + 2) and not rec.rcs("orcai_mask_scale")
    assert rec.rcs("orcai_h_dw_bwd_fused_res") == [0] and rec.rcs("orcai_h_conv0_bn_bwd_ready") == [0]
    assert torch.isfinite(out["probs"]).all() and bool(torch.isfinite(tr.P.g).all())
    masks = tr._masks(3, 6)
    assert masks["block1"].dtype == torch.float16 and masks["block1"].shape == (3, 2, 26, model.padded_width(11), 8) and masks["final"].dtype == torch.float32
    bad = dict(masks)
    bad["block2"] = masks["block2"].float()
    with pytest.raises(ValueError, match="block2 mask"):
        tr.forward_backward(x.view(-1), 48 * 21, 3, y, masks=bad)


# ---------------------------------------------------------------------------------------------------------------------------------
# 5: trajectory against f32 training
def test_half_conv1d_training_tracks_f32_training():
    """200 Adam steps of ResNet1DConv with Dropout 0.3 on the same batches, masks and initial weights in both precisions, held to the bars of
    tests/test_half_gpu.py's test_half_training_tracks_f32_training."""
    from orcai_amd.architectures import FINAL_FILTERS, ResNet1DConv
    from orcai_amd.training import Trainer

    rng = np.random.default_rng(0)
    x = rng.random((4, 16, 64, 24), dtype=np.float32)
    y = (x.reshape(4, 16, 8, 8, 24).mean(axis=(3, 4))[..., None] > 0.5).astype(np.float32).repeat(3, axis=3)
    rate, steps = 0.3, 200
    shape_model = ResNet1DConv((64, 24, 1), 3, [10, 20, 30], 3, rate, seed=1)
    shapes = shape_model.stage_shapes()
    gen = torch.Generator(device="cuda").manual_seed(5)
    mask_steps = []
    for _ in range(steps):
        m = {f"block{i}": (torch.rand((16, shapes[i][2], shapes[i][0], shapes[i][1]), generator=gen, device="cuda") > rate).float() for i in range(1, 4)}
        m["final"] = (torch.rand((16, shapes[-1][0], shapes[-1][1] * FINAL_FILTERS), generator=gen, device="cuda") > rate).float()
        mask_steps.append(m)
    curves = {}
    for precision in ("f32", "f16"):
        model = ResNet1DConv((64, 24, 1), 3, [10, 20, 30], 3, rate, seed=1, precision=precision)
        tr = Trainer(model, learning_rate=2e-3, seed=7)
        G, dt = (8, torch.float16) if precision == "f16" else (4, torch.float32)
        losses = []
        for step in range(steps):
            b = step % 4
            m = {key: (v if key == "final" else _planes(v, G, 3, dt)) for key, v in mask_steps[step].items()}
            out = tr.forward_backward(torch.from_numpy(x[b]).cuda().view(-1), 64 * 24, 16, torch.from_numpy(y[b]).cuda(), masks=m)
            tr.apply()
            a = out["acc"].cpu().numpy()
            losses.append(a[0] / a[1])
        curves[precision] = np.array(losses)
        if precision == "f16":
            assert int(tr.skipped.item()) == 0
    d = np.abs(curves["f16"] - curves["f32"])
    sm = lambda c: np.convolve(c, np.ones(20) / 20, mode="valid")  # noqa: E731
    print(f"f16 vs f32 ResNet1DConv training, {steps} steps: loss {curves['f32'][0]:.4f} -> {curves['f32'][-20:].mean():.4f} (f32), -> {curves['f16'][-20:].mean():.4f} (f16); "
          f"max|dL| = {d.max():.4f}, mean|dL| = {d.mean():.4f}, max smoothed |dL| = {np.abs(sm(curves['f16']) - sm(curves['f32'])).max():.4f}")
    assert np.isfinite(curves["f16"]).all()
    assert curves["f32"][-20:].mean() < 0.8 * curves["f32"][:5].mean() and curves["f16"][-20:].mean() < 0.8 * curves["f16"][:5].mean()
    assert np.abs(sm(curves["f16"]) - sm(curves["f32"])).max() <= 0.15
    assert abs(curves["f16"][-20:].mean() - curves["f32"][-20:].mean()) <= 0.01


# ---------------------------------------------------------------------------------------------------------------------------------
# 6, 7: fit loop on a replayed graph, workflows
CALLS = ["A", "B", "C"]


def _param(**model_over):
    from orcai_amd.io import read_json

    p = read_json(ROOT / "orcai_amd" / "defaults" / "default_orcai_parameter.json")
    p["architecture"] = "ResNet1DConv"
    p["calls"] = list(CALLS)
    p["seed"] = 1234
    del p["model"]["lstm_units"], p["model"]["lstm_initializer"]
    p["model"].update({"filters": [10, 20], "batch_size": 8, "epochs": 2, "learning_rate": 3e-3, "dropout_rate": 0.3, "precision": "f16",
                       "conv_initializer": "glorot_uniform"})
    p["model"].update(model_over)
    p["spectrogram"]["freq_range"] = [0, 1125]  # 12 frequency bins at 48 kHz / nfft 512: the synthetic datasets' snippet width
    return p


def _data(tmp_path, n_train=32, n_val=16):
    from orcai_amd.datasets import make_synthetic_dataset

    d = tmp_path / "data"
    d.mkdir()
    make_synthetic_dataset(d / "train_dataset", n_train, seed=4, input_shape=(32, 12), out_steps=8, n_labels=3)
    make_synthetic_dataset(d / "val_dataset", n_val, seed=5, input_shape=(32, 12), out_steps=8, n_labels=3)
    (d / "dataset_shapes.json").write_text(json.dumps({"spectrogram": [32, 12, 1], "labels": [8, 3]}))
    return d


def test_half_conv1d_fit_loop_on_a_replayed_graph(tmp_path):
    """Two epochs of FitLoop, f16 ResNet1DConv with Dropout 0.3, the step replayed as one hipGraph against eager steps: the masks are drawn from the
    device step counter inside the step, so both loops draw the same ones; losses and weights agree to the float-atomic reordering bar of
    tests/test_train_workflow_gpu.py's graph test."""
    from orcai_amd.architectures import ResNet1DConv
    from orcai_amd.datasets import SnippetDataset
    from orcai_amd.fit import FitLoop
    from orcai_amd.training import Trainer

    d = _data(tmp_path, n_train=48, n_val=24)
    runs = {}
    for graph in (False, True):
        model = ResNet1DConv((32, 12, 1), 3, [10, 20], 3, 0.3, seed=3, precision="f16")
        tr = Trainer(model, learning_rate=3e-3, seed=1)
        loop = FitLoop(model, tr, graph_step=graph)
        assert loop.graph_step == graph
        train = SnippetDataset(d / "train_dataset", 8, seed=[1, 2], shuffle=True)
        val = SnippetDataset(d / "val_dataset", 8, seed=[3, 4], shuffle=False)
        h = loop.fit(train, validation_data=val, epochs=2).history
        runs[graph] = (h, tr.P.w.clone(), tr._graph is not None, int(tr.counter.item()), int(tr.skipped.item()))
        tr.release_graph()
    (eh, ew, eg, ec, es), (gh, gw, gg, gc_, gs) = runs[False], runs[True]
    assert not eg and gg  # the graphed loop really replayed a graph
    assert ec == gc_ == 12 and es == gs == 0
    assert len(eh["loss"]) == len(gh["loss"]) == 2 and np.isfinite(gh["loss"]).all()
    for key in ("loss", "val_loss", "MBA", "val_MBA"):
        assert np.allclose(eh[key], gh[key], rtol=0, atol=2e-3), (key, eh[key], gh[key])
    assert float((ew - gw).abs().max()) <= 2e-3


def test_half_conv1d_hyperparameter_search(tmp_path):
    """hyperparameter_search over ResNet1DConv in f16 (no lstm_units anywhere): every trial completes, the best hyper-parameters carry no
    lstm_units, and the checkpoint's parameter sidecar records the precision."""
    import pandas as pd

    from orcai_amd.hpsearch import hyperparameter_search
    from orcai_amd.io import load_orcai_model

    d = _data(tmp_path, n_train=16, n_val=8)
    hps = {"filters": {"set1": [10, 20], "set2": [12, 24]}, "dropout_rate": [0.0, 0.3], "kernel_size": [3], "batch_size": [8]}
    out = tmp_path / "hps_out"
    out.mkdir()
    hyperparameter_search(d, out, _param(), hps, verbosity=0, max_epochs=3)
    trials = pd.read_csv(out / "hps_logs" / "all_trials.csv")
    assert (trials["status"] == "COMPLETED").all() and np.isfinite(trials["score"].astype(float)).all()
    best = json.loads((out / "hps_logs" / "best_hyperparameters.json").read_text())
    assert "lstm_units" not in best and best["filters"] in ("set1", "set2")
    ckpt = out / "orcai-v1" / "hps"
    model, p2, _ = load_orcai_model(ckpt)
    assert p2["architecture"] == "ResNet1DConv" and p2["model"]["precision"] == "f16" and "lstm_units" not in p2["model"]
    assert model.precision == "f16" and model.architecture == "ResNet1DConv"


def test_half_conv1d_train_reload_predict_and_test(tmp_path):
    """`train` in f16, reload (precision kept through orcai_parameter.json), `predict` on a short wav, then `orcai test` on test datasets."""
    import pandas as pd
    from click.testing import CliRunner

    from orcai_amd.cli import cli
    from orcai_amd.datasets import make_synthetic_dataset
    from orcai_amd.io import load_orcai_model
    from orcai_amd.predict import predict
    from orcai_amd.synthetic import synth_recording
    from orcai_amd.train import train
    from orcai_amd.wavio import write_wav_pcm16

    d = _data(tmp_path)
    make_synthetic_dataset(d / "test_dataset", 24, seed=6, input_shape=(32, 12), out_steps=8, n_labels=3)
    make_synthetic_dataset(d / "test_unfiltered_dataset", 16, seed=7, input_shape=(32, 12), out_steps=8, n_labels=3)
    out = tmp_path / "out"
    out.mkdir()
    train(d, out, _param(), verbosity=0)
    mdir = out / "orcai-v1"
    hist = json.loads((mdir / "training_history.json").read_text())
    assert len(hist["loss"]) == 2 and np.isfinite(hist["loss"]).all() and np.isfinite(hist["val_loss"]).all()
    assert json.loads((mdir / "orcai_parameter.json").read_text())["model"]["precision"] == "f16"
    model, p2, _ = load_orcai_model(mdir)
    assert model.architecture == "ResNet1DConv" and model.precision == "f16" and p2["model"]["precision"] == "f16"
    xs = np.random.default_rng(0).random((4, 32, 12, 1), dtype=np.float32)
    probs = model.predict(xs)
    assert probs.shape == (4, 8, 3) and float(np.abs(probs - M.forward_ref_1dconv(model.weights, xs)).max()) <= 5e-3
    wav = tmp_path / "rec.wav"
    write_wav_pcm16(wav, synth_recording(9.0, 48000, seed=5), 48000)
    pred = tmp_path / "rec_predicted.txt"
    predict(wav, model_dir=mdir, output_path=pred, save_probabilities=True, verbosity=0)
    table = pd.read_csv(tmp_path / "rec_predicted_probabilities.csv.gz", index_col="time")
    assert list(table.columns) == CALLS and len(table) > 0 and np.isfinite(table.to_numpy()).all()
    res = CliRunner().invoke(cli, ["test", str(mdir), str(d), "-tu", "-o", str(tmp_path / "results"), "-v", "0"], catch_exceptions=False)
    assert res.exit_code == 0, res.output
    metrics = json.loads((tmp_path / "results" / "test_data_metrics.json").read_text())
    assert set(metrics) >= {"loss", "MBA"} and np.isfinite(metrics["loss"])
