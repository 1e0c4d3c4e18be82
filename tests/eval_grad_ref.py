"""Test helper: the eval-mode network as a torch-CPU forward that autograd can differentiate w.r.t. the snippets (oracle.train_ref's conv / pool /
LSTM pieces with the moving-statistics BatchNorm of oracle.model_ref._bn_infer), the formula of orcai_sepconv_dgrad, and the seeded inputs the
CPU and GPU tests of the eval-mode input gradient share."""

import numpy as np
import torch
import torch.nn.functional as F

from oracle import model_ref as M
from oracle import train_ref as T

# ------------------------------------------------------------------------------------------------------------------ the network
STEP_CONFIGS = [  # tests/test_input_grad_gpu.py::STEP_CONFIGS (k 3 / 5 / wide / 7) with its batch sizes
    (dict(input_shape=(32, 12, 1), filters=(10, 20), kernel_size=3, lstm_units=64, num_labels=3), 3),
    (dict(input_shape=(32, 16, 1), filters=(10, 20), kernel_size=5, lstm_units=64, num_labels=2), 2),
    (dict(input_shape=(16, 120, 1), filters=(20, 24), kernel_size=3, lstm_units=64, num_labels=3), 2),
    (dict(input_shape=(48, 21, 1), filters=(12, 30, 40), kernel_size=7, lstm_units=64, num_labels=7), 2),
]
CONV1D_CONFIG = (dict(input_shape=(48, 21, 1), filters=(12, 30, 40), kernel_size=3, lstm_units=64, num_labels=5), 3)  # its ResNet1DConv config
# (name, config, batch, conv1d, seed).  Seeds chosen on the CPU: torch-CPU f32 autograd of this oracle deviates from its float64 run by the share of
# max|ref| written next to each -- all within a quarter (1.25e-4) of the 5e-4 bar, so no ReLU / pooling decision differs between the precisions
# at these seeds and the GPU test measures arithmetic, not a flipped branch.
E2E_CASES = [
    ("k3", *STEP_CONFIGS[0], False, 5),      # f32 vs f64: 1.36e-6
    ("k5", *STEP_CONFIGS[1], False, 5),      # 1.12e-6
    ("wide", *STEP_CONFIGS[2], False, 5),    # 7.3e-7
    ("k7", *STEP_CONFIGS[3], False, 5),      # 7.0e-7
    ("conv1d", *CONV1D_CONFIG, True, 6),     # 3.0e-7
]


def e2e_inputs(cfg, B, conv1d, seed):
    """(params, x [B, H, W, 1], r [B, steps, labels]): calibrated weights with perturbed gamma / beta -- the moving statistics come from
    calibrated_params' own calibration batch, not from x -- and the seeded weights r of the loss sum(probs * r)."""
    p = M.calibrated_params(seed=seed, **cfg)
    rng = np.random.default_rng(seed)
    if conv1d:
        p = {k: v for k, v in p.items() if not k.startswith(("lstm", "dense", "bn_d"))}
    for k in p:
        if k.endswith(("gamma", "beta")):
            p[k] = (p[k] + 0.2 * rng.standard_normal(p[k].shape)).astype(np.float32)
    L = cfg["num_labels"]
    if conv1d:
        p["conv1d/kernel"] = (0.1 * rng.standard_normal((36, 36, L))).astype(np.float32)
        p["conv1d/bias"] = (0.1 * rng.standard_normal(L)).astype(np.float32)
    H, W, _ = cfg["input_shape"]
    steps = H // 2 ** len(cfg["filters"])
    x = rng.random((B, H, W, 1), dtype=np.float32)
    r = rng.standard_normal((B, steps, L)).astype(np.float32)
    return p, x, r


def forward_eval(p_np: dict, x_nhwc: torch.Tensor, conv1d: bool = False, inter: dict | None = None) -> torch.Tensor:
    """Inference forward in x_nhwc's dtype, differentiable w.r.t. x_nhwc.  inter (optional) receives the trunk features [B, T, W * 36]."""
    dt = x_nhwc.dtype
    p = {k: torch.as_tensor(np.asarray(v), dtype=dt) for k, v in p_np.items()}
    n_blocks = sum(1 for k in p if k.endswith("/res/kernel"))
    bn = lambda t, name, axis=1: M._bn_infer(t, p_np, name, dt, axis=axis)  # noqa: E731
    x = x_nhwc.permute(0, 3, 1, 2)
    x = torch.relu(bn(T._conv_same(x, p["conv0/kernel"], p["conv0/bias"], 1), "bn0"))
    prev = x
    for b in range(1, n_blocks + 1):
        x = torch.relu(x)
        x = torch.relu(bn(T._sepconv(x, p, f"b{b}/sep_a"), f"b{b}/bn_a"))
        x = bn(T._sepconv(x, p, f"b{b}/sep_b"), f"b{b}/bn_b")
        x = T._maxpool_same(x) + T._conv_same(prev, p[f"b{b}/res/kernel"], p[f"b{b}/res/bias"], 2)
        prev = x
    x = torch.relu(bn(T._sepconv(x, p, "sep_f"), "bn_f"))
    B, C, H, W = x.shape
    if inter is not None:
        inter["features"] = x.permute(0, 2, 3, 1).reshape(B, H, W * C).detach()
    if conv1d:
        x = x.mean(dim=3).permute(0, 2, 1)
        w = p["conv1d/kernel"]
        K = w.shape[0]
        xp = F.pad(x.permute(0, 2, 1), ((K - 1) // 2, K // 2))
        y = F.conv1d(xp, w.permute(2, 1, 0).contiguous(), p["conv1d/bias"])
        return torch.sigmoid(y.permute(0, 2, 1))
    x = x.permute(0, 2, 3, 1).reshape(B, H, W * C)
    x = T._bilstm(x, p, "lstm1")
    x = T._bilstm(x, p, "lstm2")
    x = torch.relu(x @ p["dense1/kernel"] + p["dense1/bias"])
    x = bn(x, "bn_d", axis=2)
    return torch.sigmoid(x @ p["dense2/kernel"] + p["dense2/bias"])


def input_gradient(p_np, x, r, conv1d, dtype):
    """(probs, d sum(probs * r) / dx [B, H, W]) as float64 numpy arrays, computed in `dtype`."""
    xt = torch.tensor(x, dtype=dtype, requires_grad=True)
    probs = forward_eval(p_np, xt, conv1d)
    (probs * torch.tensor(r, dtype=dtype)).sum().backward()
    return probs.detach().numpy().astype(np.float64), xt.grad.numpy()[..., 0].astype(np.float64)


# ------------------------------------------------------------------------------------------------------------------ the kernel alone
# (Cin, Cout, H, W, k): forward channels Cin -> Cout
KERNEL_CASES = [(16, 30, 37, 43, 3), (30, 30, 16, 120, 3), (30, 30, 40, 171, 3), (60, 36, 6, 11, 3), (10, 20, 5, 3, 3), (64, 64, 24, 22, 3), (12, 30, 32, 16, 5),
                (12, 30, 48, 21, 7)]
KERNEL_B = 2


def padded_width(W, k):
    return (W + k // 2 + 3) & ~3


def kernel_case(Cin, Cout, H, W, k, B=KERNEL_B):
    """Seeded host arrays of one case: g, y (the y_gate reference), x (the x_gate reference), wts [Cout][Cin], taps [Cin][k*k] (already reversed).
    g is zero wherever y lies within 1e-3 of zero and x keeps 1e-3 away from zero, so no rounding decides a branch (the recipe of
    test_input_grad_gpu.kernel_case)."""
    rng = np.random.default_rng(100000 * k + 1000 * Cin + 10 * H + W + Cout)
    g = rng.standard_normal((B, Cout, H, W)).astype(np.float32)
    y = rng.standard_normal((B, Cout, H, W)).astype(np.float32)
    x = rng.standard_normal((B, Cin, H, W)).astype(np.float32)
    g[np.abs(y) < 1e-3] = 0.0
    x[np.abs(x) < 1e-3] = -1.0
    wts = (rng.standard_normal((Cout, Cin)) / np.sqrt(Cout)).astype(np.float32)
    taps = (rng.standard_normal((Cin, k * k)) / k).astype(np.float32)
    return dict(g=g, y=y, x=x, wts=wts, taps=taps, k=k)


def formula(case, mode, dtype):
    """dr of include/orcai_hip.h's formula by torch on the host in `dtype`; mode "both" | "y" | "none" = which gates are given."""
    c = lambda a: torch.as_tensor(a, dtype=dtype)  # noqa: E731
    g, y, x, wts, taps, k = c(case["g"]), c(case["y"]), c(case["x"]), c(case["wts"]), c(case["taps"]), case["k"]
    if mode != "none":
        g = torch.where(y > 0, g, torch.zeros_like(g))
    du = torch.einsum("oi,bohw->bihw", wts, g)
    Cin = x.shape[1]
    dr = F.conv2d(du, taps.view(Cin, 1, k, k), padding=k // 2, groups=Cin)
    if mode == "both":
        dr = torch.where(x > 0, dr, torch.zeros_like(dr))
    return dr


def to_planes(a, k, pad_value=0.0):
    """[B][C][H][W] -> padded channel-quad planes [B][ceil(C/4)][H + 2R][WP][4]; spatial pads = pad_value, channels past C = 0."""
    B, C, H, W = a.shape
    R, WP, CQ = k // 2, padded_width(W, k), (C + 3) // 4
    out = np.full((B, CQ * 4, H + 2 * R, WP), pad_value, dtype=np.float32)
    out[:, C:] = 0.0
    out[:, :C, R : R + H, :W] = a
    return np.ascontiguousarray(out.reshape(B, CQ, 4, H + 2 * R, WP).transpose(0, 1, 3, 4, 2))


def from_planes(t, C, H, W, k):
    """The interior of planes (numpy [B][CQ][HP][WP][4]) as [B][C][H][W], and a copy of the planes with that interior zeroed (the pads)."""
    B, CQ, HP, WP, _ = t.shape
    R = k // 2
    full = t.transpose(0, 1, 4, 2, 3).reshape(B, CQ * 4, HP, WP)
    pads = full.copy()
    pads[:, :C, R : R + H, :W] = 0
    return full[:, :C, R : R + H, :W].copy(), pads


def taps_layout(taps, k):
    """taps [C][k*k] -> [ceil(C/4)][k*k][4] (zero taps for the channels that pad the last quad)."""
    C = taps.shape[0]
    CQ = (C + 3) // 4
    out = np.zeros((CQ * 4, k * k), dtype=np.float32)
    out[:C] = taps
    return np.ascontiguousarray(out.reshape(CQ, 4, k * k).transpose(0, 2, 1))
