"""Test helper: the eval-mode network of tests/eval_grad_ref.py::forward_eval rebuilt so that every TRAINABLE variable is a torch leaf -- the BatchNorm
written out with the moving statistics as constants -- for autograd w.r.t. the weights (frozen-BatchNorm fine-tuning), and the formulae of one folded
separable conv's weight gradients.  The seeded inputs are eval_grad_ref's (e2e_inputs, kernel_case): g is zero where y lies within 1e-3 of zero and x
keeps 1e-3 away from zero, so no rounding decides a branch."""

import numpy as np
import torch
import torch.nn.functional as F

import eval_grad_ref as R
from oracle import model_ref as M
from oracle import train_ref as T

E2E_CASES = R.E2E_CASES
# (Cin, Cout, H, W), B = 2, k = 3.  Measured on the CPU for exactly these inputs (all four y_gate x relu_in modes): the formulae below evaluated by torch in
# f32 deviate from their float64 evaluation by at most this share of max|ref| per output tensor:
#                            G          dbeta      dWdw
WGRAD_CASES = [
    (16, 30, 37, 43),      # 4.32e-7    1.20e-7    9.99e-7
    (10, 20, 5, 3),        # 1.92e-7    7.52e-8    1.38e-7    smaller than one tile, partial quads
    (30, 30, 16, 120),     # 3.50e-7    1.20e-7    1.08e-6    wider than one strip
    (60, 36, 6, 11),       # 3.69e-7    8.88e-8    1.91e-7
    (64, 64, 24, 22),      # 3.29e-7    1.69e-7    7.33e-7    the channel limit
]
# the worst share per output tensor, and the bar on the GPU: 4 x that (the f32 summation order differs between the kernels and torch)
F32_REFERENCE_DEVIATION = {"G": 4.32e-7, "dbeta": 1.69e-7, "dWdw": 1.08e-6}
WGRAD_BAR = {k: 4 * v for k, v in F32_REFERENCE_DEVIATION.items()}
WGRAD_MODES = [(True, 1), (True, 0), (False, 1), (False, 0)]  # (y_gate given, relu_in)


def is_trainable(name: str) -> bool:
    return not name.endswith(("/mean", "/var"))


def forward_frozen(p: dict, x_nhwc: torch.Tensor, conv1d: bool) -> torch.Tensor:
    """eval_grad_ref.forward_eval on a dict of torch tensors (leaves for the trainable variables, constants for the moving statistics)."""
    n_blocks = sum(1 for k in p if k.endswith("/res/kernel"))

    def bn(t, name, axis=1):
        inv = p[name + "/gamma"] * torch.rsqrt(p[name + "/var"] + M.BN_EPS)
        shift = p[name + "/beta"] - p[name + "/mean"] * inv
        shape = [1] * t.dim()
        shape[axis] = -1
        return t * inv.view(shape) + shift.view(shape)

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


def weight_gradients(p_np: dict, x, r, conv1d: bool, dtype):
    """(probs, {variable: d sum(probs * r) / d variable} for every trainable variable, dx [B, H, W]) as float64 numpy arrays, computed in `dtype`."""
    p = {k: torch.tensor(np.asarray(v), dtype=dtype, requires_grad=is_trainable(k)) for k, v in p_np.items()}
    xt = torch.tensor(x, dtype=dtype, requires_grad=True)
    # torch's own CPU convolutions: the oneDNN f32 weight-gradient path is not needed for an oracle, and it is the one piece here that is not plain ATen
    torch.backends.mkldnn.enabled = False
    try:
        probs = forward_frozen(p, xt, conv1d)
        (probs * torch.tensor(r, dtype=dtype)).sum().backward()
    finally:
        torch.backends.mkldnn.enabled = True
    grads = {k: v.grad.numpy().astype(np.float64) for k, v in p.items() if is_trainable(k)}
    return probs.detach().numpy().astype(np.float64), grads, xt.grad.numpy()[..., 0].astype(np.float64)


def wgrad_case(Cin, Cout, H, W):
    """eval_grad_ref.kernel_case(k = 3) read as a FORWARD layer: `taps` [Cin][9] are the forward depthwise taps, `wts` [Cout][Cin] = scale (.) pw^T."""
    return R.kernel_case(Cin, Cout, H, W, 3)


def wgrad_formula(case, dtype, y_gate: bool = True, relu_in: int = 1):
    """(G [Cout][Cin], dbeta [Cout], dWdw (k, k, Cin, 1)) of include/orcai_hip.h's formulae by torch on the host in `dtype`:
    gg = g where y > 0 (y_gate), r = relu_in ? relu(x) : x, u = dw(r), G = sum gg (x) u, dbeta = sum gg, dWdw[t][ci] = sum_p r[ci][p + off(t)] * du[ci][p] with
    du = wts^T gg."""
    c = lambda a: torch.as_tensor(a, dtype=dtype)  # noqa: E731
    g, y, x, wts, taps, k = c(case["g"]), c(case["y"]), c(case["x"]), c(case["wts"]), c(case["taps"]), case["k"]
    Cin = x.shape[1]
    gg = torch.where(y > 0, g, torch.zeros_like(g)) if y_gate else g
    r = torch.relu(x) if relu_in else x
    w = taps.view(Cin, 1, k, k).clone().requires_grad_()
    u = F.conv2d(r, w, padding=k // 2, groups=Cin)
    du = torch.einsum("oi,bohw->bihw", wts, gg)
    (dw,) = torch.autograd.grad((u * du).sum(), w)
    G = torch.einsum("bohw,bihw->oi", gg, u.detach())
    return G, gg.sum(dim=(0, 2, 3)), dw.permute(2, 3, 0, 1).contiguous()


def share(got, ref) -> float:
    """max|got - ref| as a share of max|ref| (float64)."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.abs(got - ref).max()) / float(np.abs(ref).max())
