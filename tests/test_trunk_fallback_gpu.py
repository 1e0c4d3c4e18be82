"""The separate f32 trunk launchers the k = 5 / 7 training step falls back to (every fused training kernel is k = 3 only), one by one through
the C ABI against float64 arithmetic, on planes wide enough that a row of the flat padded plane needs several 64-pixel windows (W = 64, 65,
171; W = 21 for the several-rows-per-window case), heights 1 / 5 / 8, B = 2, channel counts 7 / 16 / 30 / 50 (ragged quad, 1 to 4 output tiles).

Two kinds of input where the arithmetic allows:
  exact            small integers in [-4, 4], scales 1 or a power of two, integer shifts: every partial sum is an integer below 2^24, so f32 (in any
                   summation order, float atomics included) must equal the float64 result bit for bit;
  standard normal  at the bound the nearest existing test of the same reduction uses (named at each assertion).
Outputs start from a sentinel (planes: sentinel interior, zero pads).  Afterwards the pads are still zero, accumulated outputs are right on top
of their non-zero start, and bad arguments return a negative code with the sentinel intact."""

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from oracle.model_ref import same_pad  # noqa: E402
from test_train_fused_gpu import _from_quad, _quad_planes  # noqa: E402

B = 2
SENTINEL = 777.0


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _ints(rng, *shape, lo=-4, hi=4):
    return rng.integers(lo, hi + 1, size=shape).astype(np.float32)


def _sentinel_planes(C, H, W, k, value=SENTINEL):
    """Quad planes whose interior (real channels) holds `value` and whose pads are zero."""
    return _dev(_quad_planes(np.full((B, C, H, W), value, dtype=np.float32), k))


def _pads(p, C, H, W, k):
    """max |.| over the pad rows, pad columns and pad channels of quad planes."""
    R = k // 2
    q = p.copy()
    Bq, CQ, HP, WP, _ = q.shape
    full = q.transpose(0, 1, 4, 2, 3).reshape(Bq, CQ * 4, HP, WP)
    full[:, :C, R : R + H, :W] = 0
    return float(np.abs(full).max())


def _pack_dw(dwk):
    """Keras depthwise kernel (k, k, C) -> the kernels' channel-quad layout [ceil(C/4)][k*k][4], zero for channels >= C."""
    k, _, C = dwk.shape
    CQ = (C + 3) // 4
    out = np.zeros((CQ * 4, k * k), dtype=np.float32)
    out[:C] = dwk.reshape(k * k, C).T
    return np.ascontiguousarray(out.reshape(CQ, 4, k * k).transpose(0, 2, 1))


def _depthwise_ref(x, dwk, relu_in):
    """Depthwise "same" convolution (cross-correlation, as Keras) of [B][C][H][W] in float64."""
    k = dwk.shape[0]
    R = k // 2
    Bx, C, H, W = x.shape
    xr = np.maximum(x, 0) if relu_in else x
    xp = np.zeros((Bx, C, H + 2 * R, W + 2 * R))
    xp[:, :, R : R + H, R : R + W] = xr
    u = np.zeros((Bx, C, H, W))
    for dy in range(k):
        for dx in range(k):
            u += xp[:, :, dy : dy + H, dx : dx + W] * dwk[dy, dx].astype(np.float64)[None, :, None, None]
    return u


def _sep_ref(x, dwk, pw, scale, shift, relu_in, relu_out):
    u = _depthwise_ref(x.astype(np.float64), dwk, relu_in)
    v = np.einsum("bihw,io->bohw", u, pw.astype(np.float64)) * scale.astype(np.float64)[None, :, None, None] + shift.astype(np.float64)[None, :, None, None]
    return u, (np.maximum(v, 0) if relu_out else v)


# ------------------------------------------------------------------------------------------------- orcai_sepconv_planes_u / orcai_sepconv_planes
# (Cin, Cout, H, W, ksize_planes, ktap, relu_in, relu_out, out_layout, u_out, odd H2 / W2): the branch each shape reaches
SEP_CASES = {
    "k5 forward, 4 windows per row, 2 output tiles, u kept": (16, 30, 5, 171, 5, 5, 1, 0, 0, True, False),
    "k7 forward, row pitch 176, 58 valid lanes, 4 tiles, ragged quads": (30, 50, 8, 171, 7, 7, 0, 1, 0, True, False),
    "k7, one image row, the last window hangs over the row pitch, no u (orcai_sepconv_planes)": (7, 16, 1, 65, 7, 7, 1, 1, 0, False, False),
    "k5, one window covers three rows of W = 21": (16, 7, 8, 21, 5, 5, 0, 0, 0, True, False),
    "pointwise pass on k7 planes (du = Wpw dv), 64 valid lanes": (50, 30, 5, 171, 7, 1, 0, 0, 0, False, False),
    "taps narrower than the padding: ktap 5 on k7 planes": (16, 16, 5, 65, 7, 5, 1, 0, 0, True, False),
    "taps narrower than the padding: ktap 3 on k5 planes, W = 64": (30, 16, 8, 64, 5, 3, 0, 1, 0, False, False),
    "k5 final conv, Keras Reshape layout": (30, 50, 8, 65, 5, 5, 0, 0, 1, True, False),
    "k7 final conv, Keras Reshape layout, ragged output quad": (16, 7, 5, 171, 7, 7, 1, 1, 1, False, False),
    "k5 x-pooled output (windows start on even pixels, lo 2)": (16, 30, 5, 171, 5, 5, 1, 0, 2, False, False),
    "k7 x-pooled output (lo 4), odd width": (30, 16, 8, 65, 7, 7, 0, 1, 2, False, False),
    "scatter-add to (2y, 2x), even image, k5 planes": (30, 16, 8, 64, 5, 1, 0, 0, 3, False, False),
    "scatter-add to (2y, 2x), odd image H2 = 2H - 1, W2 = 2W - 1, k7 planes": (16, 7, 5, 86, 7, 1, 0, 0, 3, False, True),
    "scatter-add to (2y, 2x), 171 -> 86 columns of k7 planes, 4 tiles": (50, 50, 1, 86, 7, 1, 0, 0, 3, False, True),
}


def _sep_launch(lib, N, use_u, xd, Cin, H, W, kp, ktap, relu_in, dwd, pwd, scd, shd, Cout, relu_out, layout, H2, W2, out, u):
    if use_u:
        return lib.orcai_sepconv_planes_u(N.ptr(xd), B, Cin, H, W, kp, ktap, relu_in, N.ptr(dwd), N.ptr(pwd), N.ptr(scd), N.ptr(shd), Cout, relu_out, layout, H2, W2,
                                          N.ptr(out), None if u is None else N.ptr(u), N.stream_ptr())
    return lib.orcai_sepconv_planes(N.ptr(xd), B, Cin, H, W, kp, ktap, relu_in, N.ptr(dwd), N.ptr(pwd), N.ptr(scd), N.ptr(shd), Cout, relu_out, layout, H2, W2, N.ptr(out),
                                    N.stream_ptr())


def _sep_case(name, exact):
    from orcai_amd import _native as N

    lib = N.lib()
    Cin, Cout, H, W, kp, ktap, relu_in, relu_out, layout, with_u, odd = SEP_CASES[name]
    rng = np.random.default_rng(Cin * 1000 + Cout * 10 + W + ktap)
    if exact:
        x, dwk, pw = _ints(rng, B, Cin, H, W), _ints(rng, ktap, ktap, Cin), _ints(rng, Cin, Cout)
        scale, shift = rng.choice([0.5, 1.0, 2.0], size=Cout).astype(np.float32), _ints(rng, Cout)
    else:
        x, dwk, pw = rng.standard_normal((B, Cin, H, W)).astype(np.float32), (rng.standard_normal((ktap, ktap, Cin)) / ktap).astype(np.float32), (rng.standard_normal((Cin, Cout)) / 4).astype(np.float32)
        scale, shift = (1 + 0.3 * rng.standard_normal(Cout)).astype(np.float32), (0.2 * rng.standard_normal(Cout)).astype(np.float32)
    u_ref, v_ref = _sep_ref(x, dwk, pw, scale, shift, relu_in, relu_out)
    xd, dwd, pwd, scd, shd = _dev(_quad_planes(x, kp)), _dev(_pack_dw(dwk)), _dev(pw), _dev(scale), _dev(shift)
    u = _sentinel_planes(Cin, H, W, kp) if with_u else None
    H2, W2 = (2 * H - 1, 2 * W - 1) if odd else (2 * H, 2 * W)
    if layout == 0:
        out = _sentinel_planes(Cout, H, W, kp)
    elif layout == 1:
        out = torch.full((B, H, W * Cout), SENTINEL, device="cuda")
    elif layout == 2:
        Wx = (W + 1) // 2
        out = torch.full((B, (Cout + 3) // 4, H, (Wx + 3) & ~3, 4), SENTINEL, device="cuda")
    else:
        start = _ints(rng, B, Cout, H2, W2) if exact else rng.standard_normal((B, Cout, H2, W2)).astype(np.float32)
        out = _dev(_quad_planes(start, kp))
    before = out.clone()
    N.check(_sep_launch(lib, N, with_u, xd, Cin, H, W, kp, ktap, relu_in, dwd, pwd, scd, shd, Cout, relu_out, layout, H2, W2, out, u), name)
    torch.cuda.synchronize()
    got = out.cpu().numpy()

    def same(a, ref, what):
        if exact:
            assert np.array_equal(a.astype(np.float64), ref), (name, what, float(np.abs(a - ref).max()))
        else:  # plane outputs of a pointwise contraction: the bound _pw_wgrad_case (tests/test_train_fused_gpu.py) holds du to
            assert np.abs(a - ref).max() <= 1e-4 * max(1.0, np.abs(ref).max()), (name, what, float(np.abs(a - ref).max()))

    if layout == 0:
        same(_from_quad(got, Cout, H, W, kp), v_ref, "out")
        assert _pads(got, Cout, H, W, kp) == 0.0, name
    elif layout == 1:
        same(got.reshape(B, H, W, Cout).transpose(0, 3, 1, 2), v_ref, "features")
    elif layout == 2:
        Wx = (W + 1) // 2
        pairs = np.full((B, Cout, H, 2 * Wx), -np.inf)
        pairs[..., :W] = v_ref
        full = got.transpose(0, 1, 4, 2, 3).reshape(B, -1, H, got.shape[3])
        same(full[:, :Cout, :, :Wx], pairs.reshape(B, Cout, H, Wx, 2).max(axis=4), "x-pooled")
        assert np.all(full[:, :, :, Wx:] == SENTINEL), name  # the columns past ceil(W / 2) are nobody's
    else:
        want = start.astype(np.float64)
        want[:, :, : 2 * H : 2, : 2 * W : 2] += v_ref
        same(_from_quad(got, Cout, H2, W2, kp), want, "scatter-add")
        assert _pads(got, Cout, H2, W2, kp) == 0.0, name
    if with_u:
        ug = u.cpu().numpy()
        same(_from_quad(ug, Cin, H, W, kp), u_ref, "u")
        assert _pads(ug, Cin, H, W, kp) == 0.0, name
    return lib, N, (xd, Cin, H, W, kp, ktap, relu_in, dwd, pwd, scd, shd, Cout, relu_out, layout, H2, W2), before


@pytest.mark.parametrize("name", list(SEP_CASES))
def test_sepconv_planes_exact(name):
    _sep_case(name, exact=True)


@pytest.mark.parametrize("name", list(SEP_CASES))
def test_sepconv_planes_standard_normal(name):
    _sep_case(name, exact=False)


def test_sepconv_planes_refuses_bad_arguments():
    name = "scatter-add to (2y, 2x), even image, k5 planes"
    lib, N, a, before = _sep_case(name, exact=True)
    xd, Cin, H, W, kp, ktap, relu_in, dwd, pwd, scd, shd, Cout, relu_out, layout, H2, W2 = a
    out = before.clone()
    st = N.stream_ptr()

    def call(**kw):
        v = dict(x=N.ptr(xd), B=B, Cin=Cin, H=H, W=W, kp=kp, ktap=ktap, dw=N.ptr(dwd), Cout=Cout, layout=layout, H2=H2, W2=W2)
        v.update(kw)
        return lib.orcai_sepconv_planes_u(v["x"], v["B"], v["Cin"], v["H"], v["W"], v["kp"], v["ktap"], relu_in, v["dw"], N.ptr(pwd), N.ptr(scd), N.ptr(shd), v["Cout"], relu_out,
                                          v["layout"], v["H2"], v["W2"], N.ptr(out), None, st)

    assert call(x=None) == N.E_BADARG and call(dw=None) == N.E_BADARG and call(B=0) == N.E_BADARG and call(W=-1) == N.E_BADARG and call(Cout=0) == N.E_BADARG
    assert call(H2=2 * H - 2) == N.E_BADARG and call(W2=2 * W - 2) == N.E_BADARG  # the image the scatter-add targets must hold pixel (2H - 2, 2W - 2)
    assert call(Cout=65) == N.E_UNSUPPORTED and call(ktap=4) == N.E_UNSUPPORTED and call(ktap=7) == N.E_UNSUPPORTED  # (taps wider than the planes' padding)
    assert call(x=N.ptr(xd) + 4) == N.E_UNSUPPORTED  # misaligned planes
    torch.cuda.synchronize()
    assert torch.equal(out, before)


# ------------------------------------------------------------------------------------------------- orcai_dw_wgrad
# (C, H, W, ksize_planes, ktap, relu_in)
DW_CASES = {
    "k7, row pitch 176, 58 valid lanes": (30, 8, 171, 7, 7, 1),
    "k5, four windows per row": (16, 5, 171, 5, 5, 0),
    "k7, one image row, ragged quad": (7, 1, 65, 7, 7, 1),
    "k5, W = 64": (50, 8, 64, 5, 5, 1),
    "k7, several rows per window": (16, 8, 21, 7, 7, 0),
    "ktap 3 on planes padded for 5 (flat kernel, not the marching one)": (30, 5, 171, 5, 3, 1),
    "ktap 5 on planes padded for 7": (16, 5, 65, 7, 5, 0),
}


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "normal"])
@pytest.mark.parametrize("name", list(DW_CASES))
def test_dw_wgrad_wide_kernels(name, exact):
    """dW[tap][c] += sum r[c][p + off(tap)] * du[c][p]: the formula of test_marching_depthwise_weight_gradient generalised to k, on top of a
    non-zero start.  Standard-normal inputs at that test's `tol`."""
    from orcai_amd import _native as N

    lib = N.lib()
    C, H, W, kp, ktap, relu = DW_CASES[name]
    rng = np.random.default_rng(C + W + ktap)
    x, du = (_ints(rng, B, C, H, W), _ints(rng, B, C, H, W)) if exact else (rng.standard_normal((B, C, H, W)).astype(np.float32), rng.standard_normal((B, C, H, W)).astype(np.float32))
    R = ktap // 2
    xr = np.maximum(x, 0) if relu else x
    xp = np.zeros((B, C, H + 2 * R, W + 2 * R))
    xp[:, :, R : R + H, R : R + W] = xr
    want = np.stack([[np.einsum("bchw,bchw->c", xp[:, :, dy : dy + H, dx : dx + W], du.astype(np.float64)) for dx in range(ktap)] for dy in range(ktap)]).reshape(ktap * ktap, C)
    xd, dud = _dev(_quad_planes(x, kp)), _dev(_quad_planes(du, kp))
    dW = torch.full((ktap * ktap, C), 3.0, device="cuda")  # the launcher ACCUMULATES into the gradient buffer
    N.check(lib.orcai_dw_wgrad(N.ptr(xd), N.ptr(dud), B, C, H, W, kp, ktap, relu, N.ptr(dW), N.stream_ptr()), name)
    got = dW.cpu().numpy().astype(np.float64) - 3.0
    if exact:
        assert np.array_equal(got, want), (name, float(np.abs(got - want).max()))
    else:
        tol = 2e-5 * np.sqrt(B * H * W) * max(1.0, np.abs(want).max() / np.sqrt(B * H * W))
        assert np.abs(got - want).max() <= max(tol, 1e-4 * np.abs(want).max()), (name, float(np.abs(got - want).max()), float(np.abs(want).max()))
    # bad arguments: refused before anything is launched
    before = dW.clone()
    st = N.stream_ptr()
    assert lib.orcai_dw_wgrad(None, N.ptr(dud), B, C, H, W, kp, ktap, relu, N.ptr(dW), st) == N.E_BADARG
    assert lib.orcai_dw_wgrad(N.ptr(xd), N.ptr(dud), 0, C, H, W, kp, ktap, relu, N.ptr(dW), st) == N.E_BADARG
    assert lib.orcai_dw_wgrad(N.ptr(xd), N.ptr(dud), B, C, H, W, kp, kp + 2, relu, N.ptr(dW), st) == N.E_BADARG  # taps wider than the padding
    assert lib.orcai_dw_wgrad(N.ptr(xd), N.ptr(dud), B, C, H, W, kp, 4 if kp > 4 else 2, relu, N.ptr(dW), st) == N.E_UNSUPPORTED
    torch.cuda.synchronize()
    assert torch.equal(dW, before)


# ------------------------------------------------------------------------------------------------- orcai_outer_reduce
# (Ca, Cb, H, W, ksize, a_stride2, odd Ha / Wa, workspace in units of Ca * Cb floats)
OUTER_CASES = {
    "k7 pointwise weight gradient, 128-pixel passes (7 tiles)": (50, 50, 8, 171, 7, 0, False, 512),
    "k5, 256-pixel passes": (16, 30, 5, 171, 5, 0, False, 512),
    "k5 residual weight gradient: A sampled at (2i, 2j) of an odd image": (16, 30, 8, 65, 5, 1, True, 512),
    "k7 residual weight gradient, even image, ragged quad": (7, 16, 5, 64, 7, 1, False, 512),
    "k7 residual weight gradient, odd image, one row": (30, 50, 1, 86, 7, 1, True, 768),
    "a workspace for three workgroups only": (30, 30, 8, 171, 7, 0, False, 3),
    "a workspace for one workgroup, stride 2": (16, 7, 5, 21, 5, 1, True, 1),
}


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "normal"])
@pytest.mark.parametrize("name", list(OUTER_CASES))
def test_outer_reduce_wide_kernels(name, exact):
    """D[ca][cb] += sum over snippets and pixels of A[ca][p] * Bq[cb][p] on top of a non-zero D.  Standard-normal inputs at the bound
    _pw_wgrad_case (tests/test_train_fused_gpu.py) holds the same reduction to: 2e-5 * max(1, max|ref|) * sqrt(n / 64 + 1)."""
    from orcai_amd import _native as N

    lib = N.lib()
    Ca, Cb, H, W, k, stride2, odd, ws_units = OUTER_CASES[name]
    rng = np.random.default_rng(Ca + Cb + W)
    Ha, Wa = ((2 * H - 1, 2 * W - 1) if odd else (2 * H, 2 * W)) if stride2 else (H, W)
    draw = (lambda *s: _ints(rng, *s)) if exact else (lambda *s: rng.standard_normal(s).astype(np.float32))
    a, b = draw(B, Ca, Ha, Wa), draw(B, Cb, H, W)
    asub = a[:, :, ::2, ::2][:, :, :H, :W] if stride2 else a
    want = np.einsum("bchw,bdhw->cd", asub.astype(np.float64), b.astype(np.float64))
    ad, bd = _dev(_quad_planes(a, k)), _dev(_quad_planes(b, k))
    D = torch.full((Ca, Cb), 2.0, device="cuda")
    ws = torch.full((ws_units * Ca * Cb,), float("nan"), device="cuda")
    st = N.stream_ptr()
    N.check(lib.orcai_outer_reduce(N.ptr(ad), Ca, N.ptr(bd), Cb, B, H, W, k, stride2, Ha if stride2 else 0, Wa if stride2 else 0, N.ptr(D), N.ptr(ws), ws.numel(), st), name)
    got = D.cpu().numpy().astype(np.float64) - 2.0
    if exact:
        assert np.array_equal(got, want), (name, float(np.abs(got - want).max()))
    else:
        n = B * H * W
        assert np.abs(got - want).max() <= 2e-5 * max(1.0, np.abs(want).max()) * np.sqrt(n / 64 + 1), (name, float(np.abs(got - want).max()), float(np.abs(want).max()))
    before = D.clone()
    assert lib.orcai_outer_reduce(N.ptr(ad), Ca, N.ptr(bd), Cb, B, H, W, k, stride2, Ha, Wa, N.ptr(D), N.ptr(ws), Ca * Cb - 1, st) == N.E_BADARG
    assert lib.orcai_outer_reduce(N.ptr(ad), 65, N.ptr(bd), Cb, B, H, W, k, stride2, Ha, Wa, N.ptr(D), N.ptr(ws), ws.numel(), st) == N.E_BADARG
    assert lib.orcai_outer_reduce(N.ptr(ad), Ca, None, Cb, B, H, W, k, stride2, Ha, Wa, N.ptr(D), N.ptr(ws), ws.numel(), st) == N.E_BADARG
    assert lib.orcai_outer_reduce(N.ptr(ad), Ca, N.ptr(bd), Cb, B, H, W, k, 1, 2 * H - 2, 2 * W, N.ptr(D), N.ptr(ws), ws.numel(), st) == N.E_BADARG
    torch.cuda.synchronize()
    assert torch.equal(D, before)


# ------------------------------------------------------------------------------------------------- orcai_bn_planes_stats / _apply / _bwd
@pytest.mark.parametrize("C,H,W,k,relu", [(30, 8, 171, 7, 1), (7, 5, 65, 5, 0), (50, 1, 64, 3, 1), (16, 8, 21, 5, 1), (50, 8, 171, 5, 0), (16, 5, 86, 7, 1)])
def test_bn_planes_wide_kernels(C, H, W, k, relu):
    """Batch mean / biased variance, y = [relu](BN(v)) and the backward (dbeta, dgamma, dv) as _pw_wgrad_case (tests/test_train_fused_gpu.py) computes
    them in float64.  Bounds: statistics at _check_step's 2e-5 * max(1, max|ref|) (tests/test_train_full_gpu.py); plane outputs at _pw_wgrad_case's
    1e-4 * max(1, max|ref|); the two backward sums at its 2e-5 * max(1, max|ref|) * sqrt(n / 64 + 1)."""
    from orcai_amd import _native as N

    lib = N.lib()
    rng = np.random.default_rng(C * 7 + W + k)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)  # noqa: E731
    v, dy = 2.0 * f(B, C, H, W) + 0.5, f(B, C, H, W)
    gamma, beta = 1 + 0.3 * f(C), 0.2 * f(C)
    gamma[0] = -gamma[0]
    st = N.stream_ptr()
    vd, gd, bd = _dev(_quad_planes(v, k)), _dev(gamma), _dev(beta)
    n = B * H * W
    v64 = v.astype(np.float64)
    mean_ref, var_ref = v64.mean(axis=(0, 2, 3)), v64.var(axis=(0, 2, 3))
    mean, var = torch.full((C,), SENTINEL, device="cuda"), torch.full((C,), SENTINEL, device="cuda")
    scratch = torch.full((8 * ((C + 3) // 4) * 32,), 5.0, dtype=torch.float64, device="cuda")  # (the launcher clears what it uses)
    N.check(lib.orcai_bn_planes_stats(N.ptr(vd), B, C, H, W, k, N.ptr(scratch), N.ptr(mean), N.ptr(var), st), "bn_planes_stats")
    gm, gv = mean.cpu().numpy(), var.cpu().numpy()
    assert np.abs(gm - mean_ref).max() <= 2e-5 * max(1.0, np.abs(mean_ref).max()) and np.abs(gv - var_ref).max() <= 2e-5 * max(1.0, np.abs(var_ref).max())
    # apply and backward with the launcher's own f32 statistics (the reference takes the same numbers)
    inv = 1.0 / np.sqrt(gv.astype(np.float64) + 1e-3)
    xh = (v64 - gm[None, :, None, None]) * inv[None, :, None, None]
    y_ref = xh * gamma[None, :, None, None] + beta[None, :, None, None]
    y = _sentinel_planes(C, H, W, k)
    N.check(lib.orcai_bn_planes_apply(N.ptr(vd), B, C, H, W, k, N.ptr(mean), N.ptr(var), N.ptr(gd), N.ptr(bd), 1e-3, relu, N.ptr(y), st), "bn_planes_apply")
    yg = y.cpu().numpy()
    want = np.maximum(y_ref, 0) if relu else y_ref
    assert np.abs(_from_quad(yg, C, H, W, k) - want).max() <= 1e-4 * max(1.0, np.abs(want).max())
    assert _pads(yg, C, H, W, k) == 0.0
    if relu:  # no gradient where the ReLU decision lies within f32 rounding of zero, so that the float64 mask is the kernel's
        dy = dy * (np.abs(y_ref) > 1e-4).astype(np.float32)
    dyd = _dev(_quad_planes(dy, k))
    de = np.where(y_ref > 0, dy.astype(np.float64), 0.0) if relu else dy.astype(np.float64)
    dbeta_ref, dgamma_ref = de.sum(axis=(0, 2, 3)), (de * xh).sum(axis=(0, 2, 3))
    dv_ref = (gamma * inv)[None, :, None, None] * (de - dbeta_ref[None, :, None, None] / n - xh * dgamma_ref[None, :, None, None] / n)
    dbeta, dgamma, dv = torch.full((C,), SENTINEL, device="cuda"), torch.full((C,), SENTINEL, device="cuda"), _sentinel_planes(C, H, W, k)
    N.check(lib.orcai_bn_planes_bwd(N.ptr(dyd), N.ptr(vd), B, C, H, W, k, N.ptr(mean), N.ptr(var), N.ptr(gd), N.ptr(bd), 1e-3, relu, N.ptr(scratch), N.ptr(dbeta), N.ptr(dgamma),
                                    N.ptr(dv), st), "bn_planes_bwd")
    sum_tol = 2e-5 * np.sqrt(n / 64 + 1)
    assert np.abs(dbeta.cpu().numpy() - dbeta_ref).max() <= sum_tol * max(1.0, np.abs(dbeta_ref).max())
    assert np.abs(dgamma.cpu().numpy() - dgamma_ref).max() <= sum_tol * max(1.0, np.abs(dgamma_ref).max())
    dvg = dv.cpu().numpy()
    assert np.abs(_from_quad(dvg, C, H, W, k) - dv_ref).max() <= 1e-4 * max(1.0, np.abs(dv_ref).max())
    assert _pads(dvg, C, H, W, k) == 0.0
    # bad arguments
    before = (mean.clone(), y.clone(), dv.clone())
    assert lib.orcai_bn_planes_stats(None, B, C, H, W, k, N.ptr(scratch), N.ptr(mean), N.ptr(var), st) == N.E_BADARG
    assert lib.orcai_bn_planes_stats(N.ptr(vd), B, 65, H, W, k, N.ptr(scratch), N.ptr(mean), N.ptr(var), st) == N.E_BADARG
    assert lib.orcai_bn_planes_apply(N.ptr(vd), 0, C, H, W, k, N.ptr(mean), N.ptr(var), N.ptr(gd), N.ptr(bd), 1e-3, relu, N.ptr(y), st) == N.E_BADARG
    assert lib.orcai_bn_planes_apply(N.ptr(vd), B, C, H, W, k, N.ptr(mean), None, N.ptr(gd), N.ptr(bd), 1e-3, relu, N.ptr(y), st) == N.E_BADARG
    assert lib.orcai_bn_planes_bwd(N.ptr(dyd), N.ptr(vd), B, 65, H, W, k, N.ptr(mean), N.ptr(var), N.ptr(gd), N.ptr(bd), 1e-3, relu, N.ptr(scratch), N.ptr(dbeta), N.ptr(dgamma),
                                   N.ptr(dv), st) == N.E_BADARG
    assert lib.orcai_bn_planes_bwd(N.ptr(dyd), N.ptr(vd), B, C, 0, W, k, N.ptr(mean), N.ptr(var), N.ptr(gd), N.ptr(bd), 1e-3, relu, N.ptr(scratch), N.ptr(dbeta), N.ptr(dgamma),
                                   N.ptr(dv), st) == N.E_BADARG
    torch.cuda.synchronize()
    assert torch.equal(mean, before[0]) and torch.equal(y, before[1]) and torch.equal(dv, before[2])


# ------------------------------------------------------------------------------------------------- orcai_pool_res_add_bn
# (C, Cp, H, W, ksize, xpooled, BatchNorm on the fly)
POOL_CASES = {
    "k5, 171 -> 86 columns, two output tiles": (30, 16, 8, 171, 5, 0, False),
    "k7, odd height and width, four tiles, ragged quads": (50, 30, 5, 65, 7, 0, False),
    "k7, x-pooled input, even sizes": (16, 7, 8, 64, 7, 1, False),
    "k5, x-pooled input, odd sizes": (30, 16, 5, 21, 5, 1, False),
    "k7 training forward: BatchNorm on the fly, 171 -> 86 columns": (30, 16, 8, 171, 7, 0, True),
    "k5 training forward, odd sizes, ragged quad": (7, 16, 5, 65, 5, 0, True),
    "k5 training forward, one row": (50, 50, 1, 171, 5, 0, True),
    "k7 training forward, W = 64": (16, 30, 8, 64, 7, 0, True),
}


@pytest.mark.parametrize("name", list(POOL_CASES))
def test_pool_res_add_bn_wide_kernels(name):
    """MaxPooling2D((3, 2), 2, "same")(BN(s)) + Conv2D(C, 1, strides 2)(prev) + bias with TensorFlow's "same" padding (oracle.model_ref.same_pad).
    Without BatchNorm: small integers, exact.  With BatchNorm (gamma of both signs): standard normal at the plane-output bound of _pw_wgrad_case
    (tests/test_train_fused_gpu.py), 1e-4 * max(1, max|ref|)."""
    from orcai_amd import _native as N

    lib = N.lib()
    C, Cp, H, W, k, xpooled, bn = POOL_CASES[name]
    rng = np.random.default_rng(C + Cp + W + k)
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    if bn:
        s, prev = (2.0 * rng.standard_normal((B, C, H, W))).astype(np.float32), rng.standard_normal((B, Cp, H, W)).astype(np.float32)
        wr, br = (rng.standard_normal((Cp, C)) / 4).astype(np.float32), (0.2 * rng.standard_normal(C)).astype(np.float32)
        mean, var = (0.3 * rng.standard_normal(C)).astype(np.float32), (0.5 + rng.random(C)).astype(np.float32)
        gamma, beta = rng.standard_normal(C).astype(np.float32), (0.2 * rng.standard_normal(C)).astype(np.float32)  # both signs: max BN(v) = BN(min v) where gamma < 0
        sc = gamma.astype(np.float64) / np.sqrt(var.astype(np.float64) + 1e-3)
        t = s.astype(np.float64) * sc[None, :, None, None] + (beta - mean * sc)[None, :, None, None]
    else:
        s, prev, wr, br = _ints(rng, B, C, H, W), _ints(rng, B, Cp, H, W), _ints(rng, Cp, C), _ints(rng, C)
        t = s.astype(np.float64)
    _, pt, pb = same_pad(H, 3, 2)
    _, pl, pr = same_pad(W, 2, 2)
    tp = np.pad(t, ((0, 0), (0, 0), (pt, pb), (pl, pr)), constant_values=-np.inf)
    pooled = np.stack([tp[:, :, dy : dy + 2 * Ho : 2, dx : dx + 2 * Wo : 2] for dy in range(3) for dx in range(2)], axis=-1).max(axis=-1)
    want = pooled + np.einsum("bihw,io->bohw", prev[:, :, ::2, ::2].astype(np.float64), wr.astype(np.float64)) + br.astype(np.float64)[None, :, None, None]
    if xpooled:  # the layout orcai_sepconv_bn(out_layout = 2) writes: [B][CQ][H][roundup4(ceil(W / 2))][4], max over the column pair (2j, 2j + 1)
        pairs = np.full((B, C, H, 2 * Wo), -np.inf, dtype=np.float32)
        pairs[..., :W] = s
        xp = pairs.reshape(B, C, H, Wo, 2).max(axis=4)
        CQ, WPx = (C + 3) // 4, (Wo + 3) & ~3
        buf = np.zeros((B, CQ * 4, H, WPx), dtype=np.float32)
        buf[:, :C, :, :Wo] = xp
        sd = _dev(buf.reshape(B, CQ, 4, H, WPx).transpose(0, 1, 3, 4, 2))
    else:
        sd = _dev(_quad_planes(s, k))
    pd, wd, bd = _dev(_quad_planes(prev, k)), _dev(wr), _dev(br)
    out = _sentinel_planes(C, Ho, Wo, k)
    bnd = [_dev(a) for a in (mean, var, gamma, beta)] if bn else []  # (kept alive over the launch)
    bnp = [N.ptr(t_) for t_ in bnd] if bn else [None] * 4
    st = N.stream_ptr()
    N.check(lib.orcai_pool_res_add_bn(N.ptr(sd), N.ptr(pd), B, C, Cp, H, W, k, N.ptr(wd), N.ptr(bd), N.ptr(out), xpooled, *bnp, 1e-3, st), name)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    g = _from_quad(got, C, Ho, Wo, k)
    if bn:
        assert np.abs(g - want).max() <= 1e-4 * max(1.0, np.abs(want).max()), (name, float(np.abs(g - want).max()))
    else:
        assert np.array_equal(g.astype(np.float64), want), (name, float(np.abs(g - want).max()))
    assert _pads(got, C, Ho, Wo, k) == 0.0, name
    before = out.clone()
    assert lib.orcai_pool_res_add_bn(None, N.ptr(pd), B, C, Cp, H, W, k, N.ptr(wd), N.ptr(bd), N.ptr(out), xpooled, *bnp, 1e-3, st) == N.E_BADARG
    assert lib.orcai_pool_res_add_bn(N.ptr(sd), N.ptr(pd), B, C, 0, H, W, k, N.ptr(wd), N.ptr(bd), N.ptr(out), xpooled, *bnp, 1e-3, st) == N.E_BADARG
    assert lib.orcai_pool_res_add_bn(N.ptr(sd), N.ptr(pd), B, C, Cp, H, W, k, N.ptr(wd), N.ptr(bd), N.ptr(out), 4, *bnp, 1e-3, st) == N.E_BADARG
    assert lib.orcai_pool_res_add_bn(N.ptr(sd), N.ptr(pd), B, 65, Cp, H, W, k, N.ptr(wd), N.ptr(bd), N.ptr(out), xpooled, *bnp, 1e-3, st) == N.E_UNSUPPORTED
    if bn:  # BatchNorm on the fly reads planes, never the x-pooled tensor; and needs all four parameter vectors
        assert lib.orcai_pool_res_add_bn(N.ptr(sd), N.ptr(pd), B, C, Cp, H, W, k, N.ptr(wd), N.ptr(bd), N.ptr(out), 1, *bnp, 1e-3, st) == N.E_BADARG
        assert lib.orcai_pool_res_add_bn(N.ptr(sd), N.ptr(pd), B, C, Cp, H, W, k, N.ptr(wd), N.ptr(bd), N.ptr(out), 0, bnp[0], None, bnp[2], bnp[3], 1e-3, st) == N.E_BADARG
    torch.cuda.synchronize()
    assert torch.equal(out, before)


# ------------------------------------------------------------------------------------------------- orcai_pool_bwd_bn_bias
@pytest.mark.parametrize("ties", [True, False], ids=["ties", "normal"])
@pytest.mark.parametrize("C,H,W,k", [(30, 8, 171, 7), (16, 5, 65, 5), (7, 1, 64, 7), (50, 8, 21, 5), (16, 5, 171, 5)])
def test_pool_bwd_bn_bias_wide_kernels(C, H, W, k, ties):
    """The max-pool backward with bn_b's backward sums and the residual bias gradient, against float64 (torch autograd's max_pool2d backward routes a
    window's gradient to its first maximum in scan order, as the kernel does): small integers full of ties -- exact --, and standard normal, where dy
    is a routing of f32 values (exact as well) and the three reductions are held to 1e-5 * max(1, max|ref|) (the dbias bound of
    test_pool_bwd_h_vs_f32_twin; the sums are accumulated in f64)."""
    import torch.nn.functional as F

    from orcai_amd import _native as N

    lib = N.lib()
    rng = np.random.default_rng(C + W + k)
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    if ties:
        v, dout = _ints(rng, B, C, H, W, lo=-2, hi=2), _ints(rng, B, C, Ho, Wo)
        mean, var = np.zeros(C, dtype=np.float32), np.ones(C, dtype=np.float32)
    else:
        v, dout = (2.0 * rng.standard_normal((B, C, H, W))).astype(np.float32), rng.standard_normal((B, C, Ho, Wo)).astype(np.float32)
        mean, var = (0.3 * rng.standard_normal(C)).astype(np.float32), (0.5 + rng.random(C)).astype(np.float32)
    gamma = rng.standard_normal(C).astype(np.float32)  # both signs: the arg-max is taken on sign(gamma) * v
    sgn = np.where(gamma < 0, -1.0, 1.0)
    x = torch.tensor(v.astype(np.float64) * sgn[None, :, None, None], requires_grad=True)
    _, pt, pb = same_pad(H, 3, 2)
    _, pl, pr = same_pad(W, 2, 2)
    F.max_pool2d(F.pad(x, (pl, pr, pt, pb), value=float("-inf")), kernel_size=(3, 2), stride=2).backward(torch.tensor(dout.astype(np.float64)))
    want = x.grad.numpy()
    xh = (v.astype(np.float64) - mean[None, :, None, None]) / np.sqrt(var.astype(np.float64) + 1e-3)[None, :, None, None]
    CQ = (C + 3) // 4
    dd, vv, gd, md, vd = _dev(_quad_planes(dout, k)), _dev(_quad_planes(v, k)), _dev(gamma), _dev(mean), _dev(var)
    dy = _sentinel_planes(C, H, W, k)
    sums, dsum = torch.full((8 * CQ,), 5.0, dtype=torch.float64, device="cuda"), torch.full((4 * CQ,), 5.0, dtype=torch.float64, device="cuda")
    dbias = torch.full((C,), SENTINEL, device="cuda")
    st = N.stream_ptr()
    N.check(lib.orcai_pool_bwd_bn_bias(N.ptr(dd), N.ptr(vv), B, C, H, W, k, N.ptr(dy), N.ptr(gd), N.ptr(md), N.ptr(vd), 1e-3, N.ptr(sums), N.ptr(dsum), N.ptr(dbias), st), "pool_bwd_bn_bias")
    torch.cuda.synchronize()
    got = dy.cpu().numpy()
    g = _from_quad(got, C, H, W, k)
    assert np.array_equal(g, want.astype(np.float32)), float(np.abs(g - want).max())  # (a pixel collects at most two windows' gradients: one correctly rounded f32 addition)
    assert _pads(got, C, H, W, k) == 0.0
    s = sums.cpu().numpy()
    for a, ref, what in ((s[:C], want.sum(axis=(0, 2, 3)), "sum dy"), (s[4 * CQ : 4 * CQ + C], (want * xh).sum(axis=(0, 2, 3)), "sum dy * xhat"),
                         (dbias.cpu().numpy(), dout.astype(np.float64).sum(axis=(0, 2, 3)), "dbias")):
        assert np.abs(a - ref).max() <= 1e-5 * max(1.0, np.abs(ref).max()), (what, float(np.abs(a - ref).max()))
    before = dy.clone()
    assert lib.orcai_pool_bwd_bn_bias(N.ptr(dd), N.ptr(vv), B, C, H, W, k, N.ptr(dy), N.ptr(gd), N.ptr(md), N.ptr(vd), 1e-3, N.ptr(sums), None, N.ptr(dbias), st) == N.E_BADARG
    assert lib.orcai_pool_bwd_bn_bias(N.ptr(dd), N.ptr(vv), B, C, H, W, k, N.ptr(dy), None, N.ptr(md), N.ptr(vd), 1e-3, N.ptr(sums), N.ptr(dsum), N.ptr(dbias), st) == N.E_BADARG
    assert lib.orcai_pool_bwd_bn_bias(N.ptr(dd), N.ptr(vv), B, 65, H, W, k, N.ptr(dy), N.ptr(gd), N.ptr(md), N.ptr(vd), 1e-3, N.ptr(sums), N.ptr(dsum), N.ptr(dbias), st) == N.E_BADARG
    torch.cuda.synchronize()
    assert torch.equal(dy, before)


# ------------------------------------------------------------------------------------------------- orcai_planes_relu_bwd / orcai_feat_to_planes
@pytest.mark.parametrize("C,H,W,k", [(30, 8, 171, 7), (7, 5, 65, 5), (50, 1, 64, 7), (16, 8, 21, 5)])
def test_planes_relu_bwd_and_feat_to_planes_exact(C, H, W, k):
    """dx = (y > 0) ? dy : 0 on whole plane buffers (in place, as the training step calls it) and the Keras-Reshape -> planes copy: pure selections
    and copies, so any input is exact."""
    from orcai_amd import _native as N

    lib = N.lib()
    rng = np.random.default_rng(C + W)
    st = N.stream_ptr()
    y, dy = _ints(rng, B, C, H, W, lo=-2, hi=2), rng.standard_normal((B, C, H, W)).astype(np.float32)
    yd, dyd = _dev(_quad_planes(y, k)), _dev(_quad_planes(dy, k))
    N.check(lib.orcai_planes_relu_bwd(N.ptr(dyd), N.ptr(yd), dyd.numel(), N.ptr(dyd), st), "planes_relu_bwd")
    got = dyd.cpu().numpy()
    assert np.array_equal(_from_quad(got, C, H, W, k), np.where(y > 0, dy, 0.0).astype(np.float32)) and _pads(got, C, H, W, k) == 0.0
    before = dyd.clone()
    assert lib.orcai_planes_relu_bwd(N.ptr(dyd), N.ptr(yd), dyd.numel() - 2, N.ptr(dyd), st) == N.E_BADARG
    assert lib.orcai_planes_relu_bwd(N.ptr(dyd), None, dyd.numel(), N.ptr(dyd), st) == N.E_BADARG and lib.orcai_planes_relu_bwd(N.ptr(dyd), N.ptr(yd), 0, N.ptr(dyd), st) == N.E_BADARG
    f = rng.standard_normal((B, H, W, C)).astype(np.float32)  # feature = x * C + c
    fd, out = _dev(f.reshape(B, H, W * C)), _sentinel_planes(C, H, W, k)
    N.check(lib.orcai_feat_to_planes(N.ptr(fd), B, C, H, W, k, N.ptr(out), st), "feat_to_planes")
    got = out.cpu().numpy()
    assert np.array_equal(_from_quad(got, C, H, W, k), f.transpose(0, 3, 1, 2)) and _pads(got, C, H, W, k) == 0.0
    before2 = out.clone()
    assert lib.orcai_feat_to_planes(None, B, C, H, W, k, N.ptr(out), st) == N.E_BADARG and lib.orcai_feat_to_planes(N.ptr(fd), B, 0, H, W, k, N.ptr(out), st) == N.E_BADARG
    torch.cuda.synchronize()
    assert torch.equal(dyd, before) and torch.equal(out, before2)


# ------------------------------------------------------------------------------------------------- the entry conv in two passes, k = 5 / 7
@pytest.mark.parametrize("H,W,k", [(8, 171, 5), (5, 65, 7), (8, 171, 7), (1, 65, 5)])
def test_entry_conv_two_passes_wide_kernels(H, W, k):
    """orcai_conv0_stats / orcai_conv0_affine_bn / orcai_conv0_bn_bwd_x at k = 5 / 7 and W = 65 / 171: the checks of
    test_entry_conv_in_two_passes_without_v0 (which stops at W = 33 / 7) at the wider shapes, and the batch statistics, y0 and the weight gradient
    against float64 (statistics at _check_step's 2e-5 * max(1, max|ref|), y0 at the plane-output bound 1e-4 * max(1, max|ref|), the reductions at
    _pw_wgrad_case's 2e-5 * max(1, max|ref|) * sqrt(n / 64 + 1))."""
    from orcai_amd import _native as N
    from test_train_fused_gpu import _entry_conv_two_passes_case

    _entry_conv_two_passes_case(H, W, B, k)
    lib = N.lib()
    rng = np.random.default_rng(H + W + k)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)  # noqa: E731
    x, w0, bias = rng.random((B, H, W), dtype=np.float32), f(k * k, 16) / k, 0.1 * f(16)
    gamma, beta = 1 + 0.3 * f(16), 0.2 * f(16)
    R = k // 2
    xp = np.zeros((B, H + 2 * R, W + 2 * R))
    xp[:, R : R + H, R : R + W] = x
    v0 = sum(xp[:, None, dy : dy + H, dx : dx + W] * w0[dy * k + dx].astype(np.float64)[None, :, None, None] for dy in range(k) for dx in range(k)) + bias.astype(np.float64)[None, :, None, None]
    xd, wd, bd, ones, gd, btd = _dev(x), _dev(w0), _dev(bias), torch.ones(16, device="cuda"), _dev(gamma), _dev(beta)
    st = N.stream_ptr()
    shards = torch.full((8 * 4 * 32,), 5.0, dtype=torch.float64, device="cuda")
    mean, var = torch.full((16,), SENTINEL, device="cuda"), torch.full((16,), SENTINEL, device="cuda")
    N.check(lib.orcai_conv0_stats(N.ptr(xd), H * W, B, H, W, k, N.ptr(wd), N.ptr(ones), N.ptr(bd), N.ptr(shards), st), "conv0_stats")
    N.check(lib.orcai_bn_finish_sharded(N.ptr(shards), B, 16, H, W, N.ptr(mean), N.ptr(var), st), "bn_finish_sharded")
    gm, gv = mean.cpu().numpy(), var.cpu().numpy()
    mref, vref = v0.mean(axis=(0, 2, 3)), v0.var(axis=(0, 2, 3))
    assert np.abs(gm - mref).max() <= 2e-5 * max(1.0, np.abs(mref).max()) and np.abs(gv - vref).max() <= 2e-5 * max(1.0, np.abs(vref).max())
    inv = 1.0 / np.sqrt(gv.astype(np.float64) + 1e-3)
    xh = (v0 - gm[None, :, None, None]) * inv[None, :, None, None]
    y_ref = xh * gamma[None, :, None, None] + beta[None, :, None, None]
    y0 = _sentinel_planes(16, H, W, k)
    N.check(lib.orcai_conv0_affine_bn(N.ptr(xd), H * W, B, H, W, k, N.ptr(wd), N.ptr(ones), N.ptr(bd), N.ptr(mean), N.ptr(var), N.ptr(gd), N.ptr(btd), 1e-3, 1, N.ptr(y0), st), "conv0_affine_bn")
    yg = y0.cpu().numpy()
    assert np.abs(_from_quad(yg, 16, H, W, k) - np.maximum(y_ref, 0)).max() <= 1e-4 * max(1.0, np.abs(y_ref).max()) and _pads(yg, 16, H, W, k) == 0.0
    # backward: dy zero where the ReLU decision is within rounding of zero, so that the float64 mask is the kernel's
    dy = f(B, 16, H, W) * (np.abs(y_ref) > 1e-4)
    n = B * H * W
    de = np.where(y_ref > 0, dy.astype(np.float64), 0.0)
    dbeta_ref, dgamma_ref = de.sum(axis=(0, 2, 3)), (de * xh).sum(axis=(0, 2, 3))
    dv = (gamma * inv)[None, :, None, None] * (de - dbeta_ref[None, :, None, None] / n - xh * dgamma_ref[None, :, None, None] / n)
    dW_ref = np.stack([np.einsum("bhw,bchw->c", xp[:, dy_ : dy_ + H, dx : dx + W], dv) for dy_ in range(k) for dx in range(k)])
    dbeta, dgamma, dW = torch.full((16,), SENTINEL, device="cuda"), torch.full((16,), SENTINEL, device="cuda"), torch.full((k * k, 16), 0.5, device="cuda")
    scratch, ws = torch.full((1024,), 5.0, dtype=torch.float64, device="cuda"), torch.full((512 * 64 * 64,), float("nan"), device="cuda")
    dyd = _dev(_quad_planes(dy.astype(np.float32), k))
    N.check(lib.orcai_conv0_bn_bwd_x(N.ptr(xd), H * W, N.ptr(dyd), B, H, W, k, N.ptr(wd), N.ptr(bd), N.ptr(mean), N.ptr(var), N.ptr(gd), N.ptr(btd), 1e-3, N.ptr(scratch), N.ptr(dbeta),
                                     N.ptr(dgamma), N.ptr(dW), N.ptr(ws), ws.numel(), st), "conv0_bn_bwd_x")
    torch.cuda.synchronize()
    tol = 2e-5 * np.sqrt(n / 64 + 1)
    for a, ref, what in ((dbeta.cpu().numpy(), dbeta_ref, "dbeta"), (dgamma.cpu().numpy(), dgamma_ref, "dgamma"), (dW.cpu().numpy() - 0.5, dW_ref, "dW0")):
        assert np.abs(a - ref).max() <= tol * max(1.0, np.abs(ref).max()), (what, float(np.abs(a - ref).max()), float(np.abs(ref).max()))
    before = (y0.clone(), dW.clone())
    assert lib.orcai_conv0_stats(None, H * W, B, H, W, k, N.ptr(wd), N.ptr(ones), N.ptr(bd), N.ptr(shards), st) == N.E_BADARG
    assert lib.orcai_conv0_affine_bn(N.ptr(xd), H * W, B, H, W, 4, N.ptr(wd), N.ptr(ones), N.ptr(bd), N.ptr(mean), N.ptr(var), N.ptr(gd), N.ptr(btd), 1e-3, 1, N.ptr(y0), st) == N.E_UNSUPPORTED
    assert lib.orcai_conv0_affine_bn(N.ptr(xd), H * W, 0, H, W, k, N.ptr(wd), N.ptr(ones), N.ptr(bd), N.ptr(mean), N.ptr(var), N.ptr(gd), N.ptr(btd), 1e-3, 1, N.ptr(y0), st) == N.E_BADARG
    assert lib.orcai_conv0_bn_bwd_x(None, H * W, N.ptr(dyd), B, H, W, k, N.ptr(wd), N.ptr(bd), N.ptr(mean), N.ptr(var), N.ptr(gd), N.ptr(btd), 1e-3, N.ptr(scratch), N.ptr(dbeta),
                                    N.ptr(dgamma), N.ptr(dW), N.ptr(ws), ws.numel(), st) < 0
    torch.cuda.synchronize()
    assert torch.equal(y0, before[0]) and torch.equal(dW, before[1])


# ------------------------------------------------------------------------------------------------- orcai_bn_planes_stats, exact
@pytest.mark.parametrize("C,H,W,k", [(30, 8, 64, 5), (7, 8, 64, 7), (50, 4, 128, 7), (16, 8, 64, 3)])
def test_bn_planes_stats_exact(C, H, W, k):
    """Small integers and n = B * H * W = 1024: the sums are integers, mean = sum / 2^10 and variance = sum of squares / 2^10 - mean^2 are exact in the
    float64 the launcher finishes them in (and in numpy's), so the f32 results must equal float32(numpy float64) bit for bit."""
    from orcai_amd import _native as N

    lib = N.lib()
    rng = np.random.default_rng(C + W + k)
    assert B * H * W == 1024
    v = _ints(rng, B, C, H, W)
    vd = _dev(_quad_planes(v, k))
    mean, var = torch.full((C,), SENTINEL, device="cuda"), torch.full((C,), SENTINEL, device="cuda")
    scratch = torch.full((8 * ((C + 3) // 4) * 32,), 5.0, dtype=torch.float64, device="cuda")
    N.check(lib.orcai_bn_planes_stats(N.ptr(vd), B, C, H, W, k, N.ptr(scratch), N.ptr(mean), N.ptr(var), N.stream_ptr()), "bn_planes_stats")
    v64 = v.astype(np.float64)
    assert np.array_equal(mean.cpu().numpy(), v64.mean(axis=(0, 2, 3)).astype(np.float32))
    assert np.array_equal(var.cpu().numpy(), v64.var(axis=(0, 2, 3)).astype(np.float32))


# ------------------------------------------------------------------------------------------------- orcai_conv0_wgrad
@pytest.mark.parametrize("exact", [True, False], ids=["exact", "normal"])
@pytest.mark.parametrize("H,W,k", [(8, 171, 7), (5, 65, 5), (1, 64, 7), (8, 21, 5)])
def test_conv0_wgrad_wide_kernels(H, W, k, exact):
    """dW0[tap][c] += sum in[p + off(tap)] * dv[c][p] on the unpadded snippet, on top of a non-zero start: exact on small integers; standard normal at
    test_marching_depthwise_weight_gradient's `tol` (the same reduction over B * H * W pixels)."""
    from orcai_amd import _native as N

    lib = N.lib()
    rng = np.random.default_rng(H + W + k)
    x, dv = (_ints(rng, B, H, W), _ints(rng, B, 16, H, W)) if exact else (rng.random((B, H, W), dtype=np.float32), rng.standard_normal((B, 16, H, W)).astype(np.float32))
    R = k // 2
    xp = np.zeros((B, H + 2 * R, W + 2 * R))
    xp[:, R : R + H, R : R + W] = x
    want = np.stack([np.einsum("bhw,bchw->c", xp[:, dy : dy + H, dx : dx + W], dv.astype(np.float64)) for dy in range(k) for dx in range(k)])
    xd, dvd = _dev(x), _dev(_quad_planes(dv, k))
    dW = torch.full((k * k, 16), 3.0, device="cuda")
    st = N.stream_ptr()
    N.check(lib.orcai_conv0_wgrad(N.ptr(xd), H * W, N.ptr(dvd), B, H, W, k, N.ptr(dW), st), "conv0_wgrad")
    got = dW.cpu().numpy().astype(np.float64) - 3.0
    if exact:
        assert np.array_equal(got, want), float(np.abs(got - want).max())
    else:
        tol = 2e-5 * np.sqrt(B * H * W) * max(1.0, np.abs(want).max() / np.sqrt(B * H * W))
        assert np.abs(got - want).max() <= max(tol, 1e-4 * np.abs(want).max()), (float(np.abs(got - want).max()), float(np.abs(want).max()))
    before = dW.clone()
    assert lib.orcai_conv0_wgrad(None, H * W, N.ptr(dvd), B, H, W, k, N.ptr(dW), st) == N.E_BADARG and lib.orcai_conv0_wgrad(N.ptr(xd), H * W, N.ptr(dvd), 0, H, W, k, N.ptr(dW), st) == N.E_BADARG
    assert lib.orcai_conv0_wgrad(N.ptr(xd), H * W, N.ptr(dvd), B, H, W, 4, N.ptr(dW), st) == N.E_UNSUPPORTED
    torch.cuda.synchronize()
    assert torch.equal(dW, before)


# ------------------------------------------------------------------------------------------------- the f16 twins: orcai_h_sepconv, orcai_h_dw_wgrad
@pytest.mark.parametrize("Cin,Cout,k,H,W", [(16, 30, 5, 5, 171), (30, 50, 7, 8, 171), (7, 16, 7, 1, 65), (50, 30, 5, 8, 65)])
def test_h_sepconv_wide_kernels_exact(Cin, Cout, k, H, W):
    """The exact-integer checks of test_sepconv_h_layouts_exact_integers (tests/test_half_gpu.py: ktap = k, layouts 0 with the depthwise output, 1 and 2,
    ReLU on load on and off, pads) at k = 5 / 7 on planes several windows wide; that test stops at W = 17 / 15 for these kernel sizes."""
    import test_half_gpu as TH
    from orcai_amd import _native as N
    from orcai_amd.half import pack_depthwise_octets, pack_pointwise_fragments

    TH._sepconv_h_exact(N.lib(), N, pack_depthwise_octets, pack_pointwise_fragments, Cin, Cout, k, H, W)


# (Cin, Cout, H, W, ksize_planes, ktap, relu_in, relu_out, out_layout, u_out, odd H2 / W2): what the k = 5 / 7 f16 backward launches besides ktap = k
H_SEP_CASES = {
    "f16 pointwise pass on k7 planes (du = Wpw dv), W = 171": (50, 30, 5, 171, 7, 1, 0, 0, 0, False, False),
    "f16 pointwise pass on k5 planes, W = 65, ragged octets": (7, 30, 8, 65, 5, 1, 0, 1, 0, False, False),
    "f16 taps narrower than the padding: ktap 5 on k7 planes, u kept": (16, 16, 5, 65, 7, 5, 1, 0, 0, True, False),
    "f16 taps narrower than the padding: ktap 1 on k5 planes, x-pooled": (30, 16, 5, 171, 5, 1, 0, 0, 2, False, False),
    "f16 scatter-add to (2y, 2x), even image, k5 planes, W = 65": (30, 16, 8, 65, 5, 1, 0, 0, 3, False, False),
    "f16 scatter-add to (2y, 2x), odd image H2 = 2H - 1, W2 = 2W - 1, k7 planes, W = 171": (16, 7, 5, 171, 7, 1, 0, 0, 3, False, True),
    "f16 scatter-add to (2y, 2x), even image, k7 planes, W = 171, 4 tiles": (50, 50, 1, 171, 7, 1, 0, 0, 3, False, False),
    "f16 scatter-add to (2y, 2x), odd image, k5 planes, W = 65": (7, 30, 8, 65, 5, 1, 0, 0, 3, False, True),
}


def _h_sep_case(name):
    """Small integers (every value and partial sum an integer below 2048: exact in f16 and in the f32 accumulators) through orcai_h_sepconv."""
    from orcai_amd import _native as N
    from orcai_amd.half import pack_depthwise_octets, pack_pointwise_fragments
    from test_half_gpu import from_octet_planes, to_octet_planes

    lib = N.lib()
    Cin, Cout, H, W, kp, ktap, relu_in, relu_out, layout, with_u, odd = H_SEP_CASES[name]
    rng = np.random.default_rng(Cin * 1000 + Cout * 10 + W + ktap)
    x = _ints(rng, B, Cin, H, W, lo=-2, hi=2)
    dwk = _ints(rng, ktap, ktap, Cin, lo=-1, hi=1) if ktap == 1 else ((rng.random((ktap, ktap, Cin)) < 0.2) * rng.integers(-1, 2, size=(ktap, ktap, Cin))).astype(np.float32)
    pw = (rng.integers(-1, 3, size=(Cin, Cout)) * (rng.random((Cin, Cout)) < 0.5)).astype(np.float32)
    scale, shift = np.ones(Cout, dtype=np.float32), _ints(rng, Cout)
    u_ref, v_ref = _sep_ref(x, dwk, pw, scale, shift, relu_in, relu_out)
    assert np.abs(u_ref).max() < 2048 and np.abs(v_ref).max() < 2040
    octets = lambda a, k: _dev(to_octet_planes(a.astype(np.float16), k))  # noqa: E731
    xd, dwd, pwd, scd, shd = octets(x, kp), _dev(pack_depthwise_octets(dwk[..., None])), _dev(pack_pointwise_fragments(pw)), _dev(scale), _dev(shift)
    u = octets(np.full((B, Cin, H, W), SENTINEL), kp) if with_u else None
    H2, W2 = (2 * H - 1, 2 * W - 1) if odd else (2 * H, 2 * W)
    if layout == 0:
        out = octets(np.full((B, Cout, H, W), SENTINEL), kp)
    elif layout == 2:
        Wx = (W + 1) // 2
        out = torch.full((B, (Cout + 7) // 8, H, (Wx + 3) & ~3, 8), SENTINEL, dtype=torch.float16, device="cuda")
    else:
        start = _ints(rng, B, Cout, H2, W2)
        out = octets(start, kp)
    before = out.clone()
    N.check(lib.orcai_h_sepconv(N.ptr(xd), B, Cin, H, W, kp, ktap, relu_in, N.ptr(dwd), N.ptr(pwd), N.ptr(scd), N.ptr(shd), Cout, relu_out, layout, H2, W2, N.ptr(out),
                                None if u is None else N.ptr(u), N.stream_ptr()), name)
    torch.cuda.synchronize()
    got = out.cpu().numpy().astype(np.float64)
    if layout == 0:
        g, pads = from_octet_planes(got, Cout, H, W, kp)
        assert np.array_equal(g, v_ref) and not pads.any(), (name, float(np.abs(g - v_ref).max()))
    elif layout == 2:
        Wx = (W + 1) // 2
        pairs = np.full((B, Cout, H, 2 * Wx), -np.inf)
        pairs[..., :W] = v_ref
        full = got.transpose(0, 1, 4, 2, 3).reshape(B, -1, H, got.shape[3])
        assert np.array_equal(full[:, :Cout, :, :Wx], pairs.reshape(B, Cout, H, Wx, 2).max(axis=4)), name
        assert np.all(full[:, :, :, Wx:] == SENTINEL), name  # the columns past ceil(W / 2) are nobody's
    else:
        want = start.astype(np.float64)
        want[:, :, : 2 * H : 2, : 2 * W : 2] += v_ref
        g, pads = from_octet_planes(got, Cout, H2, W2, kp)
        assert np.array_equal(g, want) and not pads.any(), (name, float(np.abs(g - want).max()))
    if with_u:
        gu, upads = from_octet_planes(u.cpu().numpy().astype(np.float64), Cin, H, W, kp)
        assert np.array_equal(gu, u_ref) and not upads.any(), name
    return lib, N, (xd, Cin, H, W, kp, ktap, relu_in, dwd, pwd, scd, shd, Cout, relu_out, layout, H2, W2), before


@pytest.mark.parametrize("name", list(H_SEP_CASES))
def test_h_sepconv_pointwise_and_scatter_add_exact(name):
    _h_sep_case(name)


def test_h_sepconv_refuses_bad_arguments():
    lib, N, a, before = _h_sep_case("f16 scatter-add to (2y, 2x), even image, k5 planes, W = 65")
    xd, Cin, H, W, kp, ktap, relu_in, dwd, pwd, scd, shd, Cout, relu_out, layout, H2, W2 = a
    out = before.clone()
    st = N.stream_ptr()

    def call(**kw):
        v = dict(x=N.ptr(xd), B=B, Cin=Cin, H=H, W=W, kp=kp, ktap=ktap, dw=N.ptr(dwd), Cout=Cout, layout=layout, H2=H2, W2=W2)
        v.update(kw)
        return lib.orcai_h_sepconv(v["x"], v["B"], v["Cin"], v["H"], v["W"], v["kp"], v["ktap"], relu_in, v["dw"], N.ptr(pwd), N.ptr(scd), N.ptr(shd), v["Cout"], relu_out,
                                   v["layout"], v["H2"], v["W2"], N.ptr(out), None, st)

    assert call(x=None) == N.E_BADARG and call(dw=None) == N.E_BADARG and call(B=0) == N.E_BADARG and call(W=-1) == N.E_BADARG and call(Cout=0) == N.E_BADARG
    assert call(layout=4) == N.E_BADARG and call(H2=2 * H - 2) == N.E_BADARG and call(W2=2 * W - 2) == N.E_BADARG
    assert call(Cout=65) == N.E_UNSUPPORTED and call(Cin=65) == N.E_UNSUPPORTED and call(ktap=4) == N.E_UNSUPPORTED and call(ktap=7) == N.E_UNSUPPORTED
    assert call(x=N.ptr(xd) + 8) == N.E_UNSUPPORTED  # misaligned planes
    torch.cuda.synchronize()
    assert torch.equal(out, before)


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "normal"])
@pytest.mark.parametrize("C,H,W,kp,ktap,relu", [(30, 8, 171, 7, 7, 1), (16, 5, 171, 5, 5, 0), (7, 1, 65, 7, 7, 1), (50, 8, 65, 5, 5, 1), (16, 5, 65, 7, 5, 0), (30, 5, 171, 5, 3, 1)])
def test_h_dw_wgrad_wide_kernels(C, H, W, kp, ktap, relu, exact):
    """orcai_h_dw_wgrad at k = 5 / 7 (and taps narrower than the padding) on W = 65 / 171, accumulating on top of a non-zero dW: small integers are exact
    (f16 inputs, f32 products and accumulators); f16-representable standard-normal inputs at test_dw_wgrad_h_vs_reference's 1e-4 * max(1, max|ref|)."""
    from orcai_amd import _native as N
    from test_half_gpu import to_octet_planes

    lib = N.lib()
    rng = np.random.default_rng(C + W + ktap)
    draw = (lambda: _ints(rng, B, C, H, W).astype(np.float16)) if exact else (lambda: rng.standard_normal((B, C, H, W)).astype(np.float16))
    x, du = draw(), draw()
    R = ktap // 2
    xp = np.zeros((B, C, H + 2 * R, W + 2 * R))
    xp[:, :, R : R + H, R : R + W] = np.maximum(x, 0) if relu else x
    want = np.stack([[np.einsum("bchw,bchw->c", xp[:, :, dy : dy + H, dx : dx + W], du.astype(np.float64)) for dx in range(ktap)] for dy in range(ktap)]).reshape(ktap * ktap, C)
    xd, dud = _dev(to_octet_planes(x, kp)), _dev(to_octet_planes(du, kp))
    dW = torch.full((ktap * ktap, C), 3.0, device="cuda")
    st = N.stream_ptr()
    N.check(lib.orcai_h_dw_wgrad(N.ptr(xd), N.ptr(dud), B, C, H, W, kp, ktap, relu, N.ptr(dW), st), "h_dw_wgrad")
    got = dW.cpu().numpy().astype(np.float64) - 3.0
    if exact:
        assert np.array_equal(got, want), float(np.abs(got - want).max())
    else:
        assert np.abs(got - want).max() <= 1e-4 * max(1.0, np.abs(want).max()), float(np.abs(got - want).max())
    before = dW.clone()
    assert lib.orcai_h_dw_wgrad(None, N.ptr(dud), B, C, H, W, kp, ktap, relu, N.ptr(dW), st) == N.E_BADARG
    assert lib.orcai_h_dw_wgrad(N.ptr(xd), N.ptr(dud), 0, C, H, W, kp, ktap, relu, N.ptr(dW), st) == N.E_BADARG
    assert lib.orcai_h_dw_wgrad(N.ptr(xd), N.ptr(dud), B, 65, H, W, kp, ktap, relu, N.ptr(dW), st) == N.E_BADARG
    assert lib.orcai_h_dw_wgrad(N.ptr(xd), N.ptr(dud), B, C, H, W, kp, 4, relu, N.ptr(dW), st) == N.E_UNSUPPORTED
    assert lib.orcai_h_dw_wgrad(N.ptr(xd), N.ptr(dud), B, C, H, W, kp, kp + 2, relu, N.ptr(dW), st) == N.E_BADARG  # taps wider than the padding, as the f32 twin refuses them
    assert lib.orcai_h_dw_wgrad(N.ptr(xd), N.ptr(dud), B, C, 0, W, kp, ktap, relu, N.ptr(dW), st) == N.E_BADARG and lib.orcai_h_dw_wgrad(N.ptr(xd), N.ptr(dud), B, C, H, -1, kp, ktap, relu, N.ptr(dW), st) == N.E_BADARG
    torch.cuda.synchronize()
    assert torch.equal(dW, before)
