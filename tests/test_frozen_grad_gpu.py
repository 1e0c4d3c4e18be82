"""Frozen-BatchNorm fine-tuning on the GPU: orcai_sepconv_wgrad_frozen and compose_wgrad (the training step's reduction launchers + orcai_frozen_bn_finish) against its formulae in float64,
the two launchers it leans on that had no direct test, EvalGrad.backward(wgrad=True) end to end against float64 autograd of the eval-mode oracle
(tests/frozen_grad_ref.py), the launch record, and what the feature is for: a detector that learns while its BatchNorm statistics stay frozen."""

import math

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import eval_grad_ref as R  # noqa: E402
import frozen_grad_ref as FR  # noqa: E402
from recording_lib import RecordingLib  # noqa: E402

U = 2.0 ** -24  # f32 unit roundoff
E2E_BAR = 5e-4  # of max|ref| per variable: the rule of test_eval_grad_gpu.py for dx; the CPU calibration (tests/test_frozen_grad.py) needs no more for any variable


def _bits(a):
    return a.contiguous().view(torch.int32)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _layer_variables(Cin, Cout, seed):
    rng = np.random.default_rng(seed)
    f = lambda a: a.astype(np.float32)  # noqa: E731
    return dict(pw=f(rng.standard_normal((Cin, Cout)) / np.sqrt(Cin)), bias=f(0.3 * rng.standard_normal(Cout)), gamma=f(1 + 0.3 * rng.standard_normal(Cout)),
                mean=f(0.5 * rng.standard_normal(Cout)), var=f(rng.uniform(0.5, 2.0, Cout)))


def _compose(case, yg, ri, lv):
    """One compose_wgrad on the case: (G [Cout][Cin], sums, dWdw (3, 3, Cin, 1), dWpw [Cin][Cout], dbias, dgamma, dbeta) as device tensors."""
    from orcai_amd import _native as N
    from orcai_amd.eval_grad import compose_wgrad

    B, Cout, H, W = case["g"].shape
    Cin, k = case["x"].shape[1], case["k"]
    g, y, x = (_dev(R.to_planes(case[n], k)) for n in ("g", "y", "x"))
    z = lambda *s: torch.zeros(s, device="cuda")  # noqa: E731
    out = dict(G=z(Cout, Cin), sums=z(Cout), dWdw=z(3, 3, Cin, 1), dWpw=z(Cin, Cout), dbias=z(Cout), dgamma=z(Cout), dbeta=z(Cout))
    v = {n: _dev(a) for n, a in lv.items()}
    compose_wgrad(N.lib(), g, y if yg else None, x, ri, B, Cin, Cout, H, W, k, _dev(R.taps_layout(case["taps"], k)), _dev(case["wts"]), v["pw"], v["bias"], v["gamma"],
                  v["mean"], v["var"], torch.zeros_like(x), torch.zeros_like(x), out["G"], out["sums"], torch.zeros(64, dtype=torch.float64, device="cuda"),
                  torch.empty(512 * 64 * 64, device="cuda"), out["dWdw"], out["dWpw"], out["dbias"], out["dgamma"], out["dbeta"], N.stream_ptr())
    torch.cuda.synchronize()
    return {n: t.cpu().numpy() for n, t in out.items()}


@pytest.mark.parametrize("Cin,Cout,H,W", FR.WGRAD_CASES, ids=[f"{c[0]}to{c[1]}_{c[2]}x{c[3]}" for c in FR.WGRAD_CASES])
def test_compose_wgrad_matches_its_formula(Cin, Cout, H, W):
    """compose_wgrad with and without y_gate and relu_in against the header's formulae in float64.  G, sum gg and dWdw: FR.WGRAD_BAR per tensor (4 x the worst
    share the same formulae evaluated in f32 by torch on the CPU deviate by at these seeds: the summation order differs).  orcai_frozen_bn_finish's outputs:
    against its formulae in float64 ON the G and sums it was given, element by element within the rounding of a (Cin + 2)-term f32 sum of products,
    (Cin + 6) u sum|terms| -- dbeta is a copy."""
    case = FR.wgrad_case(Cin, Cout, H, W)
    lv = _layer_variables(Cin, Cout, 7 * Cin + Cout)
    for yg, ri in FR.WGRAD_MODES:
        ref = dict(zip(("G", "dbeta", "dWdw"), (t.numpy() for t in FR.wgrad_formula(case, torch.float64, yg, ri))))
        got = _compose(case, yg, ri, lv)
        for key, have in (("G", got["G"]), ("dbeta", got["sums"]), ("dWdw", got["dWdw"])):
            err = FR.share(have, ref[key])
            print(f"{Cin}->{Cout} {H}x{W} y_gate {yg} relu_in {ri}: {key} {err:.2e} of max|ref|; bar {FR.WGRAD_BAR[key]:.2e}")
            assert np.isfinite(have).all() and err <= FR.WGRAD_BAR[key], (key, yg, ri, err)
        G, sums = got["G"].astype(np.float64), got["sums"].astype(np.float64)
        d = {n: a.astype(np.float64) for n, a in lv.items()}
        inv = 1.0 / np.sqrt(d["var"] + 1e-3)
        scale = d["gamma"] * inv
        assert np.array_equal(got["dbeta"], got["sums"])
        assert (np.abs(got["dWpw"] - (scale[:, None] * G).T) <= 6 * U * np.abs(scale[:, None] * G).T).all()
        assert (np.abs(got["dbias"] - scale * sums) <= 6 * U * np.abs(scale * sums)).all()
        terms = np.abs(d["pw"].T * G).sum(axis=1) + (np.abs(d["bias"]) + np.abs(d["mean"])) * np.abs(sums)
        want = inv * ((d["pw"].T * G).sum(axis=1) + (d["bias"] - d["mean"]) * sums)
        assert (np.abs(got["dgamma"] - want) <= (Cin + 6) * U * inv * terms).all(), np.abs(got["dgamma"] - want).max()


WS_FLOATS = 1024 * (64 * 64 + 64 + 9 * 64)


def _fused(case, yg, ri, pad_value=0.0, ws_floats=WS_FLOATS):
    """(rc, G [Cout][Cin], dbeta, dWdw (3, 3, Cin, 1)) of one orcai_sepconv_wgrad_frozen launch; the outputs are prefilled with the sentinel 7."""
    from orcai_amd import _native as N

    B, Cout, H, W = case["g"].shape
    Cin, k = case["x"].shape[1], case["k"]
    g, y = (_dev(R.to_planes(case[n], k, pad_value)) for n in ("g", "y"))
    x = _dev(R.to_planes(case["x"], k, pad_value))
    taps, wts = _dev(R.taps_layout(case["taps"], k)), _dev(case["wts"])
    f = lambda *s: torch.full(s, 7.0, device="cuda")  # noqa: E731
    G, db, dW, ws = f(Cout, Cin), f(Cout), f(k, k, Cin, 1), torch.empty(WS_FLOATS, device="cuda")
    rc = N.lib().orcai_sepconv_wgrad_frozen(x.data_ptr(), g.data_ptr(), y.data_ptr() if yg else None, ri, B, Cin, Cout, H, W, k, taps.data_ptr(), wts.data_ptr(), G.data_ptr(),
                                            db.data_ptr(), dW.data_ptr(), ws.data_ptr(), ws_floats, N.stream_ptr())
    torch.cuda.synchronize()
    return rc, G, db, dW


@pytest.mark.parametrize("Cin,Cout,H,W", FR.WGRAD_CASES, ids=[f"{c[0]}to{c[1]}_{c[2]}x{c[3]}" for c in FR.WGRAD_CASES])
def test_kernel_matches_its_formula(Cin, Cout, H, W):
    """orcai_sepconv_wgrad_frozen against the header's formulae in float64, with and without y_gate and relu_in: FR.WGRAD_BAR per output tensor (4 x the worst
    share the formulae evaluated in f32 by torch on the CPU deviate by at these seeds).  Two launches give the same bits, also with every pad of the planes
    filled with 3e30 (x's pads excepted from nothing: the kernel never reads a pad), and the kernel agrees with compose_wgrad to the same bar."""
    case = FR.wgrad_case(Cin, Cout, H, W)
    lv = _layer_variables(Cin, Cout, 7 * Cin + Cout)
    for yg, ri in FR.WGRAD_MODES:
        ref = dict(zip(("G", "dbeta", "dWdw"), (t.numpy() for t in FR.wgrad_formula(case, torch.float64, yg, ri))))
        rc, G, db, dW = _fused(case, yg, ri)
        assert rc == 0, rc
        got = {"G": G.cpu().numpy(), "dbeta": db.cpu().numpy(), "dWdw": dW.cpu().numpy()}
        comp = _compose(case, yg, ri, lv)
        comp = {"G": comp["G"], "dbeta": comp["sums"], "dWdw": comp["dWdw"]}
        for key in ("G", "dbeta", "dWdw"):
            err = FR.share(got[key], ref[key])
            dev = float(np.abs(got[key].astype(np.float64) - comp[key]).max()) / float(np.abs(ref[key]).max())
            print(f"{Cin}->{Cout} {H}x{W} y_gate {yg} relu_in {ri}: fused {key} {err:.2e} of max|ref|, vs composition {dev:.2e}; bar {FR.WGRAD_BAR[key]:.2e}")
            assert np.isfinite(got[key]).all() and err <= FR.WGRAD_BAR[key], (key, yg, ri, err)
            assert dev <= FR.WGRAD_BAR[key], (key, yg, ri, dev)
        for again in (_fused(case, yg, ri), _fused(case, yg, ri, pad_value=3.0e30)):
            assert again[0] == 0
            for a, b in zip(again[1:], (G, db, dW)):
                assert torch.equal(_bits(a), _bits(b))


def test_kernel_refusals():
    """k = 5 and 7, Cin = 65 and a too-small workspace: ORCAI_E_UNSUPPORTED with the sentinel-filled outputs untouched; null and misaligned pointers:
    ORCAI_E_BADARG."""
    from orcai_amd import _native as N

    for k in (5, 7):
        case = R.kernel_case(12, 30, 8, 6, k)
        rc, G, db, dW = _fused(case, True, 1)
        assert rc == N.E_UNSUPPORTED and bool((G == 7).all()) and bool((db == 7).all()) and bool((dW == 7).all())
    case = FR.wgrad_case(16, 30, 37, 43)
    need = min(2 * 10 * 3, 1024) * (30 * 16 + 30 + 9 * 16)
    rc, G, db, dW = _fused(case, True, 1, ws_floats=need - 1)
    assert rc == N.E_UNSUPPORTED and bool((G == 7).all()) and bool((db == 7).all()) and bool((dW == 7).all())
    assert _fused(case, True, 1, ws_floats=need)[0] == 0  # exactly the size the header states
    a = torch.zeros(1 << 16, device="cuda")
    out = torch.full((1 << 14,), 7.0, device="cuda")
    lib, st, p, o = N.lib(), N.stream_ptr(), a.data_ptr(), out.data_ptr()
    call = lambda x, g, y, Cin, Cout, k, taps, wts, G, db, dW, ws: lib.orcai_sepconv_wgrad_frozen(x, g, y, 1, 2, Cin, Cout, 6, 5, k, taps, wts, G, db, dW, ws, WS_FLOATS, st)  # noqa: E731
    big = torch.empty(WS_FLOATS, device="cuda")
    w = big.data_ptr()
    assert call(p, p, p, 65, 8, 3, p, p, o, o, o, w) == N.E_UNSUPPORTED and call(p, p, p, 8, 65, 3, p, p, o, o, o, w) == N.E_UNSUPPORTED
    for args in ((None, p, p, 8, 8, 3, p, p, o, o, o, w), (p, None, p, 8, 8, 3, p, p, o, o, o, w), (p, p, p, 8, 8, 3, None, p, o, o, o, w), (p, p, p, 8, 8, 3, p, None, o, o, o, w),
                 (p, p, p, 8, 8, 3, p, p, None, o, o, w), (p, p, p, 8, 8, 3, p, p, o, None, o, w), (p, p, p, 8, 8, 3, p, p, o, o, None, w), (p, p, p, 8, 8, 3, p, p, o, o, o, None),
                 (p + 4, p, p, 8, 8, 3, p, p, o, o, o, w), (p, p + 8, p, 8, 8, 3, p, p, o, o, o, w), (p, p, p + 4, 8, 8, 3, p, p, o, o, o, w), (p, p, p, 8, 8, 3, p + 4, p, o, o, o, w),
                 (p, p, p, 8, 8, 4, p, p, o, o, o, w), (p, p, p, 0, 8, 3, p, p, o, o, o, w), (p, p, p, 8, -1, 3, p, p, o, o, o, w)):
        assert call(*args) == N.E_BADARG, args
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())


def test_bn_eps_is_the_models():
    from orcai_amd.architectures import BN_EPS

    assert BN_EPS == 1e-3  # the eps of the float64 formulae above


def test_outer_reduce_stride2_and_dw_wgrad_relu_in_against_float64():
    """The two existing launchers this feature leans on, on the (10, 20, 5, 3) shape: orcai_outer_reduce(a_stride2 = 1) -- the residual 1x1 stride-2 conv's
    weight gradient, A sampled at (2i, 2j) -- and orcai_dw_wgrad(relu_in = 1), each against float64, element by element within the rounding of an f32 sum of
    K products however it is ordered: (K + 2) u sum|terms|."""
    from orcai_amd import _native as N

    case = FR.wgrad_case(10, 20, 5, 3)
    B, Cin, H, W = case["x"].shape
    Cout, Ho, Wo = 20, (H + 1) // 2, (W + 1) // 2
    lib, st = N.lib(), N.stream_ptr()
    a64 = case["x"].astype(np.float64)[:, :, ::2, ::2]
    b32 = case["g"][:, :, :Ho, :Wo].copy()
    D = torch.zeros((Cin, Cout), device="cuda")
    part = torch.empty(512 * 64 * 64, device="cuda")
    xp, bp = _dev(R.to_planes(case["x"], 3)), _dev(R.to_planes(b32, 3))
    N.check(lib.orcai_outer_reduce(xp.data_ptr(), Cin, bp.data_ptr(), Cout, B, Ho, Wo, 3, 1, H, W, D.data_ptr(), part.data_ptr(), part.numel(), st), "orcai_outer_reduce")
    torch.cuda.synchronize()
    want = np.einsum("bihw,bohw->io", a64, b32.astype(np.float64))
    bound = (B * Ho * Wo + 2) * U * np.einsum("bihw,bohw->io", np.abs(a64), np.abs(b32.astype(np.float64)))
    assert (np.abs(D.cpu().numpy() - want) <= bound).all(), np.abs(D.cpu().numpy() - want).max()
    # orcai_dw_wgrad(relu_in = 1): dW[t][c] = sum relu(x)[c][p + off(t)] * du[c][p]
    du = np.random.default_rng(11).standard_normal((B, Cin, H, W)).astype(np.float32)
    dW = torch.zeros((3, 3, Cin, 1), device="cuda")
    dup = _dev(R.to_planes(du, 3))
    N.check(lib.orcai_dw_wgrad(xp.data_ptr(), dup.data_ptr(), B, Cin, H, W, 3, 3, 1, dW.data_ptr(), st), "orcai_dw_wgrad")
    torch.cuda.synchronize()
    r = np.pad(np.maximum(case["x"].astype(np.float64), 0), ((0, 0), (0, 0), (1, 1), (1, 1)))
    got = dW.cpu().numpy()
    for ty in range(3):
        for tx in range(3):
            win = r[:, :, ty : ty + H, tx : tx + W]
            want = (win * du).sum(axis=(0, 2, 3))
            bound = (B * H * W + 2) * U * (np.abs(win) * np.abs(du)).sum(axis=(0, 2, 3))
            assert (np.abs(got[ty, tx, :, 0] - want) <= bound).all(), (ty, tx)


def test_new_launchers_refuse_bad_arguments():
    from orcai_amd import _native as N

    a = torch.zeros(4096, device="cuda")
    out = torch.full((4096,), 7.0, device="cuda")
    lib, st, p, o = N.lib(), N.stream_ptr(), a.data_ptr(), out.data_ptr()
    fin = lambda G, sums, pw, bias, gamma, mean, var, Cin, Cout, dWpw, dbias, dgamma, dbeta: lib.orcai_frozen_bn_finish(  # noqa: E731
        G, sums, pw, bias, gamma, mean, var, 1e-3, Cin, Cout, dWpw, dbias, dgamma, dbeta, st)
    assert fin(p, None, p, p, p, p, p, 8, 8, o, o, o, o) == N.E_BADARG
    assert fin(p, p, None, p, p, p, p, 8, 8, o, o, o, o) == N.E_BADARG
    assert fin(p, p, p, p, p, p, p, 8, 8, None, o, o, o) == N.E_BADARG
    assert fin(p, p, p, p, p, p, p, 8, 8, o, o, None, o) == N.E_BADARG
    assert fin(p, p, p, p, p, p, p, 0, 8, o, o, o, o) == N.E_BADARG and fin(p, p, p, p, p, p, p, 8, 0, o, o, o, o) == N.E_BADARG
    assert fin(None, p, None, None, p, None, p, 0, 8, None, None, None, None) == N.E_BADARG  # nothing to write
    rows = lambda dy, x, M, cols, C, mean, var, db, dg, ws: lib.orcai_rows_bn_frozen_wgrad(dy, x, M, cols, C, mean, var, 1e-3, db, dg, ws, st)  # noqa: E731
    assert rows(None, p, 4, 8, 8, p, p, o, o, o) == N.E_BADARG and rows(p, p, 4, 8, 8, p, p, o, o, None) == N.E_BADARG
    assert rows(p, p, 0, 8, 8, p, p, o, o, o) == N.E_BADARG and rows(p, p, 4, 12, 8, p, p, o, o, o) == N.E_BADARG
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())  # a refusal touches nothing


def test_rows_bn_frozen_wgrad_against_float64():
    """M = 37 rows (not a multiple of the four row groups), cols = 3 * 40 with C = 40 (two workgroups, the second partial; three columns per channel): each sum
    within (M * cols / C + 4) u sum|terms| of float64; two launches give the same bits."""
    from orcai_amd import _native as N

    rng = np.random.default_rng(5)
    M, C, cols = 37, 40, 120
    dy, x = rng.standard_normal((M, cols)).astype(np.float32), rng.standard_normal((M, cols)).astype(np.float32)
    mean, var = rng.standard_normal(C).astype(np.float32), rng.uniform(0.5, 2, C).astype(np.float32)
    runs = []
    dyd, xd, md, vd, ws = _dev(dy), _dev(x), _dev(mean), _dev(var), torch.empty(2 * cols, device="cuda")
    for _ in range(2):
        db, dg = torch.zeros(C, device="cuda"), torch.zeros(C, device="cuda")
        N.check(N.lib().orcai_rows_bn_frozen_wgrad(dyd.data_ptr(), xd.data_ptr(), M, cols, C, md.data_ptr(), vd.data_ptr(), 1e-3, db.data_ptr(), dg.data_ptr(), ws.data_ptr(),
                                                   N.stream_ptr()), "orcai_rows_bn_frozen_wgrad")
        torch.cuda.synchronize()
        runs.append((db, dg))
    assert torch.equal(_bits(runs[0][0]), _bits(runs[1][0])) and torch.equal(_bits(runs[0][1]), _bits(runs[1][1]))
    d64, x64 = dy.astype(np.float64).reshape(M, 3, C), x.astype(np.float64).reshape(M, 3, C)
    inv = 1.0 / np.sqrt(var.astype(np.float64) + 1e-3)
    K = 3 * M + 4
    assert (np.abs(runs[0][0].cpu().numpy() - d64.sum(axis=(0, 1))) <= K * U * np.abs(d64).sum(axis=(0, 1))).all()
    t = d64 * (x64 - mean.astype(np.float64))
    assert (np.abs(runs[0][1].cpu().numpy() - inv * t.sum(axis=(0, 1))) <= K * U * inv * (np.abs(d64) * (np.abs(x64) + np.abs(mean))).sum(axis=(0, 1))).all()


# ------------------------------------------------------------------------------------------------------------------ end to end
_CACHE = {}


def _model(cfg, conv1d, p):
    from orcai_amd.architectures import ResNet1DConv, ResNetLSTM

    if conv1d:
        model = ResNet1DConv(cfg["input_shape"], cfg["num_labels"], list(cfg["filters"]), cfg["kernel_size"], 0.0)
    else:
        model = ResNetLSTM(cfg["input_shape"], cfg["num_labels"], list(cfg["filters"]), cfg["kernel_size"], 0.5, cfg["lstm_units"])  # a Dropout rate the eval path must ignore
    model.set_weights_dict(p)
    return model


def _e2e(name):
    """One forward + backward(wgrad=True) of EvalGrad for an R.E2E_CASES entry (with the launch record), the backward without wgrad on the same `saved`, and
    the float64 reference, computed once and shared."""
    if name in _CACHE:
        return _CACHE[name]
    from orcai_amd.eval_grad import EvalGrad

    _, cfg, B, conv1d, seed = next(c for c in R.E2E_CASES if c[0] == name)
    p, x, r = R.e2e_inputs(cfg, B, conv1d, seed)
    model = _model(cfg, conv1d, p)
    eg = EvalGrad(model)
    xd, rd = _dev(x[..., 0]), _dev(r)
    probs, saved = eg.forward(xd)
    dx_plain = eg.backward(rd, saved)
    eg.lib = RecordingLib(eg._lib())
    dx, dw = eg.backward(rd, saved, wgrad=True)
    torch.cuda.synchronize()
    rec, eg.lib = eg.lib, eg.lib._lib
    dx_again = eg.backward(rd, saved)
    _, ref, ref_dx = FR.weight_gradients(p, x, r, conv1d, torch.float64)
    _CACHE[name] = dict(model=model, eg=eg, x=xd, r=rd, p=p, probs=probs, saved=saved, dx=dx, dw=dw, dx_plain=dx_plain, dx_again=dx_again, rec=rec, ref=ref, ref_dx=ref_dx, cfg=cfg,
                        B=B, conv1d=conv1d)
    return _CACHE[name]


@pytest.mark.parametrize("name", [c[0] for c in R.E2E_CASES])
def test_weight_gradients_vs_float64_autograd(name):
    """EvalGrad.forward + backward(wgrad=True), loss sum(probs * r), against float64 autograd of the eval-mode oracle: every variable's gradient within
    5e-4 of that variable's max|ref| (the CPU calibration shows no variable needs more: at most 5.7e-6 in f32 on the host).  dx with wgrad=True is
    bit-identical to dx with wgrad=False, before and after."""
    c = _e2e(name)
    lay = c["model"].layout()
    assert c["dw"].shape == (lay.n_w,) and c["dw"].dtype == torch.float32
    flat = c["dw"].cpu().numpy().astype(np.float64)
    assert np.isfinite(flat).all()
    shares = {n: FR.share(flat[o : o + cnt].reshape(shape), c["ref"][n]) for n, (o, cnt, shape) in lay.w.items()}
    for n, v in sorted(shares.items(), key=lambda kv: -kv[1]):
        print(f"{name}: {n:28s} {v:.2e} of max|ref| = {np.abs(c['ref'][n]).max():.3e}")
    worst = max(shares, key=shares.get)
    assert shares[worst] <= E2E_BAR, (worst, shares[worst])
    assert FR.share(c["dx"].cpu().numpy(), c["ref_dx"]) <= E2E_BAR
    assert torch.equal(_bits(c["dx"]), _bits(c["dx_plain"])) and torch.equal(_bits(c["dx"]), _bits(c["dx_again"]))


@pytest.mark.parametrize("name", [c[0] for c in R.E2E_CASES])
def test_launch_record(name):
    """k = 3 (k3, wide, conv1d): orcai_sepconv_wgrad_frozen is ACCEPTED on exactly the layers the routing rule names (EvalGrad.fused_wgrad: up to 16
    input channels, where it measured faster) and the composition's launchers run only for the others; k = 5 and 7: the launcher refuses every layer (-2) and the composition runs.  Either
    way one orcai_frozen_bn_finish per separable conv (+ one for the entry conv), the residual convs' orcai_outer_reduce / orcai_planes_sum, the entry conv's two
    passes, and the data-gradient launches of wgrad=False."""
    c = _e2e(name)
    rec, model, eg = c["rec"], c["model"], c["eg"]
    nb, k, B = len(model.filters), model.kernel_size, c["B"]
    nsep = 2 * nb + 1
    shapes = model.stage_shapes()
    cins, ch = [], 16
    for b, f in enumerate(model.filters, start=1):
        h, w, _ = shapes[b - 1]
        cins += [(f, h, w), (ch, h, w)]  # backward order inside a block: sep_b, then sep_a
        ch = f
    order = [(ch, shapes[-1][0], shapes[-1][1])]
    for b in range(nb, 0, -1):
        order += cins[2 * (b - 1) : 2 * b]
    asked = [eg.fused_wgrad(B, cin, h, w) for cin, h, w in order]
    want = [0 if k == 3 else -2 for a in asked if a]
    assert rec.rcs("orcai_sepconv_wgrad_frozen") == want
    if name in ("k3", "wide"):
        assert want and all(rc == 0 for rc in want)  # the fused launcher carries these configurations
    ncomp = nsep - sum(1 for rc in want if rc == 0)
    if name in ("k5", "k7"):
        assert ncomp == nsep
    assert rec.rcs("orcai_frozen_bn_finish") == [0] * (nsep + 1)
    assert rec.rcs("orcai_outer_reduce") == [0] * (ncomp + nb) and rec.rcs("orcai_planes_sum") == [0] * (ncomp + nb)
    assert rec.rcs("orcai_dw_wgrad") == [0] * ncomp
    assert rec.rcs("orcai_conv0_bn_bwd_x") == [0] and rec.rcs("orcai_conv0_bn_bwd_x_ready") == [0] and rec.rcs("orcai_conv0_bn_bwd_dx") == [0]
    assert rec.rcs("orcai_sepconv_dgrad") == [0 if k == 3 else -2] * nsep
    if c["conv1d"]:
        assert rec.rcs("orcai_conv1d_bwd") == [0] and rec.rcs("orcai_colsum") == [0]
    else:
        assert rec.rcs("orcai_rows_bn_frozen_wgrad") == [0] and rec.rcs("orcai_unpack_lstm_grads") == [0] and rec.rcs("orcai_lstm_hprev") == [0, 0]
    assert all(rc == 0 or (n in ("orcai_sepconv_dgrad", "orcai_sepconv_wgrad_frozen") and rc == -2) for n, rc, _ in rec.calls)


# ------------------------------------------------------------------------------------------------------------------ the point of the feature
def _bce(q, y):
    q = q.clamp(1e-7, 1 - 1e-7)
    mask = (y != -1.0).float()
    return (-(y * q.log() + (1 - y) * (1 - q).log()) * mask).sum() / mask.sum()


def test_it_stays_frozen_and_it_learns():
    """Ten SGD steps of OrcaiModule(frozen_bn=True).eval() on a fixed batch of the k3 config: the loss falls, every moving statistic is bit-identical before
    and after, no Dropout seed was drawn, and the inference path (`orcai predict`'s forward: orcai::forward(training=False)) on the updated weights gives the
    module's probabilities exactly."""
    import test_torch_ops_gpu as G
    from orcai_amd.torch_ops import OrcaiModule

    c = _e2e("k3")
    model = _model(c["cfg"], False, c["p"])
    m = OrcaiModule(model, frozen_bn=True).cuda().eval()
    stats = {n: t.detach().clone() for n, t in m.named_buffers()}
    before = {n: t.detach().clone() for n, t in m.named_parameters()}
    H, W = model.input_hw
    x = torch.rand((c["B"], H, W), device="cuda", generator=torch.Generator(device="cuda").manual_seed(4))
    y = G._labels(model, c["B"], 3)
    opt = torch.optim.SGD(m.parameters(), lr=1e-3)  # small enough for plain gradient descent to descend on this untrained, calibrated net
    losses = []
    for _ in range(10):
        opt.zero_grad()
        loss = _bce(m(x), y)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    with torch.no_grad():
        after = m(x)
        losses.append(float(_bce(after, y)))
    print("frozen-BatchNorm fine-tuning:", [f"{v:.5f}" for v in losses])
    assert all(math.isfinite(v) for v in losses) and losses[-1] < losses[0], losses
    for n, t in m.named_buffers():
        assert torch.equal(_bits(t), _bits(stats[n])), n
    assert all(p.grad is not None for p in m.parameters()) and any(not torch.equal(t.detach(), before[n]) for n, t in m.named_parameters())
    assert m.dropout_draws == 0
    m.train()  # the same op in .train(): same bits, still no Dropout, statistics still untouched
    with torch.no_grad():
        assert torch.equal(_bits(m(x)), _bits(after))
    m.eval()
    plain = OrcaiModule(m.to_model()).cuda().eval()
    with torch.no_grad():
        fwd = plain(x)
    print(f"inference path on the updated weights vs the module: max|delta| {float((fwd - after).abs().max()):.1e}")
    assert torch.equal(fwd, after)


def test_module_gradients_are_evalgrad_and_x_gets_one_too():
    from orcai_amd.torch_ops import OrcaiModule

    c = _e2e("k3")
    m = OrcaiModule(c["model"], frozen_bn=True).cuda().eval()
    x = c["x"].clone().requires_grad_()
    (m(x) * c["r"]).sum().backward()
    lay = c["model"].layout()
    assert torch.equal(_bits(x.grad), _bits(c["dx"]))
    for n, g in zip(lay.w_names, lay.split_w(c["dw"])):
        got = getattr(m, n.replace("/", "__")).grad
        assert got.shape == g.shape and FR.share(got.cpu().numpy(), g.cpu().numpy()) <= 1e-5, n  # the weight-gradient GEMMs split K with float atomics: not bit for bit
    # detect_wrt_input keeps returning no weight gradient
    m2 = OrcaiModule(c["model"], input_grad="eval").cuda().eval()
    x2 = c["x"].clone().requires_grad_()
    (m2(x2) * c["r"]).sum().backward()
    assert all(p.grad is None for p in m2.parameters()) and torch.equal(_bits(x2.grad), _bits(c["dx"]))


def test_compiled_equals_eager_for_one_step():
    from orcai_amd.torch_ops import OrcaiModule

    c = _e2e("conv1d")
    res = []
    for compiled in (False, True):
        m = OrcaiModule(_model(c["cfg"], True, c["p"]), frozen_bn=True).cuda().eval()
        fn = torch.compile(m, backend="aot_eager", fullgraph=True) if compiled else m
        opt = torch.optim.SGD(m.parameters(), lr=0.1)
        loss = (fn(c["x"]) * c["r"]).sum()
        loss.backward()
        opt.step()
        res.append((loss.detach(), [p.detach().clone() for p in m.parameters()]))
    assert torch.equal(_bits(res[0][0]), _bits(res[1][0]))
    for a, b in zip(res[0][1], res[1][1]):  # conv1d: no split-K GEMM; orcai_dw_wgrad and the entry conv add with float atomics, so to rounding, not bit for bit
        assert float((a - b).abs().max()) <= 1e-5 * max(float(a.abs().max()), 1e-30)


def test_opcheck():
    from torch.library import opcheck

    from orcai_amd.torch_ops import OrcaiModule

    c = _e2e("k3")
    m = OrcaiModule(c["model"], frozen_bn=True).cuda().eval()
    ws, st, cfg = [w.detach().clone() for w in m.weights_list()], [s.clone() for s in m.stats_list()], m.config
    x = c["x"]
    opcheck(torch.ops.orcai.detect_wrt_params.default, (x, ws, st, cfg))
    opcheck(torch.ops.orcai.detect_wrt_params.default, (x.clone().requires_grad_(), [w.clone().requires_grad_() for w in ws], st, cfg),
            test_utils=("test_schema", "test_autograd_registration", "test_faketensor"))
    probs, saved = torch.ops.orcai.detect_with_saved(x, ws, st, cfg)
    opcheck(torch.ops.orcai.detect_backward_params.default, (torch.ones_like(probs), saved, ws, st, cfg),
            test_utils=("test_schema", "test_autograd_registration", "test_faketensor"))
