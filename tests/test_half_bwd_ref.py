"""tests/half_bwd_ref.py on the CPU: the float64 references against torch float64 autograd, the case tables against the launch geometry they were
chosen for, every comparison function against the bug it is there to reject, the ReLU-gate cap, and the derived bounds against f32 emulations
of the accumulations (numpy float32, two summation orders): a bound no f32 implementation can meet would test nothing."""

import numpy as np
import pytest

import half_bwd_ref as R

torch = pytest.importorskip("torch")
F = torch.nn.functional


def _t(a, grad=False):
    return torch.tensor(np.asarray(a, dtype=np.float64), requires_grad=grad)


# ------------------------------------------------------------------------------------------------- references against autograd
@pytest.mark.parametrize("k,C,H,W", [(3, 7, 17, 6), (5, 9, 20, 21), (7, 5, 1, 64), (3, 4, 18, 1), (5, 3, 33, 11)])
def test_pool_bwd_ref_against_max_pool2d_with_ties(k, C, H, W):
    from oracle.model_ref import same_pad

    rng = np.random.default_rng([k, C, H, W])
    B, Ho, Wo = 2, (H + 1) // 2, (W + 1) // 2
    v, dout = rng.integers(-2, 3, size=(B, C, H, W)).astype(np.float64), rng.integers(-4, 5, size=(B, C, Ho, Wo)).astype(np.float64)
    mean, var, gamma, _ = R._bn_vectors(rng, C)
    sgn = np.where(gamma < 0, -1.0, 1.0)
    x = _t(v * sgn[None, :, None, None], grad=True)
    _, pt, pb = same_pad(H, 3, 2)
    _, pl, pr = same_pad(W, 2, 2)
    F.max_pool2d(F.pad(x, (pl, pr, pt, pb), value=float("-inf")), kernel_size=(3, 2), stride=2).backward(_t(dout))
    dy, s_dy, s_dyx, s_dout = R.pool_bwd_ref(v, dout, gamma, mean, var, R.EPS, k)
    assert np.array_equal(dy, x.grad.numpy())
    xh = (v - mean.astype(np.float64)[None, :, None, None]) / np.sqrt(var.astype(np.float64) + float(np.float32(R.EPS)))[None, :, None, None]
    assert np.array_equal(s_dy, dy.sum(axis=(0, 2, 3))) and np.allclose(s_dyx, (x.grad.numpy() * xh).sum(axis=(0, 2, 3)), rtol=1e-13, atol=1e-13)
    assert np.array_equal(s_dout, dout.sum(axis=(0, 2, 3))) and s_dy.sum() == dout.sum()  # every window's gradient lands exactly once


@pytest.mark.parametrize("k", [3, 5, 7])
@pytest.mark.parametrize("relu", [0, 1])
def test_bn_bwd_pointwise_ref_against_autograd(k, relu):
    """u -> 1x1 conv -> v -> BatchNorm (training mode) -> [ReLU] -> y with the gradient dy at y: dbeta, dgamma, dv = v.grad, du = u.grad."""
    rng = np.random.default_rng([k, relu])
    B, C, Cin, H, W, eps = 2, 5 + k, 4 + k, k + 2, 2 * k + 1, 2.0**-10
    u, w = _t(rng.standard_normal((B, Cin, H, W)), grad=True), _t(rng.standard_normal((C, Cin)))
    gamma, beta = _t(rng.standard_normal(C), grad=True), _t(0.2 * rng.standard_normal(C), grad=True)
    dy = rng.standard_normal((B, C, H, W))
    v = F.conv2d(u, w[:, :, None, None])
    v.retain_grad()
    y = F.batch_norm(v, None, None, gamma, beta, training=True, eps=eps)
    ((F.relu(y) if relu else y) * _t(dy)).sum().backward()
    vn = v.detach().numpy()
    args = (dy, vn, vn.mean(axis=(0, 2, 3)), vn.var(axis=(0, 2, 3)), gamma.detach().numpy(), beta.detach().numpy(), eps, relu)
    dbeta, dgamma, dv = R.bn_bwd_pointwise_ref(*args)
    for got, want in ((dbeta, beta.grad), (dgamma, gamma.grad), (dv, v.grad), (R.du_ref(dv, w.numpy())[0], u.grad)):
        assert np.allclose(got, want.numpy(), rtol=1e-11, atol=1e-11)
    handed = R.bn_bwd_pointwise_ref(*args, sums=(dbeta, dgamma))
    assert np.array_equal(handed[2], dv)
    mag = R.bn_bwd_magnitudes(*args)
    assert (mag["S"] >= np.abs(dv) * (1 - 1e-12)).all() and (mag["Sb"] >= np.abs(dbeta)).all() and (mag["Sg"] >= np.abs(dgamma)).all()


@pytest.mark.parametrize("k", [3, 5, 7])
def test_conv0_bn_wgrad_ref_against_autograd(k):
    rng = np.random.default_rng(k)
    B, H, W, eps = 2, k + 3, 2 * k + 2, 2.0**-10
    x, w = _t(rng.random((B, 1, H, W))), _t(rng.standard_normal((16, 1, k, k)) / k, grad=True)
    gamma, beta = _t(rng.standard_normal(16), grad=True), _t(0.2 * rng.standard_normal(16), grad=True)
    dy = rng.standard_normal((B, 16, H, W))
    v = F.conv2d(x, w, padding=k // 2)
    (F.relu(F.batch_norm(v, None, None, gamma, beta, training=True, eps=eps)) * _t(dy)).sum().backward()
    vn = v.detach().numpy()
    dW, dbeta, dgamma, T = R.conv0_bn_wgrad_ref(x.numpy()[:, 0], dy, vn, vn.mean(axis=(0, 2, 3)), vn.var(axis=(0, 2, 3)), gamma.detach().numpy(), beta.detach().numpy(), eps, k)
    assert np.allclose(dW, w.grad.numpy()[:, 0].reshape(16, k * k).T, rtol=1e-11, atol=1e-11)
    assert np.allclose(dbeta, beta.grad.numpy(), rtol=1e-11, atol=1e-11) and np.allclose(dgamma, gamma.grad.numpy(), rtol=1e-11, atol=1e-11)
    assert (T >= np.abs(dW) * (1 - 1e-12)).all()


def test_small_references():
    rng = np.random.default_rng(1)
    v = rng.integers(-4, 5, size=(3, 5, 4, 7)).astype(np.float64)
    m, va = R.bn_stats_ref(v)
    assert np.allclose(m, v.mean(axis=(0, 2, 3)), rtol=1e-15) and np.allclose(va, v.var(axis=(0, 2, 3)), rtol=1e-14)
    mean, var, gamma, beta = R._bn_vectors(rng, 5)
    y, S = R.bn_apply_ref(v, mean, var, gamma, beta, 2.0**-10, 1)
    want = F.relu(F.batch_norm(_t(v), _t(mean), _t(var), _t(gamma), _t(beta), training=False, eps=2.0**-10)).numpy()
    assert np.allclose(y, want, rtol=1e-13, atol=1e-13) and (S >= np.abs(y)).all()
    a, b = rng.standard_normal((2, 3, 8, 10)), rng.standard_normal((2, 4, 4, 5))
    D, S = R.outer_ref(a, b, 1)
    assert np.allclose(D, np.einsum("bchw,bdhw->cd", a[:, :, ::2, ::2], b)) and (S >= np.abs(D)).all()
    f = rng.standard_normal((2, 3, 4 * 5)).astype(np.float32)
    valid, zeros, pads = R.split_planes(R.feat_to_planes_ref(f, 5, 3, 4, 3), 5, 3, 4, 3)
    assert np.array_equal(valid, f.reshape(2, 3, 4, 5).transpose(0, 3, 1, 2).astype(np.float16)) and not zeros.any() and not pads.any()
    assert np.array_equal(R.relu_bwd_ref(np.array([1.0, 2.0, 3.0]), np.array([-1.0, 0.0, 2.0])), [0.0, 0.0, 3.0])
    shards = np.zeros((32, 1, 16))
    shards[:, 0, :8], shards[:, 0, 8:] = 2.0, 100.0
    m, va = R.shards_stats_ref(shards, 3, 64)
    assert np.array_equal(m, [1.0] * 3) and np.array_equal(va, [49.0] * 3)


# ------------------------------------------------------------------------------------------------- the case tables reach what they claim
def test_pool_cases_reach_the_chunk_paths():
    shapes = {(H, W) for _, H, W, _ in R.POOL_CASES}
    assert shapes == {(H, W) for H in (17, 18, 19, 20, 33) for W in (6, 21)} | {(33, 171), (1, 64), (18, 1)}
    assert {(C, k) for C, _, _, k in R.POOL_CASES} == {(C, k) for C in (7, 30, 64) for k in (3, 5, 7)}
    geo = {(H, W): R.pool_geometry(H, W) for H, W in shapes}
    assert all(g["Ho"] >= 9 and g["nchunk"] >= 2 for hw, g in geo.items() if hw != (1, 64)) and geo[(1, 64)]["nchunk"] == 1
    assert any(g["last_rows"] == 1 and g["nchunk"] >= 2 for g in geo.values())
    assert geo[(33, 171)]["threads"] > 256 and geo[(33, 171)]["workgroups"] == 2
    assert all(g["idle_lanes"] > 0 for g in geo.values())  # in_range == false lanes take part in every case's reduction
    assert 4 * R.PB_ROWS + 2 + R.N_XHAT == R.C_POOL_SUMS
    for case in R.POOL_CASES:
        c = R.pool_case(case, "grid")
        assert (c["gamma"] < 0).any() and (c["gamma"] > 0).any()
        assert np.array_equal(c["dy"], R.f16(c["dy"])) and np.array_equal(c["v"], R.f16(c["v"])) and np.array_equal(c["dout"], R.f16(c["dout"]))
        t = R.pool_case(case, "ties")
        assert (np.abs(t["dy"]) <= 8).all() and np.array_equal(t["dy"], np.rint(t["dy"]))


def test_pointwise_cases_cover_every_axis_at_k3_and_at_a_wide_k():
    assert len(R.PW_CASES) == 16 and sum(c[7] for c in R.PW_CASES) == 1
    for wide in (False, True):
        sel = [c for c in R.PW_CASES if (c[4] != 3) == wide]
        assert {c[:2] for c in sel} == {(7, 9), (30, 24), (44, 40), (64, 64), (9, 64)} and {c[2:4] for c in sel} == {(1, 64), (5, 65), (8, 171), (9, 21)}
        assert {c[5] for c in sel} == {0, 1} and {c[6] for c in sel} == {0, 1}
    assert {c[4] for c in R.PW_CASES} == {3, 5, 7}
    geo = [R.pointwise_geometry(*c[:5]) for c in R.PW_CASES]
    assert {g["MT"] for g in geo} == {1, 2, 3, 4} and {g["KG"] for g in geo} == {1, 2}
    assert any(g["partial_group"] for g in geo) and any(g["partial_octet"] for g in geo) and any(not g["partial_octet"] for g in geo)
    assert any(g["tasks_per_row"] > 1 for g in geo) and any(g["tasks_per_row"] < 1 for g in geo) and any(g["last_task_past_plane"] for g in geo)


def test_outer_cases_reach_the_grid_paths():
    assert {c[0] for c in R.OUTER_CASES} == {7, 16, 17, 64} and {c[1] for c in R.OUTER_CASES} == {7, 16, 17, 64}
    assert {c[2:5] for c in R.OUTER_CASES} >= {(8, 171, 7), (5, 65, 5), (1, 64, 3)}
    geo = {c: R.outer_geo(c) for c in R.OUTER_CASES}
    assert sum(g["nchunks"] > 512 and g["grid"] == 512 and g["passes"] == 2 for g in geo.values()) == 1
    limited = [c for c, g in geo.items() if g["workspace_limited"]]
    assert len(limited) == 1 and limited[0][6] == 3 * limited[0][0] * limited[0][1] and geo[limited[0]]["grid"] == 3 and geo[limited[0]]["passes"] == 2
    strided = [c for c in R.OUTER_CASES if c[7]]
    assert len(strided) == 1 and strided[0][3] == 86 and R.outer_case(strided[0], "exact")["Wa"] == 171
    for c in R.OUTER_CASES:
        assert np.abs(R.outer_case(c, "exact")["S"]).max() + 3 < 2.0**24


def test_stats_and_conv0_cases_reach_both_routes():
    geo = {c: R.stats_geometry(*c[1:4]) for c in R.STATS_CASES}
    assert geo[(9, 190, 171, 3, 1)] == dict(plane=33024, sharded=False) and sum(g["sharded"] for g in geo.values()) == 2
    assert {c[2] for c in R.CONV0_CASES} == {3, 5, 7} and {c[:2] for c in R.CONV0_CASES} == {(8, 171), (5, 65), (1, 64), (16, 12), (400, 171)}
    assert any(c[4] > 0 for c in R.CONV0_CASES) and all(c[3] == 3 for c in R.CONV0_CASES if c[:2] != (400, 171))
    ppt = {c: R.conv0_geometry(*c[:2])["pixels_per_thread"] for c in R.CONV0_CASES}
    assert ppt[(400, 171, 3, 1, 0)] == 2 and sum(p == 2 for p in ppt.values()) == 1 and max(c[0] for c in R.CONV0_CASES) == 400


def test_relu_gate_cap():
    """No case zeroes more than 1 % of its positions."""
    for case in R.PW_CASES:
        assert float(R.pw_case(case)["gated"]) <= 0.01
    for case in R.CONV0_CASES[:4] + R.CONV0_CASES[-1:]:
        assert float(R.conv0_case(case)["gated"]) <= 0.01
    rng = np.random.default_rng(0)  # the gate does zero what lies on it
    v, dy = np.zeros((1, 2, 1, 4)), rng.standard_normal((1, 2, 1, 4))
    out, share = R.relu_gate(dy, v, np.zeros(2), np.ones(2), np.ones(2), np.array([0.0, 1.0]), 0.0)
    assert not out[:, 0].any() and np.array_equal(out[:, 1], dy[:, 1]) and share == 0.5


# ------------------------------------------------------------------------------------------------- sensitivity: each comparison rejects its bug
POOL_S = (30, 18, 21, 5)  # Ho = 9: a second chunk of one row


def test_rejects_gradient_routed_to_a_later_tied_maximum():
    c = R.pool_case(POOL_S, "ties")
    H, W = POOL_S[1:3]
    first = R.pool_routing(c["v"], c["dout"], c["gamma"])
    sgn = np.where(c["gamma"] < 0, -1.0, 1.0)
    R.check_equal(R.pool_scatter(first, H, W), c["dy"])  # the baseline passes
    # one window with two tied maxima and a non-zero gradient: move its gradient from the first to the second
    t = np.pad(c["v"] * sgn[None, :, None, None], ((0, 0), (0, 0), (0, 1), (0, 1)), constant_values=-np.inf)
    done = False
    for idx in np.argwhere(first[0] != 0):  # windows whose gradient went to position 0
        b, ch, i, j = idx
        r0 = 2 * i  # pad_top = 0 at H = 18
        win = [t[b, ch, r0 + dy, 2 * j + dx] for dy in range(3) for dx in range(2)]
        later = [p for p in range(1, 6) if win[p] == win[0]]
        if later:
            moved = first.copy()
            moved[later[0], b, ch, i, j], moved[0, b, ch, i, j] = first[0, b, ch, i, j], 0.0
            done = True
            break
    assert done
    with pytest.raises(AssertionError):
        R.check_equal(R.pool_scatter(moved, H, W), c["dy"])


@pytest.mark.parametrize("family", R.POOL_FAMILIES)
def test_rejects_dropped_carry_of_a_chunks_first_shared_row(family):
    c = R.pool_case(POOL_S, family)
    H, W = POOL_S[1:3]
    contrib = R.pool_routing(c["v"], c["dout"], c["gamma"])
    assert contrib[4:, :, :, R.PB_ROWS - 1].any()
    contrib[4:, :, :, R.PB_ROWS - 1] = 0.0  # what window i0 - 1 sends to the row it shares with window i0 = 8, the second chunk's first
    dy = R.pool_scatter(contrib, H, W)
    with pytest.raises(AssertionError):
        R.check_equal(dy, c["dy"])
    xh = R.xhat_ref(c["v"], c["mean"], c["var"], R.EPS)
    with pytest.raises(AssertionError):
        R.check_within((dy * xh).sum(axis=(0, 2, 3)), c["s_dyx"], R.f32_chain_bound(c["S_dyx"], R.C_POOL_SUMS) + R.f64_sum_bound(c["S_dyx"]))


PW_S = (44, 40, 8, 171, 3, 0, 1, 0)


def _pw_bound(c):
    return R.f16_out_bound(c["dv"], c["S"], R.N_BN_BWD)


def test_rejects_channel_constants_shifted_by_one_channel_and_a_few_percent_in_a_small_channel():
    c = R.pw_case(PW_S)
    R.check_within(R.f16(c["dv"]), c["dv"], _pw_bound(c))  # the stored reference itself passes
    roll = lambda a: np.roll(a, 1)  # noqa: E731
    shifted = R.bn_bwd_pointwise_ref(c["dy"], c["v"], roll(c["mean"]), roll(c["var"]), roll(c["gamma"]), roll(c["beta"]), R.EPS, PW_S[5])[2]
    with pytest.raises(AssertionError):
        R.check_within(R.f16(shifted), c["dv"], _pw_bound(c))
    small = int(np.argmin(np.abs(c["dv"]).max(axis=(0, 2, 3))))
    off = c["dv"].copy()
    off[:, small] *= 1.03
    assert np.abs(off - c["dv"]).max() <= 3e-3 * np.abs(c["dv"]).max() or np.abs(c["dv"][:, small]).max() < np.abs(c["dv"]).max()
    with pytest.raises(AssertionError):
        R.check_within(R.f16(off), c["dv"], _pw_bound(c))


def test_rejects_last_column_zero_and_one_zero_tile_of_du():
    c = R.pw_case(PW_S)
    dv = R.f16(c["dv"])
    cut = dv.copy()
    cut[..., -1] = 0.0
    with pytest.raises(AssertionError):
        R.check_within(cut, c["dv"], _pw_bound(c))
    want, S = R.du_ref(dv, c["wt"])
    bound = R.f16_out_bound(want, S, R.mfma_sum_count(8 * 6))
    R.check_within(R.f16(want), want, bound)
    tile = R.f16(want)
    tile[:, 16:32] = 0.0
    with pytest.raises(AssertionError):
        R.check_within(tile, want, bound)


def test_rejects_written_pads_and_non_zero_channels_past_C():
    C, H, W, k = 13, 5, 6, 5
    fill = int(np.float16(30000.0).view(np.uint16))
    x = np.random.default_rng(2).standard_normal((2, C, H, W)).astype(np.float16)
    full = np.full((2, 16, H + 4, R.padded_width(W, k)), 30000.0, dtype=np.float16)  # what a correct kernel leaves of a sentinel buffer
    full[:, :, 2 : 2 + H, :W] = 0.0
    full[:, :C, 2 : 2 + H, :W] = x
    bits = np.ascontiguousarray(full.reshape(2, 2, 8, H + 4, -1).transpose(0, 1, 3, 4, 2)).view(np.uint16)
    assert np.array_equal(R.check_planes(bits, C, H, W, k, fill).view(np.float16), x)
    for where, what in (((1, 1, 3, 2, 7), "channel 15 at an image pixel"), ((0, 0, 1, 2, 0), "a pad row"), ((1, 1, 3, W, 2), "a pad column")):
        bad = bits.copy()
        bad[where] = int(np.float16(0.5).view(np.uint16))
        with pytest.raises(AssertionError):
            R.check_planes(bad, C, H, W, k, fill, what)
    unwritten = bits.copy()
    unwritten[0, 0, 2, 0, 0] = fill
    with pytest.raises(AssertionError):
        R.check_planes(unwritten, C, H, W, k, fill)
    R.check_planes(unwritten, C, H, W, k, fill, written=False)


def test_rejects_a_dropped_chunk_of_the_outer_product():
    case = (17, 7, 8, 171, 7, 52, 0, 0)
    c, geo = R.outer_case(case, "normal"), R.outer_geo(case)
    a = c["a"].copy()
    a[-1, :, -1, -86:] = 0.0  # about a third of the last 256-pixel chunk of the last snippet
    D = R.outer_ref(a, c["b"], 0)[0]
    with pytest.raises(AssertionError):
        R.check_within(D, c["D"], R.f32_chain_bound(c["S"], R.outer_chain(geo)))


# ------------------------------------------------------------------------------------------------- the bounds can be met in f32
def _two_orders(terms):
    """f32 sums over the last axis: sequential front to back, and numpy's pairwise sum back to front."""
    t = np.ascontiguousarray(terms, dtype=np.float32)
    return np.cumsum(t, axis=-1, dtype=np.float32)[..., -1].astype(np.float64), np.sum(t[..., ::-1], axis=-1, dtype=np.float32).astype(np.float64)


def _xhat32(v, mean, var):
    inv = (np.float32(1) / np.sqrt(np.asarray(var, dtype=np.float32) + np.float32(R.EPS))).astype(np.float32)
    return ((np.asarray(v, dtype=np.float32) - np.asarray(mean, dtype=np.float32)[None, :, None, None]) * inv[None, :, None, None]).astype(np.float32), inv


def _dv32(c, relu, n):
    """bn_bwd_value in numpy float32, c1 and c2 from the float64 sums as fill_bn_bwd_table forms them."""
    xh, inv = _xhat32(c["v"], c["mean"], c["var"])
    g, bt = (np.asarray(c[name], dtype=np.float32)[None, :, None, None] for name in ("gamma", "beta"))
    de = np.asarray(c["dy"], dtype=np.float32)
    if relu:
        de = np.where(xh * g + bt > 0, de, np.float32(0))
    inv_count = np.float32(1.0 / n)
    c1, c2 = ((np.asarray(c[name]).astype(np.float32) * inv_count)[None, :, None, None] for name in ("dbeta", "dgamma"))
    return ((g * inv[None, :, None, None]) * (de - c1 - xh * c2)).astype(np.float32)


@pytest.mark.parametrize("family", R.POOL_FAMILIES)
def test_f32_emulation_meets_the_pool_sums_bound(family):
    for case in R.POOL_CASES:
        c = R.pool_case(case, family)
        xh, _ = _xhat32(c["v"], c["mean"], c["var"])
        terms = (c["dy"].astype(np.float32) * xh).transpose(1, 0, 2, 3).reshape(case[0], -1)
        for got in _two_orders(terms):
            R.check_within(got, c["s_dyx"], R.f32_chain_bound(c["S_dyx"], R.C_POOL_SUMS) + R.f64_sum_bound(c["S_dyx"]), R.pool_case_id(case))


def test_f32_emulation_meets_the_pointwise_bounds():
    for case in R.PW_CASES:
        c = R.pw_case(case)
        C, Cin, H, W, k, relu = case[:6]
        dv = _dv32(c, relu, R.PW_B * H * W).astype(np.float16).astype(np.float64)
        R.check_within(dv, c["dv"], R.f16_out_bound(c["dv"], c["S"], R.N_BN_BWD), R.pw_case_id(case) + " dv")
        want, S = R.du_ref(dv, c["wt"])
        bound = R.f16_out_bound(want, S, R.mfma_sum_count(8 * ((C + 7) // 8)))
        w32 = c["wt"].astype(np.float32)
        for du in (np.einsum("bohw,oi->bihw", dv.astype(np.float32), w32), np.einsum("bohw,oi->bihw", dv.astype(np.float32)[:, ::-1], w32[::-1])):
            R.check_within(du.astype(np.float16).astype(np.float64), want, bound, R.pw_case_id(case) + " du")


def test_f32_emulation_meets_the_outer_bound():
    for case in R.OUTER_CASES:
        c, geo = R.outer_case(case, "normal"), R.outer_geo(case)
        Ca, Cb, H, W = case[:4]
        a = c["a"][:, :, ::2, ::2][:, :, :H, :W] if case[7] else c["a"]
        a32, b32 = a.astype(np.float32).transpose(1, 0, 2, 3).reshape(Ca, -1), c["b"].astype(np.float32).transpose(1, 0, 2, 3).reshape(Cb, -1)
        for ca in range(0, Ca, 5):
            for got in _two_orders(a32[ca][None, :] * b32):
                R.check_within(got, c["D"][ca], R.f32_chain_bound(c["S"][ca], R.outer_chain(geo)), R.outer_case_id(case))


def test_f32_emulation_meets_the_conv0_and_apply_bounds():
    for case in R.CONV0_CASES:
        H, W, k, B, _ = case
        c = R.conv0_case(case)
        dv = _dv32(c, 1, B * H * W)
        Rr = k // 2
        xp = np.zeros((B, H + 2 * Rr, W + 2 * Rr), dtype=np.float32)
        xp[:, Rr : Rr + H, Rr : Rr + W] = c["x"]
        bound = R.f32_chain_bound(c["T"], R.conv0_chain(B, H, W))
        for tap in (0, k * k // 2, k * k - 1):
            win = xp[:, tap // k : tap // k + H, tap % k : tap % k + W]
            for got in _two_orders((win[:, None] * dv).transpose(1, 0, 2, 3).reshape(16, -1)):
                R.check_within(got, c["dW"][tap], bound[tap], R.conv0_case_id(case))
    for C, H, W, k, relu in R.APPLY_CASES:
        rng = np.random.default_rng([C, H, W, k, relu])
        v = R.f16(2.0 * rng.standard_normal((R.APPLY_B, C, H, W)))
        mean, var, gamma, beta = R._bn_vectors(rng, C)
        want, S = R.bn_apply_ref(v, mean, var, gamma, beta, R.EPS, relu)
        s = (gamma * (np.float32(1) / np.sqrt(var + np.float32(R.EPS))).astype(np.float32)).astype(np.float32)
        y = v.astype(np.float32) * s[None, :, None, None] + (beta - mean * s).astype(np.float32)[None, :, None, None]
        y = np.maximum(y, 0) if relu else y
        R.check_within(y.astype(np.float16).astype(np.float64), want, R.f16_out_bound(want, S, R.N_BN_APPLY))
