"""tests/half_trunk_ref.py on the CPU, so that tests/test_half_trunk_gpu.py can lean on it:
  the float64 references against torch float64 (conv2d, max_pool2d) and oracle.model_ref's layers;
  every exact-kind case stays in the range where f16 holds every partial sum and stored value;
  sensitivity: the checks the GPU tests apply (half_trunk_ref.check_*) reject a mutated reference -- a subtly wrong kernel -- in every family;
  the bounds against a numpy emulation of the kernels' arithmetic (f16 multiply and add per tap, f32 accumulation of the pointwise sum, one
  f16 rounding at the store): the emulation stays inside the bounds, its worst error / bound per family is printed."""

import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import half_trunk_ref as R  # noqa: E402
from oracle import model_ref as M  # noqa: E402

F = torch.nn.functional
KINDS = [True, False]
KIND_IDS = ["exact", "normal"]
# family -> (case table, case function)
SEP_FAMILIES = {"sep3": (R.SEP3_CASES, R.sep3_case), "sepk": (R.SEPK_CASES, R.sepk_case), "stats": (R.STATS_CASES, R.stats_case),
                "stats_bn": (R.STATS_CASES, R.stats_case)}


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float64)))


def _bn_of(family, c):
    return c["bn"] if family == "stats_bn" else None


def _relu_in_of(family, c):
    """The _bn variant has no ReLU-on-load flag of its own (the launcher passes 0; the ReLU is part of BatchNorm + ReLU)."""
    return dict(c, relu_in=0) if family == "stats_bn" else c


# ------------------------------------------------------------------------------------------------- the references against torch float64
@pytest.mark.parametrize("name", [n for n in R.CONV0_CASES if "9x33" in n or "1x3" in n])
def test_conv0_ref_equals_torch_float64(name):
    c = R.conv0_case(name, False)
    k = c["k"]
    for relu in (0, 1):
        v, S = R.conv0_ref(c["x"], c["w"], c["scale"], c["shift"], relu)
        t = F.conv2d(_t(c["x"])[:, None], _t(c["w"]).t().reshape(16, 1, k, k), padding=k // 2) * _t(c["scale"])[None, :, None, None] + _t(c["shift"])[None, :, None, None]
        t = torch.relu(t) if relu else t
        assert np.abs(v - t.numpy()).max() <= 1e-12 and (S >= np.abs(v) - 1e-12).all()
    if c["stride"] < c["H"] * c["W"]:  # the sliding view: snippet 1 starts inside snippet 0
        assert np.array_equal(c["x"][1].ravel()[: c["H"] * c["W"] - c["stride"]], c["x"][0].ravel()[c["stride"] :])
    # the oracle's own layers: Conv2D "same" + bias, then inference BatchNorm + ReLU
    mean, var, gamma_, beta = c["bn"]
    p = {"c/kernel": c["w"].reshape(k, k, 1, 16).astype(np.float64), "c/bias": c["shift"].astype(np.float64), "bn/gamma": gamma_, "bn/beta": beta, "bn/mean": mean, "bn/var": var}
    v1, _ = R.conv0_ref(c["x"], c["w"], np.ones(16), c["shift"], 0)
    with torch.no_grad():
        tv = M._conv_same(_t(c["x"])[:, None], p["c/kernel"], p["c/bias"], 1, torch.float64)
        assert np.abs(v1 - tv.numpy()).max() <= 1e-12
        assert M.BN_EPS == R.BN_EPS
        y, T = R.bn_relu_ref(v1, *c["bn"], c["eps"])
        ty = torch.relu(M._bn_infer(tv, {k_: np.asarray(a, dtype=np.float64) for k_, a in p.items()}, "bn", torch.float64))
        assert np.abs(y - ty.numpy()).max() <= 1e-12 and (T >= y - 1e-12).all()
    # conv0_bn_ref forms y from the ROUNDED v
    v, S, y, T = R.conv0_bn_ref(c["x"], c["w"], c["scale"], c["shift"], *c["bn"], c["eps"])
    assert np.array_equal(y, R.bn_relu_ref(R.r16(v), *c["bn"], c["eps"])[0]) and np.abs(y - R.bn_relu_ref(v, *c["bn"], c["eps"])[0]).max() > 1e-5


def _torch_sep(c, xa):
    k, Cin = c["ktap"], c["Cin"]
    dw = _t(R.r16(c["dwk"])).permute(2, 0, 1)[:, None]  # [Cin][1][k][k]
    u = F.conv2d(_t(xa), dw, padding=k // 2, groups=Cin)
    v = F.conv2d(u, _t(R.r16(c["pw"])).t()[:, :, None, None]) * _t(c["scale"])[None, :, None, None] + _t(c["shift"])[None, :, None, None]
    return u.numpy(), (torch.relu(v) if c["relu_out"] else v)


@pytest.mark.parametrize("family,name", [("sep3", "16->30 5x21 planes+u relu in/out"), ("sep3", "40->50 8x63 x-pooled relu in"), ("sep3", "5->7 5x21 Keras reshape"),
                                         ("sepk", "k5 16->30 5x65 x-pooled (lo 2), odd W"), ("sepk", "k7 30->16 4x65 planes+u relu out"),
                                         ("sepk", "ktap 1 on k5 planes, 30->16 5x33 scatter-add onto a 9x65 start image (odd H2, W2)"), ("stats_bn", "16->30 5x21 B3")])
def test_sepconv_ref_equals_torch_float64(family, name):
    c = SEP_FAMILIES[family][1](name, False)
    bn = _bn_of(family, c)
    for a in (c["x"], c["dwk"], c["pw"]):  # what the kernel is given is what the reference sees
        assert np.array_equal(a, R.r16(a))
    u, Su, v, S = R.sepconv_ref(c["x"], c["dwk"], c["pw"], c["scale"], c["shift"], c["relu_in"] if bn is None else 0, c["relu_out"], bn, c.get("eps", R.BN_EPS))
    if bn is None:
        xa = np.maximum(c["x"], 0.0) if c["relu_in"] else c["x"]
    else:  # y_a = f16(relu(BN(v))) inside the image; conv2d's zero padding is the "same" padding of y_a
        sc, sh = R.bn_fold(*bn, c["eps"])
        xa = R.r16(np.maximum(c["x"].astype(np.float64) * sc[None, :, None, None] + sh[None, :, None, None], 0.0))
        assert (sh > 0).any()  # relu(sh) != 0: padding v instead of y_a would show
    tu, tv = _torch_sep(c, xa)
    assert np.abs(u - tu).max() <= 1e-12 and np.abs(v - tv.numpy()).max() <= 1e-12
    assert (Su >= np.abs(u) - 1e-12).all() and (S >= np.abs(v) - 1e-12).all()
    if family == "sep3" and c["relu_in"]:  # the oracle's SeparableConv2D (bias = the shift, scale 1)
        p = {"s/depthwise": R.r16(c["dwk"])[..., None], "s/pointwise": R.r16(c["pw"])[None, None], "s/bias": c["shift"].astype(np.float64)}
        with torch.no_grad():
            ts = M._sepconv(_t(xa), p, "s", torch.float64)
        v1, _ = R.pointwise_ref(u, c["pw"], np.ones(c["Cout"]), c["shift"], 0)
        assert np.abs(v1 - ts.numpy()).max() <= 1e-12
    if c["layout"] == 2:  # the (1, 2) "same" maximum: the pad right of an odd W does not count
        W = c["W"]
        tp = F.max_pool2d(F.pad(tv, (0, W % 2), value=float("-inf")), (1, 2), (1, 2))
        assert np.array_equal(R.layout2(tv.numpy()), tp.numpy())
    if c["layout"] == 1:
        feat = R.layout1(v)
        assert feat.shape == (c["B"], c["H"], c["W"] * c["Cout"]) and feat[1, 2, 3 * c["Cout"] + 4] == v[1, 4, 2, 3] and np.array_equal(R.from_layout1(feat, c["Cout"]), v)
    if c["layout"] == 3:
        out = R.layout3(c["start"], v)
        assert out.shape == (c["B"], c["Cout"], 2 * c["H"] - 1, 2 * c["W"] - 1)
        assert out[1, 3, 4, 6] == c["start"][1, 3, 4, 6] + v[1, 3, 2, 3] and out[1, 3, 3, 6] == c["start"][1, 3, 3, 6] and out[1, 3, 4, 5] == c["start"][1, 3, 4, 5]


def test_xpooled_octets_round_trip():
    v = np.random.default_rng(3).standard_normal((2, 9, 3, 5))
    p = R.to_xpooled(v, fill=R.r16(777.0))
    full = R.from_xpooled(p)
    assert full.shape == (2, 16, 3, 4) and np.array_equal(full[:, :9, :, :3], R.r16(R.layout2(v))) and (full[:, :9, :, 3] == 777.0).all() and not full[:, 9:].any()


# ------------------------------------------------------------------------------------------------- the tables cover what they claim
def test_case_tables_cover_every_value_on_each_route():
    both = [v for v in R.SEP3_CASES.values() if v[4] != 1]  # out_layout 1 is the one-window kernel in every mode
    assert {v[:2] for v in both} == {v[:2] for v in R.SEP3_CASES.values()} == {(5, 7), (16, 30), (30, 16), (40, 50), (64, 64)}
    assert {v[2:4] for v in both} == {(1, 3), (5, 21), (9, 62), (8, 63), (7, 130)}
    flags = {v[4:] for v in R.SEP3_CASES.values()}
    assert {f[0] for f in flags} == {0, 1, 2} and {(f[0], f[3]) for f in flags} >= {(0, True), (0, False)} and {(f[0], f[2]) for f in flags} >= {(2, 0), (2, 1)}
    assert {f[1] for f in flags} == {0, 1}
    assert any(v[4] == 2 and v[3] % 2 == 1 and v[6] == 0 for v in both)  # an odd-W pair with negative values left in
    assert {(v[4], v[5]) for v in R.SEPK_CASES.values()} == {(5, 5), (5, 1), (7, 7)} and {v[6] for v in R.SEPK_CASES.values()} == {0, 2, 3}
    assert {(k, H, W) for k, H, W, _ in R.CONV0_CASES.values()} == {(k, H, W) for k in (3, 5, 7) for H, W in ((1, 3), (8, 32), (9, 33), (5, 61))}
    assert {k for k, H, W, s in R.CONV0_CASES.values() if s} == {3, 5, 7}
    assert sorted(v[0] for v in R.STATS_CASES.values()) == [2, 2, 2, 3] and all((v[1:5]) in {w[:4] for w in R.SEP3_CASES.values()} for v in R.STATS_CASES.values())


def _all_cases(exact):
    for name in R.CONV0_CASES:
        yield "conv0", name, R.conv0_case(name, exact)
    for family, (table, fn) in SEP_FAMILIES.items():
        for name in table:
            yield family, name, fn(name, exact)


def test_normal_scales_are_of_both_signs_a_third_negative():
    for family, name, c in _all_cases(False):
        s = c["scale"]
        assert (np.abs(s) >= 0.5).all() and (np.abs(s) <= 2.0).all() and 3 * (s < 0).sum() >= s.size and (s > 0).any(), (family, name)
        if "bn" in c:
            g = c["bn"][2]
            assert (g < 0).any() and (g > 0).any() and (g == 0).sum() == 1 and c["eps"] == 1e-3, (family, name)
    for family, name, c in _all_cases(True):
        assert set(np.unique(c["scale"])) <= set(R.SCALES) and (c["scale"] < 0).any() and (c["scale"] > 0).any(), (family, name)


# ------------------------------------------------------------------------------------------------- the exact kind is exact
def _is_f16(a):
    return np.array_equal(R.r16(a), a)


def test_exact_cases_stay_exactly_representable():
    """Every partial sum of the depthwise stage is an integer of magnitude <= Su < 2048: exact in f16 in any order.  Every partial sum of the
    pointwise stage and of the entry convolution is an integer far below 2^24 (f32), and the stored value -- a multiple of 1/2 (scale 0.5) of
    magnitude <= S < 1024 -- is exactly representable in f16; so are y of the entry's BatchNorm twin and the scatter-add's sum."""
    for name in R.CONV0_CASES:
        c = R.conv0_case(name, True)
        v, S, y, T = R.conv0_bn_ref(c["x"], c["w"], c["scale"], c["shift"], *c["bn"], c["eps"])
        assert S.max() < 1024 and np.array_equal(2 * v, np.rint(2 * v)) and _is_f16(v), (name, S.max())
        # the fold is exact (var = 1, eps = 0: sc = gamma, a power of two; sh a multiple of 1/2), y a multiple of 1/4 of magnitude <= T < 512
        sc, sh = R.bn_fold(*c["bn"], c["eps"])
        assert c["eps"] == 0.0 and np.array_equal(sc, c["bn"][2]) and np.array_equal(2 * sh, np.rint(2 * sh))
        assert T.max() < 512 and np.array_equal(4 * y, np.rint(4 * y)) and _is_f16(y), (name, T.max())
    for family, (table, fn) in SEP_FAMILIES.items():
        for name in table:
            c = _relu_in_of(family, fn(name, True))
            bn = _bn_of(family, c)
            xa = R.load_ref(c["x"], c["relu_in"], bn, c.get("eps", 0.0))
            if bn is not None:
                assert c["eps"] == 0.0 and np.abs(xa).max() < 64 and np.array_equal(2 * xa, np.rint(2 * xa))
            u, Su = R.depthwise_ref(xa, c["dwk"])
            assert Su.max() < 2048 and np.array_equal(2 * u, np.rint(2 * u)) and _is_f16(u), (family, name, Su.max())
            if bn is not None:  # half-integers in: every partial sum a multiple of 1/2 below 1024
                assert Su.max() < 1024
            v, S = R.pointwise_ref(u, c["pw"], c["scale"], c["shift"], c["relu_out"])
            assert S.max() < 1024 and _is_f16(v), (family, name, S.max())
            grain = 4 if bn is not None else 2
            assert np.array_equal(grain * v, np.rint(grain * v)) and grain * S.max() < 2048
            if c["layout"] == 3:
                out = R.layout3(c["start"], v)
                assert np.abs(out).max() + 0 < 1024 and _is_f16(out)
            for a in (c["x"], c["dwk"], c["pw"]):
                assert _is_f16(a)


# ------------------------------------------------------------------------------------------------- an emulation of the kernels' arithmetic
def r32(a):
    return np.asarray(a).astype(np.float32).astype(np.float64)


def _fold32(bn, eps):
    """sc = gamma * rsqrtf(var + eps), sh = beta - mean * sc, every operation rounded to f32."""
    mean, var, gamma_, beta = (np.asarray(a, dtype=np.float64) for a in bn)
    sc = r32(gamma_ * r32(1.0 / np.sqrt(r32(var + r32(eps)))))
    return sc, r32(beta - r32(mean * sc))


def emu_conv0(c, relu, bn=False):
    """conv0_h_kernel: an f32 fma chain over the taps, fma with scale and shift, ReLU, one f16 rounding; BN: y from the stored value."""
    x, w, k = np.asarray(c["x"], dtype=np.float64), np.asarray(c["w"], dtype=np.float64), c["k"]
    B, H, W = x.shape
    Rr = k // 2
    xp = np.zeros((B, H + 2 * Rr, W + 2 * Rr))
    xp[:, Rr : Rr + H, Rr : Rr + W] = x
    acc = np.zeros((B, 16, H, W))
    for dy in range(k):
        for dx in range(k):
            acc = r32(xp[:, None, dy : dy + H, dx : dx + W] * w[dy * k + dx][None, :, None, None] + acc)
    v = r32(acc * R._c(c["scale"]) + R._c(c["shift"]))
    v = R.r16(np.maximum(v, 0.0) if relu else v)
    if not bn:
        return v
    sc, sh = _fold32(c["bn"], c["eps"])
    return v, R.r16(np.maximum(r32(v * R._c(sc) + R._c(sh)), 0.0))


def emu_depthwise(xa, dwk, contract):
    """dw_octet: per column offset dx a partial sum over the rows in f16 (contract: one rounding per tap, v_pk_fma_f16; else the product and the
    sum rounded separately), then the centre column plus the other columns' sums shifted in, dx ascending, one f16 addition each."""
    w = R.r16(dwk)
    k = w.shape[0]
    Rr = k // 2
    B, C, H, W = xa.shape
    xp = np.zeros((B, C, H + 2 * Rr, W + 2 * Rr))
    xp[:, :, Rr : Rr + H, Rr : Rr + W] = xa
    p = []
    for dx in range(k):
        s = np.zeros((B, C, H, W + 2 * Rr))
        for dy in range(k):
            t = xp[:, :, dy : dy + H, :] * R._c(w[dy, dx])
            s = R.r16(t + s) if contract else R.r16(R.r16(t) + s)
        p.append(s)
    acc = p[Rr][..., Rr : Rr + W]
    for dx in range(k):
        if dx != Rr:
            acc = R.r16(acc + p[dx][..., dx : dx + W])
    return acc


def emu_sep(c, contract, bn=None):
    """-> (u, out in the case's layout, the f32 values before the store)."""
    if bn is None:
        xa = R.load_ref(c["x"], c["relu_in"])
    else:
        sc, sh = _fold32(bn, c["eps"])
        xa = R.r16(np.maximum(r32(R.r16(c["x"]) * R._c(sc) + R._c(sh)), 0.0))
    u = emu_depthwise(xa, c["dwk"], contract)
    w = R.r16(c["pw"])
    acc = np.zeros((c["B"], c["Cout"]) + u.shape[2:])
    for ci in range(c["Cin"]):  # the product of two f16 is exact in f32
        acc = r32(acc + u[:, ci, None] * w[ci][None, :, None, None])
    v = r32(acc * R._c(c["scale"]) + R._c(c["shift"]))
    v = np.maximum(v, 0.0) if c["relu_out"] else v
    layout = c["layout"]
    if layout == 0:
        out = R.r16(v)
    elif layout == 1:
        out = v
    elif layout == 2:
        out = R.r16(R.layout2(v))
    else:
        out = np.array(c["start"], dtype=np.float64)
        H, W = v.shape[2:]
        out[:, :, : 2 * H : 2, : 2 * W : 2] = R.r16(out[:, :, : 2 * H : 2, : 2 * W : 2] + R.r16(v))
    return u, out, v


def emu_stats(v):
    """The DEPTH of the statistics epilogue's summation tree on f32 values v [B][C][H][W], not the kernel's pixel-to-lane map: per snippet the
    image's pixels in windows of 62, four per lane of 16, an inclusive scan over the 16 lanes, 8 windows per workgroup added one after the other;
    f64 from there (atomics, shards, finish), the results rounded to f32.  The kernel walks the flat PADDED plane of pitch WP, so pad columns
    (zeros) sit inside its windows and a pixel lands on another lane and wave; every value still passes through the same number of f32
    additions, which is all stats_bounds depends on."""
    B, C, H, W = v.shape
    N = B * H * W
    su, sq = np.zeros(C), np.zeros(C)
    for b in range(B):
        flat = v[b].reshape(C, H * W)
        nwin = -(-H * W // 62)
        buf = np.zeros((C, -(-nwin // 8) * 8, 64))
        for wi in range(nwin):
            seg = flat[:, wi * 62 : (wi + 1) * 62]
            buf[:, wi, 1 : 1 + seg.shape[1]] = seg
        t = buf.reshape(C, -1, 8, 4, 16)  # [workgroup][wave][tile][lane]
        for kind in (0, 1):
            if kind == 0:
                lane = r32(r32(t[..., 0, :] + t[..., 1, :]) + r32(t[..., 2, :] + t[..., 3, :]))
            else:
                lane = np.zeros(t[..., 0, :].shape)
                for ti in range(4):
                    lane = r32(t[..., ti, :] ** 2 + lane)
            for sh in (1, 2, 4, 8):
                shifted = np.zeros(lane.shape)
                shifted[..., sh:] = lane[..., :-sh]
                lane = r32(lane + shifted)
            row = lane[..., 15]  # [C][workgroup][wave]
            tot = np.zeros(row.shape[:2])
            for w8 in range(8):
                tot = r32(tot + row[..., w8])
            if kind == 0:
                su += tot.sum(axis=1)
            else:
                sq += tot.sum(axis=1)
    mu = su / N
    return r32(mu), r32(np.maximum(sq / N - mu * mu, 0.0))


def _worst(checks, worst, family):
    for ch in checks:
        assert ch.ok, (family, ch)
        worst[family] = max(worst.get(family, 0.0), ch.ratio)


@pytest.mark.parametrize("exact", KINDS, ids=KIND_IDS)
def test_the_emulated_arithmetic_stays_inside_the_bounds(exact):
    """The checks of the GPU tests on the emulation: exact kind equal to float64, normal kind inside every bound.  A bound that forgot a rounding
    fails here, without a GPU."""
    worst = {}
    for name in R.CONV0_CASES:
        c = R.conv0_case(name, exact)
        for relu in (0, 1):
            _worst(R.check_conv0(c, relu, emu_conv0(c, relu), exact), worst, "conv0")
        _worst(R.check_conv0_bn(c, *emu_conv0(c, 0, bn=True), exact), worst, "conv0_bn")
    for family, (table, fn) in SEP_FAMILIES.items():
        for name in table:
            c = _relu_in_of(family, fn(name, exact))
            bn = _bn_of(family, c)
            for contract in (True, False):
                u, out, v32 = emu_sep(c, contract, bn)
                _worst(R.check_sep(c, u, out, exact, bn), worst, family)
                if family.startswith("stats"):
                    _worst(R.check_stats(c, u, *emu_stats(v32)), worst, family + " mean/var")
    for family, ratio in worst.items():
        print(f"emulation, {'exact' if exact else 'normal'} kind, {family}: worst error / bound = {ratio:.3f}")
    assert exact or all(0.0 < r <= 1.0 for r in worst.values())


# ------------------------------------------------------------------------------------------------- sensitivity: mutated references
def _swap_octets(vec):
    """Channel c gets the value of channel c ^ 8 (the other octet of its 16-channel tile); a kernel holds 0 past the last channel."""
    vec = np.asarray(vec, dtype=np.float64)
    padded = np.zeros((vec.size + 15) // 16 * 16)
    padded[: vec.size] = vec
    return padded[np.arange(vec.size) ^ 8]


def _pair_max_zero_filled(v):
    """The x-pool with the missing second column of an odd W read as 0."""
    B, C, H, W = v.shape
    Wx = (W + 1) // 2
    pairs = np.zeros((B, C, H, 2 * Wx))
    pairs[..., :W] = v
    return pairs.reshape(B, C, H, Wx, 2).max(axis=4)


def sep_mutant(c, mut, bn=None):
    """(u, out) of a float64 separable convolution that is wrong in one way (mut None: right)."""
    relu_in = 0 if mut == "relu-on-load skipped" else c["relu_in"]
    xa = R.load_ref(c["x"], relu_in, bn, c.get("eps", R.BN_EPS))
    dwk = np.array(c["dwk"])
    if mut == "tap dropped":
        dwk[dwk.shape[0] // 2, -1] = 0.0  # centre row, last column: inside every image at least two pixels wide
    pad = None
    if mut == "pads normalised":
        pad = np.maximum(R.bn_fold(*bn, c["eps"])[1], 0.0)
    u = R.depthwise_ref(xa, dwk, pad)[0]
    scale, shift = (_swap_octets(c["scale"]), _swap_octets(c["shift"])) if mut == "octets swapped" else (c["scale"], c["shift"])
    v = R.pointwise_ref(u, c["pw"], scale, shift, c["relu_out"])[0]
    if c["layout"] == 2:
        if mut == "max before affine":
            acc = R.layout2(R.pointwise_ref(u, c["pw"], np.ones(c["Cout"]), np.zeros(c["Cout"]), 0)[0])
            out = acc * R._c(c["scale"]) + R._c(c["shift"])
            out = np.maximum(out, 0.0) if c["relu_out"] else out
        else:
            out = _pair_max_zero_filled(v) if mut == "odd pair zero" else R.layout2(v)
    else:
        out = R.layout3(c["start"], v) if c["layout"] == 3 else v
    if mut == "u stored scaled":
        u = u * R._c(np.resize(c["scale"], c["Cin"]))
    return u, out


# mutant -> the families it must be caught in
SEP_MUTANTS = {
    "octets swapped": ("sep3", "sepk", "stats", "stats_bn"),
    "max before affine": ("sep3", "sepk"),
    "odd pair zero": ("sep3", "sepk"),
    "relu-on-load skipped": ("sep3", "sepk", "stats"),
    "pads normalised": ("stats_bn",),
    "tap dropped": ("sep3", "sepk", "stats", "stats_bn"),
    "u stored scaled": ("sep3", "sepk", "stats", "stats_bn"),
}


@functools.lru_cache(maxsize=None)
def _caught(family, mut, exact):
    """The cases of the family whose checks reject the mutant."""
    table, fn = SEP_FAMILIES[family]
    hit = []
    for name in table:
        c = _relu_in_of(family, fn(name, exact))
        bn = _bn_of(family, c)
        u, out = sep_mutant(c, mut, bn)
        if not all(ch.ok for ch in R.check_sep(c, u, out, exact, bn)):
            hit.append(name)
    return tuple(hit)


@pytest.mark.parametrize("exact", KINDS, ids=KIND_IDS)
@pytest.mark.parametrize("family", list(SEP_FAMILIES))
def test_every_mutant_is_caught_in_every_family(family, exact):
    assert _caught(family, None, exact) == (), family  # the unmutated reference passes its own checks
    table = SEP_FAMILIES[family][0]
    for mut, families in SEP_MUTANTS.items():
        if family in families:
            hit = _caught(family, mut, exact)
            print(f"{'exact' if exact else 'normal'} kind, {family}: '{mut}' caught in {len(hit)} of {len(table)} cases")
            assert hit, (family, mut)
    # where a mutant can show at all, it does: every x-pooled case sees the maximum taken first, every case the swapped octets and the dropped tap
    if family in ("sep3", "sepk"):
        assert set(_caught(family, "max before affine", exact)) == {n for n, v in table.items() if v[-4] == 2}
    assert set(_caught(family, "octets swapped", exact)) == set(table)
    if not exact:  # (a sparse integer tap may be 0 in every channel: the real-valued taps are what sees every tap)
        assert set(_caught(family, "tap dropped", exact)) == set(table)


@pytest.mark.parametrize("exact", KINDS, ids=KIND_IDS)
def test_conv0_mutants_are_caught(exact):
    n_swap = n_y = 0
    for name in R.CONV0_CASES:
        c = R.conv0_case(name, exact)
        v, S, y, T = R.conv0_bn_ref(c["x"], c["w"], c["scale"], c["shift"], *c["bn"], c["eps"])
        assert all(ch.ok for ch in R.check_conv0_bn(c, R.r16(v), y, exact))
        for relu in (0, 1):
            want = R.conv0_ref(c["x"], c["w"], c["scale"], c["shift"], relu)[0]
            assert all(ch.ok for ch in R.check_conv0(c, relu, want, exact))
            swapped = R.conv0_ref(c["x"], c["w"], _swap_octets(c["scale"]), _swap_octets(c["shift"]), relu)[0]
            n_swap += not all(ch.ok for ch in R.check_conv0(c, relu, swapped, exact))
        # y formed from the unrounded v: next to a faithfully stored v
        y_unrounded = R.bn_relu_ref(v, *c["bn"], c["eps"])[0]
        n_y += not all(ch.ok for ch in R.check_conv0_bn(c, R.r16(v), y_unrounded, exact))
    print(f"conv0, {'exact' if exact else 'normal'} kind: octets swapped caught in {n_swap} of {2 * len(R.CONV0_CASES)}, y from the unrounded v in {n_y} of {len(R.CONV0_CASES)}")
    assert n_swap == 2 * len(R.CONV0_CASES)
    assert n_y == (0 if exact else len(R.CONV0_CASES))  # in the exact kind the rounding changes nothing: that mutant is the normal kind's to catch


def test_stats_bounds_reject_statistics_of_the_wrong_tensor():
    """The finished mean / variance: a sum that skipped one pixel per snippet, or was taken after the ReLU of a later layer, is outside the bounds;
    the float64 statistics themselves are inside."""
    for name in R.STATS_CASES:
        c = R.stats_case(name, False)
        u = R.depthwise_ref(R.load_ref(c["x"], c["relu_in"]), c["dwk"])[0]
        v = R.pointwise_ref(u, c["pw"], c["scale"], c["shift"], 0)[0]
        assert all(ch.ok for ch in R.check_stats(c, u, *R.out_stats_ref(v)))
        part = v.reshape(v.shape[0], v.shape[1], -1)[:, :, :-1] if v.shape[2] * v.shape[3] > 1 else None
        if part is not None:
            N = v.shape[0] * v.shape[2] * v.shape[3]
            m = part.sum(axis=(0, 2)) / N
            assert not all(ch.ok for ch in R.check_stats(c, u, m, (part**2).sum(axis=(0, 2)) / N - m * m))
        assert not all(ch.ok for ch in R.check_stats(c, u, *R.out_stats_ref(R.r16(v) * (1 + 2.0**-9))))
