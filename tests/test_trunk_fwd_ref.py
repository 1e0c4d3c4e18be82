"""tests/trunk_fwd_ref.py on the CPU: the float64 composition against oracle.model_ref's own layers in torch float64, the layout helpers
against each other, and the two conditions the GPU tests of tests/test_predict_trunk_gpu.py lean on: every exact-kind case stays in the range
where f32 is exact, and no standard-normal bound is loose enough to hide a failure."""

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import trunk_fwd_ref as T  # noqa: E402
from half_fwd_ref import from_quad_planes, pool_res_add_ref, to_quad_planes  # noqa: E402
from oracle import model_ref as M  # noqa: E402

F64 = torch.float64


def _bn_params(rng, name, C):
    """BatchNorm with gamma of both signs, and its fold into (scale, shift) in float64."""
    p = {f"{name}/gamma": rng.standard_normal(C), f"{name}/beta": rng.standard_normal(C), f"{name}/mean": rng.standard_normal(C), f"{name}/var": 0.5 + rng.random(C)}
    sc = p[f"{name}/gamma"] / np.sqrt(p[f"{name}/var"] + M.BN_EPS)
    return p, sc, p[f"{name}/beta"] - p[f"{name}/mean"] * sc


def test_composition_equals_the_oracle_layers_at_an_odd_shape():
    """One residual block, H = 9, W = 21, filters (30,): entry conv, sep_a, sep_b, the column-pair maximum, pooling + residual -- each stage against
    _conv_same / _bn_infer / _sepconv / _maxpool_same in float64.  A transposed tap or a wrong "same" pad shows here, without a GPU."""
    rng = np.random.default_rng(9021)
    B, H, W, C = 2, 9, 21, 30
    x = rng.standard_normal((B, H, W))
    p = {"conv0/kernel": rng.standard_normal((3, 3, 1, 16)) / 3, "conv0/bias": rng.standard_normal(16)}
    fold = {}
    for name, cin, cout in (("b1/sep_a", 16, C), ("b1/sep_b", C, C)):
        p[f"{name}/depthwise"], p[f"{name}/pointwise"], p[f"{name}/bias"] = rng.standard_normal((3, 3, cin, 1)) / 3, rng.standard_normal((1, 1, cin, cout)) / 4, rng.standard_normal(cout)
    for bn, conv, c in (("bn0", "conv0", 16), ("b1/bn_a", "b1/sep_a", C), ("b1/bn_b", "b1/sep_b", C)):
        q, sc, sh = _bn_params(rng, bn, c)
        p.update(q)
        fold[conv] = (sc, sh + p[f"{conv}/bias"] * sc)  # shift = beta - mean * scale + conv_bias * scale
        assert (sc < 0).any() and (sc > 0).any()
    p["b1/res/kernel"], p["b1/res/bias"] = rng.standard_normal((1, 1, 16, C)) / 4, rng.standard_normal(C)

    with torch.no_grad():
        t = torch.relu(M._bn_infer(M._conv_same(torch.from_numpy(x)[:, None], p["conv0/kernel"], p["conv0/bias"], 1, F64), p, "bn0", F64))
        a, S0 = T.entry_ref(x, p["conv0/kernel"].reshape(9, 16), *fold["conv0"])
        assert a.shape == (B, 16, H, W) and np.abs(a - t.numpy()).max() <= 1e-12 and (S0 >= np.abs(a) - 1e-12).all()
        ta = torch.relu(M._bn_infer(M._sepconv(torch.relu(t), p, "b1/sep_a", F64), p, "b1/bn_a", F64))
        va, Sa = T.sep_ref(a, p["b1/sep_a/depthwise"][..., 0], p["b1/sep_a/pointwise"][0, 0], *fold["b1/sep_a"], 1, 1, xS=S0)
        assert np.abs(va - ta.numpy()).max() <= 1e-12 and (Sa >= np.abs(va) - 1e-12).all()
        tb = M._bn_infer(M._sepconv(ta, p, "b1/sep_b", F64), p, "b1/bn_b", F64)
        vb, Sb = T.sep_ref(va, p["b1/sep_b/depthwise"][..., 0], p["b1/sep_b/pointwise"][0, 0], *fold["b1/sep_b"], 0, 0)
        assert np.abs(vb - tb.numpy()).max() <= 1e-12 and (Sb >= np.abs(vb) - 1e-12).all()
        assert (vb < 0).any()  # no ReLU on sep_b's output
        # the x-pooled tensor is the (1, 2) half of the pooling
        assert M.same_pad(W, 2, 2) == (11, 0, 1)
        assert np.array_equal(T.pair_max(tb.numpy()), torch.nn.functional.max_pool2d(torch.nn.functional.pad(tb, (0, 1), value=float("-inf")), (1, 2), (1, 2)).numpy())
        tout = M._maxpool_same(tb) + M._conv_same(t, p["b1/res/kernel"], p["b1/res/bias"], 2, F64)
        want, St = pool_res_add_ref(vb, a, p["b1/res/kernel"][0, 0], p["b1/res/bias"])
        assert want.shape == (B, C, 5, 11) and np.abs(want - tout.numpy()).max() <= 1e-12
        # ... and so is tail_ref's composition of the last two stages
        c = dict(x=va, dwk=p["b1/sep_b/depthwise"][..., 0], pw=p["b1/sep_b/pointwise"][0, 0], scale=fold["b1/sep_b"][0], shift=fold["b1/sep_b"][1], prev=a,
                 wr=p["b1/res/kernel"][0, 0], br=p["b1/res/bias"])
        w2, S2, b2 = T.tail_ref(c, 0)
        assert np.array_equal(w2, want) and (S2 >= np.abs(w2) - 1e-12).all() and (b2 > 0).all()
    # pooling before the folded scale, or a top pad of 0 at this odd height, gives another answer
    sc_b, sh_b = fold["b1/sep_b"]
    pooled = T.pooled_bound(vb)  # (the 3 x 2 "same" maximum of any tensor)
    assert np.array_equal(pooled, M._maxpool_same(torch.from_numpy(vb)).numpy())
    raw = (vb - sh_b[None, :, None, None]) / sc_b[None, :, None, None]
    assert np.abs(T.pooled_bound(raw) * sc_b[None, :, None, None] + sh_b[None, :, None, None] - pooled).max() > 1e-3
    xp = T.pair_max(vb)
    with_top_pad = np.stack([xp[:, :, max(2 * i - 1, 0) : 2 * i + 2].max(axis=2) for i in range(5)], axis=2)  # rows 2i - 1 .. 2i + 1
    no_top_pad = np.stack([xp[:, :, 2 * i : 2 * i + 3].max(axis=2) for i in range(5)], axis=2)  # rows 2i .. 2i + 2
    assert np.array_equal(with_top_pad, pooled) and np.abs(no_top_pad - pooled).max() > 1e-3


def test_layout_helpers_round_trip():
    rng = np.random.default_rng(5)
    x = rng.standard_normal((2, 9, 5, 7)).astype(np.float32)
    xp = T.pair_max(x)
    assert xp.shape == (2, 9, 5, 4) and np.array_equal(xp[..., :3], np.maximum(x[..., 0:6:2], x[..., 1:6:2])) and np.array_equal(xp[..., 3], x[..., 6])
    buf = T.to_xpooled_quads(xp, fill=777.0)
    assert buf.shape == (2, 3, 5, 4, 4) and buf.dtype == np.float32
    assert np.array_equal(T.from_xpooled_quads(buf)[:, :9], xp) and not T.from_xpooled_quads(buf)[:, 9:].any()
    buf = T.to_xpooled_quads(xp[..., :3], fill=777.0)  # Wx = 3: one padding column
    full = T.from_xpooled_quads(buf)
    assert np.array_equal(full[:, :9, :, :3], xp[..., :3]) and (full[:, :9, :, 3] == 777.0).all() and not full[:, 9:].any()
    cp = T.to_compact_quads(x)
    assert cp.shape == (2, 3, 3, 4, 4) and np.array_equal(T.from_compact_quads(cp)[:, :9], x[:, :, ::2, ::2]) and not T.from_compact_quads(cp)[:, 9:].any()
    # the compact subsample is the quad planes' pixels (2i, 2j)
    q = to_quad_planes(x, 3)
    assert np.array_equal(cp, q[:, :, 1:6:2, 0:7:2, :])
    back, pads = from_quad_planes(q, 9, 5, 7, 3)
    assert np.array_equal(back, x) and not pads.any()


def test_sliding_view_snippets_overlap():
    for name, (B, H, W, sliding) in T.ENTRY_CASES.items():
        c = T.entry_case(name, True)
        assert c["x"].shape == (B, H, W) and c["src"].size == (B - 1) * c["stride"] + H * W
        if sliding:
            assert c["stride"] == (H // 2) * W and np.array_equal(c["x"][0, H // 2 :], c["x"][1, : H - H // 2])


def _signs(scale):
    return (scale < 0).any() and (scale > 0).any()


def _every_case():
    """(what, exact-kind (S, grain) list, standard-normal (want, bound) list) for every case of every table, as the GPU tests compute them."""
    for name in T.ENTRY_CASES:
        def f(exact, name=name):
            c = T.entry_case(name, exact)
            assert _signs(c["scale0"])
            a, S0 = T.entry_ref(c["x"], c["w0"], c["scale0"], c["shift0"])
            return [(a, S0, 9, 0.5)]
        yield name, f
    for name in T.SEP_CASES:
        def f(exact, name=name):
            c = T.sep_case(name, exact)
            assert _signs(c["scale"])
            Cin = c["pw"].shape[0]
            return [(*T.sep_ref(c["x"], c["dwk"], c["pw"], c["scale"], c["shift"], ri, ro), 9 + Cin, 0.5) for ri in (0, 1) for ro in (0, 1)]
        yield name, f
    for name in T.FUSED_ENTRY_CASES:
        def f(exact, name=name):
            c = T.fused_entry_case(name, exact)
            assert _signs(c["scale"]) and _signs(c["scale0"])
            out = []
            for ro in (0, 1):
                a, S0, v, S = T.fused_entry_ref(c, ro)
                out += [(a, S0, 9, 0.5), (v, S, 9 + 9 + 16, 0.25)]
            return out
        yield name, f
    for name in T.POOL_CASES:
        def f(exact, name=name):
            c = T.pool_case(name, exact)
            Cp = c["wr"].shape[0]
            return [(*pool_res_add_ref(c["s"], c["prev"], c["wr"], c["br"]), Cp + 2, 1.0)]
        yield name, f
    for name in T.TAIL_CASES:
        def f(exact, name=name):
            c = T.tail_case(name, exact)
            assert _signs(c["scale"])
            out = []
            for ri in (0, 1):
                want, S, bound = T.tail_ref(c, ri)
                out.append((want, S, bound, 0.5))
            return out
        yield name, f


CASES = dict(_every_case())


@pytest.mark.parametrize("name", list(CASES))
def test_exact_cases_stay_below_2_to_the_24(name):
    """Small integers, scales +-2^k, integer shifts: every value is a multiple of the grain (0.5 after one folded scale, 0.25 after two) and the sum of
    the absolute values of all terms, in units of the grain, is below 2^24 -- so every partial sum in any order is exact in f32 and np.array_equal
    against float64 is a legitimate demand."""
    for want, S, _, grain in CASES[name](True):
        assert np.array_equal(want / grain, np.rint(want / grain))
        assert (S >= np.abs(want)).all() and S.max() / grain < 2.0**24, (name, S.max())
        assert np.array_equal(want.astype(np.float32).astype(np.float64), want)


@pytest.mark.parametrize("name", list(CASES))
def test_normal_bounds_are_not_loose(name):
    """No element's derived bound exceeds 1e-3 * max(1, max|want|): ten times the project's bar for f32 plane outputs.  A bound that loose would
    hide a failure."""
    for want, S, n, _ in CASES[name](False):
        bound = n if isinstance(n, np.ndarray) else T.chain_bound(S, n)
        assert np.isfinite(want).all() and (bound > 0).all()
        assert bound.max() <= 1e-3 * max(1.0, np.abs(want).max()), (name, bound.max(), np.abs(want).max())
