"""CPU side of the two-level shared trunk of overlapping predict snippets (orcai_amd/overlap.py: tail_stage, plan_two_level): the
level-2 cones against the float64 oracle, the store rule of orcai_pool_res_add_scatter_families restated in numpy, and the launch plan
of both levels rebuilding every snippet's block-4 output.

As in tests/test_overlap_geometry.py these check geometry, not arithmetic: a row "differs" when it is off by more than 1e-9; the GPU
kernels' bit-for-bit equality is tests/test_two_level_share_gpu.py's job."""

import numpy as np
import pytest
import torch

from oracle import model_ref as M
from row_map_rules import _families_store, _scatter_store

from orcai_amd.overlap import edge_cones, plan_two_level, plan_windows, shared_stage, tail_stage

TOL = 1e-9


def _blocks(p, x, first, last):
    """oracle.model_ref.forward_ref's residual blocks first .. last on x (B, C, H, W), float64: {tensor name: array}."""
    f64 = torch.float64
    out = {}
    with torch.no_grad():
        x = torch.as_tensor(x, dtype=f64)
        prev = x
        for b in range(first, last + 1):
            x = torch.relu(M._bn_infer(M._sepconv(torch.relu(x), p, f"b{b}/sep_a", f64), p, f"b{b}/bn_a", f64))
            out[f"b{b}/a"] = x
            x = M._bn_infer(M._sepconv(x, p, f"b{b}/sep_b", f64), p, f"b{b}/bn_b", f64)
            out[f"b{b}/b"] = x
            x = M._maxpool_same(x) + M._conv_same(prev, p[f"b{b}/res/kernel"], p[f"b{b}/res/bias"], 2, f64)
            out[f"b{b}"] = x
            prev = x
    return {k: v.numpy() for k, v in out.items()}


def _trunk(p, x, last):
    """Entry conv and blocks 1 .. last on spectrogram images x (B, H, W), float64: {tensor name: array}."""
    f64 = torch.float64
    with torch.no_grad():
        y = torch.as_tensor(x, dtype=f64)[:, None]
        y = torch.relu(M._bn_infer(M._conv_same(y, p["conv0/kernel"], p["conv0/bias"], 1, f64), p, "bn0", f64))
    return _blocks(p, y.numpy(), 1, last)


def _differing_rows(a, b):
    rows = np.flatnonzero(np.any(np.abs(a - b) > TOL, axis=(0, 2)))
    h = a.shape[1]
    top = [r for r in rows if r < h // 2]
    bot = [r for r in rows if r >= h // 2]
    return (max(top) + 1 if top else 0), (h - min(bot) if bot else 0)


def test_level_2_geometry_of_orcai_v1():
    assert edge_cones(3, 4, first=3) == [("b3/a", 1, 1), ("b3/b", 2, 2), ("b3", 1, 2), ("b4/a", 2, 3), ("b4/b", 3, 4), ("b4", 2, 3)]
    assert edge_cones(3, 4, first=None) == edge_cones(3, 4)
    geo2 = tail_stage(736, 171, 3, 3, 4, 368 * 171)
    assert (geo2.blocks, geo2.rows, geo2.period, geo2.patch_top, geo2.patch_bottom, geo2.crop, geo2.halo) == (2, 46, 23, 2, 3, 20, 12)
    # k = 5: the level-1 patches (4 / 5 rows of block 2) spread to 4 / 5 rows of block 4, more than the 3 / 4 of the level-2 image edges
    assert edge_cones(5, 4, first=3)[-1] == ("b4", 3, 4)
    geo5 = tail_stage(736, 171, 5, 3, 4, 368 * 171)
    assert (geo5.patch_top, geo5.patch_bottom, geo5.crop, geo5.halo) == (4, 5, 36, 20)


def test_level_2_refuses_other_layouts():
    assert tail_stage(744, 171, 3, 3, 4, 372 * 171) is None  # H/2 a multiple of 4 (level 1 applies) but not of 16
    assert shared_stage(744, 171, 3, 2, 372 * 171) is not None
    assert tail_stage(736, 171, 3, 3, 4, 736 * 171) is None  # materialised snippets
    assert tail_stage(736, 171, 3, 2, 4, 368 * 171) is not None and tail_stage(736, 171, 3, 1, 4, 368 * 171) is None
    assert tail_stage(128, 11, 3, 3, 4, 64 * 11) is None  # 8 block-4 rows per snippet: the cones meet


@pytest.mark.parametrize("k", [3, 5, 7])
def test_level_2_cones_bound_the_oracle_differences(k):
    """Blocks 3-4 of a snippet whose block-2 output is exact (the same rows as a taller image's) against the taller image, float64:
    every row that differs lies in the cone of edge_cones(k, 4, first=3), and for k = 3 the cones are reached."""
    H2, W2, C2 = 64, 9, 8
    p = M.random_params(seed=20 + k, input_shape=(4 * H2, 4 * W2, 1), filters=(6, C2, 8, 10), kernel_size=k, lstm_units=32)
    tall = np.random.default_rng(k).standard_normal((1, C2, 3 * H2, W2))
    a, b = _blocks(p, tall[:, :, H2 : 2 * H2], 3, 4), _blocks(p, tall, 3, 4)
    for name, t, u in edge_cones(k, 4, first=3):
        pools = int(name.split("/")[0][1:]) - 3 + ("/" not in name)
        h = H2 // 2**pools
        got = _differing_rows(a[name][0], b[name][0, :, h : 2 * h])
        assert got[0] <= t and got[1] <= u, (name, got, (t, u))
        if k == 3:
            assert got == (t, u), (name, got)


def _run_plan(geo, geo2, H, n, m, level1_rows, level2_rows):
    """Both levels of plan_two_level with level1_rows(window, b) -> the level-1 output rows of image b and level2_rows(planes, images)
    -> the block-4 output rows of level-2 images; returns (block-4 rows of every snippet, write counts of the level-2 images and the
    block-4 planes)."""
    plan = plan_two_level(geo, geo2, H, n, m)
    P, P2 = H // 2, geo.period
    dst = {"super": [[None] * plan.super_height for _ in range(plan.super_images)], "crop": [[None] * plan.crop_height for _ in range(2 * n)]}
    written = {"super": np.zeros((plan.super_images, plan.super_height), int), "crop": np.zeros((2 * n, plan.crop_height), int)}
    for w, fams in plan.level1:
        assert 0 <= w.start and w.start + (w.count - 1) * w.step + w.height <= (n + 1) * P  # nothing outside the snippets is read
        assert 1 <= len(fams) <= 4
        for b in range(w.count):
            _families_store(dst, written, level1_rows(w, b), w, b, w.base + b * w.img_step, fams)
    for key in dst:
        assert np.all(written[key] == 1), key  # every level-2 image row written exactly once
    out = [[None] * geo2.rows for _ in range(n)]
    wout = np.zeros((n, geo2.rows), int)
    for windows, key in ((plan.supers, "super"), (plan.crops, "crop")):
        for w, j in windows:
            assert 0 <= w.start and w.start + (w.count - 1) * w.step + w.height <= (n + 1) * P2
            rows = level2_rows(key, dst[key][j : j + w.count], w)
            for b in range(w.count):
                _scatter_store(out, wout, rows[b], w, w.base + b * w.img_step, geo2.rows, geo2.period, n)
    return out, written, wout


@pytest.mark.parametrize("n", [1, 2, 3, 17, 130, 305])
@pytest.mark.parametrize("m", [8, 3, 1])
def test_plan_writes_every_row_exactly_once(n, m):
    """Index-level: each level-2 image row receives the right recording row (or the right snippet's patch row) exactly once, and each
    block-4 row of each snippet exactly once from a level-2 image row outside that image's edge cones -- per tail chunk of 128."""
    H, k = 736, 3
    geo = shared_stage(H, 171, k, 2, (H // 2) * 171)
    geo2 = tail_stage(H, 171, k, 3, 4, (H // 2) * 171)
    P2 = geo.period
    for t0 in range(0, n, 128):
        nt = min(128, n - t0)
        supers1, crops1 = plan_windows(geo, H, nt, m)

        def level1_rows(w, b):
            base = w.base + b * w.img_step
            if w in crops1:  # a crop: its rows are its snippet's own (only its patch rows are exact, only those are kept)
                sn = b
                return [("snip", sn, base + r - sn * P2) for r in range(w.height // geo.scale)]
            return [("rec", base + r) for r in range(w.height // geo.scale)]

        def level2_rows(key, images, w):
            res = []
            for b, img in enumerate(images):
                start = w.start + b * w.step
                for r, v in enumerate(img):
                    R = start + r
                    if key == "super":  # a super-image holds the recording's rows
                        assert v == ("rec", R), (v, R)
                    else:  # a crop holds its snippet's rows: the level-1 patches from the crops, the rest from the super-snippets
                        y = R - b * P2
                        patch = y < geo.patch_top or y >= geo.rows - geo.patch_bottom
                        assert v == (("snip", b, y) if patch else ("rec", R)), (v, b, y)
                hb, ho = len(img) // geo2.scale, geo2.halo // geo2.scale
                if key == "super":  # rows outside the image's own edge cones, except at the recording's edges
                    lo, hi = (0 if start == 0 else ho), (hb if start + len(img) == (nt + 1) * P2 else hb - ho)
                elif w.start == 0:  # top crop: its snippet's top patch
                    lo, hi = 0, geo2.patch_top
                else:
                    lo, hi = hb - geo2.patch_bottom, hb
                res.append([("b4", start // geo2.scale + r) if lo <= r < hi else ("edge", r) for r in range(hb)])
            return res

        out, written, wout = _run_plan(geo, geo2, H, nt, m, level1_rows, level2_rows)
        assert np.all(wout == 1)
        for sn in range(nt):
            for y in range(geo2.rows):
                assert out[sn][y] == ("b4", sn * geo2.period + y), (sn, y, out[sn][y])


@pytest.mark.parametrize("k,H,n,m", [(3, 256, 1, 2), (3, 256, 2, 2), (3, 256, 5, 2), (3, 256, 9, 3), (5, 512, 4, 2), (7, 512, 3, 2)])
def test_plan_rebuilds_every_snippet(k, H, n, m):
    """Float64 end to end: both levels of the plan, with the oracle standing in for the kernels, against blocks 1-4 of each snippet."""
    W = 11
    geo = shared_stage(H, W, k, 2, (H // 2) * W)
    geo2 = tail_stage(H, W, k, 3, 4, (H // 2) * W)
    assert geo is not None and geo2 is not None
    p = M.random_params(seed=30 + k, input_shape=(H, W, 1), filters=(6, 8, 8, 10), kernel_size=k, lstm_units=32)
    P = H // 2
    rec = np.random.default_rng(n).standard_normal(((n + 1) * P, W))
    want = _trunk(p, np.stack([rec[i * P : i * P + H] for i in range(n)]), 4)["b4"]

    def level1_rows(w, b):
        img = rec[w.start + b * w.step : w.start + b * w.step + w.height]
        return list(np.moveaxis(_trunk(p, img[None], 2)["b2"][0], 1, 0))  # [rows][C][W]

    def level2_rows(key, images, w):
        x = np.stack([np.moveaxis(np.stack(img), 0, 1) for img in images])  # [B][C][rows][W]
        return [list(np.moveaxis(o, 1, 0)) for o in _blocks(p, x, 3, 4)["b4"]]

    out, _, wout = _run_plan(geo, geo2, H, n, m, level1_rows, level2_rows)
    assert np.all(wout == 1)
    got = np.stack([np.moveaxis(np.stack(rows), 0, 1) for rows in out])
    assert got.shape == want.shape
    assert np.max(np.abs(got - want)) <= TOL
