"""CPU side of the shared trunk stage of overlapping predict snippets (orcai_amd/overlap.py): the edge cones against the float64
oracle, and the launch plan -- super-snippets, crops and the row map of orcai_pool_res_add_scatter restated in numpy -- rebuilding
every snippet's stage output.

These tests check geometry, not arithmetic: torch-CPU picks its convolution algorithm by image size, so even in float64 a snippet and a
taller image can differ in the last bits on some hosts.  A row "differs" when it is off by more than 1e-9 (a row inside a cone is off
by O(0.1)); the GPU kernels' bit-for-bit equality is tests/test_overlap_share_gpu.py's job."""

import numpy as np
import pytest
import torch

from oracle import model_ref as M
from orcai_amd.overlap import edge_cones, plan_windows, shared_stage


def _stage(p, x, blocks):
    """oracle.model_ref.forward_ref up to residual block `blocks`, float64: {tensor name: (B, C, H, W)}."""
    f64 = torch.float64
    out = {}
    with torch.no_grad():
        x = torch.as_tensor(x, dtype=f64)[:, None]
        x = torch.relu(M._bn_infer(M._conv_same(x, p["conv0/kernel"], p["conv0/bias"], 1, f64), p, "bn0", f64))
        out["conv0"] = x
        prev = x
        for b in range(1, blocks + 1):
            x = torch.relu(M._bn_infer(M._sepconv(torch.relu(x), p, f"b{b}/sep_a", f64), p, f"b{b}/bn_a", f64))
            out[f"b{b}/a"] = x
            x = M._bn_infer(M._sepconv(x, p, f"b{b}/sep_b", f64), p, f"b{b}/bn_b", f64)
            out[f"b{b}/b"] = x
            x = M._maxpool_same(x) + M._conv_same(prev, p[f"b{b}/res/kernel"], p[f"b{b}/res/bias"], 2, f64)
            out[f"b{b}"] = x
            prev = x
    return {k: v.numpy() for k, v in out.items()}


TOL = 1e-9


def _differing_rows(a, b):
    """(top, bottom): rows at the edges of a (C, H, W) tensor up to and including the outermost row that differs from b."""
    rows = np.flatnonzero(np.any(np.abs(a - b) > TOL, axis=(0, 2)))
    h = a.shape[1]
    top = [r for r in rows if r < h // 2]
    bot = [r for r in rows if r >= h // 2]
    return (max(top) + 1 if top else 0), (h - min(bot) if bot else 0)


def test_cones_of_orcai_v1_blocks():
    cones = {name: (t, u) for name, t, u in edge_cones(3, 4)}
    assert [cones[n] for n in ("conv0", "b1/a", "b1/b", "b1", "b2/a", "b2/b", "b2")] == [(1, 1), (2, 2), (3, 3), (2, 2), (3, 3), (4, 4), (2, 3)]
    assert cones["b3"] == cones["b4"] == (2, 3)
    geo = shared_stage(736, 171, 3, 2, 368 * 171)
    assert (geo.rows, geo.period, geo.patch_top, geo.patch_bottom, geo.crop, geo.halo) == (184, 92, 2, 3, 20, 12)


@pytest.mark.parametrize("k", [3, 5, 7])
def test_cones_bound_the_oracle_differences(k):
    """A snippet against the same rows inside a taller image, float64: every row that differs lies in the cone,
    and for k = 3 the cones of blocks 1-2 are reached."""
    H, W, blocks = 128, 11, 2
    p = M.random_params(seed=k, input_shape=(H, W, 1), filters=(6, 8), kernel_size=k, lstm_units=32)
    rng = np.random.default_rng(k)
    tall = rng.standard_normal((1, 3 * H, W))
    snip = tall[:, H : 2 * H]
    a, b = _stage(p, snip, blocks), _stage(p, tall, blocks)
    for name, t, u in edge_cones(k, blocks):
        pools = 0 if name == "conv0" else int(name.split("/")[0][1:]) - ("/" in name)  # block b's sep convs run before its pooling
        h = H // 2**pools
        got = _differing_rows(a[name][0], b[name][0, :, h : 2 * h])
        assert got[0] <= t and got[1] <= u, (name, got, (t, u))
        if k == 3:
            assert got == (t, u), (name, got)


def test_sharing_refuses_other_layouts():
    assert shared_stage(736, 171, 3, 2, 736 * 171) is None  # materialised snippets (model.predict)
    assert shared_stage(736, 171, 3, 2, 368 * 171 + 1) is None
    assert shared_stage(740, 171, 3, 2, 370 * 171) is None  # H/2 not a multiple of 4: a shared row at two pooling phases
    assert shared_stage(736, 171, 4, 2, 368 * 171) is None
    assert shared_stage(64, 11, 7, 2, 32 * 11) is None  # crops as tall as half a snippet
    assert shared_stage(736, 171, 3, 0, 368 * 171) is None
    for k in (5, 7):
        geo = shared_stage(736, 171, k, 2, 368 * 171)
        t, u = edge_cones(k, 2)[-1][1:]
        assert (geo.patch_top, geo.patch_bottom, geo.crop, geo.halo) == (t, u, 4 * (t + u), 4 * max(t, u))


def _scatter(dst, written, img, w, b, geo, nsnip):
    """The store rule of pool_res_add_x_kernel<..., SCATTER = true> for image b of window group w; img (C, rows, W)."""
    for r in range(img.shape[1]):
        rr = w.base + b * w.img_step + r
        if not ((r >= w.r_lo or rr == r) and r < w.r_hi):
            continue
        k = rr // geo.period
        for sn in (k, k - 1):
            y = rr - sn * geo.period
            if 0 <= sn < nsnip and w.keep_lo <= y < w.keep_hi:
                dst[sn, :, y] = img[:, r]
                written[sn, y] += 1


@pytest.mark.parametrize("k,n,m", [(3, 1, 2), (3, 2, 2), (3, 7, 2), (3, 9, 3), (5, 6, 2), (7, 5, 2)])
def test_plan_rebuilds_every_snippet(k, n, m):
    H, W, blocks = 128, 11, 2
    geo = shared_stage(H, W, k, blocks, (H // 2) * W)
    assert geo is not None
    p = M.random_params(seed=10 + k, input_shape=(H, W, 1), filters=(6, 8), kernel_size=k, lstm_units=32)
    P = H // 2
    rec = np.random.default_rng(n).standard_normal(((n + 1) * P, W))
    want = _stage(p, np.stack([rec[i * P : i * P + H] for i in range(n)]), blocks)[f"b{blocks}"]
    got = np.full_like(want, np.nan)
    written = np.zeros((n, geo.rows), dtype=int)
    supers, crops = plan_windows(geo, H, n, m)
    for w in supers + crops:
        assert 0 <= w.start and w.start + (w.count - 1) * w.step + w.height <= rec.shape[0]  # nothing outside the snippets is read
        imgs = np.stack([rec[w.start + b * w.step : w.start + b * w.step + w.height] for b in range(w.count)])
        out = _stage(p, imgs, blocks)[f"b{blocks}"]
        for b in range(w.count):
            _scatter(got, written, out[b], w, b, geo, n)
    assert np.all(written == 1)  # disjoint writers, no row left out
    assert np.max(np.abs(got - want)) <= TOL
