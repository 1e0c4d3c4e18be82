"""The f16 shared trunk of overlapping predict snippets (DESIGN 4.1 on the f16 path).

The launchers alone: orcai_h_pool_res_add_scatter[_families] against orcai_h_pool_res_add on the same operands -- every kept row of every
destination image bit-equal to the plain launcher's row, every other element of the destination still the sentinel it was filled with.
End to end: predict_spectrogram of an f16 model against forward_device on materialised snippets (the per-snippet path), torch.equal."""

import ctypes
import json
from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A  # every destination starts as this f16 bit pattern (210.25): a store the row map should not make shows
HW_IN, B_WIN, STEP, R_LO, R_HI = 24, 3, 8, 2, 10  # windows of 24 rows -> 12 output rows, 8 apart, rows [2, 10) kept: every recording row in one window


def _operands(C, Cp, k, W, seed):
    from orcai_amd import _native as N
    from orcai_amd.half import pack_pointwise_fragments

    lib = N.lib()
    R, H = k // 2, HW_IN
    WP, Wo = lib.orcai_padded_width(W, k), (W + 1) // 2
    WPo, WPx = lib.orcai_padded_width(Wo, k), (Wo + 3) & ~3
    g = torch.Generator(device="cuda").manual_seed(seed)
    CO, COp = (C + 7) // 8, (Cp + 7) // 8
    s = torch.randn((B_WIN, CO, H, WPx, 8), generator=g, device="cuda").half()
    prev = torch.zeros((B_WIN, COp, H + 2 * R, WP, 8), dtype=torch.float16, device="cuda")
    vals = torch.randn((B_WIN, COp * 8, H, W), generator=g, device="cuda")
    vals[:, Cp:] = 0  # channels past Cp inside the last octet are kept at zero (half_planes.h)
    prev[:, :, R : R + H, :W, :] = vals.view(B_WIN, COp, 8, H, W).permute(0, 1, 3, 4, 2).half()
    rng = np.random.default_rng(seed)
    wrf = torch.from_numpy(pack_pointwise_fragments((rng.standard_normal((Cp, C)) / np.sqrt(Cp)).astype(np.float32))).cuda()
    br = torch.from_numpy(rng.standard_normal(C).astype(np.float32)).cuda()
    plain = torch.zeros((B_WIN, CO, H // 2 + 2 * R, WPo, 8), dtype=torch.float16, device="cuda")
    N.check(lib.orcai_h_pool_res_add(N.ptr(s), N.ptr(prev), B_WIN, C, Cp, H, W, k, N.ptr(wrf), N.ptr(br), N.ptr(plain), 1, None, None, None, None, 0.0, N.stream_ptr()),
            "orcai_h_pool_res_add")
    return dict(lib=lib, s=s, prev=prev, wrf=wrf, br=br, plain=plain, head=(N.ptr(s), N.ptr(prev), B_WIN, C, Cp, H, W, k, N.ptr(wrf), N.ptr(br)), CO=CO, R=R, Wo=Wo, WPo=WPo)


def _sentinel(op, count, Hd):
    return torch.full((count, op["CO"], Hd + 2 * op["R"], op["WPo"], 8), SENTINEL, dtype=torch.int16, device="cuda")


def _expected(op, base, fams):
    """The row map of include/orcai_hip.h in Python: fams = [(Hd, period, offset, count, keep_lo, keep_hi)].  Returns the expected destinations
    (int16 bit patterns) and how many images hold a row at most."""
    R, Wo, plain = op["R"], op["Wo"], op["plain"].view(torch.int16)
    outs = [_sentinel(op, f[3], f[0]) for f in fams]
    most = [0] * len(fams)
    for b in range(B_WIN):
        for r in range(HW_IN // 2):
            rr = base + b * STEP + r
            if not ((r >= R_LO or rr == r) and r < R_HI):
                continue
            for fi, (Hd, period, offset, count, lo, hi) in enumerate(fams):
                hits = [j for j in range(count) if lo <= rr - offset - j * period < hi]
                most[fi] = max(most[fi], len(hits))
                for j in hits:
                    y = rr - offset - j * period
                    assert int(outs[fi][j, 0, y + R, 0, 0]) == SENTINEL  # the scenario writes every destination row once
                    outs[fi][j, :, y + R, :Wo, :] = plain[b, :, r + R, :Wo, :]
    return outs, most


SHAPES = [(C, Cp, k, W) for C, Cp in ((12, 16), (20, 12), (36, 30), (64, 64)) for k in (3, 5) for W in (21, 171)]


@pytest.mark.parametrize("C,Cp,k,W", SHAPES)
def test_scatter_launcher_stores_the_plain_launchers_bits_through_the_row_map(C, Cp, k, W):
    from orcai_amd import _native as N

    op = _operands(C, Cp, k, W, seed=C + k)
    # snippets of 16 rows every 8; a window at recording row 0 (its rows above r_lo are the first snippet's own top edge) and one that is not; keep_lo > 0
    for base, nsnip, keep in ((0, 3, (0, 16)), (0, 4, (3, 13)), (5, 2, (1, 15))):
        want, most = _expected(op, base, [(16, 8, 0, nsnip, *keep)])
        assert most[0] == 2 or keep != (0, 16)
        out = _sentinel(op, nsnip, 16)
        rc = op["lib"].orcai_h_pool_res_add_scatter(*op["head"], N.ptr(out), 16, nsnip, 8, base, STEP, R_LO, R_HI, *keep, N.stream_ptr())
        assert rc == 0
        assert torch.equal(out, want[0]), (base, nsnip, keep)
        assert int((want[0] != SENTINEL).sum()) > 0


FAMILIES = [(16, 8, 0, 3, 0, 16),  # a row in two of its images
            (10, 10, 3, 3, 2, 9), (20, 12, 1, 2, 0, 20), (6, 4, 7, 4, 1, 5)]


@pytest.mark.parametrize("nfam", [1, 2, 4])
@pytest.mark.parametrize("C,Cp,k,W", SHAPES)
def test_families_launcher_stores_every_family(C, Cp, k, W, nfam):
    from orcai_amd import _native as N

    op = _operands(C, Cp, k, W, seed=C + k + nfam)
    fams = FAMILIES[:nfam]
    for base in (0, 5):
        want, most = _expected(op, base, fams)
        assert most[0] == 2
        outs = [_sentinel(op, f[3], f[0]) for f in fams]
        arr = (N.RowFamily * nfam)(*[N.RowFamily(N.ptr(o), *f) for o, f in zip(outs, fams)])
        rc = op["lib"].orcai_h_pool_res_add_scatter_families(*op["head"], base, STEP, R_LO, R_HI, ctypes.addressof(arr), nfam, N.stream_ptr())
        assert rc == 0
        for fi, (o, w) in enumerate(zip(outs, want)):
            assert torch.equal(o, w), (base, fi)


def test_launchers_refuse_before_launching():
    from orcai_amd import _native as N

    op = _operands(20, 12, 3, 21, seed=1)
    lib, st = op["lib"], N.stream_ptr()
    out = _sentinel(op, 4, 20)
    p = N.ptr(out)

    def fams(*rows, ptr=p):
        return (N.RowFamily * len(rows))(*[N.RowFamily(ptr, *r) for r in rows])

    def families(arr, head=op["head"], n=None):
        return lib.orcai_h_pool_res_add_scatter_families(*head, 0, STEP, R_LO, R_HI, ctypes.addressof(arr), len(arr) if n is None else n, st)

    def single(out_ptr, head=op["head"], Hd=16, period=8, keep=(0, 16)):
        return lib.orcai_h_pool_res_add_scatter(*head, out_ptr, Hd, 3, period, 0, STEP, R_LO, R_HI, *keep, st)

    ok = (16, 8, 0, 3, 0, 16)
    wide = op["head"][:3] + (80, 12) + op["head"][5:]  # 80 output channels: not a shape of the x-pooled kernel
    assert families(fams(ok, ok, ok, ok, ok)) == N.E_UNSUPPORTED  # more than ORCAI_ROW_FAMILIES
    assert families(fams((20, 8, 0, 3, 0, 20))) == N.E_UNSUPPORTED  # a row in three images
    assert single(p, Hd=20, period=8, keep=(0, 20)) == N.E_UNSUPPORTED
    assert families(fams(ok), head=wide) == N.E_UNSUPPORTED and single(p, head=wide) == N.E_UNSUPPORTED
    assert families(fams(ok, ptr=None)) == N.E_BADARG and single(None) == N.E_BADARG  # null out
    assert families(fams(ok, ptr=p + 8)) == N.E_BADARG and single(p + 8) == N.E_BADARG  # not 16-byte aligned
    assert families(fams(ok), n=0) == N.E_BADARG and families(fams((16, 0, 0, 3, 0, 16))) == N.E_BADARG
    assert single(p, head=op["head"][:2] + (0,) + op["head"][3:]) == N.E_BADARG
    torch.cuda.synchronize()
    assert int((out != SENTINEL).sum()) == 0


# ------------------------------------------------------------------------------------------------ end to end
H, W = 736, 171


def _model(cls=None, k=3, filters=(30, 40, 50, 60), hw=(H, W), precision="f16"):
    from orcai_amd.architectures import ResNet1DConv, ResNetLSTM

    if cls == "conv1d":
        m = ResNet1DConv((hw[0], hw[1], 1), 7, list(filters), k, 0.0, seed=1)
    else:
        m = ResNetLSTM((hw[0], hw[1], 1), 7, list(filters), k, lstm_units=128, seed=1)
    m.precision = precision
    return m


def _spectrogram(n, hw=(H, W), extra=101, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.rand(((n + 1) * (hw[0] // 2) + extra, hw[1]), generator=g, device="cuda", dtype=torch.float32)


def _per_snippet(model, spec, n):
    h, w = model.input_hw
    snippets = torch.stack([spec[i * (h // 2) : i * (h // 2) + h] for i in range(n)]).contiguous()
    out = torch.empty((n, model.out_steps, model.num_labels), dtype=torch.float32, device="cuda")
    model.forward_device(snippets.view(-1), h * w, n, out, chunk=128)
    return out


@pytest.fixture(scope="module")
def v1():
    """The f16 orcai-V1 model, one spectrogram of 17 snippets + 101 rows and the per-snippet path's result on it (shared, never modified)."""
    model = _model()
    spec = _spectrogram(17)
    want = _per_snippet(model, spec, 17)
    assert bool(torch.isfinite(want).all()) and float(want.std()) > 0
    return model, spec, want


@pytest.mark.parametrize("n", [1, 2, 3, 17])
def test_shared_trunk_matches_per_snippet_path(v1, n):
    model, spec, want = v1
    h = model.half_engine()
    assert h.shared_geometry(H // 2 * W) is not None and h.tail_geometry(H // 2 * W) is not None
    got = model.predict_spectrogram(spec[: (n + 1) * (H // 2) + 101])
    assert got.shape == (n, model.out_steps, 7)
    assert torch.equal(got, want[:n])  # a snippet's probabilities do not depend on the snippets after it


@pytest.mark.parametrize("kw", [dict(cls="conv1d"), dict(k=5), dict(filters=(12, 20, 30, 36)), dict(hw=(192, 21))],
                         ids=["ResNet1DConv", "k5", "filters_not_multiples_of_8", "smallest_192x21"])
def test_other_models_match_per_snippet_path(kw):
    """(192, 21): the smallest plane at k = 3, W = 21 that overlap.shared_stage and tail_stage both accept for blocks 1-2 | 3-4
    (tests/test_half_share.py derives it)."""
    model = _model(**kw)
    h, w = model.input_hw
    assert model.half_engine().tail_geometry(h // 2 * w) is not None
    spec = _spectrogram(17, hw=(h, w), extra=101 if h // 2 > 101 else 37, seed=5)  # fewer extra rows than a stride: 17 snippets
    got = model.predict_spectrogram(spec)
    assert got.shape[0] == 17 and torch.equal(got, _per_snippet(model, spec, 17))


def test_ragged_windows_and_several_tail_chunks(v1):
    _, spec, want = v1
    model = _model()
    model.tail_chunk, model.shared_strides = 8, 3  # tail chunks of 8, 8 and 1 snippets, each with its own plan; ragged last super-images
    assert torch.equal(model.predict_spectrogram(spec, chunk=5), want)


def test_one_level_where_only_blocks_1_2_share():
    """H/2 = 372: a multiple of 4 but not of 16 -- level 1 shared, blocks 3-4 per snippet."""
    model = _model(hw=(744, W))
    eng = model.half_engine()
    assert eng.shared_geometry(372 * W) is not None and eng.tail_geometry(372 * W) is None
    spec = _spectrogram(5, hw=(744, W), seed=11)
    assert torch.equal(model.predict_spectrogram(spec), _per_snippet(model, spec, 5))


def test_shard_style_range_starting_at_snippet_5(v1):
    model, spec, want = v1
    i0, P = 5, H // 2
    out = torch.empty((17 - i0, model.out_steps, 7), dtype=torch.float32, device="cuda")
    model.forward_device(spec.view(-1)[i0 * P * W :], P * W, 17 - i0, out)
    assert torch.equal(out, want[i0:])


def _record(monkeypatch, model, spec):
    from recording_lib import RecordingLib

    from orcai_amd import _native as N

    rec = RecordingLib(N.lib())
    with monkeypatch.context() as mp:
        mp.setattr(N, "lib", lambda: rec)
        out = model.predict_spectrogram(spec)
        torch.cuda.synchronize()
    return out, rec


UNSHARED = ["orcai_h_conv0_affine"] + ["orcai_h_sepconv", "orcai_h_sepconv", "orcai_h_pool_res_add"] * 4 + ["orcai_h_sepconv"]


def _trunk_names(rec):
    return [n for n, _, _ in rec.calls if n.startswith(("orcai_h_conv0", "orcai_h_sepconv", "orcai_h_pool"))]


def test_shared_path_launches_the_scatter_tails_and_no_plain_tail_for_them(v1, monkeypatch):
    model, spec, want = v1
    out, rec = _record(monkeypatch, model, spec)
    assert torch.equal(out, want)
    # the tails the row map replaces are those of each level's last block (blocks 2 and 4: 40 and 60 channels); blocks 1 and 3 feed the next block
    # of their own tall image through the plain launcher, as on the f32 path.  No plain tail runs on a snippet-shaped plane or for blocks 2 / 4.
    plain = [(a[3], a[5]) for n, _, a in rec.calls if n == "orcai_h_pool_res_add"]  # (C, H)
    assert plain and {c for c, _ in plain} == {30, 50} and not {h for _, h in plain} & {736, 368, 184, 92}
    for name, C in (("orcai_h_pool_res_add_scatter_families", 40), ("orcai_h_pool_res_add_scatter", 60)):
        assert {a[3] for n, _, a in rec.calls if n == name} == {C}
    assert len(rec.rcs("orcai_h_pool_res_add_scatter_families")) >= 3 and len(rec.rcs("orcai_h_pool_res_add_scatter")) >= 4
    assert set(rec.rcs("orcai_h_pool_res_add_scatter_families") + rec.rcs("orcai_h_pool_res_add_scatter")) == {0}
    assert not any(n.startswith("orcai_pool_res_add") or n in ("orcai_sepconv_bn", "orcai_conv0_sepconv") for n, _, _ in rec.calls)  # no f32 trunk launcher


@pytest.mark.parametrize("how", ["share_overlap_off", "H740"])
def test_unshared_layouts_keep_todays_launch_sequence(how, v1, monkeypatch):
    if how == "H740":  # H/2 = 370: no multiple of 4, nothing to share
        model = _model(hw=(740, W))
        spec = _spectrogram(17, hw=(740, W), seed=2)
        want = _per_snippet(model, spec, 17)
    else:
        _, spec, want = v1
        model = _model()
        model.share_overlap = False
    out, rec = _record(monkeypatch, model, spec)
    assert torch.equal(out, want)
    assert _trunk_names(rec) == UNSHARED  # 17 snippets: one trunk chunk


def test_f32_launch_record_is_the_parents(monkeypatch):
    """The f32 model's launcher names for the same recording, against the sequence recorded on the commit before the f16 shared trunk
    (tests/golden/predict_f32_launch_names_n17.json) -- before and after an f16 prediction in the same process."""
    golden = json.loads((Path(__file__).parent / "golden" / "predict_f32_launch_names_n17.json").read_text())
    spec = _spectrogram(17)
    f32 = _model(precision="f32")
    f32.predict_spectrogram(spec)  # weights prepared: the record below is the steady state
    first, rec = _record(monkeypatch, f32, spec)
    assert [n for n, _, _ in rec.calls] == golden["names"]
    _model().predict_spectrogram(spec)
    again, rec = _record(monkeypatch, f32, spec)
    assert [n for n, _, _ in rec.calls] == golden["names"] and torch.equal(first, again)
