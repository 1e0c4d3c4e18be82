"""orcai_segment_column_select / orcai_subtract_segment_floor on the GPU: one exact order statistic per (segment of rows, column) of an f32 [R, C] array,
and the in-place subtraction of the floor interpolated between the segment centres.

Everything is exact, so there is no tolerance: a value equals np.sort(segment, axis=0)[rank] by value and orcai_column_select on the segment's row range
bit for bit (both order by the same key, so -0.0 and +0.0 agree too), on BOTH routes -- the one-launch kernel (orcai_segment_column_select_fused) and the
entry that follows the route rule (a loop of orcai_column_select calls for few, long segments); a percentile equals np.percentile(..., axis=0,
method="nearest") per segment; the subtraction equals denoise.segment_denoise_ref bit for bit.  Inputs hold no NaN.

The geometry the shapes are chosen for (csrc/column_select.hip): a workgroup owns one segment and 32 adjacent columns, a tile is 8 rows, 8 tiles in
flight per trip of the loop (64 rows); S = max(1, R // W) segments, the last one of W .. 2 W - 1 rows."""

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

SHAPES = [  # (rows, cols, seg_rows)
    (1, 1, 1),
    (7, 2, 2),           # S = 3, last segment 3 rows
    (5, 33, 1),          # one-row segments, a full column group and a one-column group
    (64, 31, 64),        # exactly one trip of the tile loop, a partial group
    (127, 32, 64),       # one segment of 2 W - 1 rows
    (128, 33, 64),       # two segments of one trip each
    (1300, 171, 601),    # S = 2 (601 and 699 rows): ten trips and a partial one; segment 1 starts at element 601 * 171, on no 16-byte boundary
    (40, 4096, 8),       # 128 column groups x 5 segments
    (3000, 1, 100),      # one column: 31 lanes of every row idle
    (2100, 33, 4),       # 525 segments x 2 groups, the last of 4 rows
    (70001, 7, 35000),   # two long segments: the rule's loop side, 547 trips per workgroup on the fused route
]
KINDS = ["constant", "ties", "near_zero", "inf", "subnormal", "normal_db", "random_bits", "mixed"]
QS = (0.0, 1.0, 0.5, 0.9)  # ranks 0, last, the median and one other, inside every segment


@pytest.fixture(scope="module")
def fe():
    from orcai_amd.frontend import get_frontend

    return get_frontend()


def bits_to_f32(bits):
    return np.ascontiguousarray(bits, dtype=np.uint32).view(np.float32)


def make(kind, n, seed=5):
    """f32[n] of one kind: tests/test_column_select_gpu.py's generator (the kinds used here), and random bit patterns without NaN."""
    rng = np.random.default_rng(seed)
    if kind == "normal_db":
        return (-40 + 12 * rng.standard_normal(n)).astype(np.float32)
    if kind == "ties":
        return np.round(-50 + 25 * rng.standard_normal(n)).clip(-80, 0).astype(np.float32)
    if kind == "constant":
        return np.full(n, -100.0, dtype=np.float32)
    if kind == "near_zero":
        x = (1e-3 * rng.standard_normal(n)).astype(np.float32)
        x[rng.random(n) < 0.3] = 0.0
        x[rng.random(n) < 0.3] = -0.0
        return x
    if kind == "subnormal":  # every value subnormal, both signs
        return bits_to_f32(rng.integers(1, 2**23, n, dtype=np.uint32) | (rng.integers(0, 2, n, dtype=np.uint32) << 31))
    if kind == "inf":
        x = rng.standard_normal(n).astype(np.float32)
        x[rng.random(n) < 0.1] = np.inf
        x[rng.random(n) < 0.1] = -np.inf
        return x
    if kind == "random_bits":
        b = rng.integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32)
        nan = ((b & np.uint32(0x7F800000)) == np.uint32(0x7F800000)) & ((b & np.uint32(0x007FFFFF)) != 0)
        b[nan] &= np.uint32(0xBFFFFFFF)  # clear one exponent bit: an ordinary value
        return bits_to_f32(b)
    raise KeyError(kind)


def make_array(kind, R, C):
    """f32[R, C] of one kind, or "mixed": column c of kind c mod 7, so that the columns of one workgroup follow different prefixes."""
    if kind == "mixed":
        return np.ascontiguousarray(np.stack([make(KINDS[c % 7], R, seed=100 + c) for c in range(C)], axis=1))
    return np.ascontiguousarray(make(kind, R * C, seed=R + C).reshape(R, C))


def as_bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def segments(R, W):
    S = max(1, R // W)
    return [(s * W, (s + 1) * W if s < S - 1 else R) for s in range(S)]


def ranks_for(R, W):
    from orcai_amd.frontend import nearest_rank_index

    n_last = R - (max(1, R // W) - 1) * W
    return sorted({(min(nearest_rank_index(W, q), W - 1), nearest_rank_index(n_last, q)) for q in QS})


GUARD = -12345.0


def segment_select(fe, d, W, rank, rank_last, fused, scratch=None):
    """Through the C ABI.  out has one guard element in front of and one behind the S x C results; returns the whole tensor."""
    from orcai_amd import _native as N

    R, C = d.shape
    S = max(1, R // W)
    out = torch.full((S * C + 2,), GUARD, dtype=torch.float32, device="cuda")
    if fused:
        rc = fe.lib.orcai_segment_column_select_fused(N.ptr(d), R, C, W, rank, rank_last, out.data_ptr() + 4, N.stream_ptr())
    else:
        if scratch is None:
            scratch = torch.full((fe.lib.orcai_segment_column_select_scratch_bytes(R, C, W),), 0xFF, dtype=torch.uint8, device="cuda")
        rc = fe.lib.orcai_segment_column_select(N.ptr(d), R, C, W, rank, rank_last, out.data_ptr() + 4, N.ptr(scratch), N.stream_ptr())
    assert rc == 0
    return out


# ------------------------------------------------------------------------------------------------ 1. values and bits, both routes
def test_both_routes_occur_among_the_shapes(fe):
    routes = {shape: fe.lib.orcai_segment_column_select_route(*shape) for shape in SHAPES}
    assert routes[(40, 4096, 8)] == 1 and routes[(2100, 33, 4)] == 1 and routes[(1300, 171, 601)] == 1 and routes[(70001, 7, 35000)] == 0
    assert set(routes.values()) == {0, 1}


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_segment_select_exact(fe, shape, kind):
    from orcai_amd import _native as N

    R, C, W = shape
    x = make_array(kind, R, C)
    segs = segments(R, W)
    S = len(segs)
    sorted_segs = [np.sort(x[lo:hi], axis=0) for lo, hi in segs]
    buf = torch.full((R * C + 2,), 99.0, dtype=torch.float32, device="cuda")  # a guard element on either side of x
    buf[1:-1].copy_(torch.from_numpy(x).reshape(-1))
    d = buf[1:-1].view(R, C)
    before = buf.cpu()
    col_scratch = torch.zeros(fe.lib.orcai_column_select_scratch_bytes(C), dtype=torch.uint8, device="cuda")
    for rank, rank_last in ranks_for(R, W):
        want = np.stack([sorted_segs[s][rank_last if s == S - 1 else rank] for s in range(S)])
        single = torch.empty((S, C), dtype=torch.float32, device="cuda")
        for s, (lo, hi) in enumerate(segs):  # orcai_column_select on every row range alone
            assert fe.lib.orcai_column_select(d.data_ptr() + lo * C * 4, hi - lo, C, rank_last if s == S - 1 else rank, single[s].data_ptr(), N.ptr(col_scratch),
                                              N.stream_ptr()) == 0
        single = single.cpu().numpy()
        for fused in (True, False):
            got = segment_select(fe, d, W, rank, rank_last, fused).cpu().numpy()
            assert got[0] == np.float32(GUARD) and got[-1] == np.float32(GUARD), fused
            got = got[1:-1].reshape(S, C)
            assert np.array_equal(got, want), (fused, rank, rank_last, np.argwhere(got != want)[:8].tolist())
            assert np.array_equal(as_bits(got), as_bits(single)), (fused, rank, rank_last)
    assert torch.equal(buf.cpu().view(torch.int32), before.view(torch.int32))  # x and its guards are read only


# ------------------------------------------------------------------------------------------------ 2. state and repeatability
@pytest.mark.parametrize("shape", [(70001, 7, 35000), (2100, 33, 4)], ids=["loop", "fused"])
def test_scratch_needs_no_clear_and_calls_repeat(fe, shape):
    R, C, W = shape
    d = torch.from_numpy(make_array("mixed", R, C)).cuda()
    other = torch.from_numpy(make_array("random_bits", 3000, C)).cuda()
    nbytes = fe.lib.orcai_segment_column_select_scratch_bytes(R, C, W)
    rank, rank_last = ranks_for(R, W)[1]
    ws_before = fe.workspace.cpu()
    clean = segment_select(fe, d, W, rank, rank_last, False, torch.zeros(nbytes, dtype=torch.uint8, device="cuda")).cpu()
    used = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device="cuda")
    first = segment_select(fe, d, W, rank, rank_last, False, used).cpu()
    assert fe.lib.orcai_segment_column_select_route(3000, C, 1500) == 0  # another array and rank through the loop route and the same scratch
    segment_select(fe, other, 1500, 3, 2, False, used)
    again = segment_select(fe, d, W, rank, rank_last, False, used).cpu()
    fused = segment_select(fe, d, W, rank, rank_last, True).cpu()
    for got in (first, again, fused, segment_select(fe, d, W, rank, rank_last, True).cpu()):
        assert torch.equal(got.view(torch.int32), clean.view(torch.int32))
    assert torch.equal(fe.workspace.cpu(), ws_before)  # the front end's workspace is not touched


# ------------------------------------------------------------------------------------------------ 3. refusals
def test_refusals_leave_out_untouched(fe):
    from orcai_amd import _native as N

    lib, s = fe.lib, N.stream_ptr()
    d = torch.zeros((7, 2), device="cuda")
    out = torch.full((7,), 7.0, device="cuda")
    scratch = torch.zeros(lib.orcai_segment_column_select_scratch_bytes(7, 2, 2), dtype=torch.uint8, device="cuda")
    x, o, sc = d.data_ptr(), out.data_ptr(), scratch.data_ptr()
    bad = [(None, 7, 2, 2, 0, 0, o, sc), (x, 7, 2, 2, 0, 0, None, sc), (x, 7, 2, 2, 0, 0, o, None), (x + 2, 7, 2, 2, 0, 0, o, sc), (x, 7, 2, 2, 0, 0, o + 1, sc),
           (x, 0, 2, 2, 0, 0, o, sc), (x, 2**32, 2, 2, 0, 0, o, sc), (x, 7, 0, 2, 0, 0, o, sc), (x, 7, 4097, 2, 0, 0, o, sc), (x, 7, 2, 0, 0, 0, o, sc),
           (x, 7, 2, 2, 2, 0, o, sc), (x, 7, 2, 2, -1, 0, o, sc), (x, 7, 2, 2, 0, 3, o, sc), (x, 7, 2, 2, 0, -1, o, sc), (x, 3, 2, 5, 0, 3, o, sc)]
    for i, args in enumerate(bad):
        assert lib.orcai_segment_column_select(*args, s) == N.E_BADARG, i
        if args[7] is not None:
            assert lib.orcai_segment_column_select_fused(*args[:7], s) == N.E_BADARG, i
    m = torch.zeros((3, 2), device="cuda")
    for i, args in enumerate([(None, 7, 2, 2, m.data_ptr()), (x, 7, 2, 2, None), (x, 0, 2, 2, m.data_ptr()), (x, 7, 0, 2, m.data_ptr()), (x, 7, 4097, 2, m.data_ptr()),
                              (x, 7, 2, 0, m.data_ptr()), (x + 2, 7, 2, 2, m.data_ptr())]):
        assert lib.orcai_subtract_segment_floor(*args, s) == N.E_BADARG, i
    torch.cuda.synchronize()
    assert out.tolist() == [7.0] * 7 and float(d.abs().max()) == 0.0
    assert lib.orcai_segment_column_select(x, 7, 2, 2, 1, 2, o, sc, s) == 0  # ranks inside their segments: accepted
    assert out.tolist() == [0.0] * 6 + [7.0]
    assert lib.orcai_segment_column_select(x, 3, 2, 5, 99, 2, o, sc, s) == 0  # one segment: the full segments' rank is not read
    for bad_w in (0, -3, 2.5, True):
        with pytest.raises(ValueError, match="segment_rows"):
            fe.percentiles(d, [0.5], dim=0, segment_rows=bad_w)
    with pytest.raises(ValueError, match="segment_rows"):
        fe.percentiles(d, [0.5], segment_rows=2)


# ------------------------------------------------------------------------------------------------ 4. percentiles and the op
@pytest.mark.parametrize("shape,W", [((1300, 171), 601), ((37, 4, 5), 10), ((2100, 33), 4), ((9, 3), 20)], ids=["1300x171", "37x4x5", "2100x33", "one-segment"])
def test_segment_percentiles_equal_numpy_nearest(fe, shape, W):
    import orcai_amd.torch_ops as O

    q = [0, 0.01, 0.25, 0.5, 0.999, 1]
    x = make_array("mixed", shape[0], int(np.prod(shape[1:]))).reshape(shape)
    want = np.stack([np.percentile(x[lo:hi], [100 * v for v in q], axis=0, method="nearest") for lo, hi in segments(shape[0], W)], axis=1)
    assert want.dtype == np.float32 and want.shape == (len(q), max(1, shape[0] // W), *shape[1:])
    d = torch.from_numpy(x).cuda()
    for got in (fe.percentiles(d, q, dim=0, segment_rows=W), torch.ops.orcai.segment_column_percentile(d, [float(v) for v in q], W),
                O.segment_column_percentile(d, q, W)):
        assert got.dtype == torch.float32 and tuple(got.shape) == want.shape and got.is_cuda
        assert np.array_equal(got.cpu().numpy(), want)
    one = fe.percentiles(d, 0.25, dim=0, segment_rows=W)  # a single fraction: [S, ...]
    assert tuple(one.shape) == want.shape[1:] and np.array_equal(one.cpu().numpy(), want[2])
    xg = d.clone().requires_grad_(True)
    y = torch.ops.orcai.segment_column_percentile(xg, [0.5], W)
    assert y.requires_grad
    with pytest.raises(NotImplementedError, match="order statistic"):
        y.sum().backward()


# ------------------------------------------------------------------------------------------------ 5. the subtraction
SUBTRACT = [
    (7, 2, 2),          # S = 3, W even, the long last segment (3 = 2 W - 1 rows); a 16-byte piece spans two rows
    (9, 2, 3),          # W odd: frames 1, 4 and 7 lie exactly on the centres
    (5, 3, 9),          # S = 1
    (37, 3, 37),        # S = 1, W = T
    (128, 33, 64),      # S = 2
    (1300, 171, 601),   # S = 2, W odd, centres at 300 and 949.5
    (1025, 33, 100),    # S = 10, the last segment 125 rows
    (50, 1, 7),         # one column: a 16-byte piece spans four rows
    (4000, 171, 3),     # 1333 short segments: the interpolation weight changes with every row
]


@pytest.mark.parametrize("offset", [0, 1, 2, 3])
@pytest.mark.parametrize("shape", SUBTRACT, ids=lambda s: "x".join(map(str, s)))
def test_subtract_segment_floor_is_the_specification(fe, shape, offset):
    """offset: floats between a 16-byte boundary and x[0][0] -- the scalar head in front of the 16-byte body, and its tail.  The floors are the
    specification's own (by value), the result its Y bit for bit; with S == 1 also the bytes of orcai_subtract_columns."""
    from orcai_amd import _native as N
    from orcai_amd.denoise import segment_denoise_ref

    R, C, W = shape
    x = make_array("normal_db", R, C)
    want, m = segment_denoise_ref(x, 0.5, W)
    S = max(1, R // W)
    assert m.shape == (S, C) and want.dtype == np.float32
    buf = torch.full((R * C + 8,), 99.0, dtype=torch.float32, device="cuda")
    assert buf.data_ptr() % 16 == 0
    d = buf[offset : offset + R * C]
    d.copy_(torch.from_numpy(x).reshape(-1))
    md = torch.from_numpy(m).cuda()
    assert fe.lib.orcai_subtract_segment_floor(d.data_ptr(), R, C, W, N.ptr(md), N.stream_ptr()) == 0
    got = buf.cpu().numpy()
    assert np.array_equal(as_bits(got[offset : offset + R * C]), as_bits(want.reshape(-1)))
    assert (got[:offset] == 99.0).all() and (got[offset + R * C :] == 99.0).all()
    if S == 1:
        d.copy_(torch.from_numpy(x).reshape(-1))
        assert fe.lib.orcai_subtract_columns(d.data_ptr(), R, C, N.ptr(md), N.stream_ptr()) == 0
        assert np.array_equal(as_bits(buf.cpu().numpy()), as_bits(got))


def test_subtract_beyond_one_grid_stride(fe):
    """2048 workgroups x 256 threads x 4 floats = 2 097 152 elements per trip of the streaming loop: 2 600 000 elements take a second, partial trip, so the
    (row, column) a thread carries forward is used."""
    from orcai_amd import _native as N
    from orcai_amd.denoise import segment_denoise_ref

    R, C, W = 15205, 171, 1875
    x = make_array("normal_db", R, C)
    want, m = segment_denoise_ref(x, 0.25, W)
    d = torch.from_numpy(x).cuda()
    assert fe.lib.orcai_subtract_segment_floor(N.ptr(d), R, C, W, N.ptr(torch.from_numpy(m).cuda()), N.stream_ptr()) == 0
    assert np.array_equal(as_bits(d.cpu().numpy()), as_bits(want))
