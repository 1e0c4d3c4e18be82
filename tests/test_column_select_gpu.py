"""orcai_column_select / orcai_subtract_columns on the GPU: the exact rank-th smallest of every column of an f32 [R, C] array in one call.

Everything here is exact, so there is no tolerance: a column's order statistic equals np.sort(x, axis=0)[rank] by value and the flat radix select
(FrontEnd.select(column, method="radix")) bit for bit -- both order by the same key, so -0.0 and +0.0 agree too; a percentile equals
np.percentile(..., axis=0, method="nearest") on the host copy; the subtraction equals numpy's float32 one.  Inputs hold no NaN.

The launch geometry the shapes are chosen for (csrc/column_select.hip): a workgroup owns 32 adjacent columns and a tile of 8 rows (with C <= 16 the lanes
of a row shrink to the next power of two >= C and the tile grows to 256 / that many rows); at most 1024 / ceil(C / 32) workgroups stride over the row
tiles, four tiles in flight per trip of the loop."""

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

SHAPES = [
    (1, 1),        # one row, one lane per row
    (2, 3),        # 4 lanes per row, one of them idle
    (5, 171),      # fewer rows than a tile; five full column groups and a partial one (11 columns)
    (1025, 31),    # a partial column group ...
    (1025, 32),    # ... a full one ...
    (1025, 33),    # ... and a full one with a one-column group behind it; 129 row tiles, the last partial
    (3001, 171),   # the front end's K: 6 groups x 170 workgroups, 376 tiles -> up to three tiles per workgroup, one trip
    (4099, 64),    # 2 groups x 512 workgroups over 513 tiles: one workgroup takes a second tile
    (257, 2049),   # 65 column groups (the last one column wide), 15 workgroups each over 33 tiles
    (70001, 7),    # few columns: 8 lanes per row, so 8 lanes of a wave fall into each column; 2188 tiles of 32 rows over 1024 workgroups
    (601, 4096),   # added: the largest C; 128 groups x 8 workgroups over 76 tiles -> a workgroup makes THREE trips of its four-tile loop (the only shape that
                   # makes more than one), the last of them partial
]
KINDS = ["normal_db", "ties", "constant", "near_zero", "inf", "subnormal", "last_digit", "middle_digit", "wide", "two_values"]
QS = (0.01, 0.5, 0.999)


@pytest.fixture(scope="module")
def fe():
    from orcai_amd.frontend import get_frontend

    return get_frontend()


def bits_to_f32(bits):
    return np.ascontiguousarray(bits, dtype=np.uint32).view(np.float32)


def make(kind, n, seed=5):
    """f32[n] of one kind: tests/test_radix_select_gpu.py's generator (the kinds used here)."""
    rng = np.random.default_rng(seed)
    if kind == "normal_db":
        return (-40 + 12 * rng.standard_normal(n)).astype(np.float32)
    if kind == "ties":
        return np.round(-50 + 25 * rng.standard_normal(n)).clip(-80, 0).astype(np.float32)
    if kind == "constant":
        return np.full(n, -100.0, dtype=np.float32)
    if kind == "near_zero":
        x = (1e-3 * rng.standard_normal(n)).astype(np.float32)
        x[: min(1000, n // 4)] = 0.0
        x[min(1000, n // 4) : min(2000, n // 2)] = -0.0
        return x
    if kind == "wide":
        return (rng.standard_normal(n) * np.exp(8 * rng.standard_normal(n))).astype(np.float32)
    if kind == "subnormal":  # every value subnormal, both signs
        return bits_to_f32(rng.integers(1, 2**23, n, dtype=np.uint32) | (rng.integers(0, 2, n, dtype=np.uint32) << 31))
    if kind == "inf":
        x = rng.standard_normal(n).astype(np.float32)
        x[rng.random(n) < 0.02] = np.inf
        x[rng.random(n) < 0.02] = -np.inf
        return x
    if kind == "two_values":
        return np.where(rng.random(n) < 0.3, np.float32(-3.5), np.float32(0.0625)).astype(np.float32)
    if kind == "last_digit":  # 1 + k 2^-23, k < 1024
        return bits_to_f32(np.uint32(0x3F800000) | rng.integers(0, 1024, n, dtype=np.uint32))
    if kind == "middle_digit":
        return bits_to_f32(np.uint32(0x3F800000) | (rng.integers(0, 2048, n, dtype=np.uint32) << 10))
    raise KeyError(kind)


def make_array(kind, R, C):
    """f32[R, C] of one kind, or "mixed": column c of kind c mod len(KINDS), so that the columns of one workgroup follow different prefixes and a constant
    column sits beside a random one."""
    if kind == "mixed":
        return np.ascontiguousarray(np.stack([make(KINDS[c % len(KINDS)], R, seed=100 + c) for c in range(C)], axis=1))
    x = make(kind, R * C, seed=R + C).reshape(R, C)
    if kind == "near_zero" and R > 8:  # both zeros in every column, not only in the first flat elements
        x[1::7] = 0.0
        x[3::7] = -0.0
    return np.ascontiguousarray(x)


def ranks_for(R):
    from orcai_amd.frontend import nearest_rank_index

    return sorted({0, R - 1, R // 2, *(nearest_rank_index(R, q) for q in QS)})


def column_select(fe, d, rank, scratch=None, out=None):
    """orcai_column_select through the C ABI.  out has one guard element behind the C results; returns the whole tensor."""
    from orcai_amd import _native as N

    R, C = d.shape
    if scratch is None:
        scratch = torch.zeros(fe.lib.orcai_column_select_scratch_bytes(C), dtype=torch.uint8, device="cuda")
    if out is None:
        out = torch.full((C + 1,), -12345.0, dtype=torch.float32, device="cuda")
    assert fe.lib.orcai_column_select(N.ptr(d), R, C, rank, N.ptr(out), N.ptr(scratch), N.stream_ptr()) == 0
    return out


def as_bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).tolist()


# ------------------------------------------------------------------------------------------------ 1. values and bits
@pytest.mark.parametrize("kind", KINDS + ["mixed"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_column_select_exact(fe, shape, kind):
    R, C = shape
    x = make_array(kind, R, C)
    xs = np.sort(x, axis=0)
    d = torch.from_numpy(x).cuda()
    scratch = torch.zeros(fe.lib.orcai_column_select_scratch_bytes(C), dtype=torch.uint8, device="cuda")
    some_columns = sorted({0, C // 2, C - 1, min(C - 1, 31), min(C - 1, 32)})
    columns = {c: d[:, c].contiguous() for c in some_columns}
    for rank in ranks_for(R):
        got = column_select(fe, d, rank, scratch).cpu().numpy()
        assert got[C] == np.float32(-12345.0)
        assert np.array_equal(got[:C], xs[rank]), (rank, np.flatnonzero(got[:C] != xs[rank])[:8])
        for c in some_columns:  # bit for bit the flat radix select on that column alone
            flat = fe.select(columns[c], rank, rank, method="radix")
            assert as_bits(got[c]) == as_bits(np.float32(flat[0])) == as_bits(np.float32(flat[1])), (rank, c)


# ------------------------------------------------------------------------------------------------ 2. state and repeatability
def test_scratch_needs_no_clear_and_calls_repeat(fe):
    R, C = 3001, 171
    d = torch.from_numpy(make_array("mixed", R, C)).cuda()
    other = torch.from_numpy(make_array("wide", 1025, 171)).cuda()
    nbytes = fe.lib.orcai_column_select_scratch_bytes(C)
    ws_before = fe.workspace.cpu()
    clean = column_select(fe, d, 1500, torch.zeros(nbytes, dtype=torch.uint8, device="cuda")).cpu()
    dirty = column_select(fe, d, 1500, torch.full((nbytes,), 0xFF, dtype=torch.uint8, device="cuda")).cpu()
    assert torch.equal(clean.view(torch.int32), dirty.view(torch.int32))
    used = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device="cuda")
    first = column_select(fe, d, 1500, used).cpu()
    column_select(fe, other, 7, used)  # another array and rank through the same scratch, no reset in between
    again = column_select(fe, d, 1500, used).cpu()
    twice = column_select(fe, d, 1500, used).cpu()
    for got in (first, again, twice):
        assert torch.equal(got.view(torch.int32), clean.view(torch.int32))
    assert clean[C].item() == -12345.0  # the guard element behind out[cols - 1]
    assert np.array_equal(clean[:C].numpy(), np.sort(d.cpu().numpy(), axis=0)[1500])
    assert torch.equal(fe.workspace.cpu(), ws_before)  # hist1, pmax_bits, sel[]: the front end's workspace is not touched


# ------------------------------------------------------------------------------------------------ 3. refusals
def test_refusals_leave_out_untouched(fe):
    from orcai_amd import _native as N

    lib, s = fe.lib, N.stream_ptr()
    d = torch.zeros((10, 3), device="cuda")
    out = torch.full((4,), 7.0, device="cuda")
    scratch = torch.zeros(lib.orcai_column_select_scratch_bytes(3), dtype=torch.uint8, device="cuda")
    x, o, sc = d.data_ptr(), out.data_ptr(), scratch.data_ptr()
    bad = [(None, 10, 3, 0, o, sc), (x, 10, 3, 0, None, sc), (x, 10, 3, 0, o, None), (x, 0, 3, 0, o, sc), (x, -4, 3, 0, o, sc), (x, 2**32, 3, 0, o, sc),
           (x, 10, 0, 0, o, sc), (x, 10, -1, 0, o, sc), (x, 10, 4097, 0, o, sc), (x, 10, 3, -1, o, sc), (x, 10, 3, 10, o, sc), (x, 10, 3, 11, o, sc),
           (x + 1, 10, 3, 0, o, sc), (x + 2, 10, 3, 0, o, sc)]
    for i, args in enumerate(bad):
        assert lib.orcai_column_select(*args, s) == N.E_BADARG, i
    m = torch.zeros(3, device="cuda")
    for i, args in enumerate([(None, 10, 3, m.data_ptr()), (x, 10, 3, None), (x, 0, 3, m.data_ptr()), (x, 10, 0, m.data_ptr()), (x, 10, 4097, m.data_ptr()),
                              (x + 2, 10, 3, m.data_ptr())]):
        assert lib.orcai_subtract_columns(*args, s) == N.E_BADARG, i
    torch.cuda.synchronize()
    assert out.tolist() == [7.0] * 4 and float(d.abs().max()) == 0.0
    assert lib.orcai_column_select(x, 10, 3, 9, o, sc, s) == 0  # the same arguments with a rank inside: accepted
    assert out.tolist() == [0.0, 0.0, 0.0, 7.0]
    big = torch.zeros((2, 5000), device="cuda")
    for dim, err in ((1, "dim"), (-1, "dim"), (2, "dim")):
        with pytest.raises(ValueError, match=err):
            fe.percentiles(big, [0.5], dim=dim)
    with pytest.raises(ValueError, match="4096"):
        fe.percentiles(big, [0.5], dim=0)
    with pytest.raises(ValueError, match="two dimensions"):
        fe.percentiles(torch.zeros(8, device="cuda"), [0.5], dim=0)
    with pytest.raises(ValueError):
        fe.percentiles(d, [1.5], dim=0)
    with pytest.raises(TypeError):
        fe.percentiles(d.double(), [0.5], dim=0)


# ------------------------------------------------------------------------------------------------ 4. percentiles and subtract_columns
@pytest.mark.parametrize("shape", [(3001, 171), (37, 4, 5)], ids=["3001x171", "37x4x5"])
def test_column_percentiles_equal_numpy_nearest(fe, shape):
    import orcai_amd.torch_ops as O

    q = [0, 0.01, 0.25, 0.5, 0.999, 1]
    x = make_array("mixed", shape[0], int(np.prod(shape[1:]))).reshape(shape)
    want = np.percentile(x, [100 * v for v in q], axis=0, method="nearest")
    assert want.dtype == np.float32 and want.shape == (len(q), *shape[1:])
    d = torch.from_numpy(x).cuda()
    for got in (fe.percentiles(d, q, dim=0), torch.ops.orcai.column_percentile(d, [float(v) for v in q]), O.column_percentile(d, q)):
        assert got.dtype == torch.float32 and tuple(got.shape) == want.shape and got.is_cuda
        assert np.array_equal(got.cpu().numpy(), want)
    xg = d.clone().requires_grad_(True)
    y = torch.ops.orcai.column_percentile(xg, [0.5])
    assert y.requires_grad
    with pytest.raises(NotImplementedError, match="order statistic"):
        y.sum().backward()


def test_flat_percentiles_are_what_they_were(fe):
    x = make("wide", 171 * 301, seed=9).reshape(301, 171)
    q = [0.0, 0.01, 0.5, 0.999, 1.0]
    want = np.percentile(x, [100 * v for v in q], method="nearest")
    d = torch.from_numpy(x).cuda()
    for got in (fe.percentiles(d, q), fe.percentiles(d, q, dim=None), fe.percentiles(d, q, None)):
        assert tuple(got.shape) == (len(q),) and as_bits(got.cpu().numpy()) == as_bits(want)


@pytest.mark.parametrize("offset", [0, 1, 2, 3])
@pytest.mark.parametrize("shape", [(1025, 33), (3001, 171), (3, 1), (7, 2)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_subtract_columns_is_numpy_float32(fe, shape, offset):
    """offset: floats between a 16-byte boundary and x[0][0] -- the scalar head in front of the 16-byte body, and its tail."""
    from orcai_amd import _native as N

    R, C = shape
    x = make_array("mixed", R, C)
    m = make("normal_db", C, seed=3)
    m[0] = -0.0
    want = x - m
    assert want.dtype == np.float32
    buf = torch.full((R * C + 8,), 99.0, dtype=torch.float32, device="cuda")
    assert buf.data_ptr() % 16 == 0
    d = buf[offset : offset + R * C]
    d.copy_(torch.from_numpy(x).reshape(-1))
    md = torch.from_numpy(m).cuda()
    assert fe.lib.orcai_subtract_columns(d.data_ptr(), R, C, N.ptr(md), N.stream_ptr()) == 0
    got = buf.cpu().numpy()
    assert as_bits(got[offset : offset + R * C]) == as_bits(want.reshape(-1))
    assert (got[:offset] == 99.0).all() and (got[offset + R * C :] == 99.0).all()
