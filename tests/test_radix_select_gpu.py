"""orcai_quantile_select_radix on the GPU: exact order statistics of any f32 data at a cost that does not depend on where the values lie.

Everything here is exact, so there is no tolerance: an order statistic equals np.sort(x)[rank] by value and equals the level-1 select
(FrontEnd.select(..., method="level1")) bit for bit -- both order by the same key, so -0.0 and +0.0 agree too; a PCEN spectrogram keeps its bytes;
a percentile equals np.percentile(..., method="nearest") on the host copy.  Inputs hold no NaN."""

import numpy as np
import pytest

from orcai_amd import pcen

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

N_MANY = 171 * 3001  # about 500 workgroups
N_SWEEPS = 2 * 2048 * 1024 + 4 * 300 + 3  # the capped grid (2048 workgroups of 256 lanes, 4 values each) sweeps twice, a partial third time, and a tail
SIZES = [1, 2, 3, 5, 37, 1023, 1024, 1025, N_MANY, N_SWEEPS]
KINDS = ["normal_db", "ties", "constant", "near_zero", "wide", "tiny", "pcen_like", "subnormal", "inf", "two_values", "last_digit", "middle_digit",
         "same_first_digit", "same_second_digit"]


@pytest.fixture(scope="module")
def fe():
    from orcai_amd.frontend import get_frontend

    return get_frontend()


def bits_to_f32(bits):
    return np.ascontiguousarray(bits, dtype=np.uint32).view(np.float32)


def make(kind, n, seed=5):
    """f32[n] of one kind.  The digits are those of the key: [31:21] (sign, exponent, two mantissa bits), [20:10], [9:0]."""
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
    if kind == "tiny":
        return rng.standard_normal(n).astype(np.float32)
    if kind == "pcen_like":  # most of the mass below 0.125, 2 % exact +0.0
        x = rng.gamma(0.5, 0.02, n).astype(np.float32)
        x[rng.random(n) < 0.02] = 0.0
        return x
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
    if kind == "same_first_digit":  # [1, 1.25): one first-digit bin, the two ranks in different second-digit bins
        return bits_to_f32(np.uint32(0x3F800000) | rng.integers(0, 2**21, n, dtype=np.uint32))
    if kind == "same_second_digit":  # two first-digit bins (1.0 and 8.0), ONE second digit, any last digit: the ranks' prefixes differ from pass 2 on
        first = np.where(rng.random(n) < 0.5, np.uint32(0x3F800000), np.uint32(0x41000000))
        return bits_to_f32(first | np.uint32(77 << 10) | rng.integers(0, 1024, n, dtype=np.uint32))
    raise KeyError(kind)


def rank_pairs(n):
    lo, hi = int(0.01 * (n - 1)), int(0.999 * (n - 1))
    return [(lo, hi), (0, n - 1), (n // 2, n // 2), (hi, lo)]  # the last with rank_lo > rank_hi


def as_bits(pair):
    return tuple(int(np.float32(v).view(np.uint32)) for v in pair)


def check_exact(fe, x):
    xs = np.sort(x, axis=None)
    d = torch.from_numpy(x).cuda()
    for ranks in rank_pairs(x.size):
        got = fe.select(d, *ranks, method="radix")
        assert (np.float32(got[0]), np.float32(got[1])) == (xs[ranks[0]], xs[ranks[1]]), (ranks, got, xs[ranks[0]], xs[ranks[1]])
        assert as_bits(got) == as_bits(fe.select(d, *ranks, method="level1")), ranks


# ------------------------------------------------------------------------------------------------ (a) exactness
@pytest.mark.parametrize("kind", KINDS)
def test_radix_select_exact_on_every_kind(fe, kind):
    check_exact(fe, make(kind, 37 if kind == "tiny" else N_MANY))


@pytest.mark.parametrize("n", SIZES)
def test_radix_select_exact_at_every_size(fe, n):
    """Tail only (n < 4), n % 4 != 0, one workgroup, many, and more than one sweep of the capped grid with a tail."""
    for kind in ("normal_db", "pcen_like", "last_digit") if n != N_SWEEPS else ("pcen_like", "same_second_digit"):
        check_exact(fe, make(kind, n, seed=n))


# ------------------------------------------------------------------------------------------------ (b) state
def _select_raw(fe, ws, d, ranks):
    """orcai_quantile_select_radix + finalize(0) on the workspace tensor ws: the six statistics' bytes."""
    from orcai_amd import _native as N

    s = N.stream_ptr()
    assert fe.lib.orcai_quantile_select_radix(d.data_ptr(), d.numel(), ranks[0], ranks[1], ws.data_ptr(), s) == 0
    assert fe.lib.orcai_frontend_finalize(0, 0.0, ws.data_ptr(), s) == 0
    out = torch.empty(6, dtype=torch.float32, device="cuda")
    assert fe.lib.orcai_frontend_stats_dev(ws.data_ptr(), out.data_ptr(), s) == 0
    return out.cpu().numpy().view(np.uint32).tolist()


def test_no_reset_needed_and_repeatable(fe):
    a = torch.from_numpy(make("wide", 50001, seed=1)).cuda()
    b = torch.from_numpy(make("pcen_like", 70003, seed=2)).cuda()
    ra, rb = (17, 49000), (69000, 123)
    used = torch.zeros_like(fe.workspace)
    first_a = _select_raw(fe, used, a, ra)
    b_after_a = _select_raw(fe, used, b, rb)  # no reset in between
    assert b_after_a == _select_raw(fe, torch.zeros_like(fe.workspace), b, rb)
    assert b_after_a == _select_raw(fe, used, b, rb)  # the same call twice
    assert first_a == _select_raw(fe, used, a, ra)
    xs = np.sort(b.cpu().numpy())
    assert b_after_a[4:] == [int(xs[rb[0]].view(np.uint32)), int(xs[rb[1]].view(np.uint32))]
    dirty = torch.full_like(fe.workspace, 0xA5)  # a workspace that was never cleared: nothing of it is read
    assert _select_raw(fe, dirty, b, rb)[4:] == b_after_a[4:]


def test_radix_select_leaves_pmax_alone(fe):
    from orcai_amd import _native as N

    sp = {"sampling_rate": 48000, "nfft": 512, "n_overlap": 256, "freq_range": [0, 16000], "quantiles": [0.01, 0.999]}
    rng = np.random.default_rng(3)
    fe.make_spectrogram(torch.from_numpy((0.1 * rng.standard_normal(20000)).astype(np.float32)).cuda(), sp)
    before = fe.stats()
    assert before["pmax"] > 0.0
    hist1 = fe.workspace[: 4 * 2561].clone()  # the level-1 histogram opens the workspace
    assert int(hist1.view(torch.int32).sum()) == (1 + 20000 // 256) * 171
    d = torch.from_numpy(make("pcen_like", 40001, seed=4)).cuda()
    assert fe.lib.orcai_quantile_select_radix(d.data_ptr(), d.numel(), 400, 39000, N.ptr(fe.workspace), N.stream_ptr()) == 0
    after = fe.stats()
    assert np.float32(after["pmax"]).view(np.uint32) == np.float32(before["pmax"]).view(np.uint32)
    assert torch.equal(fe.workspace[: 4 * 2561], hist1)


# ------------------------------------------------------------------------------------------------ (c) refusals
def test_refusals(fe):
    from orcai_amd import _native as N

    lib, s, ws = fe.lib, N.stream_ptr(), N.ptr(fe.workspace)
    d = torch.zeros(64, device="cuda")
    x = d.data_ptr()
    assert x % 16 == 0
    bad = [(None, 10, 0, 9, ws), (x, 10, 0, 9, None), (x, 0, 0, 0, ws), (x, -5, 0, 0, ws), (x, 2**32, 0, 9, ws), (x, 2**40, 0, 9, ws),
           (x, 10, -1, 9, ws), (x, 10, 0, 10, ws), (x, 10, 10, 0, ws), (x, 10, 0, -1, ws), (x + 4, 10, 0, 9, ws), (x + 8, 10, 0, 9, ws)]
    for i, (xp, n, r_lo, r_hi, w) in enumerate(bad):
        assert lib.orcai_quantile_select_radix(xp, n, r_lo, r_hi, w, s) == N.E_BADARG, i
    assert lib.orcai_quantile_select_radix(x, 10, 9, 0, ws, s) == 0  # rank_lo > rank_hi is allowed
    with pytest.raises(ValueError, match="method"):
        fe.select(d, 0, 1, method="sort")
    with pytest.raises(ValueError, match="method"):
        fe.normalize_inplace(d.clone(), [0.01, 0.999], method="Radix")
    for q in ([], [1.5], [0.5, -0.1]):
        with pytest.raises(ValueError):
            fe.percentiles(d, q)
    with pytest.raises(ValueError):
        fe.percentiles(torch.empty(0, device="cuda"), [0.5])
    with pytest.raises(TypeError):
        fe.percentiles(d.double(), [0.5])
    with pytest.raises(TypeError):
        fe.percentiles(d.cpu(), [0.5])
    with pytest.raises(TypeError):
        fe.percentiles(d.cpu().numpy(), [0.5])


# ------------------------------------------------------------------------------------------------ (d) PCEN keeps its bytes
@pytest.mark.parametrize("T", [1030, 300])
@pytest.mark.parametrize("route", ["linear", "mel64"])
def test_pcen_spectrogram_keeps_its_bytes(fe, route, T):
    """orcai_make_pcen_spectrogram (the radix select inside) against the staged composition through the C ABI with the level-1 select."""
    from orcai_amd import _native as N
    from orcai_amd.frontend import nearest_rank_index, resolve_route

    sp = dict(sampling_rate=48000, nfft=512, n_overlap=256, freq_range=[0, 16000], quantiles=[0.01, 0.999], pcen={})
    if route == "mel64":
        sp["mel"] = {"n_mels": 64}
    n = (T - 1) * 256 + 17
    rng = np.random.default_rng(T)
    t = np.arange(n) / 48000.0
    x = (0.05 * rng.standard_normal(n) * (1.0 + 0.8 * np.sin(2 * np.pi * 3.0 * t)) + 0.2 * np.sin(2 * np.pi * 2500.0 * t) * (t > 0.2)).astype(np.float32)
    x[5000:9000] = 0.0  # silence: exact zeros in the energies
    xd = torch.from_numpy(x).cuda()
    got, got_stats = fe.make_spectrogram(xd, sp, return_stats=True)
    n_fft, hop, K, cfg, pc = resolve_route(sp)
    assert tuple(got.shape) == (T, K) and K == (64 if route == "mel64" else 171)

    lib, s = fe.lib, N.stream_ptr()
    ws = torch.zeros_like(fe.workspace)
    out = torch.empty((T, K), dtype=torch.float32, device="cuda")
    scratch = torch.empty(lib.orcai_pcen_scratch_bytes(T, K) // 4, dtype=torch.float32, device="cuda")
    a, b = pcen.smoother(pc["time_constant"], sp["sampling_rate"], hop)
    r_lo, r_hi = (nearest_rank_index(T * K, q) for q in sp["quantiles"])
    assert lib.orcai_frontend_reset(N.ptr(ws), s) == 0
    if cfg is None:
        assert lib.orcai_stft_energy(N.ptr(xd), n, n_fft, hop, T, K, N.ptr(out), s) == 0
    else:
        assert lib.orcai_stft_mel_energy(N.ptr(xd), n, n_fft, hop, T, K, *fe._bands(sp, cfg), N.ptr(out), s) == 0
    assert lib.orcai_pcen(N.ptr(out), T, K, a, b, pc["scale"], pc["gain"], pc["bias"], pc["power"], pc["eps"], N.ptr(scratch), s) == 0
    assert lib.orcai_hist_level1(N.ptr(out), T * K, N.ptr(ws), s) == 0
    assert lib.orcai_quantile_select(N.ptr(out), T * K, r_lo, r_hi, N.ptr(ws), s) == 0
    assert lib.orcai_frontend_finalize(0, 0.0, N.ptr(ws), s) == 0
    assert lib.orcai_clip_normalize(N.ptr(out), T * K, N.ptr(ws), s) == 0
    stats = torch.empty(6, dtype=torch.float32, device="cuda")
    assert lib.orcai_frontend_stats_dev(N.ptr(ws), N.ptr(stats), s) == 0
    assert torch.equal(got.view(torch.int32), out.view(torch.int32))
    assert torch.equal(got_stats.view(torch.int32), stats.view(torch.int32))
    assert float(out.min()) == 0.0 and float(out.max()) == 1.0


# ------------------------------------------------------------------------------------------------ (e) Python and torch
@pytest.mark.parametrize("kind", ["normal_db", "pcen_like"])
def test_normalize_inplace_same_bytes(fe, kind):
    x = torch.from_numpy(make(kind, 171 * 301, seed=8)).cuda()
    a, b = x.clone(), x.clone()
    fe.normalize_inplace(a, [0.01, 0.999])
    fe.normalize_inplace(b, [0.01, 0.999], method="radix")
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert float(a.min()) == 0.0 and float(a.max()) == 1.0


@pytest.mark.parametrize("q", [[0.0, 0.01, 0.5, 0.999, 1.0], [0.25]], ids=["five", "one"])
@pytest.mark.parametrize("shape", [(40001,), (301, 171)], ids=["flat", "2d"])
def test_percentiles_equal_numpy_nearest(fe, q, shape):
    import orcai_amd.torch_ops as O

    x = make("pcen_like", int(np.prod(shape)), seed=9).reshape(shape)
    want = np.percentile(x, [100 * v for v in q], method="nearest")
    assert want.dtype == np.float32
    d = torch.from_numpy(x).cuda()
    for got in (fe.percentiles(d, q), torch.ops.orcai.percentile(d, q), O.percentile(d, q)):
        assert got.dtype == torch.float32 and tuple(got.shape) == (len(q),) and got.is_cuda
        assert got.cpu().numpy().view(np.uint32).tolist() == want.view(np.uint32).tolist()


def test_percentile_op_has_no_gradient_and_compiles(fe):
    import orcai_amd.torch_ops  # noqa: F401  (registers the ops)
    from torch._subclasses.fake_tensor import FakeTensorMode

    q = [0.0, 0.01, 0.5, 0.999, 1.0]
    d = torch.from_numpy(make("wide", 3 * 10007, seed=10).reshape(3, -1)).cuda()
    eager = torch.ops.orcai.percentile(d, q)
    with FakeTensorMode():
        fake = torch.ops.orcai.percentile(torch.empty((7, 9), device="cuda"), q)
    assert tuple(fake.shape) == (5,) and fake.dtype == torch.float32 and fake.device.type == "cuda"
    xg = d.clone().requires_grad_(True)
    y = torch.ops.orcai.percentile(xg, q)
    assert y.requires_grad and torch.equal(y.detach().view(torch.int32), eager.view(torch.int32))
    with pytest.raises(NotImplementedError, match="order statistic"):
        y.sum().backward()
    compiled = torch.compile(lambda t: torch.ops.orcai.percentile(t, q) * 1.0, backend="aot_eager", fullgraph=True)(d)
    assert torch.equal(compiled.view(torch.int32), eager.view(torch.int32))
    with pytest.raises(TypeError):
        torch.ops.orcai.percentile(d.double(), q)
