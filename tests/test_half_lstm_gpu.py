"""The f16 path's LSTM recurrences through the C ABI -- orcai_h_lstm_train_fwd (lstm_train_fwd_h_kernel<32|64|96|128>) and orcai_h_lstm_bwd
(lstm_bwd_h_kernel<32|64|96|128>) -- against float64, and the helpers orcai_lstm_hprev, orcai_pack_lstm, orcai_unpack_lstm_grad bit for bit.

Two checks per recurrence case (tests/lstm_ref.py):
  step check   against the f16-rounding reference fed with the device's own stored out / dxz (teacher forcing), at the bars of the f32 kernels
               (1e-5 absolute forward, 5e-6 of max |dxz| backward): a wrong k block, a dropped fragment or a stale LDS buffer is orders above it.
               The kernels round the unrounded f32 product to f16 in one instruction (v_fma_mixlo_f16), so where the stored f32 value is an
               exact f16 midpoint (2^-13 of the elements) either neighbour is a correct operand: the reference takes the one the device's
               next step shows (lstm_ref.f16_ties) -- one wrong choice costs up to 4e-5 in a gate, four times the bar;
  end to end   against the plain float64 recurrence, at 2 E + the f32 bar, E = what the free-running f16-rounding reference itself loses.
The reference comes in two variants, f16-subnormal operands of the matrix unit kept or flushed; the kernel has to meet one of them and the same one
wherever the two can be told apart (_WINNERS, asserted at the end of the module).  Every output buffer has one extra batch row of -7.0."""

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from lstm_ref import _bwd_ref, _fwd_ref, bwd_ref_f16, fwd_ref_f16, lstm_inputs_bwd, lstm_inputs_fwd  # noqa: E402

SENT = -7.0
FWD_BAR, BWD_BAR = 1e-5, 5e-6  # the f32 kernels' bars (tests/test_head_widths_gpu.py): same lstm_gate_stage, same activation approximations
_WINNERS = set()  # flush variants (False = subnormal operands kept, True = flushed) that won a case where only one of them passed
_UNDECIDED = []  # cases both variants passed


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _sentinel(*shape):
    return torch.full(shape, SENT, device="cuda")


def _h_fwd(xz, Uw, entry="orcai_h_lstm_train_fwd"):
    from orcai_amd import _native as N

    B, Tn, _, U4 = xz.shape
    U = U4 // 4
    xd, ud = _dev(xz), _dev(Uw)
    h, g, c = _sentinel(B + 1, Tn, 2 * U), _sentinel(B + 1, Tn, 2, 4 * U), _sentinel(B + 1, Tn, 2, U)
    N.check(getattr(N.lib(), entry)(N.ptr(xd), N.ptr(ud), B, Tn, U, N.ptr(h), N.ptr(g), N.ptr(c), N.stream_ptr()), entry)
    torch.cuda.synchronize()
    return tuple(a.cpu().numpy() for a in (h, g, c))


def _h_bwd(dH, gates, cst, Uw, entry="orcai_h_lstm_bwd"):
    from orcai_amd import _native as N

    B, Tn, _, U4 = gates.shape
    hd, gd, cd, ud = _dev(dH), _dev(gates), _dev(cst), _dev(Uw)
    dxz = _sentinel(B + 1, Tn, 2, U4)
    N.check(getattr(N.lib(), entry)(N.ptr(hd), N.ptr(gd), N.ptr(cd), N.ptr(ud), B, Tn, U4 // 4, N.ptr(dxz), N.stream_ptr()), entry)
    torch.cuda.synchronize()
    return dxz.cpu().numpy()


def _decide(tag, errs, bar):
    """errs {flush: step-check error}: at least one variant within the bar; the winner is recorded when only one is.  Returns the better variant."""
    ok = {f: e <= bar for f, e in errs.items()}
    best = min(errs, key=errs.get)
    verdict = "not distinguished by these inputs" if all(ok.values()) else f"flush={best} wins" if any(ok.values()) else "NEITHER variant within the bar"
    print(f"{tag}: step check, subnormal operands kept {errs[False]:.2e}, flushed {errs[True]:.2e} (bar {bar:g}): {verdict}")
    assert any(ok.values()), (tag, errs)
    if all(ok.values()):
        _UNDECIDED.append(tag)
    else:
        _WINNERS.add(best)
    return best


# ------------------------------------------------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize("U", [32, 64, 96, 128])
@pytest.mark.parametrize("B,Tn", [(7, 46), (17, 2), (65, 9), (16, 1)])
def test_h_lstm_train_fwd_vs_float64(U, B, Tn):
    xz, Uw = lstm_inputs_fwd(np.random.default_rng(1000 + U + B + Tn), U, B, Tn)
    got = _h_fwd(xz, Uw)
    for a in got:
        assert (a[B] == SENT).all()  # nothing past the last batch row
        assert np.isfinite(a[:B]).all()
    got = tuple(a[:B] for a in got)
    tag = f"h forward U {U} B {B} T {Tn}"
    errs = {}
    for flush in (False, True):
        ref = fwd_ref_f16(xz, Uw, h_forced=got[0], flush=flush, gates_forced=got[1])
        per = [float(np.abs(a - b).max()) for a, b in zip(got, ref)]
        print(f"{tag} flush={flush}: max |h, gates, c - forced f16 reference| = {per}")
        errs[flush] = max(per)
    win = _decide(tag, errs, FWD_BAR)
    plain, free = _fwd_ref(xz, Uw), fwd_ref_f16(xz, Uw, flush=win)
    E = [float(np.abs(a - b).max()) for a, b in zip(free, plain)]
    gap = [float(np.abs(a - b).max()) for a, b in zip(got, plain)]
    print(f"{tag}: end to end, E = max |f16 reference - float64| = {E}, device gap {gap}")
    for e, d in zip(E, gap):
        assert d <= 2 * e + FWD_BAR, (tag, E, gap)


# ----------------------------------------------------------------------------------------------------------------------------- backward
def _check_bwd(tag, inputs, cap=None):
    dH, gates, cst, Uw = inputs
    B = gates.shape[0]
    got = _h_bwd(*inputs)
    assert (got[B] == SENT).all() and np.isfinite(got[:B]).all()
    got = got[:B]
    errs = {}
    for flush in (False, True):
        ref = bwd_ref_f16(*inputs, dxz_forced=got, flush=flush, ties=True)
        errs[flush] = float(np.abs(got - ref).max() / np.abs(ref).max())
    win = _decide(tag, errs, BWD_BAR)
    plain = _bwd_ref(*inputs)
    scale = np.abs(plain).max()
    E = float(np.abs(bwd_ref_f16(*inputs, flush=win) - plain).max() / scale)
    gap = float(np.abs(got - plain).max() / scale)
    print(f"{tag}: end to end, E / max |dxz| = {E:.2e} (free-running f16 reference vs float64), device gap {gap:.2e}, max |dH| {np.abs(dH).max():.2e}")
    return E, gap


@pytest.mark.parametrize("U", [32, 64, 96, 128])
@pytest.mark.parametrize("B,Tn,gscale", [(20, 46, 3.0), (7, 9, 0.1), (65, 2, 1e-2), (16, 1, 0.1)])
def test_h_lstm_bwd_vs_float64(U, B, Tn, gscale):
    inputs = lstm_inputs_bwd(np.random.default_rng(2000 + U + B + Tn), U, B, Tn, gscale)
    tag = f"h backward U {U} B {B} T {Tn} |dH| ~ {gscale:g}"
    E, gap = _check_bwd(tag, inputs)
    assert gap <= 2 * E + BWD_BAR, (tag, E, gap)


@pytest.mark.parametrize("gscale", [1e-4, 1e-6, 1e-9])
def test_h_lstm_bwd_small_gradients(gscale):
    """What the unscaled f16 cast of dz costs below the loss-scaled range: the kernel still does what the rounding reference does (step check,
    finite), and E / max |dxz| -- printed, a property of the method, not a bar -- is what that is worth against float64."""
    inputs = lstm_inputs_bwd(np.random.default_rng(64 + 20 + 46), 64, 20, 46, gscale)
    _check_bwd(f"h backward U 64 B 20 T 46 small |dH| ~ {gscale:g}", inputs)


def test_h_lstm_bwd_at_training_magnitudes():
    """max |dH| entering the recurrences in the float64 oracle (oracle/train_ref.py, loss x half.LOSS_SCALE = 1024; filters (10, 20) at 32 and 96
    units, B = 3, and filters (12, 30, 40) at 64 units, B = 2): 70 .. 270 into LSTM-2, 27 .. 91 into LSTM-1.  The smaller, rounded down to a power
    of ten: max |dH| = 10.  There the recurrence has to be in f16's normal range: E / max |dxz| <= 2^-9 (four f16 ulps) from the reference alone,
    and the kernel within 2 E + 5e-6 of float64."""
    from orcai_amd.half import LOSS_SCALE

    assert LOSS_SCALE == 1024.0  # the magnitudes above were taken with this scale
    dH, gates, cst, Uw = lstm_inputs_bwd(np.random.default_rng(77), 64, 20, 46, 1.0)
    dH = (dH * (10.0 / np.abs(dH).max())).astype(np.float32)
    tag = "h backward U 64 B 20 T 46 at the training magnitude max |dH| = 10"
    E, gap = _check_bwd(tag, (dH, gates, cst, Uw))
    assert E <= 2.0**-9, (tag, E)
    assert gap <= 2 * E + BWD_BAR, (tag, E, gap)


# -------------------------------------------------------------------------------------------------------------------------- wide widths
@pytest.mark.parametrize("U", [160, 256])
def test_h_entries_route_wide_widths_to_the_f32_family(U):
    """Above 128 units both orcai_h_ entries run lstm_wide_* (include/orcai_hip.h): bit for bit the f32 entries' tensors."""
    B, Tn = 20, 9
    xz, Uw = lstm_inputs_fwd(np.random.default_rng(U), U, B, Tn)
    for a, b in zip(_h_fwd(xz, Uw), _h_fwd(xz, Uw, entry="orcai_lstm_train_fwd")):
        assert (a[B] == SENT).all() and np.array_equal(a, b)
    inputs = lstm_inputs_bwd(np.random.default_rng(U + 1), U, B, Tn, 0.1)
    a, b = _h_bwd(*inputs), _h_bwd(*inputs, entry="orcai_lstm_bwd")
    assert (a[B] == SENT).all() and np.array_equal(a, b)
    assert np.abs(a[:B] - _bwd_ref(*inputs)).max() <= BWD_BAR * np.abs(a[:B]).max()


# ---------------------------------------------------------------------------------------------------------------------------- refusals
def test_h_lstm_entries_refuse_without_writing():
    from orcai_amd import _native as N

    lib, st = N.lib(), N.stream_ptr()
    B, Tn, U = 3, 4, 32
    bufs = {k: _sentinel(*s) for k, s in (("xz", (B, Tn, 2, 4 * U)), ("Uw", (2, U, 4 * U)), ("h", (B, Tn, 2 * U)), ("g", (B, Tn, 2, 4 * U)), ("c", (B, Tn, 2, U)), ("dxz", (B, Tn, 2, 4 * U)))}
    p = {k: N.ptr(v) for k, v in bufs.items()}
    fwd = lambda xz, Uw, b, t, u, h, g, c: lib.orcai_h_lstm_train_fwd(xz, Uw, b, t, u, h, g, c, st)  # noqa: E731
    bwd = lambda dH, g, c, Uw, b, t, u, dxz: lib.orcai_h_lstm_bwd(dH, g, c, Uw, b, t, u, dxz, st)  # noqa: E731
    fargs = (p["xz"], p["Uw"], B, Tn, U, p["h"], p["g"], p["c"])
    bargs = (p["h"], p["g"], p["c"], p["Uw"], B, Tn, U, p["dxz"])
    for units in (0, 16, 48, 288):
        assert fwd(*fargs[:4], units, *fargs[5:]) == N.E_UNSUPPORTED, units
        assert bwd(*bargs[:6], units, bargs[7]) == N.E_UNSUPPORTED, units
    for fn, args, sizes in ((fwd, fargs, (2, 3, 4)), (bwd, bargs, (4, 5, 6))):  # sizes: the positions of B, T, units
        for i in range(len(args)):
            if i in sizes:
                continue
            bad = list(args)
            bad[i] = None  # a null pointer
            assert fn(*bad) == N.E_BADARG, (fn, i)
        for i in sizes[:2]:  # B = 0, T = 0
            bad = list(args)
            bad[i] = 0
            assert fn(*bad) == N.E_BADARG, (fn, i)
    torch.cuda.synchronize()
    for k, v in bufs.items():
        assert bool((v == SENT).all()), k


# ----------------------------------------------------------------------------------------------------------------------------- helpers
@pytest.mark.parametrize("B,Tn,U", [(3, 1, 32), (5, 2, 96), (7, 46, 128), (2, 9, 256)])
def test_lstm_hprev_is_the_shifted_output(B, Tn, U):
    from orcai_amd import _native as N

    h = np.random.default_rng(B + Tn + U).standard_normal((B, Tn, 2 * U)).astype(np.float32)
    hd, hp = _dev(h), _sentinel(B + 1, Tn, 2, U)
    N.check(N.lib().orcai_lstm_hprev(N.ptr(hd), B, Tn, U, N.ptr(hp), N.stream_ptr()), "lstm_hprev")
    torch.cuda.synchronize()
    got = hp.cpu().numpy()
    want = np.zeros((B, Tn, 2, U), np.float32)
    want[:, 1:, 0] = h[:, :-1, :U]
    want[:, :-1, 1] = h[:, 1:, U:]
    assert np.array_equal(got[:B], want)
    assert not got[:B, 0, 0].any() and not got[:B, Tn - 1, 1].any()  # each direction's sequence start
    assert (got[B] == SENT).all()


def test_pack_lstm_both_modes_in_one_launch():
    """orcai_pack_lstm: twelve descriptors {src off, dst off, rows, u, ld_dst, col_off, mode} in one launch -- u 32 and 96, rows 1, 37 and u, a
    non-zero col_off, ld_dst larger than needed -- mode 0 (f32, permuted columns) and mode 1 (the f16 transposed copy) against
    architectures.lstm_column_permutation; every element the descriptors do not name keeps its sentinel."""
    from orcai_amd import _native as N
    from orcai_amd.architectures import lstm_column_permutation

    rng = np.random.default_rng(11)
    descs, want32, want16, srcs = [], [], [], []
    soff = off32 = off16 = 5
    for u in (32, 96):
        perm = lstm_column_permutation(u)
        for rows in (1, 37, u):
            src = rng.standard_normal((rows, 4 * u)).astype(np.float32)
            srcs.append((soff, src))
            col_off, ld = 3, 4 * u + 3 + 5
            descs.append([soff, off32, rows, u, ld, col_off, 0])
            w = np.full((rows, ld), SENT, np.float32)
            w[:, col_off : col_off + 4 * u] = src[:, perm]
            want32.append((off32, w))
            off32 += rows * ld + 7
            col_off, ld = 2, rows + 3
            descs.append([soff, off16, rows, u, ld, col_off, 1])
            w = np.full((col_off + 4 * u, ld), SENT, np.float16)
            w[col_off:, :rows] = src[:, perm].T.astype(np.float16)
            want16.append((off16, w))
            off16 += (col_off + 4 * u) * ld + 7
            soff += src.size + 3
    wflat = np.full(soff, 123.0, np.float32)
    for o, s in srcs:
        wflat[o : o + s.size] = s.ravel()
    e32, e16 = np.full(off32, SENT, np.float32), np.full(off16, SENT, np.float16)
    for o, w in want32:
        e32[o : o + w.size] = w.ravel()
    for o, w in want16:
        e16[o : o + w.size] = w.ravel()
    wd, dd = _dev(wflat), _dev(np.asarray(descs, np.int32))
    o32, o16 = _sentinel(off32), torch.full((off16,), SENT, device="cuda", dtype=torch.float16)
    N.check(N.lib().orcai_pack_lstm(N.ptr(wd), N.ptr(dd), len(descs), N.ptr(o32), N.ptr(o16), N.stream_ptr()), "pack_lstm")
    torch.cuda.synchronize()
    assert np.array_equal(o32.cpu().numpy(), e32)
    assert np.array_equal(o16.cpu().numpy(), e16)
    assert (e32 != SENT).sum() > 0 and (e16 != np.float16(SENT)).sum() > 0


@pytest.mark.parametrize("u,rows", [(32, 1), (32, 37), (96, 37), (96, 96)])
def test_unpack_lstm_grad_is_the_inverse_permutation(u, rows):
    """orcai_unpack_lstm_grad against architectures.lstm_column_permutation: G[r][perm[p]] = src[r][col_off + p] exactly (W = NULL, l2g = 0), and
    with W the fused multiply-add: float64 arithmetic rounded once to f32."""
    from orcai_amd import _native as N
    from orcai_amd.architectures import lstm_column_permutation

    rng = np.random.default_rng(u + rows)
    perm = lstm_column_permutation(u)
    col_off, ld = 5, 4 * u + 5 + 3
    src = rng.standard_normal((rows, ld)).astype(np.float32)
    W = rng.standard_normal((rows, 4 * u)).astype(np.float32)
    l2g = np.float32(1e-4 * 1024.0)
    sd, Wd = _dev(src), _dev(W)
    lib, st = N.lib(), N.stream_ptr()
    G0, G1 = _sentinel(rows * 4 * u + 9), _sentinel(rows * 4 * u + 9)
    N.check(lib.orcai_unpack_lstm_grad(N.ptr(sd), ld, col_off, rows, u, N.ptr(G0), None, 0.0, st), "unpack")
    N.check(lib.orcai_unpack_lstm_grad(N.ptr(sd), ld, col_off, rows, u, N.ptr(G1), N.ptr(Wd), float(l2g), st), "unpack")
    torch.cuda.synchronize()
    G0, G1 = G0.cpu().numpy(), G1.cpu().numpy()
    want = np.empty((rows, 4 * u), np.float32)
    want[:, perm] = src[:, col_off : col_off + 4 * u]
    assert np.array_equal(G0[: want.size].reshape(want.shape), want)
    fma = (want.astype(np.float64) + np.float64(l2g) * W.astype(np.float64)).astype(np.float32)
    assert np.array_equal(G1[: want.size].reshape(want.shape), fma)
    assert (G0[want.size :] == SENT).all() and (G1[want.size :] == SENT).all()


# ------------------------------------------------------------------------------------------------------- the subnormal verdict (keep last)
def test_one_subnormal_variant_wins_everywhere():
    """A constructed case whose dz is mostly f16-subnormal (|dH| ~ 1e-4: dz ~ 1e-5 < 2^-14), where the two reference variants are ~0.2 of
    max |dxz| apart, so the matrix unit's treatment of f16-subnormal A/B operands is decided even when this test runs alone; then every case of
    the module that could tell the variants apart must have picked the same one."""
    inputs = lstm_inputs_bwd(np.random.default_rng(9), 32, 7, 9, 1e-4)
    keep, flush = bwd_ref_f16(*inputs), bwd_ref_f16(*inputs, flush=True)
    assert np.abs(keep - flush).max() > 1e3 * BWD_BAR * np.abs(keep).max()  # the references do differ here
    dz = np.abs(keep.astype(np.float16).astype(np.float64))
    assert ((dz < 2.0**-14) & (dz > 0)).mean() > 0.5  # mostly subnormal operands
    _check_bwd("h backward U 32 B 7 T 9, dz mostly f16-subnormal", inputs)
    print(f"f16-subnormal MFMA operands: winners {sorted(_WINNERS)} (False = kept, True = flushed); undistinguished cases: {len(_UNDECIDED)}")
    assert len(_WINNERS) == 1, _WINNERS
