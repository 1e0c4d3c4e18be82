"""The small kernels that close a training step (train_head.hip, half_dropout.hip), called directly through the C ABI and compared with the
references of tests/step_scalars_ref.py: the dropout draws, mask-and-scale, the ReLU gradient, the masked loss and its gradient, the L2 penalty,
Adam, the moving-average update, the step counter and the overflow guard.

Every tolerance is one of three kinds (none is taken from what the kernels return):
  * bit-identical: the draws, mask_scale, relu_bwd, the counts of the loss, the single-survivor loss, the L2 penalty of small integers, every
    voided (ok = 0) or refused call, guarded-with-ok = 1 against unguarded;
  * a rounding bound derived in step_scalars_ref.py from the kernel's operation count (gamma_k = k u / (1 - k u), u = 2^-24; k and what it counts
    are stated there): bce_grad_bound (k = 10), adam_bounds (5 / 7 / 8), ema_bound (3), and n 2^-53 for the float64 sums of the L2 penalty;
  * the measured constant of the device's logarithm, step_scalars_ref.LOGF_ULPS (2 x the 1.8691 ulp measured for
    torch.log on the same probabilities; the measurement is recorded there), in the bound of the
    loss sum, bce_loss_bounds.

Every output buffer carries a sentinel behind its last element and starts out filled with one, so a launch that did nothing and a store past n both
show; sizes sit on either side of each launcher's block size, grid cap and (f16) eight-element lane."""

import ctypes
import functools
import math

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import step_scalars_ref as S  # noqa: E402

SENT = 12345.0
PAD = 8  # elements behind n that must keep the sentinel (16 bytes of f16)
N_LIST = S.N_LIST


def _N():
    from orcai_amd import _native as N_

    return N_, N_.lib(), N_.stream_ptr()


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()  # a copy: the shared inputs are read-only


def padded(a, fill=SENT):
    """Device copy of the 1-D array a with PAD sentinels behind it."""
    out = np.full(a.size + PAD, fill, dtype=a.dtype)
    out[: a.size] = a
    return dev(out)


def bits(t):
    """The raw bits of a device tensor as a numpy integer array (so that -0, NaN payloads and NaN == NaN are compared as stored)."""
    a = t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return a.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same_bits(t, expect):
    return np.array_equal(bits(t), bits(expect))


def counter_dev(value):
    return torch.tensor([value], dtype=torch.int64, device="cuda")  # uint64 on the device; the values used are below 2^63


# ============================================================================================================ 1. dropout draws
@pytest.mark.parametrize("keep", [0.5, 0.7, 1.0, 0.0])
def test_dropout_draws_bit_for_bit(keep):
    """orcai_dropout_mask(seed), orcai_dropout_mask_dev and orcai_h_dropout_mask_dev(seed_add, counter) equal splitmix_keep element for element at
    every n of N_LIST and counter in {0, 1, 2^33 + 5} (a counter product that needs all 64 bits); keep = 1 draws all ones, keep = 0 all zeros;
    the f16 mask equals the f32 mask; the PAD elements behind n keep their sentinel.  The largest n is 16387: an element index kept in 32 bits
    inside a kernel would pass here.  The reference is checked past 2^32 on the CPU (tests/test_step_scalars_ref.py); the kernels are not, a mask
    of that length being 16 GiB.  What is covered on the GPU is the 64-bit seed arithmetic (the counter of 2^33 + 5) and the i + 1 of every draw."""
    N_, lib, st = _N()
    seed_add = 0x1234_5678_9ABC_DEF1
    for n in N_LIST:
        for counter in (0, 1, (1 << 33) + 5):
            seed = S.dev_seed(seed_add, counter)
            want = S.splitmix_keep(seed, n, keep)
            if keep in (0.0, 1.0):
                assert bool(want.all()) == (keep == 1.0) and bool(want.any()) == (keep == 1.0)
            want32 = np.concatenate([want.astype(np.float32), np.full(PAD, SENT, np.float32)])
            c = counter_dev(counter)
            m_host = torch.full((n + PAD,), SENT, device="cuda")
            m_dev = torch.full((n + PAD,), SENT, device="cuda")
            m_h = torch.full((n + PAD,), SENT, dtype=torch.float16, device="cuda")
            N_.check(lib.orcai_dropout_mask(N_.ptr(m_host), n, ctypes.c_uint64(seed), keep, st), "dropout_mask")
            N_.check(lib.orcai_dropout_mask_dev(N_.ptr(m_dev), n, N_.ptr(c), ctypes.c_uint64(seed_add), keep, st), "dropout_mask_dev")
            N_.check(lib.orcai_h_dropout_mask_dev(N_.ptr(m_h), n, N_.ptr(c), ctypes.c_uint64(seed_add), keep, st), "h_dropout_mask_dev")
            what = (n, counter, keep)
            assert same_bits(m_host, want32), what
            assert same_bits(m_dev, want32), what
            assert same_bits(m_h, want32.astype(np.float16)), what
            assert int(c.item()) == counter


# ============================================================================================================ 2. mask_scale
@pytest.mark.parametrize("n", N_LIST)
def test_mask_scale_bit_for_bit(n):
    """f32: float32(float32(x mask) scale).  f16: float16(float32(float32(x) float32(mask)) scale), two roundings (a fused single rounding and a
    lost -0 are what the kernel's tail is written to avoid).  scale = 1 / 0.7, with the -0 product as the last element, and 1 / 0.6, with the
    value that separates two roundings from one as the last element; raw bits, out of place and in place (y == x)."""
    N_, lib, st = _N()
    for scale, witness_last in zip(np.float32(S.MS_SCALES), (False, True)):
        x16, m16 = S.mask_scale_inputs(n, witness_last)
        x32, m32 = x16.astype(np.float32), m16.astype(np.float32)
        with np.errstate(over="ignore"):
            want32 = (x32 * m32) * scale
            want16 = want32.astype(np.float16)
        assert want32.dtype == np.float32
        i_w, i_z = (n - 1, n - 2) if witness_last else (n - 2, n - 1)  # where the witness and the -0 product are
        if witness_last:
            assert want16[i_w] != S.once_and_twice(x16[i_w : i_w + 1], scale)[0][0]  # a single rounding would give another f16
        if i_z >= 0:
            assert np.signbit(want32[i_z]) and want32[i_z] == 0 and bits(want16)[i_z] == 0x8000
        if n >= 8:
            assert np.isinf(want16[n - 3])  # the overflow is in the data
        for inplace in (False, True):
            xd, md = padded(x32), dev(m32)
            yd = xd if inplace else torch.full((n + PAD,), SENT, device="cuda")
            N_.check(lib.orcai_mask_scale(N_.ptr(xd), N_.ptr(md), float(scale), n, N_.ptr(yd), st), "mask_scale")
            assert same_bits(yd, np.concatenate([want32, np.full(PAD, SENT, np.float32)])), (n, float(scale), inplace, "f32")
            xh, mh = padded(x16), dev(m16)
            yh = xh if inplace else torch.full((n + PAD,), SENT, dtype=torch.float16, device="cuda")
            assert xh.data_ptr() % 16 == 0 and mh.data_ptr() % 16 == 0 and yh.data_ptr() % 16 == 0
            N_.check(lib.orcai_h_mask_scale(N_.ptr(xh), N_.ptr(mh), float(scale), n, N_.ptr(yh), st), "h_mask_scale")
            assert same_bits(yh, np.concatenate([want16, np.full(PAD, SENT, np.float16)])), (n, float(scale), inplace, "f16")


# ============================================================================================================ 3. relu_bwd
@pytest.mark.parametrize("n", [1, 255, 256, 257, 1000])
def test_relu_bwd_bit_for_bit_in_place(n):
    """dx = dy where y > 0, else +0: y = +0, -0 and -inf block, +inf passes.  In place (dx == dy), as training.py calls it."""
    N_, lib, st = _N()
    rng = np.random.default_rng(n)
    y = rng.standard_normal(n).astype(np.float32)
    y[::5] = np.array([0.0, -0.0, np.inf, -np.inf], dtype=np.float32)[np.arange(len(y[::5])) % 4]
    dy = rng.standard_normal(n).astype(np.float32)
    want = np.where(y > 0, dy, np.float32(0.0)).astype(np.float32)
    d = padded(dy)
    N_.check(lib.orcai_relu_bwd(N_.ptr(d), N_.ptr(dev(y)), n, N_.ptr(d), st), "relu_bwd")
    assert same_bits(d, np.concatenate([want, np.full(PAD, SENT, np.float32)]))


# ============================================================================================================ 4. masked loss
def _bce_call(p, y, mask_value=-1.0, lw=None, gs=1.0, want_dz=True, acc_before=(1e30, -5.0, float("nan"))):
    """Runs orcai_masked_bce (lw None and gs 1) or orcai_masked_bce_w.  acc3 holds garbage before the call and a sentinel in a fourth double;
    dz holds sentinels throughout.  Returns (acc[0:3], dz[0:n] or None)."""
    N_, lib, st = _N()
    n = p.size
    acc = torch.tensor(list(acc_before) + [SENT], dtype=torch.float64, device="cuda")
    dz = torch.full((n + PAD,), SENT, device="cuda") if want_dz else None
    pd, yd = dev(p), dev(y)
    if lw is None and gs == 1.0:
        N_.check(lib.orcai_masked_bce(N_.ptr(pd), N_.ptr(yd), n, mask_value, N_.ptr(acc), N_.ptr(dz) if want_dz else None, st), "masked_bce")
    else:
        lwd = None if lw is None else torch.tensor([lw], dtype=torch.float32, device="cuda")
        N_.check(lib.orcai_masked_bce_w(N_.ptr(pd), N_.ptr(yd), n, mask_value, N_.ptr(acc), N_.ptr(dz) if want_dz else None,
                                        None if lw is None else N_.ptr(lwd), gs, st), "masked_bce_w")
    a = acc.cpu().numpy()
    assert a[3] == SENT
    if not want_dz:
        return a[:3], None
    d = dz.cpu().numpy()
    assert bool((d[n:] == SENT).all()) and not bool((d[:n] == SENT).any())
    return a[:3], d[:n]


@functools.lru_cache(maxsize=None)
def _bce_reference(n, lw, gs):
    p, y = S.bce_pool()
    return S.bce_ref(p[:n], y[:n], loss_weight=lw, grad_scale=gs), S.bce_loss_bounds(p[:n], y[:n], loss_weight=lw)[0], S.bce_grad_bound(
        p[:n], y[:n], loss_weight=lw, grad_scale=gs
    )


@pytest.mark.parametrize("n", S.BCE_N)
def test_masked_bce_sweep(n):
    """orcai_masked_bce / _w on the first n elements of bce_pool (about 30 % masked), n around the block size and around 65536, where
    bce_reduce_kernel's 256 blocks of 256 take a second pass, with loss_weight in {absent, 0.25, 3} x grad_scale in {1, 1024}:
      acc[1], acc[2]  equal the reference's count and correct count exactly, whatever the weight;
      acc[0]          within bce_loss_bounds' stated bound of loss_weight x the float64 sum (c = LOGF_ULPS = 3.74, + 1 where 1.0f - q is inexact);
      dz              within bce_grad_bound (gamma_10) per element, exactly 0 at masked elements; acc3's garbage is overwritten, not added to;
                      dz = NULL gives the same three sums."""
    p, y = S.bce_pool()
    p, y = p[:n], y[:n]
    for lw, gs in ((None, 1.0), (0.25, 1.0), (3.0, 1.0), (None, 1024.0), (0.25, 1024.0), (3.0, 1024.0)):
        (loss, count, correct, dz_ref), loss_bound, dz_bound = _bce_reference(n, lw, gs)
        acc, dz = _bce_call(p, y, lw=lw, gs=gs)
        what = (n, lw, gs)
        assert acc[1] == count and acc[2] == correct, what
        assert abs(acc[0] - loss) <= loss_bound, (what, acc[0], loss, loss_bound)
        excess = np.abs(dz.astype(np.float64) - dz_ref) - dz_bound
        assert excess.max() <= 0.0, (what, int(excess.argmax()), float(excess.max()))
        assert not dz[y == -1.0].any() and bool((bits(dz[y == -1.0]) == 0).all()), what
        if count:
            assert dz[y != -1.0].all(), what  # no probability of the pool is clipped: every unmasked element has a gradient
    acc_only, none = _bce_call(p, y, lw=0.25, want_dz=False)
    (loss, count, correct, _), loss_bound, _ = _bce_reference(n, 0.25, 1.0)
    assert none is None and acc_only[1] == count and acc_only[2] == correct and abs(acc_only[0] - loss) <= loss_bound


def test_masked_bce_single_survivor_identity():
    """Everything masked except element j: acc[0] equals, bit for bit, the one-element call on that (p, y) -- one term plus zeros is exact in
    double, so a dropped or doubled element shows without a tolerance.  j at the first and last element of the first pass, the first of the
    second pass, the block boundary and the last element."""
    p, _ = S.bce_pool()
    n = max(S.BCE_N)
    for j, t in ((0, 1.0), (255, 0.0), (256, 1.0), (65535, 0.0), (65536, 1.0), (n - 1, 0.0)):
        y = np.full(n, -1.0, dtype=np.float32)
        y[j] = t
        acc, dz = _bce_call(p, y)
        one, dz1 = _bce_call(p[j : j + 1], y[j : j + 1])
        assert one[0] > 0.0 and one[1] == 1.0
        assert same_bits(acc, one), (j, acc, one)
        assert same_bits(dz[j : j + 1], dz1) and np.count_nonzero(dz) == 1, j


def test_masked_bce_saturated_probabilities():
    """p in {0, 1, the two clip bounds, one float32 step inside each} against t in {0, 1}, one element per call: the loss term follows the float32
    clip (15.942 for p = 1, t = 0; the oracle's float64 clip would give 16.118), within bce_loss_bounds' rigorous bound; dz is exactly 0 at and
    outside the bounds and within gamma_10 of the reference, non-zero, one step inside."""
    f = np.float32
    lo_in, hi_in = np.nextafter(S.BOUND_LO, f(1)), np.nextafter(S.BOUND_HI, f(0))
    for t in (0.0, 1.0):
        for pv, clipped in ((0.0, True), (1.0, True), (S.BOUND_LO, True), (S.BOUND_HI, True), (lo_in, False), (hi_in, False)):
            p, y = f([pv]), f([t])
            loss, count, correct, dz_ref = S.bce_ref(p, y)
            acc, dz = _bce_call(p, y)
            bound = S.bce_loss_bounds(p, y)[1]
            assert acc[1] == 1.0 and acc[2] == correct
            assert abs(acc[0] - loss) <= bound, (pv, t, acc[0], loss, bound)
            if clipped:
                assert bits(dz)[0] == 0 and dz_ref[0] == 0.0, (pv, t, dz)
            else:
                assert dz[0] != 0.0 and abs(dz[0] - dz_ref[0]) <= S.bce_grad_bound(p, y)[0], (pv, t, dz, dz_ref)
    big = _bce_call(f([1.0]), f([0.0]))[0][0]
    assert abs(big - 23.0 * math.log(2.0)) <= S.LOGF_ULPS * S.U32 * 16.0 and abs(big - 16.118) > 0.1  # -log(2^-23), not -log(1e-7)


def test_masked_bce_all_masked_and_custom_mask_value():
    p, y = S.bce_pool()
    p = p[:1000]
    acc, dz = _bce_call(p, np.full(1000, -1.0, dtype=np.float32), lw=3.0, gs=1024.0)
    assert same_bits(acc, np.zeros(3)) and bool((bits(dz) == 0).all())
    # mask value -2: -1 is an ordinary label (never "correct"; both logarithms enter its term)
    y2 = y[:1000].copy()
    y2[::3] = -2.0
    assert (y2 == -1.0).sum() > 100
    loss, count, correct, dz_ref = S.bce_ref(p, y2, mask_value=-2.0)
    acc, dz = _bce_call(p, y2, mask_value=-2.0)
    assert acc[1] == count == 1000 - len(y2[::3]) and acc[2] == correct
    assert abs(acc[0] - loss) <= S.bce_loss_bounds(p, y2, mask_value=-2.0)[0]
    assert (np.abs(dz - dz_ref) - S.bce_grad_bound(p, y2, mask_value=-2.0)).max() <= 0.0
    assert not dz[y2 == -2.0].any() and dz[y2 == -1.0].all()


# ============================================================================================================ 5. L2 penalty
def _l2_value(w, lam, out0):
    N_, lib, st = _N()
    out = torch.tensor([out0, SENT], dtype=torch.float64, device="cuda")
    N_.check(lib.orcai_l2_value(N_.ptr(dev(w)), w.size, lam, N_.ptr(out), st), "l2_value")
    o = out.cpu().numpy()
    assert o[1] == SENT
    return float(o[0])


@pytest.mark.parametrize("n", [1, 255, 32767, 32768, 32769, 100003])
def test_l2_value(n):
    """orcai_l2_value around 32768 elements, where l2_value_kernel's 128 blocks take a second pass.  Small integers, lambda = 0.5, onto out = 3:
    every partial sum is an exact integer or half-integer, so the result equals the float64 value bit for bit.  Standard normal weights onto
    out = 0: within n 2^-53 relative of l2_ref (squares of float32 are exact in double; fewer than n additions reach any element)."""
    rng = np.random.default_rng(n)
    wi = rng.integers(-3, 4, n).astype(np.float32)
    assert _l2_value(wi, 0.5, 3.0) == 3.0 + S.l2_ref(wi, 0.5)
    wf = rng.standard_normal(n).astype(np.float32)
    ref = S.l2_ref(wf, 1e-3)
    got = _l2_value(wf, 1e-3, 0.0)
    assert got != 0.0 and abs(got - ref) <= n * S.U64 * ref, (n, got, ref)


L2_SEGMENTS = (1, 16383, 16384, 16385, 70001, 255, 3, 4097)  # around 16384, where l2_values_kernel's 64 blocks per segment take a second pass


@pytest.mark.parametrize("count", [1, 8])
def test_l2_values(count):
    """orcai_l2_values over `count` segments at odd offsets of one buffer (with count = 1 each segment size in turn): the same two comparisons."""
    N_, lib, st = _N()
    rng = np.random.default_rng(count)
    offs, o = [], 1
    for n in L2_SEGMENTS:
        offs.append(o)
        o += n + (2 if (n % 2 == 0) else 1)  # keeps every offset odd
    assert all(x % 2 == 1 for x in offs)
    total = o + 8
    groups = [list(range(8))] if count == 8 else [[i] for i in range(5)]
    for kind, lam, out0 in (("int", 0.5, 3.0), ("float", 1e-3, 0.0)):
        flat = rng.integers(-3, 4, total).astype(np.float32) if kind == "int" else rng.standard_normal(total).astype(np.float32)
        fd = dev(flat)
        for grp in groups:
            off_a = (ctypes.c_int64 * len(grp))(*[offs[i] for i in grp])
            n_a = (ctypes.c_int64 * len(grp))(*[L2_SEGMENTS[i] for i in grp])
            out = torch.tensor([out0, SENT], dtype=torch.float64, device="cuda")
            N_.check(lib.orcai_l2_values(N_.ptr(fd), off_a, n_a, len(grp), lam, N_.ptr(out), st), "l2_values")
            got = out.cpu().numpy()
            assert got[1] == SENT
            sel = np.concatenate([flat[offs[i] : offs[i] + L2_SEGMENTS[i]] for i in grp])
            ref = S.l2_ref(sel, lam)
            if kind == "int":
                assert got[0] == out0 + ref, (grp, got[0], ref)
            else:
                assert got[0] != 0.0 and abs(got[0] - ref) <= sel.size * S.U64 * ref, (grp, got[0], ref)


# ============================================================================================================ 6. Adam
ADAM_N = (1, 255, 256, 257, 70001)
LR, B1, B2, EPS = 1e-3, 0.9, 0.999, 1e-7


@functools.lru_cache(maxsize=None)
def _adam_inputs(n):
    """w standard normal; g and m with magnitudes 1e-6 ... 1; v > 0 over twelve decades (all float32, read-only)."""
    rng = np.random.default_rng(n)
    w = rng.standard_normal(n).astype(np.float32)
    g = (rng.standard_normal(n) * 10.0 ** rng.integers(-6, 1, size=n)).astype(np.float32)
    m = (rng.standard_normal(n) * 10.0 ** rng.integers(-6, 1, size=n)).astype(np.float32)
    v = (rng.standard_normal(n) ** 2 * 10.0 ** rng.integers(-12, 1, size=n)).astype(np.float32) + np.float32(1e-30)
    for a in (w, g, m, v):
        a.setflags(write=False)
    return w, g, m, v


def _adam_run(kind, n, counter, gscale, ok=None):
    """One step by orcai_adam_step (kind "host", step = counter + 1), _dev or _guarded; returns the padded w, m, v as numpy."""
    N_, lib, st = _N()
    w, g, m, v = _adam_inputs(n)
    wd, md, vd, gd = padded(w), padded(m), padded(v), dev(g)
    lr = torch.tensor([LR], dtype=torch.float32, device="cuda")
    c = counter_dev(counter)
    if kind == "host":
        N_.check(lib.orcai_adam_step(N_.ptr(wd), N_.ptr(gd), N_.ptr(md), N_.ptr(vd), n, LR, B1, B2, EPS, counter + 1, gscale, st), "adam_step")
    elif kind == "dev":
        N_.check(lib.orcai_adam_step_dev(N_.ptr(wd), N_.ptr(gd), N_.ptr(md), N_.ptr(vd), n, N_.ptr(lr), B1, B2, EPS, N_.ptr(c), gscale, st), "adam_step_dev")
    else:
        okd = torch.tensor([ok, 777], dtype=torch.int32, device="cuda")
        N_.check(lib.orcai_adam_step_guarded(N_.ptr(wd), N_.ptr(gd), N_.ptr(md), N_.ptr(vd), n, N_.ptr(lr), B1, B2, EPS, N_.ptr(c), gscale, N_.ptr(okd), st),
                 "adam_step_guarded")
        assert okd.tolist() == [ok, 777]
    assert int(c.item()) == counter and same_bits(gd, g)
    return wd.cpu().numpy(), md.cpu().numpy(), vd.cpu().numpy()


@pytest.mark.parametrize("counter", [0, 1, 999, 10**6])
@pytest.mark.parametrize("n", ADAM_N)
def test_adam_three_launchers(n, counter):
    """orcai_adam_step at step = counter + 1, orcai_adam_step_dev and orcai_adam_step_guarded (ok = 1) at `counter`, gscale in {1, 1/1024, 1/3}:
    w, m, v within adam_bounds (gamma_5, gamma_7 and the propagated bound on w) of adam_ref per element; _dev within two such bounds of the
    host-step launcher; _guarded with ok = 1 bit-identical to _dev; with ok = 0 w, m, v keep their bits, sentinels included.  At counter = 10^6
    both powers underflow and alpha = lr."""
    w, g, m, v = _adam_inputs(n)
    tail = np.full(PAD, SENT, np.float32)
    for gscale in (1.0, 1.0 / 1024.0, 1.0 / 3.0):
        ref = S.adam_ref(w, g, m, v, counter, LR, B1, B2, EPS, gscale)
        bounds = S.adam_bounds(w, g, m, v, counter, LR, B1, B2, EPS, gscale)
        host, devr, grd = (_adam_run(k, n, counter, gscale, ok=1) for k in ("host", "dev", "guarded"))
        for name, got_h, got_d, got_g, want, bound in zip("wmv", host, devr, grd, ref, bounds):
            what = (name, n, counter, gscale)
            for got in (got_h, got_d):
                assert same_bits(got[n:], tail), what
                excess = np.abs(got[:n].astype(np.float64) - want) - bound
                assert excess.max() <= 0.0, (what, int(excess.argmax()), float(excess.max()))
            assert (np.abs(got_h[:n].astype(np.float64) - got_d[:n]) - 2.0 * bound).max() <= 0.0, what
            assert same_bits(got_g, got_d), what
            if name != "w":  # the step was applied (w itself may keep its bits where the update is below half an ulp of it)
                assert not same_bits(got_d[:n], m if name == "m" else v), what
        void = _adam_run("guarded", n, counter, gscale, ok=0)
        for got, before in zip(void, (w, m, v)):
            assert same_bits(got, np.concatenate([before, tail])), (n, counter, gscale)


# ============================================================================================================ 7. EMA, counter
@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_ema_update_and_guard(n):
    """moving = moving momentum + batch (1 - momentum) within gamma_3 (|moving| momentum + |batch| (1 - momentum)) of float64; the guarded launcher
    with ok = 1 is bit-identical to the plain one, with ok = 0 it leaves the buffer's bits alone."""
    N_, lib, st = _N()
    rng = np.random.default_rng(n)
    mv, bt = rng.standard_normal(n).astype(np.float32), (rng.standard_normal(n) * 3).astype(np.float32)
    tail = np.full(PAD, SENT, np.float32)
    ref, bound = S.ema_ref(mv, bt, 0.99), S.ema_bound(mv, bt, 0.99)
    btd = dev(bt)
    plain = padded(mv)
    N_.check(lib.orcai_ema_update(N_.ptr(plain), N_.ptr(btd), n, 0.99, st), "ema_update")
    got = plain.cpu().numpy()
    assert same_bits(got[n:], tail) and (np.abs(got[:n].astype(np.float64) - ref) - bound).max() <= 0.0
    assert not same_bits(got[:n], mv)
    for ok in (1, 0):
        okd = torch.tensor([ok], dtype=torch.int32, device="cuda")
        guarded = padded(mv)
        N_.check(lib.orcai_ema_update_guarded(N_.ptr(guarded), N_.ptr(btd), n, 0.99, N_.ptr(okd), st), "ema_update_guarded")
        assert same_bits(guarded, got if ok else np.concatenate([mv, tail])), (n, ok)
        assert okd.item() == ok and same_bits(btd, bt)


@pytest.mark.parametrize("start", [0, 1 << 40])
def test_counter_advance_and_guard(start):
    N_, lib, st = _N()
    c = torch.tensor([start, 4242], dtype=torch.int64, device="cuda")
    N_.check(lib.orcai_counter_advance(N_.ptr(c), st), "counter_advance")
    assert c.tolist() == [start + 1, 4242]
    for ok, want in ((0, start + 1), (1, start + 2), (0, start + 2), (5, start + 3)):  # any non-zero verdict is "ok", as for the other guarded kernels
        okd = torch.tensor([ok], dtype=torch.int32, device="cuda")
        N_.check(lib.orcai_counter_advance_guarded(N_.ptr(c), N_.ptr(okd), st), "counter_advance_guarded")
        assert c.tolist() == [want, 4242] and okd.item() == ok


# ============================================================================================================ 8. the overflow guard
NG = 2 * 262144 + 77  # all_finite_kernel: 1024 blocks of 256 = 262144 floats per pass; three passes, the last one 77 long
G_POS = (0, 63, 64, 255, 256, 262143, 262144, 262145, NG - 1)
BAD = (0x7F800000, 0xFF800000, 0x7FC00000, 0x7F800001)  # +inf, -inf, a quiet NaN, a signalling NaN with the smallest payload
FLT_MAX, FLT_MIN = np.float32(3.4028234663852886e38), np.float32(1.1754943508222875e-38)


@functools.lru_cache(maxsize=None)
def _clean(n, seed):
    """Finite float32 with +-FLT_MAX, +-0 and the smallest normal at both ends (the largest finite exponent must not count as non-finite)."""
    a = np.random.default_rng(seed).standard_normal(n).astype(np.float32)
    edge = np.array([FLT_MAX, -FLT_MAX, 0.0, -0.0, FLT_MIN, -FLT_MIN], dtype=np.float32)
    k = min(n, edge.size)
    a[:k] = edge[:k]
    if n > 2 * edge.size:
        a[-edge.size :] = edge
    a.setflags(write=False)
    return a


def _step_ok(g, stats, ns, ok0, skipped0):
    N_, lib, st = _N()
    ok = torch.tensor([ok0, 777], dtype=torch.int32, device="cuda")
    skipped = torch.tensor([skipped0, 4242], dtype=torch.int64, device="cuda")
    N_.check(lib.orcai_step_ok(N_.ptr(g), NG, N_.ptr(stats) if ns else None, ns, N_.ptr(ok), N_.ptr(skipped), st), "step_ok")
    ok, skipped = ok.tolist(), skipped.tolist()
    assert ok[1] == 777 and skipped[1] == 4242
    return ok[0], skipped[0]


@pytest.mark.parametrize("ns", [0, 300, 262144 + 5])
def test_step_ok_finds_every_position(ns):
    """orcai_step_ok over ng = 2 x 262144 + 77 gradient values and ns statistics (0 with stats = NULL, 300, 262144 + 5: a second pass).  Clean
    buffers (with +-FLT_MAX, +-0, the smallest normal) give ok = 1 over a stale 0 and leave `skipped` alone; one +inf, -inf, quiet or signalling
    NaN at any of G_POS (first and last lane of a wavefront, of a block, of a pass, the last element) or at the first or last statistic gives
    ok = 0 and skipped + 1; g and stats keep their bits.  orcai_poison_if_nonfinite on the same statistics sets g[0] to NaN and nothing else,
    and writes nothing when they are clean."""
    N_, lib, st = _N()
    g_clean = _clean(NG, 1)
    g = padded(g_clean)
    gi = g.view(torch.int32)
    s_clean = _clean(ns, 2) if ns else None
    stats = padded(s_clean) if ns else None
    si = stats.view(torch.int32) if ns else None
    g_bits, s_bits = bits(g), bits(stats) if ns else None
    for stale in (0, 1):
        assert _step_ok(g, stats, ns, stale, 5) == (1, 5)

    def to_i32(b):
        return b - (1 << 32) if b >= 1 << 31 else b

    cases = [(gi, g_bits, pos) for pos in G_POS] + ([(si, s_bits, pos) for pos in (0, ns - 1)] if ns else [])
    for view, clean_bits, pos in cases:
        for bad in BAD:
            view[pos] = to_i32(bad)
            assert _step_ok(g, stats, ns, 1, 5) == (0, 6), (ns, view is gi, pos, hex(bad))
            expect = clean_bits.copy()
            expect[pos] = bad
            assert np.array_equal(bits(g if view is gi else stats), expect), (ns, pos, hex(bad))  # read only: even a signalling NaN keeps its payload
            if view is si:
                g2 = padded(g_clean)
                N_.check(lib.orcai_poison_if_nonfinite(N_.ptr(stats), ns, N_.ptr(g2), st), "poison_if_nonfinite")
                got = g2.cpu().numpy()
                assert math.isnan(got[0]) and np.array_equal(bits(got)[1:], g_bits[1:]), (ns, pos, hex(bad))
            view[pos] = int(clean_bits.view(np.int32)[pos])
    assert np.array_equal(bits(g), g_bits) and (not ns or np.array_equal(bits(stats), s_bits))
    assert _step_ok(g, stats, ns, 0, 5) == (1, 5)  # and clean again
    if ns:
        N_.check(lib.orcai_poison_if_nonfinite(N_.ptr(stats), ns, N_.ptr(g), st), "poison_if_nonfinite")
        assert np.array_equal(bits(g), g_bits)


# ============================================================================================================ 9. refused arguments
def test_refused_arguments_launch_nothing():
    """Null pointers, n <= 0, a grad_scale that is 0, negative or NaN, step < 1, f16 pointers off 16-byte alignment, count outside 1...8, a negative
    offset: ORCAI_E_BADARG from every launcher above, and every output keeps its sentinel."""
    N_, lib, st = _N()
    BA = N_.E_BADARG
    n = 64
    out = torch.full((n,), SENT, device="cuda")
    m_, v_ = torch.full((n,), SENT, device="cuda"), torch.full((n,), SENT, device="cuda")
    outh = torch.full((n,), SENT, dtype=torch.float16, device="cuda")
    src, src2 = torch.ones(n, device="cuda"), torch.ones(n, device="cuda")
    srch, srch2 = torch.ones(n, dtype=torch.float16, device="cuda"), torch.ones(n, dtype=torch.float16, device="cuda")
    acc = torch.full((4,), SENT, dtype=torch.float64, device="cuda")
    c = torch.tensor([3], dtype=torch.int64, device="cuda")
    ok = torch.tensor([1], dtype=torch.int32, device="cuda")
    sk = torch.tensor([9], dtype=torch.int64, device="cuda")
    lr = torch.tensor([LR], dtype=torch.float32, device="cuda")
    o, mm, vv, oh, s, s2, sh, sh2, a, cp, okp, skp, lrp = (N_.ptr(t) for t in (out, m_, v_, outh, src, src2, srch, srch2, acc, c, ok, sk, lr))
    u64 = ctypes.c_uint64

    def each_null(fn, args, pointer_slots):
        """fn refuses every argument list with one of its pointers replaced by NULL."""
        for i in pointer_slots:
            assert fn(*[None if j == i else x for j, x in enumerate(args)]) == BA, (fn.__name__, i)

    def each_n(fn, args, slot):
        for bad in (0, -1):
            assert fn(*[bad if j == slot else x for j, x in enumerate(args)]) == BA, (fn.__name__, bad)

    each_null(lib.orcai_dropout_mask, (o, n, u64(1), 0.5, st), [0])
    each_n(lib.orcai_dropout_mask, (o, n, u64(1), 0.5, st), 1)
    for fn, dst in ((lib.orcai_dropout_mask_dev, o), (lib.orcai_h_dropout_mask_dev, oh)):
        each_null(fn, (dst, n, cp, u64(1), 0.5, st), [0, 2])
        each_n(fn, (dst, n, cp, u64(1), 0.5, st), 1)
    assert lib.orcai_h_dropout_mask_dev(oh + 2, n - 1, cp, u64(1), 0.5, st) == BA
    for fn, x, k, y in ((lib.orcai_mask_scale, s, s2, o), (lib.orcai_h_mask_scale, sh, sh2, oh)):
        each_null(fn, (x, k, 2.0, n, y, st), [0, 1, 4])
        each_n(fn, (x, k, 2.0, n, y, st), 3)
    for args in ((sh + 2, sh2, 2.0, n - 1, oh, st), (sh, sh2 + 2, 2.0, n - 1, oh, st), (sh, sh2, 2.0, n - 1, oh + 2, st)):
        assert lib.orcai_h_mask_scale(*args) == BA
    each_null(lib.orcai_relu_bwd, (s, s2, n, o, st), [0, 1, 3])
    each_n(lib.orcai_relu_bwd, (s, s2, n, o, st), 2)
    each_null(lib.orcai_masked_bce, (s, s2, n, -1.0, a, o, st), [0, 1, 4])
    each_n(lib.orcai_masked_bce, (s, s2, n, -1.0, a, o, st), 2)
    each_null(lib.orcai_masked_bce_w, (s, s2, n, -1.0, a, o, lrp, 1.0, st), [0, 1, 4])
    each_n(lib.orcai_masked_bce_w, (s, s2, n, -1.0, a, o, lrp, 1.0, st), 2)
    for gs in (0.0, -1.0, float("nan")):
        assert lib.orcai_masked_bce_w(s, s2, n, -1.0, a, o, lrp, gs, st) == BA, gs
    each_null(lib.orcai_l2_value, (s, n, 0.5, a, st), [0, 3])
    each_n(lib.orcai_l2_value, (s, n, 0.5, a, st), 1)
    i64x9 = ctypes.c_int64 * 9
    offs, cnts = i64x9(*range(9)), i64x9(*([4] * 9))
    each_null(lib.orcai_l2_values, (s, offs, cnts, 2, 0.5, a, st), [0, 1, 2, 5])
    for count in (0, -1, 9):
        assert lib.orcai_l2_values(s, offs, cnts, count, 0.5, a, st) == BA, count
    assert lib.orcai_l2_values(s, i64x9(0, -1), cnts, 2, 0.5, a, st) == BA
    assert lib.orcai_l2_values(s, offs, i64x9(4, 0), 2, 0.5, a, st) == BA and lib.orcai_l2_values(s, offs, i64x9(4, -3), 2, 0.5, a, st) == BA
    adam = (o, s, mm, vv, n, LR, B1, B2, EPS, 1, 1.0, st)
    each_null(lib.orcai_adam_step, adam, [0, 1, 2, 3])
    each_n(lib.orcai_adam_step, adam, 4)
    each_n(lib.orcai_adam_step, adam, 9)  # step < 1
    adam_dev = (o, s, mm, vv, n, lrp, B1, B2, EPS, cp, 1.0, st)
    each_null(lib.orcai_adam_step_dev, adam_dev, [0, 1, 2, 3, 5, 9])
    each_n(lib.orcai_adam_step_dev, adam_dev, 4)
    adam_g = (o, s, mm, vv, n, lrp, B1, B2, EPS, cp, 1.0, okp, st)
    each_null(lib.orcai_adam_step_guarded, adam_g, [0, 1, 2, 3, 5, 9, 11])
    each_n(lib.orcai_adam_step_guarded, adam_g, 4)
    each_null(lib.orcai_ema_update, (o, s, n, 0.99, st), [0, 1])
    each_n(lib.orcai_ema_update, (o, s, n, 0.99, st), 2)
    each_null(lib.orcai_ema_update_guarded, (o, s, n, 0.99, okp, st), [0, 1, 4])
    each_n(lib.orcai_ema_update_guarded, (o, s, n, 0.99, okp, st), 2)
    assert lib.orcai_counter_advance(None, st) == BA
    each_null(lib.orcai_counter_advance_guarded, (cp, okp, st), [0, 1])
    each_null(lib.orcai_step_ok, (s, n, s2, n, okp, skp, st), [0, 2, 4, 5])
    each_n(lib.orcai_step_ok, (s, n, s2, n, okp, skp, st), 1)
    assert lib.orcai_step_ok(s, n, s2, -1, okp, skp, st) == BA
    each_null(lib.orcai_poison_if_nonfinite, (s, n, o, st), [0, 2])
    each_n(lib.orcai_poison_if_nonfinite, (s, n, o, st), 1)

    torch.cuda.synchronize()
    for t in (out, m_, v_, outh, acc):
        assert bool((t == SENT).all())
    assert bool((src == 1).all()) and bool((src2 == 1).all()) and bool((srch == 1).all()) and bool((srch2 == 1).all())
    assert c.item() == 3 and ok.item() == 1 and sk.item() == 9
    # the same arguments, valid: the launchers do run
    assert lib.orcai_dropout_mask(o, n, u64(1), 1.0, st) == 0 and bool((out == 1).all())
    assert lib.orcai_h_mask_scale(sh, sh2, 2.0, n, oh, st) == 0 and bool((outh == 2).all())
