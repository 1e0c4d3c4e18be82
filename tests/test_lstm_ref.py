"""tests/lstm_ref.py on the CPU: the float64 backward against torch autograd, the teacher-forced f16 references against a float32 emulation of
the f16 kernels (a stand-in device), the subnormal-flush switch, and the saturating forward case with the shape tables the GPU modules share."""

import numpy as np
import pytest

from lstm_ref import (
    HOT_LEVEL,
    LSTM_BWD_CASES,
    LSTM_FWD_SHAPES,
    LSTM_HOT_SHAPE,
    LSTM_HOT_WIDTHS,
    LSTM_WIDTHS,
    _bwd_ref,
    _fwd_ref,
    _gates,
    bwd_ref_f16,
    f16_ties,
    fwd_ref_f16,
    lstm_inputs_bwd,
    lstm_inputs_fwd,
    lstm_inputs_fwd_hot,
    round_f16,
)

f32 = np.float32


def _sig32(a):
    return (f32(1) / (f32(1) + np.exp(-a))).astype(f32)


def _emu_fwd_f16(xz, Uw):
    """lstm_train_fwd_h_kernel in float32 numpy: the product f16(h) f16(U) accumulated in f32 on the f32 input projection, gates, cell state and
    the stored tensors in f32.  (f16 x f16 products are exact in f32, as in the MFMA.)"""
    B, Tn, _, U4 = xz.shape
    U = U4 // 4
    h, g, c = np.zeros((B, Tn, 2 * U), f32), np.zeros((B, Tn, 2, 4 * U), f32), np.zeros((B, Tn, 2, U), f32)
    for d in range(2):
        hh, cc = np.zeros((B, U), f32), np.zeros((B, U), f32)
        W = Uw[d].astype(np.float16).astype(f32)
        for step in range(Tn):
            t = Tn - 1 - step if d else step
            zz = (xz[:, t, d] + hh.astype(np.float16).astype(f32) @ W).astype(f32).reshape(B, U // 8, 4, 8)
            i_, f_, g_, o_ = _sig32(zz[:, :, 0]), _sig32(zz[:, :, 1]), np.tanh(zz[:, :, 2]), _sig32(zz[:, :, 3])
            cc = (f_ * cc.reshape(B, U // 8, 8) + i_ * g_).reshape(B, U)
            hh = (o_ * np.tanh(cc.reshape(B, U // 8, 8))).reshape(B, U)
            h[:, t, d * U : (d + 1) * U], c[:, t, d] = hh, cc
            g[:, t, d] = np.stack([i_, f_, g_, o_], axis=2).reshape(B, 4 * U)
    assert h.dtype == g.dtype == c.dtype == f32
    return h, g, c


def _emu_bwd_f16(dH, gates, cst, Uw):
    """lstm_bwd_h_kernel in float32 numpy: dz in f32, the recurrent term f16(dz) f16(U)^T accumulated in f32."""
    B, Tn, _, U4 = gates.shape
    U = U4 // 4
    dxz = np.zeros((B, Tn, 2, 4 * U), f32)
    for d in range(2):
        W = Uw[d].astype(np.float16).astype(f32)
        dc, dhr = np.zeros((B, U), f32), np.zeros((B, U), f32)
        for step in range(Tn):
            t = step if d else Tn - 1 - step
            tp = t + 1 if d else t - 1
            gv = gates[:, t, d].reshape(B, U // 8, 4, 8)
            i_, f_, g_, o_ = (gv[:, :, q].reshape(B, U) for q in range(4))
            c = cst[:, t, d]
            cp = cst[:, tp, d] if 0 <= tp < Tn else np.zeros((B, U), f32)
            dh = dH[:, t, d * U : (d + 1) * U] + dhr
            tc = np.tanh(c)
            dct = dc + dh * o_ * (1 - tc * tc)
            dc = dct * f_
            dz = np.stack([dct * g_ * i_ * (1 - i_), dct * cp * f_ * (1 - f_), dct * i_ * (1 - g_ * g_), dh * tc * o_ * (1 - o_)], axis=1)
            dz = dz.reshape(B, 4, U // 8, 8).transpose(0, 2, 1, 3).reshape(B, 4 * U)
            assert dz.dtype == f32
            dxz[:, t, d] = dz
            dhr = dz.astype(np.float16).astype(f32) @ W.T
    return dxz


def test_bwd_ref_is_the_gradient_of_fwd_ref():
    """_bwd_ref against torch float64 autograd through a plain-torch _fwd_ref (U = 32, B = 3, T = 5): 1e-12 of the largest dxz."""
    torch = pytest.importorskip("torch")
    U, B, Tn = 32, 3, 5
    rng = np.random.default_rng(1)
    xz, Uw = lstm_inputs_fwd(rng, U, B, Tn)
    dH = rng.standard_normal((B, Tn, 2 * U))
    xt = torch.tensor(xz, dtype=torch.float64, requires_grad=True)
    Ut = torch.tensor(Uw, dtype=torch.float64)
    rows = [[None] * Tn for _ in range(2)]
    for d in range(2):
        hh, cc = torch.zeros(B, U, dtype=torch.float64), torch.zeros(B, U // 8, 8, dtype=torch.float64)
        for step in range(Tn):
            t = Tn - 1 - step if d else step
            zz = (xt[:, t, d] + hh @ Ut[d]).reshape(B, U // 8, 4, 8)
            cc = torch.sigmoid(zz[:, :, 1]) * cc + torch.sigmoid(zz[:, :, 0]) * torch.tanh(zz[:, :, 2])
            hh = (torch.sigmoid(zz[:, :, 3]) * torch.tanh(cc)).reshape(B, U)
            rows[d][t] = hh
    h = torch.stack([torch.cat([rows[0][t], rows[1][t]], dim=1) for t in range(Tn)], dim=1)
    href, gref, cref = _fwd_ref(xz, Uw)
    assert np.abs(h.detach().numpy() - href).max() <= 1e-14
    (h * torch.tensor(dH)).sum().backward()
    want = xt.grad.numpy()
    got = _bwd_ref(dH, gref, cref, Uw)
    err = float(np.abs(got - want).max() / np.abs(want).max())
    print(f"_bwd_ref vs autograd: {err:.1e}")
    assert err <= 1e-12


@pytest.mark.parametrize("U,B,Tn", [(64, 20, 46), (128, 17, 9)])
def test_forced_references_agree_with_a_float32_emulation(U, B, Tn):
    """The float32 emulation of the f16 kernels as a stand-in device: the teacher-forced references reproduce it within 1e-6 (h, gates, c) and
    1e-6 of max |dxz|, where the free-running reference is off by an f16 rounding flip (> 1e-5)."""
    rng = np.random.default_rng(U + B + Tn)
    xz, Uw = lstm_inputs_fwd(rng, U, B, Tn)
    dev = _emu_fwd_f16(xz, Uw)
    forced = fwd_ref_f16(xz, Uw, h_forced=dev[0])
    free = fwd_ref_f16(xz, Uw)
    errs = [float(np.abs(a - b).max()) for a, b in zip(dev, forced)]
    errs_free = [float(np.abs(a - b).max()) for a, b in zip(dev, free)]
    print(f"U {U} B {B} T {Tn}: emulation vs forced {errs}, vs free-running {errs_free}")
    assert max(errs) <= 1e-6, errs
    dH, gates, cst, Uw = lstm_inputs_bwd(rng, U, B, Tn, 0.1)
    dxz = _emu_bwd_f16(dH, gates, cst, Uw)
    ref = bwd_ref_f16(dH, gates, cst, Uw, dxz_forced=dxz)
    err = float(np.abs(dxz - ref).max() / np.abs(ref).max())
    err_free = float(np.abs(dxz - bwd_ref_f16(dH, gates, cst, Uw)).max() / np.abs(ref).max())
    print(f"backward: emulation vs forced {err:.1e}, vs free-running {err_free:.1e} of max |dxz|")
    assert err <= 1e-6, err


def test_forced_reference_uses_the_forced_operand_only():
    """Teacher forcing replaces the operand, nothing else: forcing a reference's own h (or dxz) gives that reference back up to the f16
    rounding of float64 vs f32 storage, and a T = 1 sequence ignores the forced tensor."""
    rng = np.random.default_rng(5)
    xz, Uw = lstm_inputs_fwd(rng, 32, 3, 1)
    a, b = fwd_ref_f16(xz, Uw), fwd_ref_f16(xz, Uw, h_forced=np.full((3, 1, 64), 9.0, f32))
    assert all(np.array_equal(x, y) for x, y in zip(a, b)) and all(np.array_equal(x, y) for x, y in zip(a, _fwd_ref(xz, Uw)))
    xz, Uw = lstm_inputs_fwd(rng, 32, 3, 4)
    free = fwd_ref_f16(xz, Uw)
    again = fwd_ref_f16(xz, Uw, h_forced=free[0])  # float64 in: the same roundings
    assert all(np.array_equal(x, y) for x, y in zip(free, again))


def _no_subnormal(a):
    """a with every magnitude at least 1e-3 (far from the f16 subnormal range and from zero)."""
    return (np.where(a < 0, -1.0, 1.0) * np.maximum(np.abs(a), 1e-3)).astype(f32)


def test_flush_switch_forward():
    U, B, Tn = 32, 3, 4
    rng = np.random.default_rng(7)
    xz, Uw = lstm_inputs_fwd(rng, U, B, Tn)
    Uw = _no_subnormal(Uw)
    hf = _no_subnormal(np.tanh(rng.standard_normal((B, Tn, 2 * U))))
    keep, flush = fwd_ref_f16(xz, Uw, h_forced=hf), fwd_ref_f16(xz, Uw, h_forced=hf, flush=True)
    assert all(np.array_equal(a, b) for a, b in zip(keep, flush))  # no operand is subnormal: the switch changes nothing
    hf[1, 2, 5] = 3.0e-5  # subnormal in f16 (2^-15 < 2^-14), not zero: read by direction 0 at t = 3
    assert round_f16(hf[1, 2, 5]) != 0.0 and round_f16(hf[1, 2, 5], flush=True) == 0.0
    keep, flush = fwd_ref_f16(xz, Uw, h_forced=hf), fwd_ref_f16(xz, Uw, h_forced=hf, flush=True)
    diff = np.abs(keep[0] - flush[0])
    assert diff[1, 3, :U].max() > 0.0
    diff[1, 3, :U] = 0.0
    assert not diff.any()  # and nowhere else
    # a subnormal element of U
    Uw[1, 4, 9] = 2.0e-5
    hf[1, 2, 5] = 0.25
    keep, flush = fwd_ref_f16(xz, Uw, h_forced=hf), fwd_ref_f16(xz, Uw, h_forced=hf, flush=True)
    assert np.abs(keep[1] - flush[1])[:, :, 1, 9].max() > 0.0 and np.array_equal(keep[1][:, :, 0], flush[1][:, :, 0])


def test_flush_switch_backward():
    U, B, Tn = 32, 3, 4
    rng = np.random.default_rng(8)
    dH, gates, cst, Uw = lstm_inputs_bwd(rng, U, B, Tn, 0.1)
    Uw = _no_subnormal(Uw)
    zf = _no_subnormal(0.1 * rng.standard_normal((B, Tn, 2, 4 * U)))
    keep, flush = bwd_ref_f16(dH, gates, cst, Uw, dxz_forced=zf), bwd_ref_f16(dH, gates, cst, Uw, dxz_forced=zf, flush=True)
    assert np.array_equal(keep, flush)
    zf[2, 1, 0, 17] = -4.0e-5  # f16-subnormal dz of direction 0 at t = 1: enters the step at t = 0
    keep, flush = bwd_ref_f16(dH, gates, cst, Uw, dxz_forced=zf), bwd_ref_f16(dH, gates, cst, Uw, dxz_forced=zf, flush=True)
    diff = np.abs(keep - flush)
    assert diff[2, 0, 0].max() > 0.0
    diff[2, 0, 0] = 0.0
    assert not diff.any()
    # free-running at a gradient scale whose dz is mostly f16-subnormal: the two variants part
    dH, gates, cst, Uw = lstm_inputs_bwd(rng, U, B, Tn, 1e-4)
    keep, flush = bwd_ref_f16(dH, gates, cst, Uw), bwd_ref_f16(dH, gates, cst, Uw, flush=True)
    assert np.abs(keep - flush).max() > 5e-6 * np.abs(keep).max()


def test_f16_midpoints_are_found_and_resolved_from_the_next_step():
    """f16_ties marks exactly the f32 values halfway between two f16 numbers (normal and subnormal range) and names the other neighbour; a
    teacher-forced reference given the next step's tensor of a device that took that other neighbour reproduces the device, forward and backward."""
    x = np.array([0.107574462890625, -0.077484130859375, 0.1075439453125, 0.3, 2.0**-24 * 2.5, 0.0], f32)  # two midpoints, an f16 number, a generic value, a subnormal midpoint, zero
    mask, other = f16_ties(x)
    assert mask.tolist() == [True, True, False, False, True, False]
    for v, r, o in zip(x[mask], round_f16(x)[mask], other[mask]):
        assert o != r and abs(o - v) == abs(r - v) and float(np.float16(o)) == o
    assert f16_ties(x, flush=True)[1][4] == 0.0
    U, B, Tn = 32, 3, 2
    rng = np.random.default_rng(12)
    xz, Uw = lstm_inputs_fwd(rng, U, B, Tn)
    hf = np.tanh(rng.standard_normal((B, Tn, 2 * U))).astype(f32)
    hf[1, 0, 7] = x[0]
    op = round_f16(hf[:, 0, :U])
    op[1, 7] = f16_ties(hf[:, 0, :U])[1][1, 7]  # the device took the other neighbour
    zz = (xz[:, 1, 0].astype(np.float64) + op @ round_f16(Uw[0])).reshape(B, U // 8, 4, 8)
    dev_gates = np.zeros((B, Tn, 2, 4 * U))
    dev_gates[:, 1, 0] = np.stack([1 / (1 + np.exp(-zz[:, :, 0])), 1 / (1 + np.exp(-zz[:, :, 1])), np.tanh(zz[:, :, 2]), 1 / (1 + np.exp(-zz[:, :, 3]))], axis=2).reshape(B, 4 * U)
    plain, hinted = fwd_ref_f16(xz, Uw, h_forced=hf), fwd_ref_f16(xz, Uw, h_forced=hf, gates_forced=dev_gates)
    assert np.abs(plain[1][:, 1, 0] - dev_gates[:, 1, 0]).max() > 1e-6 and np.abs(hinted[1][:, 1, 0] - dev_gates[:, 1, 0]).max() <= 1e-14
    dH, gates, cst, Uw = lstm_inputs_bwd(rng, U, B, Tn, 0.1)
    dev = bwd_ref_f16(dH, gates, cst, Uw)
    dev[2, 1, 0, 40] = x[1]  # direction 0 runs t = 1 then t = 0: a midpoint in the stored dz of t = 1 ...
    op = round_f16(dev[:, 1, 0].astype(f32))
    op[2, 40] = f16_ties(dev[:, 1, 0].astype(f32))[1][2, 40]
    forced = dev.astype(f32)
    shifted = forced.copy()
    shifted[2, 1, 0, 40] = op[2, 40]  # ... whose other neighbour the device used: the reference forced with that operand is the device's t = 0
    forced[:, 0, 0] = bwd_ref_f16(dH, gates, cst, Uw, dxz_forced=shifted)[:, 0, 0].astype(f32)
    plain, hinted = bwd_ref_f16(dH, gates, cst, Uw, dxz_forced=forced), bwd_ref_f16(dH, gates, cst, Uw, dxz_forced=forced, ties=True)
    scale = np.abs(forced).max()
    assert np.abs(plain - forced)[2, 0, 0].max() > 1e-5 * scale and np.abs(hinted - forced)[:, 0, 0].max() <= 1e-6 * scale


def test_shared_shape_tables():
    """The tables tests/test_lstm_f32_gpu.py is parametrised by: every width the launchers accept, T = 1 and T = 2, B = 1 and B at 15, 16, 17."""
    assert LSTM_WIDTHS == tuple(range(32, 257, 32))
    for shapes in (LSTM_FWD_SHAPES, [c[:2] for c in LSTM_BWD_CASES]):
        assert {1, 2} <= {t for _, t in shapes} and {1, 15, 16, 17} <= {b for b, _ in shapes}
    assert [c for c in LSTM_BWD_CASES if c[2] == 0.0] and set(LSTM_HOT_WIDTHS) <= set(LSTM_WIDTHS)


@pytest.mark.parametrize("U", LSTM_HOT_WIDTHS)
def test_hot_forward_inputs_saturate_and_grow(U):
    """lstm_inputs_fwd_hot: Uw and the odd rows past 3 are lstm_inputs_fwd's; the float64 reference stays finite without an overflow (|z| far
    below 700); row 1's cell state ends above T - 1 and row 3's below -(T - 1) in the forward direction; and the even rows really saturate."""
    B, Tn = LSTM_HOT_SHAPE
    xz, Uw = lstm_inputs_fwd_hot(np.random.default_rng(U), U, B, Tn)
    plain_xz, plain_Uw = lstm_inputs_fwd(np.random.default_rng(U), U, B, Tn)
    assert xz.dtype == Uw.dtype == f32 and np.array_equal(Uw, plain_Uw) and np.array_equal(xz[5::2], plain_xz[5::2])
    assert np.array_equal(xz[0::2], plain_xz[0::2] * f32(30.0))
    for row, g_level in ((1, HOT_LEVEL), (3, -HOT_LEVEL)):  # through the reader of the layout, not by index: sigmoid / tanh of the levels
        i_, f_, g_, o_ = _gates(xz[row].reshape(Tn * 2, 4 * U).astype(np.float64))
        s = 1.0 / (1.0 + np.exp(-HOT_LEVEL))
        assert (i_ == s).all() and (f_ == s).all() and (o_ == s).all() and (g_ == np.tanh(g_level)).all()
    zmax = float(np.abs(xz).max() + np.abs(Uw).sum(axis=1).max())  # |h| <= 1
    assert zmax < 350.0, zmax
    with np.errstate(over="raise", invalid="raise", divide="raise"):
        h, g, c = _fwd_ref(xz, Uw)
    assert all(np.isfinite(a).all() for a in (h, g, c))
    assert c[1, Tn - 1, 0].min() > Tn - 1 and c[3, Tn - 1, 0].max() < -(Tn - 1)
    ge = g[0::2].reshape(-1, Tn, 2, U // 8, 4, 8)
    lo, hi = 1e-4, 1.0 - 1e-4
    sat = np.concatenate([((ge[..., q, :] < lo) | (ge[..., q, :] > hi)).ravel() for q in (0, 1, 3)] + [(np.abs(ge[..., 2, :]) > hi).ravel()])
    print(f"U {U}: {sat.mean():.2f} of the even rows' gate activations are saturated, max |c| {np.abs(c).max():.1f}, bound on |z| {zmax:.0f}")
    assert sat.mean() >= 0.25
