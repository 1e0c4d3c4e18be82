"""The f32 path's LSTM recurrences through the C ABI, one launcher at a time, against float64 (tests/lstm_ref.py) -- every width 32..256, both
orcai_lstm_split settings, and the batch / time edges of kernels that work on 16-row tiles, double-buffer on step & 1 and prefetch step + 1:
  orcai_lstm_recurrent   lstm_kernel / lstm_split_kernel<32|64|96|128>, lstm_wide_fwd_kernel<160|192|224|256, false>
  orcai_lstm_train_fwd   lstm_train_fwd_kernel / lstm_train_fwd_split_kernel<...>, lstm_wide_fwd_kernel<..., true>
  orcai_lstm_bwd         lstm_bwd_kernel / lstm_bwd_split_kernel<...> (with lstm_grad_max / lstm_grad_scale), lstm_wide_bwd_kernel<...>
Bars: 1e-5 absolute on h, gates and cell state, 5e-6 of max |dxz| on the backward -- the f32 bars of tests/test_head_widths_gpu.py.  Every output
buffer has one extra batch row of -7.0 that must survive, everything written is finite, and every launch is repeated and gives the same bytes
(no recurrence kernel uses atomics).  Above 128 units both split settings run one kernel: the same bytes.  The module prints, per width, the
largest forward and backward error it saw."""

import contextlib
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from lstm_ref import (  # noqa: E402
    LSTM_BWD_CASES,
    LSTM_FWD_SHAPES,
    LSTM_HOT_SHAPE,
    LSTM_HOT_WIDTHS,
    LSTM_WIDTHS,
    _bwd_ref,
    _fwd_ref,
    lstm_inputs_bwd,
    lstm_inputs_fwd,
    lstm_inputs_fwd_hot,
)

SENT = -7.0
FWD_BAR, BWD_BAR = 1e-5, 5e-6
RECURRENT, TRAIN_FWD, BWD = "orcai_lstm_recurrent", "orcai_lstm_train_fwd", "orcai_lstm_bwd"
WIDE = tuple(u for u in LSTM_WIDTHS if u > 128)
_MAXIMA = {}  # (what, U) -> the largest error against float64 over the cases that ran


@pytest.fixture(scope="module", autouse=True)
def _report_maxima():
    yield
    for what in ("forward", "forward, saturating", "backward"):
        for U in LSTM_WIDTHS:
            if (what, U) in _MAXIMA:
                print(f"f32 LSTM {what}, U {U}: largest error against float64 {_MAXIMA[what, U]:.2e}")


def _record(what, U, err):
    _MAXIMA[what, U] = max(_MAXIMA.get((what, U), 0.0), err)


@contextlib.contextmanager
def _split(on):
    from orcai_amd import _native as N

    lib = N.lib()
    prev = lib.orcai_lstm_split(-1)
    try:
        lib.orcai_lstm_split(on)
        yield
    finally:
        lib.orcai_lstm_split(prev)


def _dev(a):
    return torch.tensor(a, device="cuda")  # a copy: the shared host arrays stay as they are


def _sentinel(*shape):
    return torch.full(shape, SENT, device="cuda")


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=2)
def _fwd_case(U, B, Tn, hot=False):
    """Inputs and float64 reference of one forward case, computed once for the entries and split settings that share it."""
    xz, Uw = (lstm_inputs_fwd_hot if hot else lstm_inputs_fwd)(np.random.default_rng(3000 + U + 7 * B + 1000 * Tn), U, B, Tn)
    return _frozen(xz, Uw, *_fwd_ref(xz, Uw))


@functools.lru_cache(maxsize=2)
def _bwd_case(U, B, Tn, gscale):
    inputs = lstm_inputs_bwd(np.random.default_rng(4000 + U + 7 * B + 1000 * Tn), U, B, Tn, gscale)
    return _frozen(*inputs, _bwd_ref(*inputs))


def _bits(a):
    return a.view(np.uint32)


def _same_bytes(xs, ys):
    return all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(xs, ys))


def _run_fwd(entry, xd, ud, B, Tn, U):
    """One launch of a forward entry into sentinel-filled buffers of B + 1 batch rows: (h,) of the inference entry, (h, gates, c) of the others."""
    from orcai_amd import _native as N

    outs = [_sentinel(B + 1, Tn, 2 * U)]
    if entry != RECURRENT:
        outs += [_sentinel(B + 1, Tn, 2, 4 * U), _sentinel(B + 1, Tn, 2, U)]
    N.check(getattr(N.lib(), entry)(N.ptr(xd), N.ptr(ud), B, Tn, U, *(N.ptr(o) for o in outs), N.stream_ptr()), entry)
    torch.cuda.synchronize()
    return tuple(o.cpu().numpy() for o in outs)


def _run_bwd(entry, hd, gd, cd, ud, B, Tn, U):
    from orcai_amd import _native as N

    dxz = _sentinel(B + 1, Tn, 2, 4 * U)
    N.check(getattr(N.lib(), entry)(N.ptr(hd), N.ptr(gd), N.ptr(cd), N.ptr(ud), B, Tn, U, N.ptr(dxz), N.stream_ptr()), entry)
    torch.cuda.synchronize()
    return dxz.cpu().numpy()


def _written(arrays, B):
    """Nothing past the last batch row, everything before it finite; the live rows."""
    for a in arrays:
        assert (a[B] == SENT).all()
        assert np.isfinite(a[:B]).all()
    return tuple(a[:B] for a in arrays)


def _forward(U, B, Tn, entry, split, hot):
    xz, Uw, *ref = _fwd_case(U, B, Tn, hot)
    xd, ud = _dev(xz), _dev(Uw)
    with _split(split):
        first, again = _run_fwd(entry, xd, ud, B, Tn, U), _run_fwd(entry, xd, ud, B, Tn, U)
        train = first if entry == TRAIN_FWD else _run_fwd(TRAIN_FWD, xd, ud, B, Tn, U)
    assert _same_bytes(first, again)  # launched twice: the same bytes
    if U > 128 and split == 1:  # one kernel for both settings
        with _split(0):
            assert _same_bytes(first, _run_fwd(entry, xd, ud, B, Tn, U))
    got, train = _written(first, B), _written(train, B)
    return got, train, ref


# ------------------------------------------------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize("split", [0, 1])
@pytest.mark.parametrize("entry", [RECURRENT, TRAIN_FWD])
@pytest.mark.parametrize("B,Tn", LSTM_FWD_SHAPES)
@pytest.mark.parametrize("U", LSTM_WIDTHS)
def test_lstm_forward_vs_float64(U, B, Tn, entry, split):
    """h (and gates and cell state of the training entry) within 1e-5 of the float64 recurrence; the inference entry's h against the training
    entry's: within 1e-6 up to 128 units, the same array above (one kernel body for both)."""
    got, train, ref = _forward(U, B, Tn, entry, split, hot=False)
    errs = [float(np.abs(a - b).max()) for a, b in zip(got, ref)]
    print(f"{entry} U {U} B {B} T {Tn} split {split}: max |{'h, gates, c' if len(errs) == 3 else 'h'} - float64| = {errs}")
    _record("forward", U, max(errs))
    assert max(errs) <= FWD_BAR, errs
    if entry == RECURRENT:
        if U <= 128:
            assert np.abs(got[0] - train[0]).max() <= 1e-6
        else:
            assert np.array_equal(got[0], train[0])


@pytest.mark.parametrize("split", [0, 1])
@pytest.mark.parametrize("entry", [RECURRENT, TRAIN_FWD])
@pytest.mark.parametrize("U", LSTM_HOT_WIDTHS)
def test_lstm_forward_saturating(U, entry, split):
    """lstm_inputs_fwd_hot: pre-activations of +-20 and 30 x normal drive rcp(1 + __expf(-x)) and 1 - 2 rcp(__expf(2x) + 1) to their limits
    (exp overflows to inf for |x| > 88.7, and rcp(inf) = 0 is the exact limit), and rows 1 and 3 walk the cell state to +-T.  h and gates are
    bounded by 1 and keep the absolute bar; the cell state reaches 46, where one f32 ulp is 3.8e-6, so its bar is 1e-5 max(1, |c|) element by
    element -- the same bar at unit scale.  No NaN from 0 x inf or inf - inf."""
    B, Tn = LSTM_HOT_SHAPE
    got, _, ref = _forward(U, B, Tn, entry, split, hot=True)
    errs = [float(np.abs(a - b).max()) for a, b in zip(got[:2], ref[:2])]
    if entry == TRAIN_FWD:
        errs.append(float((np.abs(got[2] - ref[2]) / np.maximum(1.0, np.abs(ref[2]))).max()))
        assert np.abs(got[2][1, Tn - 1, 0]).min() > Tn - 1 and got[2][3, Tn - 1, 0].max() < -(Tn - 1)  # the device's cell state did travel
    print(f"{entry} saturating U {U} B {B} T {Tn} split {split}: max |h{', gates' if len(errs) > 1 else ''} - float64|, max |c - float64| / max(1, |c|) = {errs}")
    _record("forward, saturating", U, max(errs))
    assert max(errs) <= FWD_BAR, errs


# ----------------------------------------------------------------------------------------------------------------------------- backward
def _backward(U, B, Tn, gscale, split, entry=BWD):
    *inputs, ref = _bwd_case(U, B, Tn, gscale)
    dH, gates, cst, Uw = inputs
    dev = tuple(_dev(a) for a in inputs)
    with _split(split):
        first, again = _run_bwd(entry, *dev, B, Tn, U), _run_bwd(entry, *dev, B, Tn, U)
    assert _same_bytes([first], [again])
    if U > 128 and split == 1:  # one kernel, no gradient scale, for both settings
        with _split(0):
            assert _same_bytes([first], [_run_bwd(entry, *dev, B, Tn, U)])
    return first, ref


@pytest.mark.parametrize("split", [0, 1])
@pytest.mark.parametrize("B,Tn,gscale", LSTM_BWD_CASES)
@pytest.mark.parametrize("U", LSTM_WIDTHS)
def test_lstm_backward_vs_float64(U, B, Tn, gscale, split):
    """dxz within 5e-6 of max |dxz| of the float64 backward through time, at incoming gradients of 1e-9 .. 3; dH = 0 (the max = 0 -> S = 1
    branch of lstm_grad_scale_kernel with split on) gives dxz = 0 exactly."""
    full, ref = _backward(U, B, Tn, gscale, split)
    (got,) = _written([full], B)
    scale = float(np.abs(ref).max())
    if gscale == 0.0:
        assert scale == 0.0 and not got.any()
        print(f"{BWD} U {U} B {B} T {Tn} dH = 0 split {split}: dxz = 0")
        return
    err = float(np.abs(got - ref).max()) / scale
    print(f"{BWD} U {U} B {B} T {Tn} |dH| ~ {gscale:g} split {split}: max |dxz - float64| / max |dxz| = {err:.2e}")
    _record("backward", U, err)
    assert err <= BWD_BAR, err


@pytest.mark.parametrize("U", LSTM_WIDTHS)
def test_lstm_backward_scale_does_not_leak_between_launches(U):
    """Split on: the power-of-two gradient scale travels through a device global.  |dH| ~ 3, then |dH| ~ 1e-9 (a scale 2^31 times larger), then
    |dH| ~ 3 again: the same bytes as the first time."""
    big, tiny = (c for c in LSTM_BWD_CASES if c[2] in (3.0, 1e-9))
    assert big[2] == 3.0 and tiny[2] == 1e-9
    first, ref = _backward(U, *big, 1)
    _backward(U, *tiny, 1)
    again, _ = _backward(U, *big, 1)
    assert _same_bytes([first], [again])
    assert np.abs(again[: big[0]] - ref).max() <= BWD_BAR * np.abs(ref).max()


# ------------------------------------------------------------------------------------------------------- the f16 entries' wide dispatch
@pytest.mark.parametrize("B,Tn", [(17, 2), (7, 9)])
@pytest.mark.parametrize("U", WIDE)
def test_h_entries_run_the_f32_wide_kernels(U, B, Tn):
    """Above 128 units orcai_h_lstm_train_fwd and orcai_h_lstm_bwd launch lstm_wide_*: the f32 entries' bytes, sentinel row included."""
    xz, Uw, *_ = _fwd_case(U, B, Tn)
    xd, ud = _dev(xz), _dev(Uw)
    f32, f16 = _run_fwd(TRAIN_FWD, xd, ud, B, Tn, U), _run_fwd("orcai_h_lstm_train_fwd", xd, ud, B, Tn, U)
    _written(f16, B)
    assert _same_bytes(f32, f16)
    *inputs, _ = _bwd_case(U, B, Tn, 0.1)
    dev = tuple(_dev(a) for a in inputs)
    f32, f16 = _run_bwd(BWD, *dev, B, Tn, U), _run_bwd("orcai_h_lstm_bwd", *dev, B, Tn, U)
    _written([f16], B)
    assert _same_bytes([f32], [f16])


# ---------------------------------------------------------------------------------------------------------------------------- refusals
class _Refusals:
    """Sentinel-filled buffers of a small case and the three entries as functions of (pointers..., B, T, units) in the C argument order."""

    def __init__(self, U, B=3, Tn=4, pad=0):
        from orcai_amd import _native as N

        self.N, self.U, self.B, self.Tn = N, U, B, Tn
        shapes = {"xz": (B, Tn, 2, 4 * U), "Uw": (2, U, 4 * U), "h": (B, Tn, 2 * U), "g": (B, Tn, 2, 4 * U), "c": (B, Tn, 2, U), "dxz": (B, Tn, 2, 4 * U)}
        self.bufs = {k: _sentinel(int(np.prod(s)) + pad) for k, s in shapes.items()}
        self.p = {k: N.ptr(v) for k, v in self.bufs.items()}
        lib, st = N.lib(), N.stream_ptr()
        self.calls = {
            RECURRENT: (lambda xz, Uw, b, t, u, h: lib.orcai_lstm_recurrent(xz, Uw, b, t, u, h, st), ("xz", "Uw", B, Tn, U, "h")),
            TRAIN_FWD: (lambda xz, Uw, b, t, u, h, g, c: lib.orcai_lstm_train_fwd(xz, Uw, b, t, u, h, g, c, st), ("xz", "Uw", B, Tn, U, "h", "g", "c")),
            BWD: (lambda dH, g, c, Uw, b, t, u, dxz: lib.orcai_lstm_bwd(dH, g, c, Uw, b, t, u, dxz, st), ("h", "g", "c", "Uw", B, Tn, U, "dxz")),
        }

    def call(self, entry, **change):
        """The entry with its good arguments, except: B, T, units replaced by value, a buffer's pointer replaced by name = new pointer."""
        fn, args = self.calls[entry]
        sizes = iter(("B", "T", "units"))
        values = []
        for a in args:
            key, good = (a, self.p[a]) if isinstance(a, str) else (next(sizes), a)
            values.append(change.get(key, good))
        assert not set(change) - {"B", "T", "units", *self.p}
        return fn(*values)

    def pointers(self, entry):
        return [a for a in self.calls[entry][1] if isinstance(a, str)]

    def untouched(self):
        torch.cuda.synchronize()
        for k, v in self.bufs.items():
            assert bool((v == SENT).all()), k


@pytest.mark.parametrize("split", [0, 1])
def test_lstm_entries_refuse_without_launching(split):
    r = _Refusals(32)
    N = r.N
    with _split(split):
        for entry in (RECURRENT, TRAIN_FWD, BWD):
            for units in (0, 16, 48, 288):
                assert r.call(entry, units=units) == N.E_UNSUPPORTED, (entry, units)
            assert r.call(entry, B=0) == N.E_BADARG and r.call(entry, T=0) == N.E_BADARG, entry
            for name in r.pointers(entry):  # a null xz (dH for the backward), and every other pointer
                assert r.call(entry, **{name: None}) == N.E_BADARG, (entry, name)
        for entry in (TRAIN_FWD, BWD):  # 2^34 elements: 32-bit element offsets inside the kernels.  Not orcai_lstm_recurrent: 64-bit offsets, no guard
            assert r.call(entry, B=1 << 20, T=64, units=32) == N.E_UNSUPPORTED, entry
    r.untouched()


def test_refusal_helper_passes_good_arguments_through():
    """The helper above with nothing changed is an ordinary launch: return code 0 and outputs written, so its refusals are the entries' doing."""
    r = _Refusals(32)
    xz, Uw, *_ = _fwd_case(32, r.B, r.Tn)
    r.bufs["xz"].copy_(_dev(xz).reshape(-1))
    r.bufs["Uw"].copy_(_dev(Uw).reshape(-1))
    for entry in (RECURRENT, TRAIN_FWD):
        assert r.call(entry) == 0
    torch.cuda.synchronize()
    assert not bool((r.bufs["h"] == SENT).any()) and not bool((r.bufs["g"] == SENT).any()) and not bool((r.bufs["c"] == SENT).any())
    assert r.call(BWD) == 0
    torch.cuda.synchronize()
    assert not bool((r.bufs["dxz"] == SENT).any())


@pytest.mark.parametrize("U", WIDE)
def test_wide_backward_refuses_misaligned_pointers(U):
    """lstm_wide_bwd_kernel reads U rows and stores dxz rows as float4: Uw or dxz one float off a 16-byte boundary is ORCAI_E_BADARG, nothing
    written.  (The narrow launchers make no alignment promise and are given none to break.)"""
    r = _Refusals(U, pad=4)
    N = r.N
    assert r.p["Uw"] % 16 == 0 and r.p["dxz"] % 16 == 0
    for split in (0, 1):
        with _split(split):
            for name in ("Uw", "dxz"):
                assert r.call(BWD, **{name: r.p[name] + 4}) == N.E_BADARG, (name, split)
    r.untouched()
