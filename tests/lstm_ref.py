"""float64 references of the BiLSTM recurrence kernels (numpy only: no GPU, no torch), in the kernels' permuted column order: 32-column groups
(i, f | g, o) of 8 units.  `_fwd_ref` / `_bwd_ref` are the plain recurrences the f32 kernels are held to.  `fwd_ref_f16` / `bwd_ref_f16` model the
f16 path's kernels (lstm_train_fwd_h_kernel, lstm_bwd_h_kernel): the recurrent product's two operands rounded to f16, everything else float64.

A free-running f16-rounded reference cannot be tight: the kernel's f32 h and the reference's float64 h differ by ~1e-7, which flips f16 roundings
(an f16 ulp of h is up to 5e-4).  So both take the device's own stored tensor (`h_forced` = out, `dxz_forced` = dxz, f32 arrays) and round THAT
for the operand of the next step -- exactly the number the kernel rounded -- while gates, cell state and dc still run free in float64."""

import numpy as np

F16_MIN_NORMAL = 2.0**-14

sig = lambda a: 1.0 / (1.0 + np.exp(-a))  # noqa: E731


def round_f16(a, flush=False):
    """a rounded to f16 (round to nearest even, as the kernels' casts) and returned as float64; flush: f16 subnormals become zero."""
    r = np.asarray(a).astype(np.float16).astype(np.float64)
    if flush:
        r = np.where(np.abs(r) < F16_MIN_NORMAL, 0.0, r)
    return r


def f16_ties(a, flush=False):
    """Where the f32 array a lies exactly midway between two neighbouring f16 numbers: (mask, the neighbour round_f16 did NOT take).  The kernels
    store the f32 product (out = o tanh c, dxz = dz) but round the UNROUNDED product to f16 in one step (v_fma_mixlo_f16), so at such a midpoint
    -- 2^-13 of the elements -- the stored value does not say which neighbour the operand was."""
    x = np.asarray(a).astype(np.float64)
    r16 = np.asarray(a).astype(np.float16)
    r = r16.astype(np.float64)
    lo, hi = np.nextafter(r16, np.float16(-np.inf)).astype(np.float64), np.nextafter(r16, np.float16(np.inf)).astype(np.float64)
    with np.errstate(invalid="ignore"):
        other = np.where((x < r) & (x - lo == r - x), lo, np.where((x > r) & (hi - x == x - r), hi, np.nan))
    mask = np.isfinite(other)
    if flush:
        other = np.where(np.abs(other) < F16_MIN_NORMAL, 0.0, other)
    return mask, other


def _resolve_ties(a, forced, flush, row_error, max_ties=6):
    """a = round_f16(forced) [B][K]: for every row with midpoint elements, try both neighbours of each (up to 2^max_ties combinations) and keep
    the combination row_error(b, operand row) likes best -- the only freedom the teacher-forced references have."""
    mask, other = f16_ties(forced, flush)
    for b in np.flatnonzero(mask.any(axis=1)):
        ks = np.flatnonzero(mask[b])[:max_ties]
        best, best_err = None, np.inf
        for combo in range(1 << len(ks)):
            row = a[b].copy()
            for j, k in enumerate(ks):
                if combo >> j & 1:
                    row[k] = other[b, k]
            e = row_error(b, row)
            if e < best_err:
                best, best_err = row, e
        a[b] = best
    return a


def _gates(zz):
    """[rows][4U] pre-activations in the permuted order -> i, f, g, o [rows][U/8][8] each."""
    zz = zz.reshape(zz.shape[0], -1, 4, 8)
    return sig(zz[:, :, 0]), sig(zz[:, :, 1]), np.tanh(zz[:, :, 2]), sig(zz[:, :, 3])


def _fwd_ref(xz, Uw):
    """float64 recurrence in the kernels' permuted column order (32-column groups (i, f | g, o) of 8 units): h, gates, cell states."""
    return _fwd(xz, Uw, None, None)


def fwd_ref_f16(xz, Uw, h_forced=None, flush=False, gates_forced=None):
    """_fwd_ref with U rounded to f16 once and the h operand of h U rounded to f16 at every step.  h_forced f32[B][T][2U] (the device's stored
    out): the operand at step t is f16(h_forced[t -+ 1]); cell state and gates run free.  flush: f16-subnormal operand values count as zero.
    gates_forced (the device's stored gates): where an element of h_forced is an exact f16 midpoint (f16_ties) the neighbour is taken that
    brings this step's gates of that batch row closest to the device's."""
    return _fwd(xz, Uw, lambda a: round_f16(a, flush), h_forced, flush, gates_forced)


def _fwd(xz, Uw, rnd, h_forced, flush=False, gates_forced=None):
    B, Tn, _, U4 = xz.shape
    U = U4 // 4
    h = np.zeros((B, Tn, 2 * U))
    g = np.zeros((B, Tn, 2, 4 * U))
    c = np.zeros((B, Tn, 2, U))
    for d in range(2):
        hh, cc = np.zeros((B, U)), np.zeros((B, U))
        W = Uw[d].astype(np.float64) if rnd is None else rnd(Uw[d])
        for step in range(Tn):
            t = Tn - 1 - step if d else step
            tp = t + 1 if d else t - 1
            if h_forced is not None:
                hh = h_forced[:, tp, d * U : (d + 1) * U] if 0 <= tp < Tn else np.zeros((B, U))
            a = hh if rnd is None else rnd(hh)
            x64 = xz[:, t, d].astype(np.float64)
            if gates_forced is not None and h_forced is not None:
                want = gates_forced[:, t, d].astype(np.float64)
                a = _resolve_ties(a, hh, flush, lambda b, row: np.abs(np.stack(_gates((x64[b] + row @ W)[None]), axis=2).reshape(-1) - want[b]).max())
            i_, f_, g_, o_ = _gates(x64 + a @ W)
            cc = (f_ * cc.reshape(B, U // 8, 8) + i_ * g_).reshape(B, U)
            hh = (o_ * np.tanh(cc.reshape(B, U // 8, 8))).reshape(B, U)
            h[:, t, d * U : (d + 1) * U] = hh
            c[:, t, d] = cc
            g[:, t, d] = np.stack([i_, f_, g_, o_], axis=2).reshape(B, 4 * U)
    return h, g, c


def _bwd_ref(dH, gates, cst, Uw):
    """float64 backward through time of the same recurrence: dxz in the permuted column order."""
    return _bwd(dH, gates, cst, Uw, None, None)


def bwd_ref_f16(dH, gates, cst, Uw, dxz_forced=None, flush=False, ties=False):
    """_bwd_ref with the recurrent term f16(dz) f16(U)^T.  dxz_forced f32[B][T][2][4U] (the device's stored dxz): dz of the product is the
    device's dxz of the step processed just before; dc runs free.  flush: f16-subnormal operand values count as zero.  ties: where an element
    of dxz_forced is an exact f16 midpoint (f16_ties) the neighbour is taken that brings the NEXT step's dz of that batch row closest to the
    device's."""
    return _bwd(dH, gates, cst, Uw, lambda a: round_f16(a, flush), dxz_forced, flush, ties)


def _bwd(dH, gates, cst, Uw, rnd, dxz_forced, flush=False, ties=False):
    B, Tn, _, U4 = gates.shape
    U = U4 // 4
    dxz = np.zeros((B, Tn, 2, 4 * U))
    for d in range(2):
        W = Uw[d].astype(np.float64) if rnd is None else rnd(Uw[d])
        dc, a_prev, prev_forced = np.zeros((B, U)), None, None

        def cell(t, tp, rows, dc_in, dhr):
            gv = gates[rows, t, d].astype(np.float64).reshape(len(dhr), U // 8, 4, 8)
            i_, f_, g_, o_ = (gv[:, :, q].reshape(-1, U) for q in range(4))
            c = cst[rows, t, d].astype(np.float64)
            cp = cst[rows, tp, d].astype(np.float64) if 0 <= tp < Tn else np.zeros_like(c)
            dh = dH[rows, t, d * U : (d + 1) * U].astype(np.float64) + dhr
            tc = np.tanh(c)
            dct = dc_in + dh * o_ * (1 - tc * tc)
            dz = np.stack([dct * g_ * i_ * (1 - i_), dct * cp * f_ * (1 - f_), dct * i_ * (1 - g_ * g_), dh * tc * o_ * (1 - o_)], axis=1)  # [rows][4][U]
            return dz.reshape(-1, 4, U // 8, 8).transpose(0, 2, 1, 3).reshape(-1, 4 * U), dct * f_

        for step in range(Tn):
            t = step if d else Tn - 1 - step
            tp = t + 1 if d else t - 1
            if a_prev is not None and ties and dxz_forced is not None:
                want = dxz_forced[:, t, d].astype(np.float64)
                a_prev = _resolve_ties(a_prev, prev_forced, flush, lambda b, row: np.abs(cell(t, tp, [b], dc[b : b + 1], (row @ W.T)[None])[0][0] - want[b]).max())
            dhr = np.zeros((B, U)) if a_prev is None else a_prev @ W.T
            dz, dc = cell(t, tp, slice(None), dc, dhr)
            dxz[:, t, d] = dz
            if dxz_forced is not None:
                dz = dxz_forced[:, t, d]
            a_prev, prev_forced = (dz if rnd is None else rnd(dz)), dz
    return dxz


# The shapes the recurrence tests share (tests/test_lstm_f32_gpu.py): every width the launchers accept, and the batch / time edges of kernels
# that work on 16-row batch tiles, double-buffer on step & 1 and prefetch step + 1.
LSTM_WIDTHS = (32, 64, 96, 128, 160, 192, 224, 256)  # up to 128 the register-resident kernels, above the L2-streamed family (lstm_wide.hip)
LSTM_FWD_SHAPES = (
    (1, 1),  # smallest batch and time
    (16, 1),  # exactly one tile
    (17, 2),  # the second tile holds one live row; one buffer flip
    (15, 3),  # ragged single tile
    (33, 9),  # three tiles, ragged last
    (7, 46),  # the model's own T
)
LSTM_BWD_CASES = (  # (B, T, gscale)
    (1, 1, 0.1),
    (16, 1, 0.1),
    (17, 2, 1e-2),
    (15, 3, 3.0),
    (33, 9, 1e-9),
    (20, 46, 1e-4),
    (7, 9, 0.0),  # dH identically zero
)
LSTM_HOT_WIDTHS = (32, 128, 224)  # one narrow width, the shipped one, and the wide width no other shape list has
LSTM_HOT_SHAPE = (17, 46)
HOT_SCALE, HOT_LEVEL = 30.0, 20.0


def lstm_inputs_fwd(rng, U, B, Tn):
    """The f32 tests' forward inputs: xz standard normal, Uw standard normal x 0.8 / sqrt(U)."""
    xz = rng.standard_normal((B, Tn, 2, 4 * U)).astype(np.float32)
    Uw = (rng.standard_normal((2, U, 4 * U)) * (0.8 / np.sqrt(U))).astype(np.float32)
    return xz, Uw


def lstm_inputs_fwd_hot(rng, U, B, Tn):
    """Forward inputs that saturate the activations and let the cell state grow: Uw (and the draws) of lstm_inputs_fwd, and xz by batch row --
    even rows: HOT_SCALE x standard normal; row 1: every pre-activation +HOT_LEVEL at every step (i = f = o = 1 and g = 1 to f32: the cell state
    climbs by about 1 per step); row 3: the same with g at -HOT_LEVEL (the cell state falls); the other odd rows: plain standard normal."""
    xz, Uw = lstm_inputs_fwd(rng, U, B, Tn)
    xz[0::2] *= np.float32(HOT_SCALE)
    for row, g_level in ((1, HOT_LEVEL), (3, -HOT_LEVEL)):
        if row < B:
            z = np.empty((U // 8, 4, 8), np.float32)  # the layout _gates reads: groups of 32 columns = [gate i, f, g, o][8 units]
            z[:, (0, 1, 3)] = HOT_LEVEL
            z[:, 2] = g_level
            xz[row] = z.reshape(4 * U)
    return xz, Uw


def lstm_inputs_bwd(rng, U, B, Tn, gscale):
    """The f32 tests' backward inputs: gates sigmoid / tanh of normals, cst 0.7 x normal, dH gscale x normal, Uw as in the forward."""
    f = lambda *s: rng.standard_normal(s).astype(np.float32)  # noqa: E731
    gates = sig(f(B, Tn, 2, 4 * U)).astype(np.float32)
    gv = gates.reshape(B, Tn, 2, U // 8, 4, 8)
    gv[..., 2, :] = np.tanh(f(B, Tn, 2, U // 8, 8))
    cst = f(B, Tn, 2, U) * 0.7
    dH = (f(B, Tn, 2 * U) * gscale).astype(np.float32)
    Uw = (f(2, U, 4 * U) * (0.8 / np.sqrt(U))).astype(np.float32)
    return dH, gates, cst, Uw
