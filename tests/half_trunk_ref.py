"""Float64 references, derived error bounds and the case tables for the forward trunk launchers of the f16 path (csrc/half_fwd.hip):
orcai_h_conv0_affine, orcai_h_conv0_affine_bn, orcai_h_sepconv (the one-window kernel sepconv_h_kernel<1|3|5|7> and the flat-tile kernel
sepconv_h_ftile_kernel), orcai_h_sepconv_stats and orcai_h_sepconv_stats_bn.  Plain numpy; tests/test_half_trunk_ref.py checks this module on
the CPU (against torch float64, against mutated references and against an emulation of the kernels' arithmetic), tests/test_half_trunk_gpu.py
holds the kernels to it.

Every input a kernel sees in f16 enters a reference as the float64 value of its f16 rounding: the planes, the depthwise taps
(pack_depthwise_octets casts them) and the pointwise weights (pack_pointwise_fragments casts them).  The entry convolution reads f32 snippets
and f32 weights, which enter as they are.

Every reference returns its result with the sum of the absolute values of the terms a kernel adds up for that element (S, Su, T): the bounds
below are multiples of it.

Two kinds of input, as tests/test_predict_trunk_gpu.py:
  exact   integers in [-2, 2], sparse integer taps and weights, scales from {-2, -1, 0.5, 1, 2}, integer shifts, drawn so that every partial sum
          is an integer below 2048 and every stored value is exactly representable in f16 (tests/test_half_trunk_ref.py verifies it for every
          case): the kernel must reproduce the float64 result under np.array_equal;
  normal  standard-normal data rounded to f16, taps N(0, 1) / k, pointwise weights N(0, 1) / sqrt(Cin), scales of both signs with magnitude in
          [0.5, 2] and at least a third of them negative: element by element at the bounds below.

Bounds (u16 = 2^-11, u32 = 2^-24: the unit roundoffs of f16 and f32; gamma(n, u) = n u / (1 - n u)):
  dw_bound      depthwise output u:  gamma(2 k^2 + k, u16) Su + 2^-24, Su = sum |x w|.  Each tap is allowed one multiply and one add rounding
                (whether or not the compiler contracts them), plus the k - 1 lane-shift additions and the store; 2^-24 is the f16 subnormal grain.
  pw_bound      pointwise + epilogue on the u THE DEVICE STORED:  (Cin + 8) 2^-23 S, S = |scale| sum_c |u_c pw_c| + |shift|: the forward error of a
                Cin-term f32 sum in any order with the unit roundoff doubled for the matrix unit's internal rounding and a few roundings for scale
                and shift (half_fwd_ref.gemm_bound, the bar of the f16 head GEMM).
  store16       an f16 store of `want`:  u16 |want| + 2^-24.
  scatter16     layout 3, out = f16(start + f16(val)):  u16 |val| + u16 |start + val| + 2 * 2^-24 (the addition happens in f16).
  conv0_bound   (k^2 + 8) 2^-23 S + store16(want): a k^2-term f32 fma chain, S = |scale| sum |x w| + |shift|.
  bn_y_bound    y = f16(relu(fma(v, sc, sh))) formed from a stored f16 v:  4 u32 (|v sc| + |sh|) + store16(y): four f32 roundings,
                counted for the add, the reciprocal square root and the product of the fold, and the fma.  A count, not a rigorous bound: the error of sh = beta - mean sc
                grows with |mean sc|, which exceeds |sh| where the two cancel, and the device's rsqrtf is not correctly rounded (about 1 ulp).
                It rests on |v sc| and |sh| both being charged (eight roundings' worth where y is small) and on the store term, 2^13 times
                larger, dominating wherever y is not tiny.
  stats_bounds  see the function."""

import numpy as np

from half_fwd_ref import bn_fold, from_octet_planes, split_planes, to_octet_planes, to_xpooled  # noqa: F401  (re-exported for the tests)
from trunk_fwd_ref import pair_max

U16, U32 = 2.0**-11, 2.0**-24
SCALES = (-2.0, -1.0, 0.5, 1.0, 2.0)  # the exact kind's scales: powers of two of both signs
BN_EPS = 1e-3


def r16(a):
    """The float64 value of the f16 rounding (to nearest even)."""
    return np.asarray(a).astype(np.float16).astype(np.float64)


def _c(v):
    """A per-channel vector against [B][C][H][W]."""
    return np.asarray(v, dtype=np.float64)[None, :, None, None]


def gamma(n, u):
    return n * u / (1.0 - n * u)


# ------------------------------------------------------------------------------------------------- references
def conv0_ref(x, w, scale, shift, relu):
    """[relu](scale * Conv2D(16, k, "same")(x) + shift) in float64: cross-correlation of the one-channel x [B][H][W] with w [k * k][16] (tap
    dy * k + dx).  Returns (v [B][16][H][W], S = |scale| sum |x| |w| + |shift|)."""
    x, w = np.asarray(x, dtype=np.float64), np.asarray(w, dtype=np.float64)
    B, H, W = x.shape
    k = int(round(np.sqrt(w.shape[0])))
    R = k // 2
    xp = np.zeros((B, H + 2 * R, W + 2 * R))
    xp[:, R : R + H, R : R + W] = x
    conv, S = np.zeros((B, 16, H, W)), np.zeros((B, 16, H, W))
    for dy in range(k):
        for dx in range(k):
            win, wt = xp[:, None, dy : dy + H, dx : dx + W], w[dy * k + dx][None, :, None, None]
            conv += win * wt
            S += np.abs(win) * np.abs(wt)
    v = conv * _c(scale) + _c(shift)
    return (np.maximum(v, 0.0) if relu else v), S * np.abs(_c(scale)) + np.abs(_c(shift))


def bn_relu_ref(v, mean, var, gamma_, beta, eps):
    """relu(BatchNorm(v)) in float64 of v as given.  Returns (y, T = |v sc| + |sh|)."""
    sc, sh = bn_fold(mean, var, gamma_, beta, eps)
    v = np.asarray(v, dtype=np.float64)
    return np.maximum(v * _c(sc) + _c(sh), 0.0), np.abs(v * _c(sc)) + np.abs(_c(sh))


def conv0_bn_ref(x, w, scale, shift, mean, var, gamma_, beta, eps):
    """The training forward's entry: v = scale * conv + shift (no ReLU) and y = relu(BatchNorm(v_stored)), v_stored the f16 rounding of v: the
    kernel forms y from the value it has just stored.  Returns (v, S, y, T)."""
    v, S = conv0_ref(x, w, scale, shift, 0)
    y, T = bn_relu_ref(r16(v), mean, var, gamma_, beta, eps)
    return v, S, y, T


def load_ref(x, relu_in, bn=None, eps=BN_EPS):
    """What the depthwise stage is given: the f16 planes, ReLU'd on load, or -- bn = (mean, var, gamma, beta) -- y_a = f16(relu(fma(v, sc, sh)))
    of the pre-normalisation planes (one rounding, to f16, of the f32 value)."""
    x = r16(x)
    if bn is not None:
        return r16(bn_relu_ref(x, *bn, eps)[0])
    return np.maximum(x, 0.0) if relu_in else x


def depthwise_ref(xa, dwk, pad=None):
    """Depthwise k x k "same" cross-correlation of xa [B][C][H][W] with dwk [k][k][C] (rounded to f16 here) in float64.  The padding is zero, or
    the per-channel value `pad` (what a kernel that normalised its zero pads would see).  Returns (u, Su = sum |xa| |w|)."""
    w = r16(dwk)
    k = w.shape[0]
    R = k // 2
    B, C, H, W = xa.shape
    xp = np.zeros((B, C, H + 2 * R, W + 2 * R)) + (0.0 if pad is None else _c(pad))
    xp[:, :, R : R + H, R : R + W] = xa
    u, Su = np.zeros((B, C, H, W)), np.zeros((B, C, H, W))
    for dy in range(k):
        for dx in range(k):
            t = xp[:, :, dy : dy + H, dx : dx + W] * _c(w[dy, dx])
            u += t
            Su += np.abs(t)
    return u, Su


def pointwise_ref(u, pw, scale, shift, relu_out):
    """The second stage on its own: [relu](scale * (u . f16(pw)) + shift) in float64 of u [B][Cin][H][W] as given (the depthwise output the
    device stored), pw [Cin][Cout].  Returns (v, S = |scale| sum_c |u_c pw_c| + |shift|)."""
    u, w = np.asarray(u, dtype=np.float64), r16(pw)
    v = np.einsum("bihw,io->bohw", u, w) * _c(scale) + _c(shift)
    S = np.einsum("bihw,io->bohw", np.abs(u), np.abs(w)) * np.abs(_c(scale)) + np.abs(_c(shift))
    return (np.maximum(v, 0.0) if relu_out else v), S


def sepconv_ref(x, dwk, pw, scale, shift, relu_in, relu_out, bn=None, eps=BN_EPS):
    """[ReLU | BatchNorm + ReLU on load] -> depthwise k x k "same" -> pointwise 1 x 1 -> scale, shift -> [ReLU].  With bn the planes hold the
    pre-normalisation tensor; y_a is ZERO outside the image ("same" padding pads y_a, not v: relu(sh) there is wrong).  Returns (u, Su, v, S);
    v here is formed from the float64 u, pointwise_ref takes any other."""
    u, Su = depthwise_ref(load_ref(x, relu_in, bn, eps), dwk)
    v, S = pointwise_ref(u, pw, scale, shift, relu_out)
    return u, Su, v, S


def out_stats_ref(v):
    """BatchNorm batch statistics of the UNROUNDED v (the kernel sums its f32 values before the f16 rounding): mean and biased variance over (B, H, W)."""
    return v.mean(axis=(0, 2, 3)), v.var(axis=(0, 2, 3))


# ------------------------------------------------------------------------------------------------- output layouts
def layout1(v):
    """Keras Reshape((-1, W * C)) of NHWC, f32 [B][H][W * C]: feature = x * C + c."""
    B, C, H, W = v.shape
    return np.ascontiguousarray(v.transpose(0, 2, 3, 1)).reshape(B, H, W * C)


def from_layout1(feat, C):
    B, H, WC = feat.shape
    return feat.reshape(B, H, WC // C, C).transpose(0, 3, 1, 2)


def layout2(v):
    """x-pooled [B][C][H][ceil(W / 2)]: maximum over the column pair (2j, 2j + 1); the last pair of an odd W has ONE member."""
    return pair_max(v)


def from_xpooled(p):
    """x-pooled octets [B][CO][H][WPx][8] -> [B][8 CO][H][WPx]"""
    B, CO, H, WPx, _ = p.shape
    return p.transpose(0, 1, 4, 2, 3).reshape(B, CO * 8, H, WPx)


def layout3(start, val):
    """Scatter-add: val [B][C][H][W] onto pixels (2y, 2x) of start [B][C][H2][W2], in float64."""
    H, W = val.shape[2:]
    out = np.array(start, dtype=np.float64)
    out[:, :, : 2 * H : 2, : 2 * W : 2] += val
    return out


# ------------------------------------------------------------------------------------------------- bounds (the module docstring has the reasons)
def store16(want):
    return U16 * np.abs(want) + 2.0**-24


def scatter16(start_sub, val):
    return U16 * np.abs(val) + U16 * np.abs(start_sub + val) + 2 * 2.0**-24


def dw_bound(Su, k):
    return gamma(2 * k * k + k, U16) * Su + 2.0**-24


def pw_bound(S, Cin):
    return (Cin + 8) * 2.0**-23 * S


def conv0_bound(S, want, k):
    return (k * k + 8) * 2.0**-23 * S + store16(want)


def bn_y_bound(T, y):
    return 4 * U32 * T + store16(y)


STATS_DEPTH = 16


def stats_bounds(v, ev):
    """Bounds on |mean - mean64| and |var - var64| of orcai_h_sepconv_stats[_bn] + orcai_h_bn_finish_sharded, from the kernel's summation structure.
    v [B][C][H][W]: the float64 result (unrounded) of the pointwise stage on the device's u; ev: the bound on the kernel's f32 value of each
    element, pw_bound(S, Cin).

    What one value passes through before it reaches f64 (sepconv_h_ftile_kernel<.., STATS>):
      lane       st += l0 + l1 for the two tile pairs: at most 2 f32 additions (the first lands on st = 0);  the square enters as
                 fmaf(l, l, st), four deep: at most 4 roundings, the product itself exact inside the fma;
      row        the inclusive DPP scan over 16 lanes (row_shr 1, 2, 4, 8): 4 additions;
      workgroup  wave 0 adds the 8 waves' LDS slots one after the other: at most 8 additions;
    so at most 2 + 4 + 8 = 14 (sums) and 4 + 4 + 8 = 16 (squares) f32 roundings, in a tree no value passes twice: the f32 partial sum of a
    workgroup is off by at most gamma(16, u32) times the sum of the absolute values it holds (STATS_DEPTH = 16 for both).  Then f64: one
    atomic per workgroup into one of 32 shards, the 32 shards added by orcai_h_bn_finish_sharded, mu = su / N, var = sq / N - mu^2 (clamped at 0,
    which moves it towards the true value), each 2^-53 relative: below 2^-40 of the absolute sums for any launch of fewer than 2^12 workgroups.
    Last, one rounding of each result to f32.  With e = ev the error of a value, its square is off by 2 |v| e + e^2:
      E_su = sum e + (gamma16 + 2^-40) sum (|v| + e)
      E_sq = sum (2 |v| e + e^2) + (gamma16 + 2^-40) sum (|v| + e)^2
      |mean - mean64| <= E_su / N + u32 (|mean64| + E_su / N)
      |var - var64|   <= E_sq / N + (2 |mean64| + E_su / N) E_su / N, plus u32 of var64 and of that."""
    N = v.shape[0] * v.shape[2] * v.shape[3]
    g = gamma(STATS_DEPTH, U32) + 2.0**-40
    a = np.abs(v) + ev
    E_su = (ev.sum(axis=(0, 2, 3)) + g * a.sum(axis=(0, 2, 3))) / N
    E_sq = ((2 * np.abs(v) * ev + ev * ev).sum(axis=(0, 2, 3)) + g * (a * a).sum(axis=(0, 2, 3))) / N
    mean, var = out_stats_ref(v)
    b_mean = E_su + U32 * (np.abs(mean) + E_su)
    e_var = E_sq + (2 * np.abs(mean) + E_su) * E_su
    return b_mean, e_var + U32 * (var + e_var)


# ------------------------------------------------------------------------------------------------- draws
def _rng(*key):
    return np.random.default_rng([int(v) for v in key])


def _ints(rng, *shape, lo=-2, hi=2, keep=1.0):
    """Integers in [lo, hi], each kept with probability `keep` (else 0), f32."""
    a = rng.integers(lo, hi + 1, size=shape)
    if keep < 1.0:
        a = a * (rng.random(shape) < keep)
    return a.astype(np.float32)


def _normal16(rng, *shape, div=1.0):
    """N(0, 1) / div rounded to f16, as f32."""
    return (rng.standard_normal(shape) / div).astype(np.float16).astype(np.float32)


def scale_shift(rng, C, exact):
    """Per-channel scale of both signs and shift.  exact: scales from SCALES, integer shifts; normal: magnitude in [0.5, 2], the sign negative on
    ceil(C / 2) randomly placed channels (at least a third), shift N(0, 1)."""
    neg = np.zeros(C, dtype=bool)
    neg[rng.permutation(C)[: (C + 1) // 2]] = True
    if exact:
        return np.where(neg, rng.choice((-2.0, -1.0), size=C), rng.choice((0.5, 1.0, 2.0), size=C)).astype(np.float32), _ints(rng, C, lo=-4, hi=4)
    mag = 0.5 + 1.5 * rng.random(C)
    return np.where(neg, -mag, mag).astype(np.float32), rng.standard_normal(C).astype(np.float32)


def bn_params(rng, C, exact):
    """(mean, var, gamma, beta), eps of a BatchNorm.  exact: var = 1 and eps = 0 (rsqrt(1) = 1), gamma from SCALES, integer mean and beta: the
    fold and the fma are exact.  normal: gamma ~ N(0, 1) of both signs, gamma[C // 2] exactly 0, gamma[C - 1] < 0, eps = 1e-3."""
    if exact:
        gamma_, _ = scale_shift(rng, C, True)
        return (_ints(rng, C), np.ones(C, dtype=np.float32), gamma_, _ints(rng, C)), 0.0
    gamma_ = rng.standard_normal(C).astype(np.float32)
    gamma_[0], gamma_[C - 1] = abs(gamma_[0]) + 0.25, -abs(gamma_[C - 1]) - 0.25
    gamma_[C // 2] = 0.0
    mean, beta = (0.5 * rng.standard_normal(C)).astype(np.float32), (0.5 * rng.standard_normal(C)).astype(np.float32)
    return (mean, (0.5 + rng.random(C)).astype(np.float32), gamma_, beta), BN_EPS


# ------------------------------------------------------------------------------------------------- orcai_h_conv0_affine[_bn]: cases
# (k, H, W, sliding): what conv0_h_kernel<k> (8 x 32 pixel tiles, halo of k / 2) reaches there; B = 2
CONV0_SHAPES = {
    "1x3: one row, narrower than the halo": (1, 3, 0),
    "8x32: exactly one tile": (8, 32, 0),
    "9x33: one past the tile in both directions": (9, 33, 0),
    "5x61: ragged, two column tiles": (5, 61, 0),
    "9x33 sliding view, snippet_stride 4 * 33 < H * W (the snippets share five rows)": (9, 33, 1),
}
CONV0_CASES = {f"k{k} {name}": (k,) + shape for k in (3, 5, 7) for name, shape in CONV0_SHAPES.items()}
CONV0_B = 2


def conv0_case(name, exact):
    """The snippets (src with its stride, and x as the kernel reads them), f32 weights [k * k][16], scale / shift, and a BatchNorm for the _bn twin."""
    k, H, W, sliding = CONV0_CASES[name]
    rng = _rng(10, k, H, W, sliding, exact)
    B = CONV0_B
    stride = (H // 2) * W if sliding else H * W
    n = (B - 1) * stride + H * W
    src = _ints(rng, n) if exact else rng.standard_normal(n).astype(np.float32)
    x = np.stack([src[b * stride : b * stride + H * W].reshape(H, W) for b in range(B)])
    w = _ints(rng, k * k, 16, lo=-1, hi=1, keep=min(1.0, 9.0 / (k * k))) if exact else (rng.standard_normal((k * k, 16)) / k).astype(np.float32)
    scale, shift = scale_shift(rng, 16, exact)
    bn, eps = bn_params(rng, 16, exact)
    return dict(k=k, B=B, H=H, W=W, src=src, stride=stride, x=x, w=w, scale=scale, shift=shift, bn=bn, eps=eps)


# ------------------------------------------------------------------------------------------------- orcai_h_sepconv: cases
def sep_inputs(rng, B, Cin, Cout, H, W, ktap, exact):
    if exact:
        x = _ints(rng, B, Cin, H, W)
        dwk = _ints(rng, ktap, ktap, Cin, lo=-1, hi=1, keep=min(1.0, 6.0 / (ktap * ktap)))
        pw = _ints(rng, Cin, Cout, lo=-1, hi=1, keep=min(1.0, 12.0 / Cin))
    else:
        x, dwk, pw = _normal16(rng, B, Cin, H, W), _normal16(rng, ktap, ktap, Cin, div=ktap), _normal16(rng, Cin, Cout, div=np.sqrt(Cin))
    scale, shift = scale_shift(rng, Cout, exact)
    return dict(B=B, Cin=Cin, Cout=Cout, H=H, W=W, ktap=ktap, x=x, dwk=dwk, pw=pw, scale=scale, shift=shift)


# k = 3, planes of R = 1.  (Cin, Cout, H, W, out_layout, relu_in, relu_out, u_out).  Each case runs on both routes -- orcai_sepconv_tile_mode(0):
# sepconv_h_kernel<3, MT>; (1): sepconv_h_ftile_kernel<MT, XP, UOUT> -- except out_layout 1, which is the one-window kernel in every mode.
# Channels: (5, 7) one ragged octet each side, MT 1; (16, 30) 2 octets -> MT 2, ragged out; (30, 16) ragged in, 1 K group; (40, 50) 5 octets: two
# K groups with the o < CO guard, MT 4 with the oq >= COo skip; (64, 64) 8 octets, MT 4 full.
# Planes: 1x3 one window; 5x21 several rows per window; 9x62 rows of pitch 64 (the plane row ends at a window edge); 8x63 odd W: the x-pooled
# pair with one member; 7x130 15 windows: two workgroups on the flat route.
SEP3_CASES = {
    "5->7 1x3 planes+u": (5, 7, 1, 3, 0, 0, 0, True),
    "16->30 5x21 planes+u relu in/out": (16, 30, 5, 21, 0, 1, 1, True),
    "30->16 9x62 planes relu out": (30, 16, 9, 62, 0, 0, 1, False),
    "40->50 8x63 x-pooled relu in": (40, 50, 8, 63, 2, 1, 0, False),
    "64->64 7x130 x-pooled relu out": (64, 64, 7, 130, 2, 0, 1, False),
    "16->30 7x130 planes+u relu in": (16, 30, 7, 130, 0, 1, 0, True),
    "30->16 8x63 x-pooled": (30, 16, 8, 63, 2, 0, 0, False),
    "40->50 1x3 x-pooled relu in/out": (40, 50, 1, 3, 2, 1, 1, False),
    "64->64 5x21 planes relu in": (64, 64, 5, 21, 0, 1, 0, False),
    "5->7 9x62 x-pooled relu in": (5, 7, 9, 62, 2, 1, 0, False),
    "64->64 9x62 planes+u relu out": (64, 64, 9, 62, 0, 0, 1, True),
    "40->50 7x130 Keras reshape relu in/out": (40, 50, 7, 130, 1, 1, 1, False),
    "5->7 5x21 Keras reshape": (5, 7, 5, 21, 1, 0, 0, False),
}
SEP_B = 2


def sep3_case(name, exact):
    Cin, Cout, H, W, layout, relu_in, relu_out, with_u = SEP3_CASES[name]
    c = sep_inputs(_rng(20, Cin, Cout, H, W, layout, exact), SEP_B, Cin, Cout, H, W, 3, exact)
    c.update(kp=3, layout=layout, relu_in=relu_in, relu_out=relu_out, with_u=with_u)
    return c


# k = 5 and 7 and the pointwise pass: sepconv_h_kernel<ktap, MT> only.  (Cin, Cout, H, W, ksize_planes, ktap, out_layout, relu_in, relu_out, u_out).
# W = 65: wider than one window (60 / 58 valid lanes; 60 / 56 x-pooled).
SEPK_CASES = {
    "k5 16->30 5x65 planes+u relu in": (16, 30, 5, 65, 5, 5, 0, 1, 0, True),
    "k5 16->30 5x65 x-pooled (lo 2), odd W": (16, 30, 5, 65, 5, 5, 2, 0, 0, False),
    "k7 30->16 4x65 planes+u relu out": (30, 16, 4, 65, 7, 7, 0, 0, 1, True),
    "k7 30->16 4x65 x-pooled (lo 4) relu in": (30, 16, 4, 65, 7, 7, 2, 1, 0, False),
    "ktap 1 on k5 planes, 30->16 5x33 scatter-add onto a 9x65 start image (odd H2, W2)": (30, 16, 5, 33, 5, 1, 3, 0, 0, False),
}


def sepk_case(name, exact):
    Cin, Cout, H, W, kp, ktap, layout, relu_in, relu_out, with_u = SEPK_CASES[name]
    rng = _rng(30, Cin, Cout, H, W, kp, ktap, layout, exact)
    c = sep_inputs(rng, SEP_B, Cin, Cout, H, W, ktap, exact)
    c.update(kp=kp, layout=layout, relu_in=relu_in, relu_out=relu_out, with_u=with_u)
    if layout == 3:
        H2, W2 = 2 * H - 1, 2 * W - 1
        c.update(H2=H2, W2=W2, start=_ints(rng, SEP_B, Cout, H2, W2, lo=-4, hi=4) if exact else _normal16(rng, SEP_B, Cout, H2, W2))
    return c


# orcai_h_sepconv_stats / _stats_bn: sepconv_h_ftile_kernel<MT, false, true, true[, true]>.  (B, Cin, Cout, H, W, relu_in of the variant without BatchNorm).
# B = 3 once: the shard index is (bx + 7 b) & 31.
STATS_CASES = {
    "5->7 1x3": (2, 5, 7, 1, 3, 0),
    "16->30 5x21 B3": (3, 16, 30, 5, 21, 1),
    "40->50 8x63": (2, 40, 50, 8, 63, 0),
    "64->64 7x130 (two workgroups per snippet)": (2, 64, 64, 7, 130, 1),
}


def stats_case(name, exact):
    """As a k = 3 case; bn / eps: the BatchNorm of the INPUT for the _bn variant (there x holds the pre-normalisation planes)."""
    B, Cin, Cout, H, W, relu_in = STATS_CASES[name]
    rng = _rng(40, B, Cin, Cout, H, W, exact)
    c = sep_inputs(rng, B, Cin, Cout, H, W, 3, exact)
    bn, eps = bn_params(rng, Cin, exact)
    c.update(kp=3, layout=0, relu_in=relu_in, relu_out=0, with_u=True, bn=bn, eps=eps)
    return c


# ------------------------------------------------------------------------------------------------- the checks (shared by the GPU tests and the CPU tests of the tests)
class Check:
    """One comparison: `ok` under the kind's rule, the largest error, and (normal kind) the largest error / bound."""

    def __init__(self, what, got, want, bound, exact):
        got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
        assert got.shape == want.shape, (what, got.shape, want.shape)
        err = np.abs(got - want)
        self.what, self.err = what, float(err.max())
        if exact:
            self.ratio, self.ok = 0.0, bool(np.array_equal(got, want))
        else:
            with np.errstate(divide="ignore", invalid="ignore"):
                r = np.where(err > 0, err / np.broadcast_to(bound, err.shape), 0.0)  # err = 0 passes a bound of 0 (pixels nobody adds to)
            self.ratio, self.ok = float(r.max()), bool((err <= bound).all() and np.isfinite(got).all())

    def __repr__(self):
        return f"{self.what}: max error {self.err:.3e}, largest error / bound {self.ratio:.3f}, {'ok' if self.ok else 'FAILS'}"


def check_conv0(c, relu, got, exact):
    """out of orcai_h_conv0_affine [B][16][H][W] against conv0_ref:  (k^2 + 8) 2^-23 S + u16 |want| + 2^-24."""
    want, S = conv0_ref(c["x"], c["w"], c["scale"], c["shift"], relu)
    return [Check(f"conv0 relu={relu}", got, want, conv0_bound(S, want, c["k"]), exact)]


def check_conv0_bn(c, v_got, y_got, exact):
    """orcai_h_conv0_affine_bn: v as check_conv0; y against relu(BatchNorm(.)) of the v THE DEVICE STORED:  4 u32 (|v sc| + |sh|) + u16 |y| + 2^-24."""
    v, S = conv0_ref(c["x"], c["w"], c["scale"], c["shift"], 0)
    y, T = bn_relu_ref(v_got, *c["bn"], c["eps"])
    return [Check("conv0_bn v", v_got, v, conv0_bound(S, v, c["k"]), exact), Check("conv0_bn y", y_got, y, bn_y_bound(T, y), exact)]


def check_sep(c, u_dev, out, exact, bn=None):
    """One launch of orcai_h_sepconv / _stats / _stats_bn.  u_dev [B][Cin][H][W]: the depthwise output the device stored; out: the result in the
    case's layout as [B][Cout][H][W] (0, 1), [B][Cout][H][ceil(W / 2)] (2) or [B][Cout][H2][W2] (3).
      u    against depthwise_ref:  gamma(2 k^2 + k, u16) sum |x w| + 2^-24
      out  against pointwise_ref(u_dev):  (Cin + 8) 2^-23 S, plus u16 |want| + 2^-24 for the f16 store of layouts 0 and 2 (layout 2: want is
           the pair maximum and the pointwise term the larger one of the column pair -- a maximum moves by no more than its operands; the
           store term is that of the maximum alone, the losing member is never stored), plus
           u16 |val| + u16 |start + val| + 2 * 2^-24 for layout 3, whose other pixels keep the start image's value exactly."""
    u, Su = depthwise_ref(load_ref(c["x"], c["relu_in"], bn, c.get("eps", BN_EPS)), c["dwk"])
    checks = [Check("u", u_dev, u, dw_bound(Su, c["ktap"]), exact)]
    v, S = pointwise_ref(u_dev, c["pw"], c["scale"], c["shift"], c["relu_out"])
    bound, layout = pw_bound(S, c["Cin"]), c["layout"]
    if layout == 0:
        want, bound = v, bound + store16(v)
    elif layout == 1:
        want = v
    elif layout == 2:
        want = layout2(v)
        bound = layout2(bound) + store16(want)
    else:
        start = np.asarray(c["start"], dtype=np.float64)
        want, full = layout3(start, v), np.zeros(start.shape)
        H, W = v.shape[2:]
        full[:, :, : 2 * H : 2, : 2 * W : 2] = bound + scatter16(start[:, :, : 2 * H : 2, : 2 * W : 2], v)
        bound = full
    return checks + [Check(f"out (layout {layout})", out, want, bound, exact)]


def check_stats(c, u_dev, mean, var):
    """The finished statistics against float64 mean / biased variance of the unrounded pointwise_ref(u_dev), at stats_bounds (both kinds: the
    division by N is not exact)."""
    v, S = pointwise_ref(u_dev, c["pw"], c["scale"], c["shift"], 0)
    b_mean, b_var = stats_bounds(v, pw_bound(S, c["Cin"]))
    m64, v64 = out_stats_ref(v)
    return [Check("mean", mean, m64, b_mean, False), Check("var", var, v64, b_var, False)]
