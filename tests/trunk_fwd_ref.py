"""Float64 references, layout helpers and the case tables for the k = 3 f32 inference trunk launchers (orcai_conv0_bn_relu, orcai_sepconv_bn,
orcai_conv0_sepconv, orcai_pool_res_add, orcai_sepconv_pool_res).  Plain numpy; tests/test_trunk_fwd_ref.py checks this module on the CPU
(against oracle.model_ref's layers in torch float64), tests/test_predict_trunk_gpu.py holds the kernels to it.

Every reference returns (want, S): S is the sum of the absolute values of the terms a kernel adds up for that element.  It serves twice:
  exact            S (in units of the finest grain of the result) below 2^24 means every partial sum, in any order, is an integer multiple of
                   the grain that f32 holds exactly, so the kernel must reproduce the float64 result bit for bit;
  standard normal  |got - want| <= chain_bound(S, n_terms) = (n_terms + 8) 2^-23 S: the forward error of an n_terms-long f32 chain in any order
                   with the unit roundoff doubled for the matrix unit's internal rounding and a few roundings for scale and shift (the shape of
                   half_fwd_ref.gemm_bound)."""

import numpy as np

from half_fwd_ref import pool_res_add_ref
from test_trunk_fallback_gpu import _depthwise_ref, _ints, _sep_ref

SCALES = (-2.0, -1.0, 0.5, 1.0, 2.0)  # folded BatchNorm scales of the exact kind: powers of two of both signs


def chain_bound(S, n_terms):
    return (n_terms + 8) * 2.0**-23 * S


def _rng(*key):
    return np.random.default_rng([int(v) for v in key])


def _normal(rng, *shape, div=1.0):
    return (rng.standard_normal(shape) / div).astype(np.float32)


def scale_shift(rng, C, exact):
    """Folded BatchNorm of C channels with scales of both signs: channel 0 and channel C - 1 (in the last, usually ragged, quad) negative,
    channel C // 2 positive."""
    if exact:
        scale, shift = rng.choice(SCALES, size=C).astype(np.float32), _ints(rng, C)
    else:
        scale, shift = (1 + 0.3 * rng.standard_normal(C)).astype(np.float32), (0.2 * rng.standard_normal(C)).astype(np.float32)
    scale[0], scale[C - 1], scale[C // 2] = -abs(scale[0]), -abs(scale[C - 1]), abs(scale[C // 2])
    return scale, shift


# ------------------------------------------------------------------------------------------------- layouts
def pair_max(v):
    """[B][C][H][W] -> [B][C][H][ceil(W/2)]: maximum over the column pair (2j, 2j + 1); the column "same" padding adds right of an odd W does
    not count."""
    B, C, H, W = v.shape
    Wx = (W + 1) // 2
    pairs = np.full((B, C, H, 2 * Wx), -np.inf, dtype=v.dtype)
    pairs[..., :W] = v
    return pairs.reshape(B, C, H, Wx, 2).max(axis=4)


def to_xpooled_quads(xp, fill):
    """[B][C][H][Wx] -> the x-pooled layout f32 [B][ceil(C/4)][H][roundup4(Wx)][4].  Columns past Wx hold `fill`, channels >= C zero."""
    B, C, H, Wx = xp.shape
    CQ, WPx = (C + 3) // 4, (Wx + 3) & ~3
    out = np.zeros((B, CQ * 4, H, WPx), dtype=np.float32)
    out[:, :C] = fill
    out[:, :C, :, :Wx] = xp
    return np.ascontiguousarray(out.reshape(B, CQ, 4, H, WPx).transpose(0, 1, 3, 4, 2))


def from_xpooled_quads(p):
    """-> [B][4 CQ][H][WPx]"""
    B, CQ, H, WPx, _ = p.shape
    return p.transpose(0, 1, 4, 2, 3).reshape(B, CQ * 4, H, WPx)


def to_compact_quads(x):
    """[B][C][H][W] -> the compact subsample f32 [B][ceil(C/4)][ceil(H/2)][ceil(W/2)][4] of pixels (2i, 2j), channels >= C zero."""
    sub = x[:, :, ::2, ::2]
    B, C, Ho, Wo = sub.shape
    CQ = (C + 3) // 4
    out = np.zeros((B, CQ * 4, Ho, Wo), dtype=np.float32)
    out[:, :C] = sub
    return np.ascontiguousarray(out.reshape(B, CQ, 4, Ho, Wo).transpose(0, 1, 3, 4, 2))


def from_compact_quads(p):
    B, CQ, Ho, Wo, _ = p.shape
    return p.transpose(0, 1, 4, 2, 3).reshape(B, CQ * 4, Ho, Wo)


# ------------------------------------------------------------------------------------------------- references
def entry_ref(x, w0, scale0, shift0):
    """relu(scale0 * Conv2D(16, 3, "same")(x) + shift0) in float64: cross-correlation of the one-channel [B][H][W] with w0 [9][16] (tap dy * 3 + dx).
    Returns (a [B][16][H][W], S0 = |scale0| sum |x| |w0| + |shift0|); S0 >= |a|."""
    x, w0, scale0, shift0 = (np.asarray(v, dtype=np.float64) for v in (x, w0, scale0, shift0))
    B, H, W = x.shape
    xp = np.zeros((B, H + 2, W + 2))
    xp[:, 1 : H + 1, 1 : W + 1] = x
    conv, S = np.zeros((B, 16, H, W)), np.zeros((B, 16, H, W))
    for dy in range(3):
        for dx in range(3):
            win, w = xp[:, None, dy : dy + H, dx : dx + W], w0[dy * 3 + dx][None, :, None, None]
            conv += win * w
            S += np.abs(win) * np.abs(w)
    v = conv * scale0[None, :, None, None] + shift0[None, :, None, None]
    return np.maximum(v, 0.0), S * np.abs(scale0)[None, :, None, None] + np.abs(shift0)[None, :, None, None]


def sep_ref(x, dwk, pw, scale, shift, relu_in, relu_out, xS=None):
    """[ReLU] -> SeparableConv2D(Cout, 3, "same") -> scale, shift -> [ReLU] in float64 (test_trunk_fallback_gpu._sep_ref).  Returns (v, S),
    S = |scale| sum_ci (sum_taps X |dw|) |pw| + |shift| with X = |x| after the ReLU on load, or xS where x is itself a computed quantity whose
    terms sum to xS >= |x| (the fused entry convolution)."""
    _, v = _sep_ref(np.asarray(x), dwk, pw, scale, shift, relu_in, relu_out)
    x64 = np.asarray(x, dtype=np.float64)
    X = np.abs(np.maximum(x64, 0.0) if relu_in else x64) if xS is None else xS
    uS = _depthwise_ref(X, np.abs(dwk), 0)
    S = np.einsum("bihw,io->bohw", uS, np.abs(np.asarray(pw, dtype=np.float64))) * np.abs(np.asarray(scale, dtype=np.float64))[None, :, None, None]
    return v, S + np.abs(np.asarray(shift, dtype=np.float64))[None, :, None, None]


def pooled_bound(bound):
    """The largest bound inside every 3 x 2 "same" pooling window: a maximum moves by no more than its operands do."""
    C = bound.shape[1]
    return pool_res_add_ref(bound, np.zeros_like(bound), np.zeros((C, C)), np.zeros(C))[0]


# ------------------------------------------------------------------------------------------------- orcai_conv0_bn_relu: cases
# (B, H, W, sliding view): what conv0_kernel<3> (8 x 32 pixel tiles) reaches there
ENTRY_CASES = {
    "9x70: a one-row second row tile, three column tiles, the last 6 wide": (3, 9, 70, 0),
    "1x33: one image row, one pixel in the second column tile": (2, 1, 33, 0),
    "5x3: narrower than the tap window's halo": (2, 5, 3, 0),
    "sliding view of [T][33], H = 8, snippet_stride 4 * 33": (3, 8, 33, 1),
    "sliding view of [T][33], H = 9, snippet_stride 4 * 33 (the snippets share five rows)": (3, 9, 33, 1),
    "B = 9 at 5x3": (9, 5, 3, 0),
}


def entry_inputs(rng, B, H, W, sliding, exact):
    stride = (H // 2) * W if sliding else H * W
    n = (B - 1) * stride + H * W
    src = _ints(rng, n) if exact else _normal(rng, n)
    x = np.stack([src[b * stride : b * stride + H * W].reshape(H, W) for b in range(B)])
    w0 = _ints(rng, 9, 16) if exact else _normal(rng, 9, 16, div=3.0)
    scale0, shift0 = scale_shift(rng, 16, exact)
    return dict(src=src, stride=stride, x=x, w0=w0, scale0=scale0, shift0=shift0)


def entry_case(name, exact):
    B, H, W, sliding = ENTRY_CASES[name]
    return entry_inputs(_rng(1, B, H, W, sliding, exact), B, H, W, sliding, exact)


# ------------------------------------------------------------------------------------------------- orcai_sepconv_bn: cases
# (B, Cin, Cout, H, W): the kernel launch_sepconv_impl<3, MT> picks for plane (0) / x-pooled (2) output in tile mode 1.  Mode 2 is sepconv_ftile_kernel
# and mode 0 sepconv_kernel everywhere; out_layout 1 is sepconv_kernel in every mode.
SEP_CASES = {
    "MT 2, 4 quads, two strips >= 85 %: sepconv_tile_kernel<2, 4>, a one-row tail tile": (2, 16, 30, 9, 118),
    "MT 2, 8 quads, three strips below the 85 % rule: sepconv_ftile_kernel<2>": (3, 29, 32, 9, 130),
    "MT 2, ragged quads in and out, two strips at 56 %: sepconv_ftile_kernel<2>": (2, 13, 17, 5, 70),
    "MT 4, 10 input quads, three rows per window: sepconv_ftile_kernel<4>": (2, 37, 64, 3, 21),
    "MT 1, one image row over five windows: sepconv_ftile_kernel<1>": (2, 7, 9, 1, 300),
    "MT 4, 15 quads, ceil(W/2) = 11 odd: sepconv_ftile_kernel<4>": (2, 60, 60, 2, 22),
    "MT 4, 15 quads, odd W, ceil(W/2) = 12 even: sepconv_ftile_kernel<4>": (2, 60, 60, 2, 23),
    "B = 9, MT 2, ragged quads: sepconv_ftile_kernel<2>": (9, 13, 17, 5, 70),
}


def sep_inputs(rng, B, Cin, Cout, H, W, exact):
    if exact:
        x, dwk, pw = _ints(rng, B, Cin, H, W), _ints(rng, 3, 3, Cin), _ints(rng, Cin, Cout)
    else:  # scaled as test_trunk_fallback_gpu._sep_case scales them
        x, dwk, pw = _normal(rng, B, Cin, H, W), _normal(rng, 3, 3, Cin, div=3.0), _normal(rng, Cin, Cout, div=4.0)
    scale, shift = scale_shift(rng, Cout, exact)
    return dict(x=x, dwk=dwk, pw=pw, scale=scale, shift=shift)


def sep_case(name, exact):
    B, Cin, Cout, H, W = SEP_CASES[name]
    return sep_inputs(_rng(2, B, Cin, Cout, H, W, exact), B, Cin, Cout, H, W, exact)


# ------------------------------------------------------------------------------------------------- orcai_conv0_sepconv: cases
# (B, Cout, H, W, ((orcai_entry_tile, orcai_entry_windows), ...)); windows 0 = leave the default
FUSED_ENTRY_CASES = {
    "Cout 30, two strips >= 85 %: conv0_sep_tile_kernel<2, 10>, <2, 16> and, tiles off, conv0_sep_kernel<2>": (2, 30, 9, 118, ((10, 0), (16, 0), (0, 0))),
    "Cout 20, two strips at 56 %: conv0_sep_kernel<2>": (3, 20, 5, 70, ((10, 1), (10, 0))),
    "Cout 64: conv0_sep_kernel<4>": (2, 64, 3, 33, ((10, 1), (10, 0))),
    "Cout 12, one row of 9: conv0_sep_kernel<1>": (2, 12, 1, 9, ((10, 0),)),
}


def fused_entry_case(name, exact):
    B, Cout, H, W, _ = FUSED_ENTRY_CASES[name]
    rng = _rng(3, B, Cout, H, W, exact)
    c = entry_inputs(rng, B, H, W, 0, exact)
    if exact:
        dwk, pw = _ints(rng, 3, 3, 16), _ints(rng, 16, Cout)
    else:
        dwk, pw = _normal(rng, 3, 3, 16, div=3.0), _normal(rng, 16, Cout, div=4.0)
    scale, shift = scale_shift(rng, Cout, exact)
    c.update(dwk=dwk, pw=pw, scale=scale, shift=shift)
    return c


def fused_entry_ref(c, relu_out):
    """-> (a, S0, v, S): the entry activation and block 1's first separable convolution of it (ReLU on load)."""
    a, S0 = entry_ref(c["x"], c["w0"], c["scale0"], c["shift0"])
    v, S = sep_ref(a, c["dwk"], c["pw"], c["scale"], c["shift"], 1, relu_out, xS=S0)
    return a, S0, v, S


# ------------------------------------------------------------------------------------------------- orcai_pool_res_add: cases
# (B, C, Cp, H, W, orcai_pool_vertical settings): flags 1 / 3 run pool_res_add_x_kernel (stacked tiles where ceil(W/2) >= 40 and the knob is on),
# flags 0 / 2 pool_res_add_kernel
POOL_CASES = {
    "odd H (pad_top 1, last row clamped), Wo 44: stacked tiles, MT 2": (2, 30, 16, 9, 87, (1,)),
    "even H, Wo 44: stacked tiles and, knob off, flat windows": (2, 30, 16, 8, 87, (0, 1)),
    "Wo 11: flat windows, MT 3, ragged quads": (3, 40, 30, 5, 22, (1,)),
    "H = 1: pad_top 1 and both row clamps at once; Wo 81 stacked, MT 4": (2, 50, 40, 1, 161, (1,)),
    "MT 4 full, 13 quads of prev, 7x9": (2, 64, 50, 7, 9, (1,)),
    "2x3: one output row of two pixels, Cp 9": (2, 20, 9, 2, 3, (1,)),
    "B = 9, odd H, flat windows": (9, 40, 30, 5, 22, (1,)),
}


def pool_inputs(rng, B, C, Cp, H, W, exact):
    if exact:
        s, prev, wr, br = _ints(rng, B, C, H, W), _ints(rng, B, Cp, H, W), _ints(rng, Cp, C), _ints(rng, C)
    else:
        s, prev, wr, br = 2.0 * _normal(rng, B, C, H, W), _normal(rng, B, Cp, H, W), _normal(rng, Cp, C, div=4.0), 0.2 * _normal(rng, C)
    return dict(s=s, prev=prev, wr=wr, br=br)


def pool_case(name, exact):
    B, C, Cp, H, W, _ = POOL_CASES[name]
    return pool_inputs(_rng(4, B, C, Cp, H, W, exact), B, C, Cp, H, W, exact)


# ------------------------------------------------------------------------------------------------- orcai_sepconv_pool_res: cases
# (B, C = Cin, Cp, H, W): sepconv_pool_march_kernel<CQ, RELU>; Ho = H / 2 pooled rows in segments of 4 NT - 1 (orcai_pool_fused(NT))
TAIL_CASES = {
    "8 quads, Ho 7: three segments at NT 1, one at NT 2 and at the default; two strips, the second 58 wide": (2, 30, 16, 14, 118),
    "5 quads (ragged), Cp 9, Ho 3, second strip 44 wide": (3, 20, 9, 6, 104),
}
TAIL_NT = (1, 2, 0)  # 0 = leave the default


def tail_case(name, exact):
    B, C, Cp, H, W = TAIL_CASES[name]
    rng = _rng(5, B, C, Cp, H, W, exact)
    c = sep_inputs(rng, B, C, C, H, W, exact)
    p = pool_inputs(rng, B, C, Cp, H, W, exact)
    c.update(prev=p["prev"], wr=p["wr"], br=p["br"])
    return c


def tail_ref(c, relu_in):
    """-> (want, S, bound): MaxPooling2D((3, 2), 2, "same")(sep_b) + Conv2D(C, 1, strides 2)(prev) + br.
    bound = the largest separable-conv bound (9 + Cin terms) in the pooling window + the tail's own (Cp + 2 terms) on its S."""
    Cin, Cp = c["pw"].shape[0], c["wr"].shape[0]
    vb, Sb = sep_ref(c["x"], c["dwk"], c["pw"], c["scale"], c["shift"], relu_in, 0)
    want, St = pool_res_add_ref(vb, c["prev"], c["wr"], c["br"])
    return want, pooled_bound(Sb) + St, pooled_bound(chain_bound(Sb, 9 + Cin)) + chain_bound(St, Cp + 2)
