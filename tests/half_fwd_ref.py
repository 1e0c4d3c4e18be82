"""Float64 references, layout helpers and the case tables for two forward launchers of the f16 path: orcai_h_pool_res_add (the pooling tail,
with BatchNorm on the fly) and orcai_h_gemm_bias_act (the head GEMM).  Plain numpy; tests/test_half_fwd_ref.py checks this module on the
CPU (against torch float64), tests/test_half_forward_gpu.py holds the kernels to it."""

import numpy as np

from oracle.model_ref import same_pad


# ------------------------------------------------------------------------------------------------- layouts
def to_octet_planes(x, ksize):
    """[B][C][H][W] -> f16 [B][ceil(C/8)][H + 2R][WP][8] with zero pads."""
    B, C, H, W = x.shape
    R = ksize // 2
    WP = (W + R + 3) & ~3
    CO = (C + 7) // 8
    out = np.zeros((B, CO * 8, H + 2 * R, WP), dtype=np.float16)
    out[:, :C, R : R + H, :W] = x
    return np.ascontiguousarray(out.reshape(B, CO, 8, H + 2 * R, WP).transpose(0, 1, 3, 4, 2))


def from_octet_planes(p, C, H, W, ksize):
    B, CO, HP, WP, _ = p.shape
    R = ksize // 2
    full = p.transpose(0, 1, 4, 2, 3).reshape(B, CO * 8, HP, WP)
    pads = full.copy()
    pads[:, :C, R : R + H, :W] = 0
    return full[:, :C, R : R + H, :W], pads


def split_planes(out, C, H, W, k):
    """Octet planes [B][CO][H + 2R][WP][8] (any dtype) -> (valid, written_zeros, pads):
    valid [B][C][H][W]: the real channels inside the image; written_zeros [B][8 CO - C][H][W]: the channels >= C of the last octet at the
    image's pixels (a kernel stores whole octets, so it writes these, as zeros); pads [B][8 CO][pixels outside the image]: the pad rows
    and columns of every channel, which a kernel leaves alone."""
    B, CO, HP, WP, _ = out.shape
    R = k // 2
    assert HP == H + 2 * R and WP == ((W + R + 3) & ~3), (out.shape, C, H, W, k)
    full = out.transpose(0, 1, 4, 2, 3).reshape(B, CO * 8, HP, WP)
    inside = np.zeros((HP, WP), dtype=bool)
    inside[R : R + H, :W] = True
    return full[:, :C, R : R + H, :W], full[:, C:, R : R + H, :W], full[:, :, ~inside]


def to_quad_planes(x, ksize):
    """[B][C][H][W] -> f32 [B][ceil(C/4)][H + 2R][WP][4] with zero pads (the f32 path's layout)."""
    B, C, H, W = x.shape
    R = ksize // 2
    WP = (W + R + 3) & ~3
    CQ = (C + 3) // 4
    out = np.zeros((B, CQ * 4, H + 2 * R, WP), dtype=np.float32)
    out[:, :C, R : R + H, :W] = x
    return np.ascontiguousarray(out.reshape(B, CQ, 4, H + 2 * R, WP).transpose(0, 1, 3, 4, 2))


def from_quad_planes(p, C, H, W, ksize):
    """-> (the image [B][C][H][W], the planes with the image zeroed: whatever is left is in a pad)."""
    B, CQ, HP, WP, _ = p.shape
    R = ksize // 2
    full = p.transpose(0, 1, 4, 2, 3).reshape(B, CQ * 4, HP, WP)
    pads = full.copy()
    pads[:, :C, R : R + H, :W] = 0
    return full[:, :C, R : R + H, :W], pads


def to_xpooled(s, fill):
    """[B][C][H][W] -> the x-pooled layout f16 [B][CO][H][roundup4(ceil(W/2))][8]: maximum over the column pair (2j, 2j + 1); the column "same"
    padding adds on the right of an odd W does not count.  Columns past ceil(W/2) hold `fill`, channels >= C zero."""
    B, C, H, W = s.shape
    Wx = (W + 1) // 2
    WPx, CO = (Wx + 3) & ~3, (C + 7) // 8
    pairs = np.full((B, C, H, 2 * Wx), -np.inf)
    pairs[..., :W] = s
    out = np.zeros((B, CO * 8, H, WPx), dtype=np.float16)
    out[:, :C] = fill
    out[:, :C, :, :Wx] = pairs.reshape(B, C, H, Wx, 2).max(axis=-1)
    return np.ascontiguousarray(out.reshape(B, CO, 8, H, WPx).transpose(0, 1, 3, 4, 2))


# ------------------------------------------------------------------------------------------------- references
def bn_fold(mean, var, gamma, beta, eps):
    """BatchNorm as y = x * sc + sh, float64."""
    mean, var, gamma, beta = (np.asarray(a, dtype=np.float64) for a in (mean, var, gamma, beta))
    sc = gamma / np.sqrt(var + float(eps))
    return sc, beta - mean * sc


def pool_res_add_ref(s, prev, wr, br, bn=None, eps=1e-3):
    """MaxPooling2D((3, 2), 2, "same")(BN(s)) + Conv2D(C, 1, strides 2)(prev) + br in float64, TensorFlow "same" padding (the pad is -inf).
    s [B][C][H][W], prev [B][Cp][H][W], wr [Cp][C], br [C]; bn = (mean, var, gamma, beta) or None.  BatchNorm is applied to every element
    BEFORE the maximum is taken.  Returns (want, S) with S = |sc v_sel| + |sh| + sum |prev| |wr| + |br| per output element, v_sel the element
    of s the maximum selected: the size of the terms a kernel adds up."""
    s, prev, wr, br = (np.asarray(a, dtype=np.float64) for a in (s, prev, wr, br))
    B, C, H, W = s.shape
    if bn is None:
        sc, sh = np.ones(C), np.zeros(C)
    else:
        sc, sh = bn_fold(*bn, eps)
    t = s * sc[None, :, None, None] + sh[None, :, None, None]
    Ho, pt, pb = same_pad(H, 3, 2)
    Wo, pl, pr = same_pad(W, 2, 2)
    padw = ((0, 0), (0, 0), (pt, pb), (pl, pr))
    tp, vp = np.pad(t, padw, constant_values=-np.inf), np.pad(s, padw, constant_values=0.0)
    win = lambda a: np.stack([a[:, :, dy : dy + 2 * Ho : 2, dx : dx + 2 * Wo : 2] for dy in range(3) for dx in range(2)], axis=-1)  # noqa: E731
    tw = win(tp)
    sel = np.argmax(tw, axis=-1)[..., None]
    pooled = np.take_along_axis(tw, sel, axis=-1)[..., 0]
    v_sel = np.take_along_axis(win(vp), sel, axis=-1)[..., 0]
    ps = prev[:, :, ::2, ::2]
    want = pooled + np.einsum("bihw,io->bohw", ps, wr) + br[None, :, None, None]
    S = (np.abs(sc[None, :, None, None] * v_sel) + np.abs(sh)[None, :, None, None] + np.einsum("bihw,io->bohw", np.abs(ps), np.abs(wr))
         + np.abs(br)[None, :, None, None])
    return want, S


def gemm_ref(A, W, bias, scale, shift, act):
    """act(f16(A) f16(W) + bias) [* scale + shift]: the operands rounded to f16 (round to nearest even), everything after that in float64.
    A [M][K], W [K][N]; bias, scale, shift [N] or None; act 1 = ReLU.  Returns (want, S), S = sum_k |a| |w| + |bias|."""
    a, w = np.asarray(A).astype(np.float16).astype(np.float64), np.asarray(W).astype(np.float16).astype(np.float64)
    b = np.zeros(w.shape[1]) if bias is None else np.asarray(bias, dtype=np.float64)
    z = a @ w + b
    S = np.abs(a) @ np.abs(w) + np.abs(b)
    if act == 1:
        z = np.maximum(z, 0.0)
    if scale is not None:
        z = z * np.asarray(scale, dtype=np.float64) + np.asarray(shift, dtype=np.float64)
    return z, S


def gemm_bound(S, K, scale, shift):
    """(K + 8) 2^-23 S_epi, S_epi = |scale| S + |shift| (S without an epilogue): the forward error of a K-term f32 sum in any order, with the unit
    roundoff doubled for the matrix unit's internal rounding and a few roundings for bias, scale and shift."""
    S_epi = S if scale is None else np.abs(np.asarray(scale, dtype=np.float64)) * S + np.abs(np.asarray(shift, dtype=np.float64))
    return (K + 8) * 2.0**-23 * S_epi


# ------------------------------------------------------------------------------------------------- orcai_h_pool_res_add: cases
# (C, Cp, H, W, k): what pool_res_add_h_body reaches there
POOL_SHAPES = {
    (30, 16, 12, 21, 3): "MT = 2, one K group, odd W",
    (12, 40, 9, 14, 3): "odd H; COp = 5: second K group with the o < COp guard",
    (33, 9, 7, 130, 3): "MT = 3, CO = 5: the oq >= CO skip; one channel in the last octet; several 64-pixel tasks",
    (64, 50, 6, 9, 3): "MT = 4, full octets",
    (7, 16, 5, 65, 5): "C < 8, R = 2, odd sizes",
    (50, 50, 1, 171, 5): "H = 1: pad_top = 1, both clamps; Wo = 86 over two tasks",
    (16, 30, 8, 64, 7): "R = 3, W = 64",
    (17, 64, 2, 3, 3): "W = 3, H = 2, Cp = 64",
}
POOL_B9 = (30, 16, 12, 21, 3)  # B = 9 there: 1 x 9 workgroups, so xcd_remap wraps past eight
POOL_EPS01 = (12, 40, 9, 14, 3)  # bn_eps = 0.1 there (1e-3 everywhere else)
POOL_CASES = [(shape, 2) for shape in POOL_SHAPES] + [(POOL_B9, 9)]


def pool_case_id(case):
    (C, Cp, H, W, k), B = case
    return f"C{C}-Cp{Cp}-{H}x{W}-k{k}-B{B}"


def pool_eps(shape):
    return 0.1 if tuple(shape) == POOL_EPS01 else 1e-3


def _pool_rng(shape, B, mode):
    C, Cp, H, W, k = shape
    return np.random.default_rng([C, Cp, H, W, k, B, mode])


def pool_int_case(shape, B):
    """Small integers: every product, sum and the result are integers below 2048, exact in f16 and in f32 in any order."""
    C, Cp, H, W, k = shape
    rng = _pool_rng(shape, B, 1)
    s = rng.integers(-50, 50, size=(B, C, H, W)).astype(np.float64)
    prev = rng.integers(-3, 4, size=(B, Cp, H, W)).astype(np.float64)
    wr = rng.integers(-1, 2, size=(Cp, C)).astype(np.float64)
    br = rng.integers(-3, 4, size=C).astype(np.float32)
    return s, prev, wr, br


def pool_bn_case(shape, B):
    """Real-valued data for BatchNorm on the fly.  s, prev and wr are f16-representable (a kernel stores them as f16, the reference must see what
    the kernel sees); br and the BatchNorm vectors are f32.  gamma ~ N(0, 1): both signs; channel C // 2 is exactly 0 and channel C - 1 (in the
    last, usually partial, octet) is negative."""
    C, Cp, H, W, k = shape
    rng = _pool_rng(shape, B, 2)
    f16 = lambda a: a.astype(np.float16).astype(np.float64)  # noqa: E731
    s, prev, wr = f16(2.0 * rng.standard_normal((B, C, H, W))), f16(rng.standard_normal((B, Cp, H, W))), f16(rng.standard_normal((Cp, C)) / 4)
    br = rng.standard_normal(C).astype(np.float32)
    mean, var = rng.standard_normal(C).astype(np.float32), (0.5 + rng.random(C)).astype(np.float32)
    gamma, beta = rng.standard_normal(C).astype(np.float32), rng.standard_normal(C).astype(np.float32)
    gamma[C // 2] = 0.0
    gamma[C - 1] = -0.5 - abs(gamma[C - 1])
    return s, prev, wr, br, (mean, var, gamma, beta)


# ------------------------------------------------------------------------------------------------- orcai_h_gemm_bias_act: cases
# (M, N, K).  Every M in {1, 5, 33, 70, 129}, N in {7, 17, 64, 65, 130}, K in {4, 12, 32, 36, 44, 60, 64, 100, 396}; every K with a tail (K % 32
# != 0) meets an M and an N that are no multiple of a tile (N = 64 is the only tile multiple: it goes with K = 64).
GEMM_SHAPES = {
    (1, 17, 4): "K < 32, K < 8: one partial 8-group; one row",
    (5, 7, 12): "K < 32; the second 8-group partial",
    (33, 65, 32): "exactly one K step; three 16-row tiles, N one past a block",
    (70, 130, 36): "K % 32 = 4: the second step holds half an 8-group; two row blocks, three column blocks",
    (129, 7, 44): "K % 32 = 12; three row blocks, the last one one row",
    (5, 130, 60): "K % 32 = 28: the last 8-group of the second step partial",
    (70, 64, 64): "two full K steps, N one full block",
    (33, 17, 100): "four K steps, the prefetch off on the last; K % 32 = 4",
    (129, 65, 396): "Dense-128's K: thirteen K steps, K % 32 = 12",
    (1, 130, 396): "one row at the longest K",
}
# (act, scale, with shift): scale "pm" = both signs
GEMM_EPILOGUES = [(0, None), (1, "pm"), (0, "pm")]


def _gemm_rng(shape, kind):
    return np.random.default_rng([*shape, kind])


def gemm_epilogue(rng, N, scale_kind, integers):
    """scale of both signs and a non-zero shift, or (None, None)."""
    if scale_kind is None:
        return None, None
    if integers:
        scale = np.where(np.arange(N) % 2 == 0, 2.0, -2.0).astype(np.float32)
        return scale, np.ones(N, dtype=np.float32)
    scale = rng.standard_normal(N).astype(np.float32)
    scale[0], scale[N - 1] = -abs(scale[0]) - 0.5, abs(scale[N - 1]) + 0.5
    return scale, (1.0 + rng.standard_normal(N)).astype(np.float32)


def gemm_int_case(shape):
    """Small integers, 70 % of the weights zero: exact in f16 operands and f32 sums."""
    M, N, K = shape
    rng = _gemm_rng(shape, 1)
    A = rng.integers(-2, 3, size=(M, K)).astype(np.float32)
    W = (rng.integers(-1, 2, size=(K, N)) * (rng.random((K, N)) < 0.3)).astype(np.float32)
    bias = rng.integers(-4, 5, size=N).astype(np.float32)
    return rng, A, W, bias


def gemm_float_case(shape):
    """A ~ N(0, 1) in f32, NOT rounded to f16 (the kernel's cast has to round it to nearest even as the reference does); W ~ N(0, 1) / sqrt(K)."""
    M, N, K = shape
    rng = _gemm_rng(shape, 2)
    A = rng.standard_normal((M, K)).astype(np.float32)
    W = (rng.standard_normal((K, N)) / np.sqrt(K)).astype(np.float32)
    bias = rng.standard_normal(N).astype(np.float32)
    return rng, A, W, bias
