"""Float64 references, launch geometry, case tables, derived bounds and comparison functions for the backward launchers of the f16 training
path (orcai_amd/csrc/half_bwd.hip) and the f32 pooling backward that shares their structure (pool_bwd_kernel of train_trunk.hip).  Plain numpy;
tests/test_half_bwd_ref.py checks this module on the CPU (against torch float64 autograd, and that every comparison rejects the bug it is there
for), tests/test_half_bwd_gpu.py holds the kernels to it.

Every reference models the f16 path's storage: an output the kernel stores in f16 is compared as f16, a reduction it finishes in float64 as
float64.  The bounds are functions of the reference (u16 = 2^-11, u32 = 2^-24); each is derived next to the kernel lines it counts."""

import functools

import numpy as np

from half_fwd_ref import from_quad_planes, split_planes, to_octet_planes, to_quad_planes  # noqa: F401  (the GPU tests take the layouts from here)
from oracle.model_ref import same_pad

U16, U32 = 2.0**-11, 2.0**-24
PB_ROWS = 8  # pooled rows per thread of pool_bwd_h_kernel / pool_bwd_kernel
EPS = 1e-3


def f16(a):
    return np.asarray(a).astype(np.float16).astype(np.float64)


def f32eps(eps):
    """The launchers take eps as a float: the reference uses that value, not the Python double."""
    return float(np.float32(eps))


def padded_width(W, k):
    return (W + k // 2 + 3) & ~3


def _cdiv(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------------- launch geometry (mirrors of the launchers)
def pool_geometry(H, W):
    """h_pool_bwd_bn_impl / pool_bwd_h_kernel: one thread per (chunk of PB_ROWS pooled rows, pooled column), 256 threads per workgroup."""
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    nchunk = _cdiv(Ho, PB_ROWS)
    threads = nchunk * Wo
    return dict(Ho=Ho, Wo=Wo, nchunk=nchunk, last_rows=Ho - PB_ROWS * (nchunk - 1), threads=threads, workgroups=_cdiv(threads, 256),
                idle_lanes=_cdiv(threads, 256) * 256 - threads)


def pointwise_geometry(C, Cin, H, W, k):
    """orcai_h_bn_bwd_pointwise / bn_bwd_pw_h_kernel<MT>: MT tiles of 16 conv-input channels, KG groups of 4 octets of conv-output channels, one wave
    per 64 flat pixels of the H image rows of the padded plane."""
    WP, CO = padded_width(W, k), _cdiv(C, 8)
    return dict(MT=_cdiv(Cin, 16), KG=_cdiv(CO, 4), CO=CO, WP=WP, tasks=_cdiv(H * WP, 64), partial_group=CO % 4 != 0, partial_octet=C % 8 != 0,
                tasks_per_row=WP / 64.0, last_task_past_plane=(k // 2) * WP + _cdiv(H * WP, 64) * 64 > (H + 2 * (k // 2)) * WP)


def outer_geometry(Ca, Cb, B, H, W, k, workspace_floats):
    """orcai_h_outer_reduce: 256-pixel chunks of the whole padded plane, at most 512 workgroups, at most workspace_floats / (Ca Cb) of them."""
    plane = (H + 2 * (k // 2)) * padded_width(W, k)
    nchunks = B * _cdiv(plane, 256)
    grid = min(nchunks, 512)
    limited = grid * Ca * Cb > workspace_floats
    if limited:
        grid = workspace_floats // (Ca * Cb)
    return dict(plane=plane, nchunks=nchunks, grid=grid, passes=_cdiv(nchunks, grid), workspace_limited=limited)


def stats_geometry(H, W, k):
    """orcai_h_bn_planes_stats: planes under 32768 16-byte vectors go through the sharded accumulators."""
    plane = (H + 2 * (k // 2)) * padded_width(W, k)
    return dict(plane=plane, sharded=plane < 32768)


def conv0_geometry(H, W):
    """h_conv0_bn_bwd_impl: a 256 x 256 grid-stride over the H W pixels of a snippet."""
    return dict(pixels_per_thread=_cdiv(H * W, 65536), blocks_with_work=min(256, _cdiv(H * W, 256)))


# ------------------------------------------------------------------------------------------------- references
def xhat_ref(v, mean, var, eps):
    v, mean, var = np.asarray(v, dtype=np.float64), np.asarray(mean, dtype=np.float64), np.asarray(var, dtype=np.float64)
    return (v - mean[None, :, None, None]) / np.sqrt(var + f32eps(eps))[None, :, None, None]


def pool_routing(v, dout, gamma):
    """-> contrib [6][B][C][Ho][Wo]: contrib[p] = the gradient window (i, j) sends to its position p = 2 dy + dx (Keras "same" 3 x 2 window, stride 2),
    all of dout[i][j] at the FIRST maximum of sign(gamma) * v in scan order, 0 elsewhere (the pad is -inf and never wins)."""
    v, dout = np.asarray(v, dtype=np.float64), np.asarray(dout, dtype=np.float64)
    H, W = v.shape[2:]
    sgn = np.where(np.asarray(gamma) < 0, -1.0, 1.0)
    Ho, pt, pb = same_pad(H, 3, 2)
    Wo, pl, pr = same_pad(W, 2, 2)
    tp = np.pad(v * sgn[None, :, None, None], ((0, 0), (0, 0), (pt, pb), (pl, pr)), constant_values=-np.inf)
    tw = np.stack([tp[:, :, dy : dy + 2 * Ho : 2, dx : dx + 2 * Wo : 2] for dy in range(3) for dx in range(2)])
    sel = np.argmax(tw, axis=0)  # the first maximum
    return np.stack([np.where(sel == p, dout, 0.0) for p in range(6)])


def pool_scatter(contrib, H, W):
    """The window gradients summed per input pixel -> dy [B][C][H][W]."""
    Ho, pt, pb = same_pad(H, 3, 2)
    Wo, pl, pr = same_pad(W, 2, 2)
    gp = np.zeros(contrib.shape[1:3] + (H + pt + pb, W + pl + pr))
    for p in range(6):
        dy, dx = divmod(p, 2)
        gp[:, :, dy : dy + 2 * Ho : 2, dx : dx + 2 * Wo : 2] += contrib[p]
    return gp[:, :, pt : pt + H, pl : pl + W]


def pool_bwd_ref(v, dout, gamma, mean, var, eps, k=3):
    """-> (dy, sum dy [C], sum dy * xhat [C], sum dout [C]).  k only names the planes' padding: the operation does not depend on it."""
    H, W = np.asarray(v).shape[2:]
    dy = pool_scatter(pool_routing(v, dout, gamma), H, W)
    xh = xhat_ref(v, mean, var, eps)
    return dy, dy.sum(axis=(0, 2, 3)), (dy * xh).sum(axis=(0, 2, 3)), np.asarray(dout, dtype=np.float64).sum(axis=(0, 2, 3))


def _bn_bwd(dy, v, mean, var, gamma, beta, eps, relu, sums=None):
    dy, v = np.asarray(dy, dtype=np.float64), np.asarray(v, dtype=np.float64)
    gamma64, beta64 = np.asarray(gamma, dtype=np.float64), np.asarray(beta, dtype=np.float64)
    n = dy.shape[0] * dy.shape[2] * dy.shape[3]
    xh = xhat_ref(v, mean, var, eps)
    bc = lambda a: np.asarray(a, dtype=np.float64)[None, :, None, None]  # noqa: E731
    de = np.where(xh * bc(gamma64) + bc(beta64) > 0, dy, 0.0) if relu else dy
    Sb, Sg = np.abs(de).sum(axis=(0, 2, 3)), np.abs(de * xh).sum(axis=(0, 2, 3))
    if sums is None:
        dbeta, dgamma = de.sum(axis=(0, 2, 3)), (de * xh).sum(axis=(0, 2, 3))
    else:
        dbeta, dgamma = (np.asarray(a, dtype=np.float64) for a in sums)
        Sb, Sg = np.maximum(Sb, np.abs(dbeta)), np.maximum(Sg, np.abs(dgamma))
    A = gamma64 / np.sqrt(np.asarray(var, dtype=np.float64) + f32eps(eps))
    dv = bc(A) * (de - bc(dbeta) / n - xh * bc(dgamma) / n)
    S = np.abs(bc(A)) * (np.abs(de) + bc(Sb) / n + np.abs(xh) * bc(Sg) / n)
    return dict(dbeta=dbeta, dgamma=dgamma, dv=dv, S=S, Sb=Sb, Sg=Sg, xhat=xh, de=de)


def bn_bwd_pointwise_ref(dy, v, mean, var, gamma, beta, eps, relu, sums=None):
    """BatchNorm (training mode) backward with the ReLU mask of its output: -> (dbeta [C], dgamma [C], dv [B][C][H][W]).  sums = (dbeta, dgamma) handed
    in (sums_ready = 1).  du is defined on a given stored dv (du_ref), so that it is judged on its own."""
    r = _bn_bwd(dy, v, mean, var, gamma, beta, eps, relu, sums)
    return r["dbeta"], r["dgamma"], r["dv"]


def bn_bwd_magnitudes(dy, v, mean, var, gamma, beta, eps, relu, sums=None):
    """-> dict: S = |A| (|de| + sum |de| / N + |xhat| sum |de xhat| / N) per element of dv (the size of what the kernel subtracts), Sb = sum |de|,
    Sg = sum |de xhat| per channel."""
    return _bn_bwd(dy, v, mean, var, gamma, beta, eps, relu, sums)


def du_ref(dv, wt):
    """du[b][i] = sum_o wt[o][i] dv[b][o] on the dv the kernel STORED (f16) and the f16 weights wt [C][Cin] -> (du, S = sum |wt| |dv|)."""
    dv, wt = np.asarray(dv, dtype=np.float64), np.asarray(wt, dtype=np.float64)
    return np.einsum("bohw,oi->bihw", dv, wt), np.einsum("bohw,oi->bihw", np.abs(dv), np.abs(wt))


def conv0_bn_wgrad_ref(x, dy, v, mean, var, gamma, beta, eps, k, sums=None):
    """The entry conv's weight gradient with bn0 + ReLU backward applied on the fly: dW[tap][c] = sum_{b, p} x[b][p + off(tap)] dv[b][c][p], zero
    outside the snippet.  x [B][H][W], dy / v [B][16][H][W] -> (dW [k k][16], dbeta, dgamma, T [k k][16] = sum |x| S: the size of the terms)."""
    r = _bn_bwd(dy, v, mean, var, gamma, beta, eps, 1, sums)
    x = np.asarray(x, dtype=np.float64)
    Bx, H, W = x.shape
    Rr = k // 2
    xp = np.zeros((Bx, H + 2 * Rr, W + 2 * Rr))
    xp[:, Rr : Rr + H, Rr : Rr + W] = x
    dW, T = np.zeros((k * k, 16)), np.zeros((k * k, 16))
    for dyy in range(k):
        for dx in range(k):
            win = xp[:, dyy : dyy + H, dx : dx + W]
            dW[dyy * k + dx] = np.einsum("bhw,bchw->c", win, r["dv"])
            T[dyy * k + dx] = np.einsum("bhw,bchw->c", np.abs(win), r["S"])
    return dW, r["dbeta"], r["dgamma"], T


def bn_stats_ref(v):
    """Mean and (biased) variance per channel of integer-valued v, each one correctly rounded float64 division of exact integers."""
    v = np.asarray(v, dtype=np.float64)
    n = v.shape[0] * v.shape[2] * v.shape[3]
    s, q = v.sum(axis=(0, 2, 3)), (v * v).sum(axis=(0, 2, 3))
    assert np.abs(q).max() * n < 2.0**53 and np.array_equal(s, np.rint(s))
    return s / n, (q * n - s * s) / (float(n) * n)


def shards_stats_ref(shards, C, count):
    """orcai_h_bn_finish_sharded on integer-valued shards [32][CO][16] (sum | sum of squares per octet)."""
    t = np.asarray(shards, dtype=np.float64).sum(axis=0)
    s, q = t[:, :8].reshape(-1)[:C], t[:, 8:].reshape(-1)[:C]
    return s / count, np.maximum((q * count - s * s) / (float(count) * count), 0.0)


def bn_apply_ref(v, mean, var, gamma, beta, eps, relu):
    """-> (y, S = |v s| + |beta| + |mean s|), s = gamma / sqrt(var + eps)."""
    v = np.asarray(v, dtype=np.float64)
    s = np.asarray(gamma, dtype=np.float64) / np.sqrt(np.asarray(var, dtype=np.float64) + f32eps(eps))
    bc = lambda a: np.asarray(a, dtype=np.float64)[None, :, None, None]  # noqa: E731
    y = v * bc(s) + bc(beta) - bc(mean) * bc(s)
    S = np.abs(v * bc(s)) + np.abs(bc(beta)) + np.abs(bc(mean) * bc(s))
    return (np.maximum(y, 0.0) if relu else y), S + 0.0 * y


def planes_sum_ref(x):
    return np.asarray(x, dtype=np.float64).sum(axis=(0, 2, 3))


def outer_ref(a, b, a_stride2):
    """D[ca][cb] = sum over snippets and pixels (i, x) of b's plane of a[ca][i][x] b[cb][i][x]; a_stride2: a lives on the plane twice as fine and is
    read at (2 i, 2 x).  -> (D, S = the same sum of |a| |b|)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    H, W = b.shape[2:]
    if a_stride2:
        a = a[:, :, ::2, ::2][:, :, :H, :W]
    return np.einsum("bchw,bdhw->cd", a, b), np.einsum("bchw,bdhw->cd", np.abs(a), np.abs(b))


def feat_to_planes_ref(f, C, H, W, k):
    """Keras Reshape layout f32 [B][H][W * C] -> f16 octet planes (round to nearest even), zero pads."""
    f = np.asarray(f)
    return to_octet_planes(f.reshape(f.shape[0], H, W, C).transpose(0, 3, 1, 2).astype(np.float16), k)


def relu_bwd_ref(dy, y):
    return np.where(np.asarray(y) > 0, dy, np.zeros_like(dy))


def relu_gate(dy, v, mean, var, gamma, beta, eps):
    """dy with zeros where xhat gamma + beta lies within 8 u32 (|xhat gamma| + |beta|) of zero (the kernel forms xhat with five f32 roundings and the
    gate with one fma: 6 u32 at the most), so that the float64 mask is the kernel's mask.  Inputs only.  -> (dy, share of positions zeroed)."""
    xh = xhat_ref(v, mean, var, eps)
    g, b = np.asarray(gamma, dtype=np.float64)[None, :, None, None], np.asarray(beta, dtype=np.float64)[None, :, None, None]
    near = np.abs(xh * g + b) <= 8 * U32 * (np.abs(xh * g) + np.abs(b))
    return np.where(near, 0.0, dy), float(near.mean())


# ------------------------------------------------------------------------------------------------- bounds
def f16_out_bound(ref, S, n_ops):
    """An f16 output of f32 arithmetic: e32 = n_ops u32 S for the f32 value (S >= |ref| is the size of the terms the expression adds up; with no
    cancellation it is |ref| itself), half an ulp of the f16 store of that value, and half the smallest subnormal."""
    e32 = n_ops * U32 * np.asarray(S, dtype=np.float64)
    return U16 * (np.abs(ref) + e32) + e32 + 2.0**-25


def f32_chain_bound(S, c):
    """An f32 result of f32 accumulation: c u32 sum |terms|, c the longest sequential chain plus the roundings inside one term."""
    return c * U32 * np.asarray(S, dtype=np.float64)


def f64_sum_bound(S):
    return 1e-12 * np.asarray(S, dtype=np.float64)


# Operation counts, from the kernels' expressions (half_bwd.hip).
# inv = rsqrtf(var + eps): one addition, v_rsq_f32 within 1 ulp = 2 u32                                              -> 3
# xhat = (v - mean) * inv: one subtraction, one product                                                              -> 3 + 2 = 5
N_XHAT = 5
# pool_bwd_h_kernel::emit: bqs = fmaf(gg, xhat, bqs) over a thread's own emits -- PB_ROWS windows x (2 rows x 2 columns) + the 2 of the image's last
# row = 34 sequential fma -- then float64 (wave_sum_lane63(double), LDS, atomicAdd(double)): 34 + N_XHAT.  pool_bwd_kernel (f32): the same loop.
C_POOL_SUMS = 4 * PB_ROWS + 2 + N_XHAT
# bn_bwd_value / fill_bn_bwd_table: dv = A (de - c1 - xhat c2)
#   c1 = (float)dbeta * inv_count: the cast, inv_count's own rounding, the product                                   -> 3
#   c2 likewise 3, and the kernel's float64 dgamma is a sum of f32 xhat values: 5 u32 sum |de xhat| -- counted on S's sum |de xhat| / N   -> 8
#   xhat * c2: 5 + 8 + 1 = 14; the two subtractions 2; A = gamma * inv 3 + 1 and the last product 1                   -> 14 + 2 + 5 = 21
N_BN_BWD = 21
# bn_planes_apply_h_kernel: r = fmaf(v, s, beta - mean * s), s = gamma * inv (4): mean * s 5, the subtraction 1, the fma 1                     -> 7
N_BN_APPLY = 7
# bn_planes_bwd_sums_h_kernel: q += (double)de * (double)xhat -- exact products of an f32 xhat                      -> N_XHAT u32 sum |de xhat|; + the f32 store
N_DGAMMA = N_XHAT


def mfma_sum_count(n_products):
    """A sum of n products accumulated in f32 in ANY order is within (n - 1) u32 sum |terms|; the unit roundoff is doubled for the matrix unit's
    internal rounding, as tests/half_fwd_ref.gemm_bound does."""
    return 2 * n_products


def outer_chain(geo):
    """outer_reduce_h_kernel: an accumulator takes `passes` passes of 256 pixels (8 MFMA of 32); add_partials_h_kernel: a thread adds
    ceil(ceil(grid / 8) / 4) partials into each of four sums, three additions join them, up to 8 float atomics land on D, which holds a start value."""
    return mfma_sum_count(256 * geo["passes"]) + _cdiv(_cdiv(geo["grid"], 8), 4) + 3 + 8 + 1


def conv0_chain(B, H, W):
    """conv0_bn_wgrad_h_kernel: B * pixels_per_thread sequential fma per accumulator, wave_sum_lane63 6 levels, 3 additions over the waves, up to
    256 workgroups' float atomics on dW (which holds a start value), and the N_BN_BWD roundings inside a term."""
    return B * conv0_geometry(H, W)["pixels_per_thread"] + 6 + 3 + 256 + 1 + N_BN_BWD


# ------------------------------------------------------------------------------------------------- comparison functions
def check_planes(bits, C, H, W, k, fill_bits, tag="", group=8, written=True):
    """Octet (or quad) planes as bit patterns, pre-filled with fill_bits: every pad keeps the fill, the channels >= C of the last group are zero at
    the image's pixels, every real element was written (written = False: the fill is a value a result may take, as in an in-place call).
    -> the real elements [B][C][H][W] (bits)."""
    if group == 8:
        valid, zeros, pads = split_planes(bits, C, H, W, k)
    else:
        Bq, CQ, HP, WP, _ = bits.shape
        Rr = k // 2
        full = bits.transpose(0, 1, 4, 2, 3).reshape(Bq, CQ * 4, HP, WP)
        inside = np.zeros((HP, WP), dtype=bool)
        inside[Rr : Rr + H, :W] = True
        valid, zeros, pads = full[:, :C, Rr : Rr + H, :W], full[:, C:, Rr : Rr + H, :W], full[:, :, ~inside]
    sign = 0x7FFF if bits.dtype == np.uint16 else 0x7FFFFFFF
    assert (pads == fill_bits).all(), f"{tag}: {(pads != fill_bits).sum()} pad elements written"
    assert ((zeros & sign) == 0).all(), f"{tag}: {((zeros & sign) != 0).sum()} elements of channels >= C are not zero"
    assert not written or (valid != fill_bits).all(), f"{tag}: {(valid == fill_bits).sum()} real elements not written"
    return np.ascontiguousarray(valid)


def check_equal(got, want, tag=""):
    """Bit equality of values (-0 equals +0)."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (tag, got.shape, want.shape)
    bad = got != want
    assert not bad.any(), f"{tag}: {bad.sum()} of {bad.size} differ, first at {tuple(np.argwhere(bad)[0])}, max |got - want| = {np.abs(got - want)[bad].max():.3e}"
    return 0.0


def check_within(got, want, bound, tag=""):
    """|got - want| <= bound per element -> the largest error / bound (printed by the GPU tests, recorded in DESIGN.md)."""
    got, want, bound = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    assert got.shape == want.shape, (tag, got.shape, want.shape)
    assert np.isfinite(got).all(), f"{tag}: not finite"
    err = np.abs(got - want)
    ratio = np.where(err == 0, 0.0, err / np.maximum(bound, 1e-300))
    worst = float(ratio.max())
    assert worst <= 1.0, f"{tag}: error / bound = {worst:.3f} at {np.unravel_index(np.argmax(ratio), ratio.shape)} (|got - want| = {err.reshape(-1)[np.argmax(ratio)]:.3e})"
    return worst


# ------------------------------------------------------------------------------------------------- cases: pooling backward
# (C, H, W, k), B = 2.  Every H in {17, 18, 19, 20, 33} with W in {6, 21}; (33, 171): two workgroups per (snippet, octet); (1, 64): one row, one
# chunk; (18, 1): one column.  C and k rotate so that every pair of C in {7, 30, 64} and k in {3, 5, 7} occurs.
_POOL_HW = [(H, W) for H in (17, 18, 19, 20, 33) for W in (6, 21)] + [(33, 171), (1, 64), (18, 1)]
POOL_B = 2
POOL_CASES = [((7, 30, 64)[i % 3], H, W, (3, 5, 7)[(i // 3) % 3]) for i, (H, W) in enumerate(_POOL_HW)]
POOL_FAMILIES = ("ties", "grid")


def pool_case_id(case):
    C, H, W, k = case
    return f"C{C}-{H}x{W}-k{k}"


def _bn_vectors(rng, C):
    """mean, var, gamma, beta in f32; gamma of both signs (channel 0 negative, channel C - 1 positive)."""
    mean, var = (0.3 * rng.standard_normal(C)).astype(np.float32), (0.5 + rng.random(C)).astype(np.float32)
    gamma, beta = rng.standard_normal(C).astype(np.float32), (0.2 * rng.standard_normal(C)).astype(np.float32)
    gamma[0], gamma[C - 1] = -0.5 - abs(gamma[0]), 0.5 + abs(gamma[C - 1])
    return mean, var, gamma, beta


@functools.lru_cache(maxsize=None)
def pool_case(case, family):
    """-> dict(v, dout, mean, var, gamma, dy, s_dy, s_dyx, s_dout, S_dyx): inputs (float64 values that f16 holds exactly) and the reference, computed once.
    ties: small integers.  grid: v normal f16, dout multiples of 2^-6 in [-4, 4]: a pixel collects at most two windows' gradients, the sum is a
    multiple of 2^-6 below 8 -- exact in f16 -- and every f32 sum of them is exact in any order."""
    C, H, W, k = case
    rng = np.random.default_rng([C, H, W, k, POOL_FAMILIES.index(family)])
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    if family == "ties":
        v = rng.integers(-2, 3, size=(POOL_B, C, H, W)).astype(np.float64)
        dout = rng.integers(-4, 5, size=(POOL_B, C, Ho, Wo)).astype(np.float64)
    else:
        v = f16(2.0 * rng.standard_normal((POOL_B, C, H, W)))
        dout = rng.integers(-256, 257, size=(POOL_B, C, Ho, Wo)).astype(np.float64) / 64.0
    mean, var, gamma, _ = _bn_vectors(rng, C)
    dy, s_dy, s_dyx, s_dout = pool_bwd_ref(v, dout, gamma, mean, var, EPS, k)
    S_dyx = np.abs(dy * xhat_ref(v, mean, var, EPS)).sum(axis=(0, 2, 3))
    out = dict(v=v, dout=dout, mean=mean, var=var, gamma=gamma, dy=dy, s_dy=s_dy, s_dyx=s_dyx, s_dout=s_dout, S_dyx=S_dyx)
    for a in out.values():
        a.setflags(write=False)
    return out


# ------------------------------------------------------------------------------------------------- cases: orcai_h_bn_bwd_pointwise
# (C, Cin, H, W, k, relu, sums_ready, in_place), B = 2
_PW_CC = {"a": (7, 9), "b": (30, 24), "c": (44, 40), "d": (64, 64), "e": (9, 64)}
_PW_HW = {"p": (1, 64), "q": (5, 65), "r": (8, 171), "s": (9, 21)}
_PW_TABLE = [("a", "p", 3, 0, 0, 0), ("b", "q", 3, 1, 1, 0), ("c", "r", 3, 0, 1, 0), ("d", "s", 3, 1, 0, 0), ("e", "q", 3, 1, 0, 0), ("a", "r", 5, 1, 1, 0),
             ("b", "s", 7, 0, 0, 0), ("c", "p", 5, 1, 0, 0), ("d", "q", 7, 0, 1, 0), ("e", "r", 7, 1, 1, 0), ("a", "s", 3, 1, 1, 0), ("b", "p", 3, 0, 1, 0),
             ("c", "s", 5, 0, 1, 0), ("d", "r", 3, 0, 0, 0), ("e", "p", 5, 0, 0, 0), ("b", "q", 3, 1, 0, 1)]
PW_B = 2
PW_CASES = [_PW_CC[row[0]] + _PW_HW[row[1]] + row[2:] for row in _PW_TABLE]


def pw_case_id(case):
    C, Cin, H, W, k, relu, ready, inplace = case
    return f"C{C}-Cin{Cin}-{H}x{W}-k{k}-relu{relu}-ready{ready}" + ("-inplace" if inplace else "")


@functools.lru_cache(maxsize=None)
def pw_case(case):
    """dy ~ N(0, 1), v ~ 2 N(0, 1), wt ~ N(0, 1) / 4 [C][Cin], all f16-representable; dy zeroed at the ReLU gate (relu_gate)."""
    C, Cin, H, W, k, relu, ready, inplace = case
    rng = np.random.default_rng([C, Cin, H, W, k, relu, ready, inplace])
    dy, v = f16(rng.standard_normal((PW_B, C, H, W))), f16(2.0 * rng.standard_normal((PW_B, C, H, W)))
    mean, var, gamma, beta = _bn_vectors(rng, C)
    wt = f16(rng.standard_normal((C, Cin)) / 4)
    gated = 0.0
    if relu:
        dy, gated = relu_gate(dy, v, mean, var, gamma, beta, EPS)
    r = _bn_bwd(dy, v, mean, var, gamma, beta, EPS, relu)
    out = dict(dy=dy, v=v, mean=mean, var=var, gamma=gamma, beta=beta, wt=wt, gated=np.float64(gated), **r)
    for a in out.values():
        np.asarray(a).setflags(write=False)
    return out


# ------------------------------------------------------------------------------------------------- cases: orcai_h_outer_reduce
# (Ca, Cb, H, W, k, B, workspace_floats or 0 = ample, a_stride2), what the case is there for
OUTER_CASES = {
    (7, 16, 8, 171, 7, 2, 0, 0): "ragged Ca, one column tile",
    (16, 17, 5, 65, 5, 2, 0, 0): "two column tiles, one channel in the second",
    (17, 64, 1, 64, 3, 2, 0, 0): "two row tiles, four column tiles: two tiles per wave",
    (64, 7, 8, 171, 7, 2, 0, 0): "four row tiles",
    (64, 64, 5, 65, 5, 2, 0, 0): "16 tiles: four per wave",
    (17, 7, 8, 171, 7, 52, 0, 0): "B ceil(plane / 256) = 520 > 512: the grid-stride loop",
    (17, 16, 5, 65, 5, 2, 3 * 17 * 16, 0): "a workspace of exactly 3 Ca Cb floats: three workgroups, two passes each",
    (16, 17, 4, 86, 7, 2, 0, 1): "a_stride2: A on the 8 x 171 plane, read at (2 i, 2 x)",
}
OUTER_AMPLE = 512 * 64 * 64
OUTER_FAMILIES = ("exact", "normal")


def outer_case_id(case):
    Ca, Cb, H, W, k, B, ws, s2 = case
    return f"Ca{Ca}-Cb{Cb}-{H}x{W}-k{k}-B{B}" + (f"-ws{ws}" if ws else "") + ("-stride2" if s2 else "")


def outer_geo(case):
    Ca, Cb, H, W, k, B, ws, s2 = case
    return outer_geometry(Ca, Cb, B, H, W, k, ws or OUTER_AMPLE)


@functools.lru_cache(maxsize=None)
def outer_case(case, family):
    """exact: integers in [-2, 2] (every partial sum an integer below 2^24); normal: N(0, 1) rounded to f16.  -> dict(a, b, D, S, Ha, Wa)."""
    Ca, Cb, H, W, k, B, ws, s2 = case
    rng = np.random.default_rng([Ca, Cb, H, W, k, B, s2, OUTER_FAMILIES.index(family)])
    Ha, Wa = (2 * H, 2 * W - 1) if s2 else (H, W)
    if family == "exact":
        a, b = rng.integers(-2, 3, size=(B, Ca, Ha, Wa)).astype(np.float64), rng.integers(-2, 3, size=(B, Cb, H, W)).astype(np.float64)
    else:
        a, b = f16(rng.standard_normal((B, Ca, Ha, Wa))), f16(rng.standard_normal((B, Cb, H, W)))
    D, S = outer_ref(a, b, s2)
    out = dict(a=a, b=b, D=D, S=S)
    for x in out.values():
        x.setflags(write=False)
    out.update(Ha=Ha, Wa=Wa)
    return out


# ------------------------------------------------------------------------------------------------- cases: BatchNorm statistics and apply
# (C, H, W, k, B)
STATS_CASES = {(30, 8, 16, 3, 8): "sharded route, 1024 elements per channel", (13, 5, 65, 5, 3): "sharded route, odd sizes, ragged octet",
               (9, 190, 171, 3, 1): "plane of 192 x 172 = 33024 >= 32768 vectors: the unsharded route"}
# (C, H, W, k, relu)
APPLY_CASES = [(9, 5, 65, 5, 1), (30, 8, 171, 7, 0), (64, 1, 64, 3, 1), (7, 9, 21, 3, 0)]
APPLY_B = 2


def ints_case(shape, seed, lo=-4, hi=4):
    return np.random.default_rng(seed).integers(lo, hi + 1, size=shape).astype(np.float64)


# ------------------------------------------------------------------------------------------------- cases: orcai_h_conv0_bn_bwd
# (H, W, k, B, snippet_stride - H W)
CONV0_CASES = [(H, W, k, 3, (0, 37)[(i + j) % 2]) for i, k in enumerate((3, 5, 7)) for j, (H, W) in enumerate(((8, 171), (5, 65), (1, 64), (16, 12)))] + [(400, 171, 3, 1, 0)]


def conv0_case_id(case):
    H, W, k, B, extra = case
    return f"{H}x{W}-k{k}-B{B}" + (f"-stride+{extra}" if extra else "")


@functools.lru_cache(maxsize=None)
def conv0_case(case):
    """x in [0, 1), dy ~ N(0, 1), v ~ 2 N(0, 1), all f16-representable; dy zeroed at the ReLU gate."""
    H, W, k, B, extra = case
    rng = np.random.default_rng([H, W, k, B, extra])
    x = f16(rng.random((B, H, W)))
    dy, v = f16(rng.standard_normal((B, 16, H, W))), f16(2.0 * rng.standard_normal((B, 16, H, W)))
    mean, var, gamma, beta = _bn_vectors(rng, 16)
    dy, gated = relu_gate(dy, v, mean, var, gamma, beta, EPS)
    dW, dbeta, dgamma, T = conv0_bn_wgrad_ref(x, dy, v, mean, var, gamma, beta, EPS, k)
    mag = bn_bwd_magnitudes(dy, v, mean, var, gamma, beta, EPS, 1)
    out = dict(x=x, dy=dy, v=v, mean=mean, var=var, gamma=gamma, beta=beta, dW=dW, dbeta=dbeta, dgamma=dgamma, T=T, Sb=mag["Sb"], Sg=mag["Sg"], gated=np.float64(gated))
    for a in out.values():
        np.asarray(a).setflags(write=False)
    return out
