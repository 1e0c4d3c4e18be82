"""The recurrent head's two f32 GEMM launchers, called directly through the C ABI and compared with float64.

orcai_gemm_strided (train_head.hip) hides three kernels and three shape-dependent choices behind one entry point:
gemm_tiled_kernel<0,0> for A^T B (weight gradients), gemm_tiled_kernel<1,1> for A B^T (data gradients), the generic
gemm_strided_kernel for every other stride pattern; split-K with float atomics behind a zero fill; a 16-byte or a scalar
load path per operand (pointer alignment and leading dimension); and the L2 term Wreg, which a split product must add once.
orcai_gemm_bias_act (model_fwd.hip) is the forward GEMM and the eval-mode input gradient's GEMM.

Two comparisons, each blind where the other sees:
  * exact integers: small integer operands, power-of-two alpha / beta_w; every partial sum in any order (atomics included)
    is exact below 2^24, so the result equals the float64 product bit for bit.  Sees any indexing, clamping, zero-fill or
    add-once error; cannot see an operand rounded to a narrower type (small integers survive that).
  * standard-normal operands against float64 with the worst-case summation bound
        |got - ref| <= gamma_n (|alpha| (|A| |B|) + |beta_w Wreg| + |C0|),   gamma_n = n u / (1 - n u),  u = 2^-24,
    n = K + splits + 3: K products summed in any order, one rounding per split from the atomic add, and the epilogue
    (alpha, the Wreg fma, the accumulate add).  Derived, not measured.  Sees a narrower operand type at small K."""

import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

U = 2.0**-24
SENTINEL = 12345.0  # what C holds before an accumulate = 0 call: a missing zero fill in front of the atomics shows as + 12345


def gamma(n):
    return n * U / (1.0 - n * U)


def split_plan(M, N, K):
    """The launcher's rule for the two tiled layouts: (splits, k_per_split)."""
    tiles = -(-N // 64) * -(-M // 64)
    splits = 1
    if tiles < 768 and K >= 256:
        splits = max(1, min(-(-1024 // tiles), K // 128))
    kps = -(-(-(-K // splits)) // 32) * 32
    return -(-K // kps), kps


# (M, N, K): (splits, length of the last split, the launcher branch the case is there for)
CASES = {
    (60, 512, 144): (1, 144, "no split (K < 256); last 32-tile holds 16 of K"),
    (60, 512, 255): (1, 255, "no split, one below the threshold; last 32-tile holds 31 of K"),
    (60, 512, 256): (2, 128, "the threshold: 2 splits of 128"),
    (60, 512, 257): (2, 97, "160 + 97: ragged last split, 1 of K in its last 32-tile"),
    (256, 128, 2944): (23, 128, "orcai-V1's dW1 at batch 64: 23 even splits"),
    (256, 128, 2949): (19, 69, "19 splits of 160, the last one 69 long"),
    (1, 1, 300): (2, 140, "one row, one column, split"),
    (65, 63, 300): (2, 140, "row tail across two 64-tiles, column tail inside one, split"),
    (130, 7, 320): (2, 160, "three row tiles, 7 columns (dz2 with 7 labels), two even splits"),
    (1800, 1800, 256): (1, 256, "841 tiles >= 768: no split although K >= 256"),
    (5, 3, 1): (1, 1, "degenerate: K = 1"),
    (64, 64, 32): (1, 32, "exactly one 64 x 64 x 32 tile"),
    (33, 130, 31): (1, 31, "tails in M, N and K, no split"),
    (70, 20, 8): (1, 8, "small K = 8 (a narrower operand type shows against the float bound)"),
}
SPLIT_CASES = [c for c, v in CASES.items() if v[0] > 1]

# (alpha, accumulate, Wreg present); beta_w = 2 wherever Wreg is present
FLAGS = [(1.0, 0, False), (0.5, 0, False), (-2.0, 0, False), (1.0, 1, False), (1.0, 0, True), (0.5, 1, True), (-2.0, 1, True)]
BETA_W = 2.0

# how an operand [rows][extent] lies in memory: (leading dimension, offset of the base pointer in floats)
#   "v": a column slice of a wider tensor (as training.py passes hp.view(-1)[d*u:] with ld = 2u), 16-byte aligned, ld % 4 == 0 -> 16-byte loads
#   "o": the same slice one float further on -> scalar loads because of the pointer
#   "l": ld = the smallest value >= extent with ld % 4 == 3 (7 for dz2's 7 labels) -> scalar loads because of the leading dimension
#   "c": contiguous, ld = extent
PLACEMENTS = {
    "v": lambda e: ((e + 3) // 4 * 4 + 8, 4),
    "o": lambda e: ((e + 3) // 4 * 4 + 8, 1),
    "l": lambda e: (e + (3 - e) % 4, 0),
    "c": lambda e: (e, 0),
}


def _takes_vector_path(place, extent):
    ld, off = PLACEMENTS[place](extent)
    return off % 4 == 0 and ld % 4 == 0


def test_case_table_reaches_the_branches_it_names():
    """The split count of every case, recomputed from the launcher's rule: a later change of the rule must not silently empty a case."""
    for (M, N, K), (splits, last, _) in CASES.items():
        s, kps = split_plan(M, N, K)
        assert (s, K - (s - 1) * kps) == (splits, last), ((M, N, K), s, kps)
        assert 0 < K - (s - 1) * kps <= kps
    assert split_plan(60, 512, 257) == (2, 160) and split_plan(256, 128, 2944) == (23, 128) and split_plan(256, 128, 2949) == (19, 160)
    assert (-(-1800 // 64)) ** 2 == 841 >= 768
    assert len(SPLIT_CASES) == 7
    # both values of the launcher's vector-path predicate, and ld = 7
    assert _takes_vector_path("v", 130) and not _takes_vector_path("o", 130) and not _takes_vector_path("l", 130)
    assert PLACEMENTS["l"](7) == (7, 0) and PLACEMENTS["l"](130)[0] % 4 == 3


def _draw(rng, shape, kind, sparse=False):
    if kind == "float":
        return rng.standard_normal(shape).astype(np.float32)
    v = rng.integers(-2, 3, size=shape)
    if sparse:
        v = rng.integers(-1, 2, size=shape) * (rng.random(shape) < 0.3)
    return v.astype(np.float32)


def _embed(rng, logical, place, kind, elem_stride=1):
    """Store logical [rows][extent] with the placement's leading dimension behind `off` floats; everything around it is filled with values of
    the same kind, so a read outside the operand changes the result.  elem_stride = 2 interleaves a second value after every element.
    Returns (device tensor that owns the memory, base pointer, ld in floats)."""
    rows, extent = logical.shape
    ld, off = PLACEMENTS[place](extent * elem_stride)
    flat = _draw(rng, off + rows * ld + 8, kind)
    view = flat[off : off + rows * ld].reshape(rows, ld)
    view[:, : extent * elem_stride : elem_stride] = logical
    dev = torch.from_numpy(flat).cuda()
    return dev, dev.data_ptr() + 4 * off, ld


@functools.lru_cache(maxsize=4)
def _problem(M, N, K, kind):
    """Operands, Wreg, the prior C and the float64 products of one case (shared by every layout, placement and flag; never modified)."""
    rng = np.random.default_rng(1000 * M + 10 * N + K)
    A, B = _draw(rng, (M, K), kind), _draw(rng, (K, N), kind, sparse=True)
    W = _draw(rng, (M, N), kind) * (1.0 if kind == "float" else 2.0)
    C0 = _draw(rng, (M, N), kind) * (1.0 if kind == "float" else 4.0)
    A64, B64 = A.astype(np.float64), B.astype(np.float64)
    out = dict(A=A, B=B, W=W.astype(np.float32), C0=C0.astype(np.float32), P=A64 @ B64, absP=np.abs(A64) @ np.abs(B64))
    for v in out.values():
        v.setflags(write=False)
    return out


def _layout_operands(rng, pb, layout, pa, pbm, kind):
    """(owner tensors, A pointer, sam, sak, B pointer, sbk, sbn) of pb's operands stored in `layout`."""
    A, B = pb["A"], pb["B"]
    if layout == "AtB":  # A stored [K][lda], B stored [K][ldb]
        ta, a, lda = _embed(rng, np.ascontiguousarray(A.T), pa, kind)
        tb, b, ldb = _embed(rng, B, pbm, kind)
        return (ta, tb), a, 1, lda, b, ldb, 1
    if layout == "ABt":  # A stored [M][lda], B stored [N][ldb]
        ta, a, lda = _embed(rng, A, pa, kind)
        tb, b, ldb = _embed(rng, np.ascontiguousarray(B.T), pbm, kind)
        return (ta, tb), a, lda, 1, b, 1, ldb
    if layout == "mixed":  # A [M][K] and B [K][N], both row-major: the generic kernel
        ta, a, lda = _embed(rng, A, pa, kind)
        tb, b, ldb = _embed(rng, B, pbm, kind)
        return (ta, tb), a, lda, 1, b, ldb, 1
    assert layout == "strided"  # neither stride of A is 1: A [M][K][2], element 0 of every pair
    ta, a, lda = _embed(rng, A, pa, kind, elem_stride=2)
    tb, b, ldb = _embed(rng, B, pbm, kind)
    return (ta, tb), a, lda, 2, b, ldb, 1


def _expected_kernel(sam, sak, sbk, sbn):
    am = 0 if sam == 1 else (1 if sak == 1 else -1)
    bm = 0 if sbn == 1 else (1 if sbk == 1 else -1)
    return "tiled" if am >= 0 and am == bm else "generic"


def _check_case(M, N, K, layout, kind, placements, flags):
    from orcai_amd import _native as N_

    lib = N_.lib()
    pb = _problem(M, N, K, kind)
    splits = split_plan(M, N, K)[0] if layout in ("AtB", "ABt") else 1
    rng = np.random.default_rng(7)
    Wd, C0d = torch.from_numpy(pb["W"].copy()).cuda(), torch.from_numpy(pb["C0"].copy()).cuda()
    for pa, pbm in placements:
        owners, a, sam, sak, b, sbk, sbn = _layout_operands(rng, pb, layout, pa, pbm, kind)
        # the kernel the launcher picks for these strides (a contiguous operand of extent 1 has two unit strides: still a tiled kernel)
        assert _expected_kernel(sam, sak, sbk, sbn) == ("tiled" if layout in ("AtB", "ABt") else "generic"), (layout, sam, sak, sbk, sbn)
        for alpha, accumulate, wreg in flags:
            C = C0d.clone() if accumulate else torch.full((M, N), SENTINEL, dtype=torch.float32, device="cuda")
            N_.check(lib.orcai_gemm_strided(a, sam, sak, b, sbk, sbn, N_.ptr(C), M, N, K, alpha, accumulate, N_.ptr(Wd) if wreg else None, BETA_W if wreg else 0.0,
                                            N_.stream_ptr()), "orcai_gemm_strided")
            got = C.cpu().numpy().astype(np.float64)
            ref = alpha * pb["P"] + (BETA_W * pb["W"] if wreg else 0.0) + (pb["C0"] if accumulate else 0.0)
            mag = abs(alpha) * pb["absP"] + (np.abs(BETA_W * pb["W"]) if wreg else 0.0) + (np.abs(pb["C0"]) if accumulate else 0.0)
            what = (M, N, K, layout, pa + pbm, alpha, accumulate, wreg, f"splits={splits}")
            if kind == "int":
                assert float(np.max(mag)) < 2.0**24, what  # every partial sum in any order is an exactly representable integer or half-integer
                assert np.array_equal(got, ref), (what, float(np.abs(got - ref).max()), int((got != ref).sum()))
            else:
                bound = gamma(K + splits + 3) * mag
                excess = np.abs(got - ref) - bound
                assert float(excess.max()) <= 0.0, (what, float(np.abs(got - ref).max()), float(bound.flat[int(excess.argmax())]))


# the full flag list on aligned column slices and on contiguous storage; every other value of the two vector-path predicates with the plain product and with all flags at once
_TILED_PLAN = [([("v", "v")], FLAGS), ([("c", "c")], FLAGS[:1] + FLAGS[-1:]), ([("o", "v"), ("v", "o"), ("l", "l"), ("o", "l")], FLAGS[:1] + FLAGS[-2:])]


@pytest.mark.parametrize("kind", ["int", "float"])
@pytest.mark.parametrize("layout", ["AtB", "ABt"])
@pytest.mark.parametrize("shape", list(CASES), ids=lambda s: "x".join(map(str, s)))
def test_gemm_strided_tiled_layouts(shape, layout, kind):
    """gemm_tiled_kernel<0,0> (A^T B) and <1,1> (A B^T) at every case of CASES (each names the launcher branch it reaches): alpha in {1, 0.5, -2},
    accumulate onto a non-zero C, Wreg with beta_w = 2, a sentinel in C where accumulate = 0, and both load paths of each operand."""
    for placements, flags in _TILED_PLAN:
        _check_case(*shape, layout, kind, placements, flags)


@pytest.mark.parametrize("kind", ["int", "float"])
@pytest.mark.parametrize("layout", ["mixed", "strided"])
@pytest.mark.parametrize("shape", [(60, 512, 257), (65, 63, 300), (130, 7, 320), (5, 3, 1), (64, 64, 32), (33, 130, 31), (70, 20, 8)], ids=lambda s: "x".join(map(str, s)))
def test_gemm_strided_generic_kernel(shape, layout, kind):
    """gemm_strided_kernel: A [M][K] with B [K][N] (both row-major), and an A neither of whose strides is 1.  It never splits (K tail of its
    16-wide tiles at K = 257, 300, 31, 8, 1)."""
    _check_case(*shape, layout, kind, [("v", "v"), ("o", "l")], FLAGS)


def test_gemm_strided_argument_checks():
    from orcai_amd import _native as N_

    lib = N_.lib()
    A, B = torch.ones(8, 8, device="cuda"), torch.ones(8, 8, device="cuda")
    C = torch.full((8, 8), SENTINEL, device="cuda")
    a, b, c, st = N_.ptr(A), N_.ptr(B), N_.ptr(C), N_.stream_ptr()
    call = lambda a_, b_, c_, M, N, K: lib.orcai_gemm_strided(a_, 1, 8, b_, 8, 1, c_, M, N, K, 1.0, 0, None, 0.0, st)  # noqa: E731
    assert call(None, b, c, 8, 8, 8) == N_.E_BADARG and call(a, None, c, 8, 8, 8) == N_.E_BADARG and call(a, b, None, 8, 8, 8) == N_.E_BADARG
    assert call(a, b, c, 0, 8, 8) == N_.E_BADARG and call(a, b, c, 8, 0, 8) == N_.E_BADARG and call(a, b, c, 8, 8, 0) == N_.E_BADARG
    assert call(a, b, c, -1, 8, 8) == N_.E_BADARG
    assert bool((C == SENTINEL).all())  # nothing was launched
    assert call(a, b, c, 8, 8, 8) == 0
    assert bool((C == 8.0).all())


# ------------------------------------------------------------------------------------------------------------------------------------
# orcai_gemm_bias_act: C = act(A B + bias) [* scale + shift], A [M][K], B [K][N] row-major, contiguous.
# Float bound: gamma_{K+3} ((|A| |B| + |bias|) |scale| + |shift|): K products, the bias add, the scale / shift fma; ReLU is 1-Lipschitz and exact.
# ------------------------------------------------------------------------------------------------------------------------------------
GBA_M, GBA_N, GBA_K = (1, 127, 128, 129, 300), (1, 7, 128, 130, 512), (1, 31, 32, 33, 36, 60, 396)


def _gba_vec(K, N, a_off):
    """The launcher's predicate for 16-byte loads (the allocations themselves are 16-byte aligned)."""
    return K % 4 == 0 and N % 4 == 0 and a_off % 4 == 0


def test_gemm_bias_act_cases_cover_both_load_paths():
    shapes = [(K, N) for K in GBA_K for N in GBA_N]
    assert any(_gba_vec(K, N, 0) for K, N in shapes) and any(K % 4 and N % 4 for K, N in shapes)
    assert any(K % 4 == 0 and N % 4 for K, N in shapes) and any(K % 4 and N % 4 == 0 for K, N in shapes)
    assert not _gba_vec(396, 512, 1)


@pytest.mark.parametrize("kind", ["int", "float"])
@pytest.mark.parametrize("K", GBA_K)
def test_gemm_bias_act_vs_float64(K, kind):
    """gemm_kernel at M in {1, 127, 128, 129, 300} x N in {1, 7, 128, 130, 512} for one K: bias present / null (as the eval-mode gradient passes it),
    act 0 / 1, scale + shift present / absent, and A one float off 16-byte alignment (scalar loads where the shape alone would allow 16-byte ones)."""
    from orcai_amd import _native as N_

    lib, st = N_.lib(), N_.stream_ptr()
    rng = np.random.default_rng(40 + K)
    for M in GBA_M:
        A = _draw(rng, (M, K), kind)
        # A behind one extra float: the view from element 1 is the same matrix at a pointer that is 4 bytes past a 16-byte boundary
        Aoff = torch.from_numpy(np.concatenate([_draw(rng, 1, kind), A.ravel(), _draw(rng, 8, kind)])).cuda()
        Ad = torch.from_numpy(A).cuda()
        assert Ad.data_ptr() % 16 == 0 and Aoff.data_ptr() % 16 == 0
        for N in GBA_N:
            B = _draw(rng, (K, N), kind, sparse=True)
            bias, scale, shift = _draw(rng, N, kind), _draw(rng, N, kind), _draw(rng, N, kind)
            if kind == "int":
                bias, scale, shift = bias * 2.0, scale + 3.0, shift * 2.0  # small integers: the epilogue stays exact
            Bd, bd, sd, hd = (torch.from_numpy(v).cuda() for v in (B, bias, scale, shift))
            assert Bd.data_ptr() % 16 == 0
            P = A.astype(np.float64) @ B.astype(np.float64)
            absP = np.abs(A).astype(np.float64) @ np.abs(B).astype(np.float64)
            for use_bias in (1, 0):
                for act in (0, 1):
                    for use_scale in (0, 1):
                        for a_off in (0, 1) if (use_bias, act, use_scale) in ((1, 0, 0), (0, 1, 1)) else (0,):
                            C = torch.full((M, N), SENTINEL, dtype=torch.float32, device="cuda")
                            a = Ad.data_ptr() if a_off == 0 else Aoff.data_ptr() + 4
                            N_.check(lib.orcai_gemm_bias_act(a, N_.ptr(Bd), N_.ptr(bd) if use_bias else None, N_.ptr(sd) if use_scale else None,
                                                             N_.ptr(hd) if use_scale else None, N_.ptr(C), M, N, K, act, st), "orcai_gemm_bias_act")
                            got = C.cpu().numpy().astype(np.float64)
                            ref = P + (bias if use_bias else 0.0)
                            mag = absP + (np.abs(bias) if use_bias else 0.0)
                            if act:
                                ref = np.maximum(ref, 0.0)
                            if use_scale:
                                ref, mag = ref * scale + shift, mag * np.abs(scale) + np.abs(shift)
                            what = (M, N, K, f"bias={use_bias} act={act} scale={use_scale} a_off={a_off} vec={_gba_vec(K, N, a_off)}")
                            if kind == "int":
                                assert float(np.max(mag)) < 2.0**24, what
                                assert np.array_equal(got, ref), (what, float(np.abs(got - ref).max()), int((got != ref).sum()))
                            else:
                                excess = np.abs(got - ref) - gamma(K + 3) * mag
                                assert float(excess.max()) <= 0.0, (what, float(np.abs(got - ref).max()), float((gamma(K + 3) * mag).flat[int(excess.argmax())]))


def test_gemm_bias_act_argument_checks():
    from orcai_amd import _native as N_

    lib, st = N_.lib(), N_.stream_ptr()
    A, B, v = torch.ones(8, 8, device="cuda"), torch.ones(8, 8, device="cuda"), torch.ones(8, device="cuda")
    C = torch.full((8, 8), SENTINEL, device="cuda")
    a, b, c, s = N_.ptr(A), N_.ptr(B), N_.ptr(C), N_.ptr(v)
    assert lib.orcai_gemm_bias_act(a, b, None, s, None, c, 8, 8, 8, 0, st) == N_.E_BADARG  # scale without shift
    assert lib.orcai_gemm_bias_act(None, b, None, None, None, c, 8, 8, 8, 0, st) == N_.E_BADARG
    assert lib.orcai_gemm_bias_act(a, None, None, None, None, c, 8, 8, 8, 0, st) == N_.E_BADARG
    assert lib.orcai_gemm_bias_act(a, b, None, None, None, None, 8, 8, 8, 0, st) == N_.E_BADARG
    for M, N, K in ((0, 8, 8), (8, 0, 8), (8, 8, 0)):
        assert lib.orcai_gemm_bias_act(a, b, None, None, None, c, M, N, K, 0, st) == N_.E_BADARG
    assert bool((C == SENTINEL).all())  # nothing was launched
    assert lib.orcai_gemm_bias_act(a, b, None, None, s, c, 8, 8, 8, 0, st) == 0  # a shift without a scale is ignored
    assert bool((C == 8.0).all())
