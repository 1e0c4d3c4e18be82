"""Two forward launchers of the f16 path through the C ABI against float64 (tests/half_fwd_ref.py, itself checked against torch float64 in
tests/test_half_fwd_ref.py):

orcai_h_pool_res_add   the pooling tail of every block, with BatchNorm on the fly in the training forward.  Exact integers without BatchNorm
    (plane and x-pooled input), real-valued data with BatchNorm: gamma of both signs (the kernel pools the window MINIMUM where the folded scale
    is negative), one gamma exactly 0, bn_eps = 1e-3 and, for one shape, 0.1.  Bound per element
        |got - want| <= 2^-11 |want| + 2^-24 + 1e-4 max(1, max |want|):
    half an ulp of the f16 store (derived) plus the f32 twin's bar for the same operation (tests/test_trunk_fallback_gpu.py).  out starts from
    a sentinel: every real element is overwritten, the channels >= C of the last octet are 0, every pad row and column keeps the sentinel's
    bits.  The pad rows and columns of s hold +-60000 on the side the pooling would pick, so a coordinate that is not clamped shows.
    The f32 twin orcai_pool_res_add_bn runs the same cases (k = 3 included) at its 1e-4 bar.

orcai_h_gemm_bias_act  both LSTM input projections and Dense-128.  Exact integers, and A ~ N(0, 1) in f32 that the kernel has to round to f16
    to nearest even, W ~ N(0, 1) / sqrt(K), against
        |got - want| <= (K + 8) 2^-23 S_epi,   S_epi = |scale| (sum_k |a| |w| + |bias|) + |shift|:
    the forward error of a K-term f32 sum in any order with the unit roundoff doubled (the matrix unit's internal rounding) and a few
    roundings for the epilogue.  Derived, not measured; an f16 accumulator misses it by a factor 30 to 1000.  A, Wt and C are 16-byte-aligned
    views inside larger buffers; behind A and Wt lie NaN, so a read past K on the last row, of a row >= M or of a Wt row >= N puts NaN into C
    (NaN times the zero pad of Wt is NaN); around C lies a sentinel.

Observed on an MI355X, worst error / bound: pooling tail with BatchNorm 0.77, its f32 twin 0.002 of its bar, GEMM 0.048; per case in the
docstrings of the tests, which print them."""

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import half_fwd_ref as R  # noqa: E402

SENT = 30000.0  # a finite f16 no result comes near
SENT_BITS = int(np.float16(SENT).view(np.uint16))
POISON = 60000.0  # in the pad rows and columns of s
POOL_IDS = [R.pool_case_id(c) for c in R.POOL_CASES]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ------------------------------------------------------------------------------------------------- orcai_h_pool_res_add
def _s_planes(s, k, sign):
    """s as octet planes whose pad rows and columns hold sign[c] * POISON (channels >= C zero): outside what a clamped coordinate reads."""
    B, C, H, W = s.shape
    p = R.to_octet_planes(s.astype(np.float16), k)
    CO, HP, WP = p.shape[1], p.shape[2], p.shape[3]
    full = np.ascontiguousarray(p.transpose(0, 1, 4, 2, 3)).reshape(B, CO * 8, HP, WP)
    Rr = k // 2
    inside = np.zeros((HP, WP), dtype=bool)
    inside[Rr : Rr + H, :W] = True
    fill = np.zeros(CO * 8, dtype=np.float16)
    fill[:C] = (np.asarray(sign) * POISON).astype(np.float16)
    full[:, :, ~inside] = fill[None, :, None]
    return np.ascontiguousarray(full.reshape(B, CO, 8, HP, WP).transpose(0, 1, 3, 4, 2))


class _HPool:
    """One case of orcai_h_pool_res_add on the device: the operands, and out as the first B images of B + 1 sentinel images."""

    def __init__(self, shape, B, s, prev, wr, br, bn=None, xpooled=0):
        from orcai_amd import _native as N
        from orcai_amd.half import pack_pointwise_fragments

        self.N, self.lib = N, N.lib()
        self.shape, self.B, self.xpooled = shape, B, xpooled
        C, Cp, H, W, k = shape
        self.Ho, self.Wo = (H + 1) // 2, (W + 1) // 2
        if xpooled:
            self.sd = _dev(R.to_xpooled(s, fill=POISON))
        else:
            sign = np.ones(C) if bn is None else np.where(bn[2] < 0, -1.0, 1.0)  # the side a maximum of BN(s) would pick
            self.sd = _dev(_s_planes(s, k, sign))
        self.pd = _dev(R.to_octet_planes(prev.astype(np.float16), k))
        self.wd = _dev(pack_pointwise_fragments(wr.astype(np.float32)))
        self.bd = _dev(br.astype(np.float32))
        self.bn = None if bn is None else [_dev(np.asarray(a, dtype=np.float32)) for a in bn]
        Rr = k // 2
        self.out_all = torch.full((B + 1, (C + 7) // 8, self.Ho + 2 * Rr, (self.Wo + Rr + 3) & ~3, 8), SENT, dtype=torch.float16, device="cuda")
        self.out = self.out_all[:B]

    def call(self, eps=0.0, **over):
        N = self.N
        C, Cp, H, W, k = self.shape
        a = dict(s=N.ptr(self.sd), C=C, Cp=Cp, xpooled=self.xpooled, bn=[None] * 4 if self.bn is None else [N.ptr(t) for t in self.bn])
        a.update(over)
        return self.lib.orcai_h_pool_res_add(a["s"], N.ptr(self.pd), self.B, a["C"], a["Cp"], H, W, k, N.ptr(self.wd), N.ptr(self.bd), N.ptr(self.out), a["xpooled"],
                                             *a["bn"], eps, N.stream_ptr())

    def bits(self):
        torch.cuda.synchronize()
        return self.out_all.cpu().numpy().view(np.uint16)

    def check_regions(self, tag):
        """-> the real elements as float64, after the three assertions on what the kernel may and must write."""
        C, k = self.shape[0], self.shape[4]
        bits = self.bits()
        assert (bits[self.B] == SENT_BITS).all(), f"{tag}: wrote behind the last image"
        valid, zeros, pads = R.split_planes(bits[: self.B], C, self.Ho, self.Wo, k)
        assert (valid != SENT_BITS).all(), f"{tag}: {(valid == SENT_BITS).sum()} real elements not written"
        assert (zeros == 0).all(), f"{tag}: channels >= C of the last octet are not +0"
        assert (pads == SENT_BITS).all(), f"{tag}: {(pads != SENT_BITS).sum()} pad elements written"
        return np.ascontiguousarray(valid).view(np.float16).astype(np.float64)


def _pool_bound(want):
    return 2.0**-11 * np.abs(want) + 2.0**-24 + 1e-4 * max(1.0, float(np.abs(want).max()))


@pytest.mark.parametrize("case", R.POOL_CASES, ids=POOL_IDS)
def test_h_pool_res_add_exact_integers(case):
    """No BatchNorm, plane and x-pooled s: bit-for-bit equal to the float64 reference."""
    shape, B = case
    s, prev, wr, br = R.pool_int_case(shape, B)
    want, _ = R.pool_res_add_ref(s, prev, wr, br)
    assert np.abs(want).max() < 2048
    for xpooled in (0, 1):
        h = _HPool(shape, B, s, prev, wr, br, xpooled=xpooled)
        h.N.check(h.call(), "h_pool_res_add")
        got = h.check_regions(f"{R.pool_case_id(case)} xpooled={xpooled}")
        assert np.array_equal(got, want), (xpooled, float(np.abs(got - want).max()))


@pytest.mark.parametrize("case", R.POOL_CASES, ids=POOL_IDS)
def test_h_pool_res_add_batchnorm_on_the_fly(case):
    """BatchNorm folded into the pooling, gamma of both signs and one exact zero.  Observed on an MI355X: worst |got - want| / bound per case
    0.51 to 0.77 (0.77 at C12-Cp40-9x14-k3 with bn_eps = 0.1; channels with gamma < 0 and gamma >= 0 alike), nearly all of it the half ulp of
    the f16 store (max |got - want| 3.9e-3 = 2^-8 at |want| in [8, 16)).  The bound is derived, see the module docstring."""
    shape, B = case
    s, prev, wr, br, bn = R.pool_bn_case(shape, B)
    eps = R.pool_eps(shape)
    want, S = R.pool_res_add_ref(s, prev, wr, br, bn, eps)
    h = _HPool(shape, B, s, prev, wr, br, bn=bn)
    h.N.check(h.call(eps=eps), "h_pool_res_add")
    got = h.check_regions(R.pool_case_id(case))
    assert np.isfinite(got).all()
    ratio = np.abs(got - want) / _pool_bound(want)
    neg = bn[2] < 0
    print(f"h_pool_res_add BN {R.pool_case_id(case)} eps={eps:g}: worst |got - want| / bound = {ratio.max():.3f} (gamma < 0: {ratio[:, neg].max():.3f}, "
          f"gamma >= 0: {ratio[:, ~neg].max():.3f}); max |got - want| = {np.abs(got - want).max():.2e}, max |want| = {np.abs(want).max():.2f}, max S = {S.max():.2f}")
    assert ratio.max() <= 1.0, (float(ratio.max()), np.unravel_index(np.argmax(ratio), ratio.shape))


@pytest.mark.parametrize("case", R.POOL_CASES, ids=POOL_IDS)
def test_h_pool_res_add_f32_twin_same_cases(case):
    """orcai_pool_res_add_bn on quad planes, the same data and reference: exact on the integers, 1e-4 max(1, max |want|) with BatchNorm (the bar of
    test_pool_res_add_bn_wide_kernels, which stops at k = 5 and 7).  Observed on an MI355X: worst error / bar 0.002."""
    from orcai_amd import _native as N

    lib = N.lib()
    shape, B = case
    C, Cp, H, W, k = shape
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    for mode in (1, 2):
        if mode == 1:
            s, prev, wr, br = R.pool_int_case(shape, B)
            bn, eps = None, 0.0
        else:
            s, prev, wr, br, bn = R.pool_bn_case(shape, B)
            eps = R.pool_eps(shape)
        want, _ = R.pool_res_add_ref(s, prev, wr, br, bn, eps)
        sd, pd = _dev(R.to_quad_planes(s, k)), _dev(R.to_quad_planes(prev, k))
        wd, bd = _dev(wr.astype(np.float32)), _dev(br.astype(np.float32))
        bnd = [] if bn is None else [_dev(np.asarray(a, dtype=np.float32)) for a in bn]
        out = _dev(R.to_quad_planes(np.full((B, C, Ho, Wo), SENT, dtype=np.float32), k))  # sentinel inside, zero pads: this launcher may store zeros there
        N.check(lib.orcai_pool_res_add_bn(N.ptr(sd), N.ptr(pd), B, C, Cp, H, W, k, N.ptr(wd), N.ptr(bd), N.ptr(out), 0, *([N.ptr(t) for t in bnd] or [None] * 4), eps,
                                          N.stream_ptr()), "pool_res_add_bn")
        torch.cuda.synchronize()
        got, pads = R.from_quad_planes(out.cpu().numpy().astype(np.float64), C, Ho, Wo, k)
        assert not pads.any()
        if mode == 1:
            assert np.array_equal(got, want), float(np.abs(got - want).max())
        else:
            bar = 1e-4 * max(1.0, float(np.abs(want).max()))
            print(f"pool_res_add_bn (f32 twin) {R.pool_case_id(case)} eps={eps:g}: max |got - want| / bar = {np.abs(got - want).max() / bar:.3f}")
            assert np.abs(got - want).max() <= bar


def test_h_pool_res_add_refusals():
    """Bad arguments come back as their code, with out untouched."""
    shape, B = (30, 16, 12, 21, 3), 2
    s, prev, wr, br, bn = R.pool_bn_case(shape, B)
    h = _HPool(shape, B, s, prev, wr, br, bn=bn)
    N = h.N
    ptrs = [N.ptr(t) for t in h.bn]
    assert h.call(eps=1e-3, s=None) == N.E_BADARG
    assert h.call(eps=1e-3, Cp=0) == N.E_BADARG
    assert h.call(eps=1e-3, xpooled=2, bn=[None] * 4) == N.E_BADARG
    assert h.call(eps=1e-3, xpooled=1) == N.E_BADARG  # BatchNorm on the fly reads planes, never the x-pooled tensor
    assert h.call(eps=1e-3, bn=[ptrs[0], None, ptrs[2], ptrs[3]]) == N.E_BADARG
    assert h.call(eps=1e-3, C=65) == N.E_BADARG
    assert (h.bits() == SENT_BITS).all()
    N.check(h.call(eps=1e-3), "h_pool_res_add")  # and the same object does run
    h.check_regions("after the refusals")


# ------------------------------------------------------------------------------------------------- orcai_h_gemm_bias_act
GUARD = 64  # elements in front of and behind every operand


class _HGemm:
    """A [M][K] f32 and Wt [N][roundup32(K)] f16 with NaN in front and behind, C [M][N] inside a sentinel; all three 16-byte aligned."""

    def __init__(self, A, W):
        from orcai_amd import _native as N
        from orcai_amd.half import pack_transposed

        self.N, self.lib = N, N.lib()
        self.M, self.K = A.shape
        self.Nn = W.shape[1]
        wt = pack_transposed(W)
        assert wt.shape == (self.Nn, (self.K + 31) // 32 * 32) and not wt[:, self.K :].any()  # the zero pad is part of the contract: left as it is
        a_buf = np.full(GUARD + A.size + GUARD, np.nan, dtype=np.float32)
        a_buf[GUARD : GUARD + A.size] = A.ravel()
        w_buf = np.full(GUARD + wt.size + GUARD, np.nan, dtype=np.float16)
        w_buf[GUARD : GUARD + wt.size] = wt.ravel()
        self.a_buf, self.w_buf = _dev(a_buf), _dev(w_buf)
        self.c_buf = torch.full((GUARD + self.M * self.Nn + GUARD,), SENT, dtype=torch.float32, device="cuda")
        self.pa, self.pw, self.pc = self.a_buf.data_ptr() + 4 * GUARD, self.w_buf.data_ptr() + 2 * GUARD, self.c_buf.data_ptr() + 4 * GUARD
        assert self.pa % 16 == 0 and self.pw % 16 == 0 and self.pc % 16 == 0
        self.keep = []

    def call(self, bias, scale, shift, act, **over):
        N = self.N
        self.keep = [None if v is None else _dev(np.asarray(v, dtype=np.float32)) for v in (bias, scale, shift)]
        a = dict(A=self.pa, Wt=self.pw, M=self.M, K=self.K)
        a.update(over)
        return self.lib.orcai_h_gemm_bias_act(a["A"], a["Wt"], *[None if t is None else N.ptr(t) for t in self.keep], self.pc, a["M"], self.Nn, a["K"], act, N.stream_ptr())

    def result(self, tag):
        torch.cuda.synchronize()
        c = self.c_buf.cpu().numpy()
        assert (c[:GUARD] == SENT).all() and (c[-GUARD:] == SENT).all(), f"{tag}: wrote outside C"
        got = c[GUARD:-GUARD].reshape(self.M, self.Nn)
        assert np.isfinite(got).all(), f"{tag}: {np.isnan(got).sum()} NaN in C: a read outside A[M][K] or Wt[N][Kp]"
        assert (got != SENT).all(), f"{tag}: elements of C not written"
        self.c_buf.fill_(SENT)
        return got.astype(np.float64)


def _flushed(a):
    """f16 rounding with subnormal results flushed to zero (diagnostics only)."""
    h = np.asarray(a).astype(np.float16).astype(np.float64)
    return np.where(np.abs(h) < 2.0**-14, 0.0, h)


@pytest.mark.parametrize("shape", list(R.GEMM_SHAPES), ids=lambda s: "x".join(map(str, s)))
def test_h_gemm_exact_integers(shape):
    """Integer operands: equal to float64 bit for bit, with and without bias, all three epilogues."""
    M, Nn, K = shape
    rng, A, W, bias = R.gemm_int_case(shape)
    g = _HGemm(A, W)
    for act, sk in R.GEMM_EPILOGUES:
        scale, shift = R.gemm_epilogue(rng, Nn, sk, integers=True)
        for b in (bias, None):
            tag = f"{shape} act={act} scale={sk} bias={'yes' if b is not None else 'no'}"
            want, _ = R.gemm_ref(A, W, b, scale, shift, act)
            g.N.check(g.call(b, scale, shift, act), "h_gemm")
            got = g.result(tag)
            assert np.array_equal(got, want), (tag, float(np.abs(got - want).max()))


@pytest.mark.parametrize("shape", list(R.GEMM_SHAPES), ids=lambda s: "x".join(map(str, s)))
def test_h_gemm_real_operands(shape):
    """A ~ N(0, 1) in f32 (rounded to f16 by the kernel), W ~ N(0, 1) / sqrt(K), against (K + 8) 2^-23 S_epi.  Observed on an MI355X: worst
    |got - want| / bound over all cases and epilogues 0.048 (K = 4), falling to 0.001 at K = 396 (the bound is derived, see the module docstring).
    The same comparison against a reference that flushes f16-subnormal operands misses by up to 3.2 at K = 36, 60, 64: the matrix unit keeps them."""
    M, Nn, K = shape
    rng, A, W, bias = R.gemm_float_case(shape)
    g = _HGemm(A, W)
    worst = 0.0
    for act, sk in R.GEMM_EPILOGUES:
        scale, shift = R.gemm_epilogue(rng, Nn, sk, integers=False)
        for b in (bias, None):
            tag = f"{shape} act={act} scale={sk} bias={'yes' if b is not None else 'no'}"
            want, S = R.gemm_ref(A, W, b, scale, shift, act)
            bound = R.gemm_bound(S, K, scale, shift)
            g.N.check(g.call(b, scale, shift, act), "h_gemm")
            got = g.result(tag)
            ratio = np.abs(got - want) / bound
            # for the record only: the same comparison had the matrix unit flushed f16-subnormal operands, and had A not been rounded at all
            z = _flushed(A) @ _flushed(W) + (0.0 if b is None else b.astype(np.float64))
            z = np.maximum(z, 0.0) if act else z
            z = z if scale is None else z * scale.astype(np.float64) + shift.astype(np.float64)
            print(f"h_gemm {tag}: worst |got - want| / bound = {ratio.max():.3f} (against a subnormal-flushing reference {(np.abs(got - z) / bound).max():.3f}); "
                  f"max |got - want| = {np.abs(got - want).max():.2e}")
            worst = max(worst, float(ratio.max()))
            assert ratio.max() <= 1.0, (tag, float(ratio.max()), np.unravel_index(np.argmax(ratio), ratio.shape))
    print(f"h_gemm {shape}: worst ratio over the epilogues {worst:.3f}")


def test_h_gemm_refusals():
    """Bad arguments come back as their code, with C untouched."""
    rng, A, W, bias = R.gemm_float_case((33, 17, 100))
    g = _HGemm(A, W)
    N = g.N
    scale, shift = R.gemm_epilogue(rng, 17, "pm", integers=False)
    assert g.call(bias, None, None, 0, K=6) == N.E_UNSUPPORTED  # 16-byte loads along k need K % 4 == 0
    assert g.call(bias, None, None, 0, A=g.pa + 4) == N.E_UNSUPPORTED
    assert g.call(bias, None, None, 0, Wt=g.pw + 4) == N.E_UNSUPPORTED
    assert g.call(bias, None, None, 0, A=None) == N.E_BADARG
    assert g.call(bias, None, None, 0, M=0) == N.E_BADARG
    assert g.call(bias, scale, None, 1) == N.E_BADARG
    torch.cuda.synchronize()
    assert (g.c_buf == SENT).all()
    N.check(g.call(bias, scale, shift, 1), "h_gemm")  # and the same object does run
    want, S = R.gemm_ref(A, W, bias, scale, shift, 1)
    assert (np.abs(g.result("after the refusals") - want) <= R.gemm_bound(S, 100, scale, shift)).all()
