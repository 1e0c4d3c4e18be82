"""The k = 3 f32 inference trunk launchers `orcai predict` runs on (orcai_conv0_bn_relu, orcai_sepconv_bn, orcai_conv0_sepconv, orcai_pool_res_add,
orcai_sepconv_pool_res), one by one through the C ABI against float64 arithmetic (tests/trunk_fwd_ref.py, itself checked against oracle.model_ref on
the CPU by tests/test_trunk_fwd_ref.py): odd heights and widths, ragged channel quads, one to four output tiles, every kernel the dispatch rules of
launch_sepconv, orcai_conv0_sepconv, orcai_pool_res_add_bn and orcai_sepconv_pool_res pick (the branch is named at each case of the tables).

Two kinds of input, as tests/test_trunk_fallback_gpu.py:
  exact            integers in [-4, 4], folded scales from {-2, -1, 0.5, 1, 2}, integer shifts: every partial sum is exact in f32
                   (test_exact_cases_stay_below_2_to_the_24), so the result must equal the float64 one under np.array_equal;
  standard normal  scales of both signs, |got - want| <= (n_terms + 8) 2^-23 S per element, S the sum of the absolute values of the terms the kernel
                   adds up and n_terms the longest chain (trunk_fwd_ref.chain_bound; the formula is repeated at each assertion).
No case needed the fallback bar 1e-4 * max(1, max|ref|).
Outputs start from a sentinel (planes: 777 in the interior, zero in the pads).  Afterwards the pad rows, columns and channels are still zero and the
columns of an x-pooled buffer past ceil(W/2) still hold the sentinel.  The process-wide knobs are set and restored in try / finally."""

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import trunk_fwd_ref as T  # noqa: E402
from half_fwd_ref import from_quad_planes, pool_res_add_ref, to_quad_planes  # noqa: E402
from test_trunk_fallback_gpu import SENTINEL, _dev, _pack_dw, _pads  # noqa: E402

KINDS = [True, False]
KIND_IDS = ["exact", "normal"]


def _sentinel_planes(B, C, H, W):
    """k = 3 quad planes whose interior (real channels) holds the sentinel and whose pads are zero."""
    return _dev(to_quad_planes(np.full((B, C, H, W), SENTINEL, dtype=np.float32), 3))


def _same(got, want, exact, bound, what):
    """exact: equal to the float64 result; standard normal: within the derived bound, element by element."""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err = np.abs(got - want)
    print(what, "max error", float(err.max()), "largest error / bound", 0.0 if exact else float((err / bound).max()))
    if exact:
        assert np.array_equal(got, want), (what, float(err.max()), int((err > 0).sum()))
    else:
        assert (err <= bound).all(), (what, float(err.max()), float((err / bound).max()))


class _Knobs:
    """Process-wide launcher knobs, restored on exit.  A value of None leaves the knob alone."""

    def __init__(self, lib, **values):
        self.lib, self.values, self.saved = lib, values, []

    def __enter__(self):
        try:
            for name, v in self.values.items():
                if v is not None:
                    f = getattr(self.lib, name)
                    self.saved.append((f, f(v)))
        except BaseException:
            self.__exit__()
            raise
        return self

    def __exit__(self, *exc):
        while self.saved:
            f, v = self.saved.pop()
            f(v)
        return False


# ------------------------------------------------------------------------------------------------- (1) orcai_conv0_bn_relu, k = 3: conv0_kernel<3>
@pytest.mark.parametrize("exact", KINDS, ids=KIND_IDS)
@pytest.mark.parametrize("name", list(T.ENTRY_CASES))
def test_entry_conv(name, exact):
    """relu(scale0 * (3 x 3 "same" cross-correlation of one channel into 16) + shift0); one case per shape reads the snippets as a sliding,
    overlapping view of one [T][W] array."""
    from orcai_amd import _native as N

    lib = N.lib()
    B, H, W, _ = T.ENTRY_CASES[name]
    c = T.entry_case(name, exact)
    want, S0 = T.entry_ref(c["x"], c["w0"], c["scale0"], c["shift0"])
    src, w0, sc0, sh0 = _dev(c["src"]), _dev(c["w0"]), _dev(c["scale0"]), _dev(c["shift0"])
    out = _sentinel_planes(B, 16, H, W)
    N.check(lib.orcai_conv0_bn_relu(N.ptr(src), c["stride"], B, H, W, 3, N.ptr(w0), N.ptr(sc0), N.ptr(sh0), N.ptr(out), N.stream_ptr()), name)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    _same(from_quad_planes(got, 16, H, W, 3)[0], want, exact, T.chain_bound(S0, 9), name)  # (9 + 8) 2^-23 S0
    assert _pads(got, 16, H, W, 3) == 0.0, name


# ------------------------------------------------------------------------------------------------- (2) orcai_sepconv_bn, k = 3
@pytest.mark.parametrize("exact", KINDS, ids=KIND_IDS)
@pytest.mark.parametrize("name", list(T.SEP_CASES))
def test_sepconv(name, exact):
    """Every out_layout, ReLU on load and on store both ways, tile modes 0 (sepconv_kernel), 1 (the launcher's choice, named in SEP_CASES) and 2
    (sepconv_ftile_kernel), each against float64; out_layout 1 is sepconv_kernel in every mode and runs once."""
    from orcai_amd import _native as N

    lib = N.lib()
    B, Cin, Cout, H, W = T.SEP_CASES[name]
    c = T.sep_case(name, exact)
    xd, dwd, pwd, scd, shd = _dev(to_quad_planes(c["x"], 3)), _dev(_pack_dw(c["dwk"])), _dev(c["pw"]), _dev(c["scale"]), _dev(c["shift"])
    Wx = (W + 1) // 2
    for relu_in in (0, 1):
        for relu_out in (0, 1):
            want, S = T.sep_ref(c["x"], c["dwk"], c["pw"], c["scale"], c["shift"], relu_in, relu_out)
            bound = T.chain_bound(S, 9 + Cin)  # (9 + Cin + 8) 2^-23 S
            for layout, mode in ((0, 0), (0, 1), (0, 2), (1, 1), (2, 0), (2, 1), (2, 2)):
                what = (name, "relu_in", relu_in, "relu_out", relu_out, "layout", layout, "mode", mode)
                if layout == 0:
                    out = _sentinel_planes(B, Cout, H, W)
                elif layout == 1:
                    out = torch.full((B, H, W * Cout), SENTINEL, device="cuda")
                else:
                    out = _dev(T.to_xpooled_quads(np.full((B, Cout, H, Wx), SENTINEL, dtype=np.float32), SENTINEL))
                with _Knobs(lib, orcai_sepconv_tile_mode=mode):
                    rc = lib.orcai_sepconv_bn(N.ptr(xd), B, Cin, H, W, 3, relu_in, N.ptr(dwd), N.ptr(pwd), N.ptr(scd), N.ptr(shd), Cout, relu_out, layout, N.ptr(out),
                                              N.stream_ptr())
                N.check(rc, str(what))
                torch.cuda.synchronize()
                got = out.cpu().numpy()
                if layout == 0:
                    _same(from_quad_planes(got, Cout, H, W, 3)[0], want, exact, bound, what)
                    assert _pads(got, Cout, H, W, 3) == 0.0, what
                elif layout == 1:  # Keras Reshape((-1, W * C)) of NHWC: feature = x * Cout + c
                    _same(got.reshape(B, H, W, Cout).transpose(0, 3, 1, 2), want, exact, bound, what)
                else:  # the column-pair maximum of the float64 result; a maximum moves by no more than its operands: the pair's larger bound
                    full = T.from_xpooled_quads(got)
                    _same(full[:, :Cout, :, :Wx], T.pair_max(want), exact, T.pair_max(bound), what)
                    assert np.all(full[:, :Cout, :, Wx:] == SENTINEL) and not full[:, Cout:].any(), what  # the columns past ceil(W / 2) are nobody's


# ------------------------------------------------------------------------------------------------- (3) orcai_conv0_sepconv
@pytest.mark.parametrize("exact", KINDS, ids=KIND_IDS)
@pytest.mark.parametrize("name", list(T.FUSED_ENTRY_CASES))
def test_fused_entry(name, exact):
    """out against the float64 composition of the entry conv and block 1's first separable conv (ReLU on load); prev_sub, f32[B][4][ceil(H/2)][ceil(W/2)][4],
    against the float64 entry activation at pixels (2i, 2j); with and without prev_sub, ReLU on store both ways."""
    from orcai_amd import _native as N

    lib = N.lib()
    B, Cout, H, W, knobs = T.FUSED_ENTRY_CASES[name]
    c = T.fused_entry_case(name, exact)
    # every array the launcher wants 16-byte aligned is a tensor of its own
    xd, w0, sc0, sh0 = _dev(c["src"]), _dev(c["w0"]), _dev(c["scale0"]), _dev(c["shift0"])
    dwd, pwd, scd, shd = _dev(_pack_dw(c["dwk"])), _dev(c["pw"]), _dev(c["scale"]), _dev(c["shift"])
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    for relu_out in (0, 1):
        a, S0, want, S = T.fused_entry_ref(c, relu_out)
        for tile, windows in knobs:
            for with_sub in (True, False):
                what = (name, "relu_out", relu_out, "entry_tile", tile, "entry_windows", windows, "prev_sub", with_sub)
                out = _sentinel_planes(B, Cout, H, W)
                sub = torch.full((B, 4, Ho, Wo, 4), SENTINEL, device="cuda") if with_sub else None
                with _Knobs(lib, orcai_entry_tile=tile, orcai_entry_windows=windows or None):
                    rc = lib.orcai_conv0_sepconv(N.ptr(xd), c["stride"], B, H, W, N.ptr(w0), N.ptr(sc0), N.ptr(sh0), N.ptr(dwd), N.ptr(pwd), N.ptr(scd), N.ptr(shd), Cout,
                                                 relu_out, N.ptr(out), N.ptr(sub) if with_sub else None, N.stream_ptr())
                N.check(rc, str(what))
                torch.cuda.synchronize()
                got = out.cpu().numpy()
                _same(from_quad_planes(got, Cout, H, W, 3)[0], want, exact, T.chain_bound(S, 9 + 9 + 16), what)  # (9 + 9 + 16 + 8) 2^-23 S
                assert _pads(got, Cout, H, W, 3) == 0.0, what
                if with_sub:
                    g = T.from_compact_quads(sub.cpu().numpy())
                    _same(g, a[:, :, ::2, ::2], exact, T.chain_bound(S0[:, :, ::2, ::2], 9), (*what, "sub"))  # (9 + 8) 2^-23 S0


# ------------------------------------------------------------------------------------------------- (4) orcai_pool_res_add, k = 3
@pytest.mark.parametrize("exact", KINDS, ids=KIND_IDS)
@pytest.mark.parametrize("name", list(T.POOL_CASES))
def test_pool_res_add(name, exact):
    """MaxPooling2D((3, 2), 2, "same")(s) + Conv2D(C, 1, strides 2)(prev) + br against half_fwd_ref.pool_res_add_ref, all four flag words: bit 0, s is
    the x-pooled tensor (the column-pair maximum of the same s, taken in f32 on the host); bit 1, prev is the compact (2i, 2j) subsample.
    Flag word 2 (s planes, compact prev) is the combination no caller in the package uses: pool_res_add_kernel once stepped through the quad planes
    of s with the compact subsample's pitch there."""
    from orcai_amd import _native as N

    lib = N.lib()
    B, C, Cp, H, W, verticals = T.POOL_CASES[name]
    c = T.pool_case(name, exact)
    want, S = pool_res_add_ref(c["s"], c["prev"], c["wr"], c["br"])
    bound = T.chain_bound(S, Cp + 2)  # (Cp + 2 + 8) 2^-23 S
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    assert want.shape == (B, C, Ho, Wo)
    s_planes, s_x = _dev(to_quad_planes(c["s"], 3)), _dev(T.to_xpooled_quads(T.pair_max(c["s"]), SENTINEL))
    p_planes, p_sub = _dev(to_quad_planes(c["prev"], 3)), _dev(T.to_compact_quads(c["prev"]))
    wd, bd = _dev(c["wr"]), _dev(c["br"])
    for vert in verticals:
        for flags in (0, 1, 2, 3):
            what = (name, "pool_vertical", vert, "flags", flags)
            out = _sentinel_planes(B, C, Ho, Wo)
            sd, pd = s_x if flags & 1 else s_planes, p_sub if flags & 2 else p_planes
            with _Knobs(lib, orcai_pool_vertical=vert):
                rc = lib.orcai_pool_res_add(N.ptr(sd), N.ptr(pd), B, C, Cp, H, W, 3, N.ptr(wd), N.ptr(bd), N.ptr(out), flags, N.stream_ptr())
            N.check(rc, str(what))
            torch.cuda.synchronize()
            got = out.cpu().numpy()
            _same(from_quad_planes(got, C, Ho, Wo, 3)[0], want, exact, bound, what)
            assert _pads(got, C, Ho, Wo, 3) == 0.0, what


# ------------------------------------------------------------------------------------------------- (5) orcai_sepconv_pool_res
@pytest.mark.parametrize("exact", KINDS, ids=KIND_IDS)
@pytest.mark.parametrize("name", list(T.TAIL_CASES))
def test_fused_block_tail(name, exact):
    """sepconv_pool_march_kernel against the float64 composition of the separable conv (x-pooled) and the pooling tail: marching segments of 1 and 2
    tiles and the default, both layouts of prev, ReLU on load both ways.  Bound: the largest (9 + Cin + 8) 2^-23 S_sep inside the pooling window (a
    maximum moves by no more than its operands) + (Cp + 2 + 8) 2^-23 S_tail (trunk_fwd_ref.tail_ref)."""
    from orcai_amd import _native as N

    lib = N.lib()
    B, C, Cp, H, W = T.TAIL_CASES[name]
    c = T.tail_case(name, exact)
    Ho, Wo = H // 2, (W + 1) // 2
    xd, dwd, pwd, scd, shd = _dev(to_quad_planes(c["x"], 3)), _dev(_pack_dw(c["dwk"])), _dev(c["pw"]), _dev(c["scale"]), _dev(c["shift"])
    p_planes, p_sub = _dev(to_quad_planes(c["prev"], 3)), _dev(T.to_compact_quads(c["prev"]))
    wd, bd = _dev(c["wr"]), _dev(c["br"])
    for relu_in in (0, 1):
        want, _, bound = T.tail_ref(c, relu_in)
        assert want.shape == (B, C, Ho, Wo)
        for nt in T.TAIL_NT:
            for compact in (0, 1):
                what = (name, "relu_in", relu_in, "pool_fused", nt, "prev_compact", compact)
                out = _sentinel_planes(B, C, Ho, Wo)
                with _Knobs(lib, orcai_pool_fused=nt or None):
                    rc = lib.orcai_sepconv_pool_res(N.ptr(xd), N.ptr(p_sub if compact else p_planes), B, C, C, Cp, H, W, 3, relu_in, N.ptr(dwd), N.ptr(pwd), N.ptr(scd),
                                                    N.ptr(shd), 0, N.ptr(wd), N.ptr(bd), N.ptr(out), compact, N.stream_ptr())
                N.check(rc, str(what))
                torch.cuda.synchronize()
                got = out.cpu().numpy()
                _same(from_quad_planes(got, C, Ho, Wo, 3)[0], want, exact, bound, what)
                assert _pads(got, C, Ho, Wo, 3) == 0.0, what
