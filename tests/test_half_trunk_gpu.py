"""The forward trunk launchers of the f16 path (csrc/half_fwd.hip), one by one through the C ABI against float64 (tests/half_trunk_ref.py, itself
checked on the CPU by tests/test_half_trunk_ref.py against torch float64, against mutated references and against an emulation of the arithmetic):

orcai_h_conv0_affine, orcai_h_conv0_affine_bn   conv0_h_kernel<3|5|7>[, BN]: one row, an exact 8 x 32 tile, one past it, ragged, and a sliding
    overlapping view of the snippets; y of the BN twin against relu(BatchNorm(.)) of the v the device stored.
orcai_h_sepconv   k = 3 on both routes -- orcai_sepconv_tile_mode(0): sepconv_h_kernel<3, MT>, (1): sepconv_h_ftile_kernel<MT, XP, UOUT>, the route
    asserted through orcai_sepconv_route -- 1 to 8 input octets, 1 to 4 output tiles, ragged octets on both sides, every out_layout, ReLU on load and
    on store; k = 5 and 7 on planes wider than one window; the pointwise pass (ktap = 1) scatter-added onto a non-zero odd-sized image.
orcai_h_sepconv_stats, orcai_h_sepconv_stats_bn   the STATS and BNIN instantiations of the flat-tile kernel: out, u and the finished mean / biased
    variance; the _bn variant against the float64 BatchNorm-on-load reference (zero outside the image), not against its two-launch twin.

Every scale vector has both signs.  Two kinds of input (half_trunk_ref's module docstring): exact -- np.array_equal with float64 -- and normal --
element by element at the DERIVED bounds stated there and repeated at half_trunk_ref.check_*: the depthwise output u at
gamma(2 k^2 + k, u16) sum |x w| + 2^-24; everything after it evaluated on the u the device stored, at (Cin + 8) 2^-23 S plus the f16 store's
u16 |want| + 2^-24 (layout 2: want the pair maximum, the pointwise term the larger of the pair; layout 3: u16 |val| + u16 |start + val| + 2 * 2^-24); the entry convolution at (k^2 + 8) 2^-23 S plus the store.  A launch
that keeps no u gets it from a second launch of the same route with u_out: the kernels are deterministic, and the window and flat routes'
u_out have identical bits (asserted).

Outputs start from the sentinel 30000 everywhere, pads included: afterwards every real element is written, the channels past C of the last
octet are 0 at the image's pixels, the pad rows and columns -- and the columns of an x-pooled buffer past ceil(W / 2) -- still hold the
sentinel's bits.  The process-wide tile mode is set and restored by _Knobs.

Observed on an MI355X, worst error / bound of the normal kind (for the record; no bar is derived from these), the same on the window and the
flat route:
  conv0 v 0.984, conv0_bn y 0.996; out of orcai_h_sepconv by layout: planes 0.985 (k = 3) and 0.984 (k = 5, 7), x-pooled 0.972 (k = 3, either
  route) and 0.969 (k = 5, 7), scatter-add 0.927, Keras reshape (f32, no store rounding) 0.077; out of _stats 0.982, of _stats_bn 0.974 -- each
  the half ulp of the f16 store at a value just above a power of two, which is what the bound allows and the emulation of
  tests/test_half_trunk_ref.py gives to the digit;
  u 0.125 (k = 3), 0.33 (k = 5, 7, 1), 0.21 (_stats), 0.34 (_stats_bn: the f32 y_a may round to the other f16 neighbour);
  mean 0.015, variance 0.005 (the bound charges every element its full pointwise bound with one sign).
The exact kind matched float64 under np.array_equal in every case."""

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import half_trunk_ref as R  # noqa: E402
from test_predict_trunk_gpu import _Knobs  # noqa: E402

SENT = 30000.0  # a finite f16 no result comes near
SENT_BITS = int(np.float16(SENT).view(np.uint16))
KINDS = [True, False]
KIND_IDS = ["exact", "normal"]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _sent(*shape, dtype=torch.float16):
    return torch.full(shape, SENT, dtype=dtype, device="cuda")


def _both_signs(v):
    v = np.asarray(v)
    assert (v < 0).any() and (v > 0).any() and not (v == 1).all()
    return _dev(v.astype(np.float32))


def _planes(t, C, H, W, k, what):
    """Octet planes that started from the sentinel -> the real elements [B][C][H][W] as float64, after the assertions on what a kernel may and
    must write."""
    bits = t.cpu().numpy().view(np.uint16)
    valid, zeros, pads = R.split_planes(bits, C, H, W, k)
    assert (valid != SENT_BITS).all(), f"{what}: {(valid == SENT_BITS).sum()} real elements not written"
    assert (zeros.view(np.float16) == 0).all(), f"{what}: channels >= C of the last octet are not 0"
    assert (pads == SENT_BITS).all(), f"{what}: {(pads != SENT_BITS).sum()} pad elements written"
    return np.ascontiguousarray(valid).view(np.float16).astype(np.float64)


def _xpooled(t, C, W, what):
    """An x-pooled buffer that started from the sentinel -> [B][C][H][ceil(W / 2)] as float64."""
    full = R.from_xpooled(t.cpu().numpy().view(np.uint16))
    Wx = (W + 1) // 2
    assert (full[:, :C, :, :Wx] != SENT_BITS).all(), f"{what}: real elements not written"
    assert (full[:, :, :, Wx:] == SENT_BITS).all(), f"{what}: columns past ceil(W / 2) written"
    assert (np.ascontiguousarray(full[:, C:, :, :Wx]).view(np.float16) == 0).all(), f"{what}: channels >= C of the last octet are not 0"
    return np.ascontiguousarray(full[:, :C, :, :Wx]).view(np.float16).astype(np.float64)


def _report(what, checks, family):
    for ch in checks:
        print(f"{family} | {what} | {ch}")
    for ch in checks:
        assert ch.ok, (what, ch)


# ------------------------------------------------------------------------------------------------- orcai_h_conv0_affine, orcai_h_conv0_affine_bn
class _Conv0:
    def __init__(self, c):
        from orcai_amd import _native as N

        self.N, self.lib, self.c = N, N.lib(), c
        n = c["src"].size
        buf = np.full(n + 64, np.nan, dtype=np.float32)  # NaN behind the last snippet: a read past it shows in the result
        buf[:n] = c["src"]
        self.src = _dev(buf)
        self.w, self.scale, self.shift = _dev(c["w"]), _both_signs(c["scale"]), _dev(c["shift"])
        Rr = c["k"] // 2
        self.shape = (c["B"], 2, c["H"] + 2 * Rr, (c["W"] + Rr + 3) & ~3, 8)

    def planes(self, t, what):
        c = self.c
        torch.cuda.synchronize()
        return _planes(t, 16, c["H"], c["W"], c["k"], what)


@pytest.mark.parametrize("exact", KINDS, ids=KIND_IDS)
@pytest.mark.parametrize("name", list(R.CONV0_CASES))
def test_h_conv0_affine(name, exact):
    """[relu](scale * conv + shift) into octet planes, ReLU off and on:  |got - want| <= (k^2 + 8) 2^-23 S + u16 |want| + 2^-24."""
    c = R.conv0_case(name, exact)
    h = _Conv0(c)
    N = h.N
    for relu in (0, 1):
        out = _sent(*h.shape)
        N.check(h.lib.orcai_h_conv0_affine(N.ptr(h.src), c["stride"], c["B"], c["H"], c["W"], c["k"], N.ptr(h.w), N.ptr(h.scale), N.ptr(h.shift), relu, N.ptr(out), N.stream_ptr()), name)
        _report(name, R.check_conv0(c, relu, h.planes(out, name), exact), "conv0")


@pytest.mark.parametrize("exact", KINDS, ids=KIND_IDS)
@pytest.mark.parametrize("name", list(R.CONV0_CASES))
def test_h_conv0_affine_bn(name, exact):
    """v as orcai_h_conv0_affine without ReLU; y against float64 relu(BatchNorm(v the device stored)):
    |y - want| <= 4 u32 (|v sc| + |sh|) + u16 |want| + 2^-24.  gamma of both signs, one exactly 0 (normal kind)."""
    c = R.conv0_case(name, exact)
    h = _Conv0(c)
    N = h.N
    bn = [_dev(np.asarray(a, dtype=np.float32)) for a in c["bn"]]
    v, y = _sent(*h.shape), _sent(*h.shape)
    N.check(h.lib.orcai_h_conv0_affine_bn(N.ptr(h.src), c["stride"], c["B"], c["H"], c["W"], c["k"], N.ptr(h.w), N.ptr(h.scale), N.ptr(h.shift), *[N.ptr(t) for t in bn],
                                          c["eps"], N.ptr(v), N.ptr(y), N.stream_ptr()), name)
    _report(name, R.check_conv0_bn(c, h.planes(v, name + " v"), h.planes(y, name + " y"), exact), "conv0_bn")


# ------------------------------------------------------------------------------------------------- orcai_h_sepconv
class _Sep:
    """One case's operands on the device."""

    def __init__(self, c, bn=None):
        from orcai_amd import _native as N
        from orcai_amd.half import pack_depthwise_octets, pack_pointwise_fragments

        self.N, self.lib, self.c = N, N.lib(), c
        self.x = _dev(R.to_octet_planes(c["x"].astype(np.float16), c["kp"]))
        self.dw, self.pw = _dev(pack_depthwise_octets(c["dwk"][..., None])), _dev(pack_pointwise_fragments(c["pw"]))
        self.scale, self.shift = _both_signs(c["scale"]), _dev(c["shift"])
        self.bn = None if bn is None else [_dev(np.asarray(a, dtype=np.float32)) for a in bn]
        Rr = c["kp"] // 2
        self.WP = (c["W"] + Rr + 3) & ~3
        self.HP = c["H"] + 2 * Rr

    def sepconv(self, layout, with_u, what):
        """orcai_h_sepconv under the current tile mode -> (out in the layout's canonical shape as float64, u as float64 or None, the raw out and u)."""
        c, N = self.c, self.N
        B, Cin, Cout, H, W, kp = c["B"], c["Cin"], c["Cout"], c["H"], c["W"], c["kp"]
        COo, Wx = (Cout + 7) // 8, (W + 1) // 2
        H2, W2 = c.get("H2", 0), c.get("W2", 0)
        if layout == 0:
            out = _sent(B, COo, self.HP, self.WP, 8)
        elif layout == 1:
            out = _sent(B, H, W * Cout, dtype=torch.float32)
        elif layout == 2:
            out = _sent(B, COo, H, (Wx + 3) & ~3, 8)
        else:  # the start image inside the sentinel's pads
            p = np.full((B, COo * 8, H2 + 2 * (kp // 2), (W2 + kp // 2 + 3) & ~3), SENT, dtype=np.float16)
            p[:, :, kp // 2 : kp // 2 + H2, :W2] = 0
            p[:, :Cout, kp // 2 : kp // 2 + H2, :W2] = c["start"]
            out = _dev(p.reshape(B, COo, 8, p.shape[2], p.shape[3]).transpose(0, 1, 3, 4, 2))
        u = _sent(B, (Cin + 7) // 8, self.HP, self.WP, 8) if with_u else None
        N.check(self.lib.orcai_h_sepconv(N.ptr(self.x), B, Cin, H, W, kp, c["ktap"], c["relu_in"], N.ptr(self.dw), N.ptr(self.pw), N.ptr(self.scale), N.ptr(self.shift), Cout,
                                         c["relu_out"], layout, H2, W2, N.ptr(out), None if u is None else N.ptr(u), N.stream_ptr()), what)
        torch.cuda.synchronize()
        if layout == 0:
            got = _planes(out, Cout, H, W, kp, what)
        elif layout == 1:
            feat = out.cpu().numpy()
            assert (feat != SENT).all(), what
            got = R.from_layout1(feat.astype(np.float64), Cout)
        elif layout == 2:
            got = _xpooled(out, Cout, W, what)
        else:
            bits = out.cpu().numpy().view(np.uint16)
            valid, zeros, pads = R.split_planes(bits, Cout, H2, W2, kp)
            assert (pads == SENT_BITS).all() and (zeros.view(np.float16) == 0).all(), what
            got = np.ascontiguousarray(valid).view(np.float16).astype(np.float64)
        return got, (None if u is None else _planes(u, Cin, H, W, kp, what + " u")), out, u


def _expected_route(mode, layout):
    return 2 if mode != 0 and layout in (0, 2) else 0


@pytest.mark.parametrize("exact", KINDS, ids=KIND_IDS)
@pytest.mark.parametrize("name", list(R.SEP3_CASES))
def test_h_sepconv_k3_both_routes(name, exact):
    """Each case under tile mode 0 (sepconv_h_kernel<3, MT>) and 1 (sepconv_h_ftile_kernel<MT, XP, UOUT>; out_layout 1 stays on the one-window
    kernel): orcai_sepconv_route names the kernel, u and out are checked against float64 (check_sep), and the two routes' u_out have identical bits."""
    c = R.sep3_case(name, exact)
    s = _Sep(c)
    layout, with_u = c["layout"], c["with_u"]
    u_raw, routes = {}, set()
    for mode in (0, 1):
        what = f"{name}, tile mode {mode}"
        with _Knobs(s.lib, orcai_sepconv_tile_mode=mode):
            # the launch that stores u (for a planes + u case: the case itself)
            assert s.lib.orcai_sepconv_route(1, c["Cin"], c["Cout"], c["H"], c["W"], 0, 1) == _expected_route(mode, 0), what
            out, u_dev, _, u_raw[mode] = s.sepconv(0, True, what + " (u_out)")
            if not (layout == 0 and with_u):
                route = s.lib.orcai_sepconv_route(1, c["Cin"], c["Cout"], c["H"], c["W"], layout, 0)
                assert route == _expected_route(mode, layout), (what, route)
                routes.add(route)
                out = s.sepconv(layout, False, what)[0]
            else:
                routes.add(_expected_route(mode, 0))
        _report(what, R.check_sep(c, u_dev, out, exact), "sep3 window" if mode == 0 else "sep3 flat")
    assert routes == ({0} if layout == 1 else {0, 2})
    assert torch.equal(u_raw[0].view(torch.int16), u_raw[1].view(torch.int16)), f"{name}: the two routes' depthwise outputs differ in bits"


@pytest.mark.parametrize("exact", KINDS, ids=KIND_IDS)
@pytest.mark.parametrize("name", list(R.SEPK_CASES))
def test_h_sepconv_k5_k7_and_pointwise_scatter(name, exact):
    """sepconv_h_kernel<5|7|1, MT> on planes wider than one window: plane output with u, x-pooled output, and the ktap = 1 pass scatter-added in f16
    onto a non-zero start image with odd H2, W2 (u16 |val| + u16 |start + val| + 2 * 2^-24 on top of the pointwise bound; every other pixel keeps
    its value exactly)."""
    c = R.sepk_case(name, exact)
    s = _Sep(c)
    out, u_dev, _, _ = s.sepconv(0, True, name + " (u_out)")
    if not (c["layout"] == 0 and c["with_u"]):
        out = s.sepconv(c["layout"], False, name)[0]
    _report(name, R.check_sep(c, u_dev, out, exact), "sepk")


# ------------------------------------------------------------------------------------------------- orcai_h_sepconv_stats, orcai_h_sepconv_stats_bn
def _stats_launch(s, c, bn, what):
    """-> (out, u as float64, mean, var of orcai_h_bn_finish_sharded, raw out, raw u)."""
    N, lib = s.N, s.lib
    B, Cin, Cout, H, W = c["B"], c["Cin"], c["Cout"], c["H"], c["W"]
    COo = (Cout + 7) // 8
    out, u = _sent(B, COo, s.HP, s.WP, 8), _sent(B, (Cin + 7) // 8, s.HP, s.WP, 8)
    shards = torch.full((32 * COo * 16 + 16,), SENT, dtype=torch.float64, device="cuda")  # the launcher zeroes its own [32][COo][16]
    mean, var = _sent(Cout + 1, dtype=torch.float32), _sent(Cout + 1, dtype=torch.float32)
    with _Knobs(lib, orcai_sepconv_tile_mode=1):
        assert lib.orcai_sepconv_route(1, Cin, Cout, H, W, 0, 3 if bn else 2) == 2, what
        if bn:
            rc = lib.orcai_h_sepconv_stats_bn(N.ptr(s.x), B, Cin, H, W, *[N.ptr(t) for t in s.bn], c["eps"], N.ptr(s.dw), N.ptr(s.pw), N.ptr(s.scale), N.ptr(s.shift), Cout, N.ptr(out),
                                              N.ptr(u), N.ptr(shards), N.stream_ptr())
        else:
            rc = lib.orcai_h_sepconv_stats(N.ptr(s.x), B, Cin, H, W, c["relu_in"], N.ptr(s.dw), N.ptr(s.pw), N.ptr(s.scale), N.ptr(s.shift), Cout, N.ptr(out), N.ptr(u),
                                           N.ptr(shards), N.stream_ptr())
    N.check(rc, what)
    N.check(lib.orcai_h_bn_finish_sharded(N.ptr(shards), B, Cout, H, W, N.ptr(mean), N.ptr(var), N.stream_ptr()), what + " finish")
    torch.cuda.synchronize()
    assert (shards[-16:] == SENT).all() and mean[Cout] == SENT and var[Cout] == SENT, what
    return (_planes(out, Cout, H, W, 3, what), _planes(u, Cin, H, W, 3, what + " u"), mean[:Cout].cpu().numpy().astype(np.float64), var[:Cout].cpu().numpy().astype(np.float64),
            out, u)


@pytest.mark.parametrize("exact", KINDS, ids=KIND_IDS)
@pytest.mark.parametrize("name", list(R.STATS_CASES))
def test_h_sepconv_stats(name, exact):
    """sepconv_h_ftile_kernel<MT, false, true, true>: out and u as orcai_h_sepconv's (and bit for bit equal to them), the finished mean and biased
    variance of the unrounded output at half_trunk_ref.stats_bounds (derived from the summation tree; both kinds)."""
    c = R.stats_case(name, exact)
    s = _Sep(c)
    out, u_dev, mean, var, out_raw, u_raw = _stats_launch(s, c, False, name)
    _report(name, R.check_sep(c, u_dev, out, exact), "stats")
    _report(name, R.check_stats(c, u_dev, mean, var), "stats mean/var")
    with _Knobs(s.lib, orcai_sepconv_tile_mode=1):
        _, _, out2, u2 = s.sepconv(0, True, name + " (orcai_h_sepconv)")
    assert torch.equal(out_raw.view(torch.int16), out2.view(torch.int16)) and torch.equal(u_raw.view(torch.int16), u2.view(torch.int16)), name


@pytest.mark.parametrize("exact", KINDS, ids=KIND_IDS)
@pytest.mark.parametrize("name", list(R.STATS_CASES))
def test_h_sepconv_stats_bn(name, exact):
    """sepconv_h_ftile_kernel<MT, false, true, true, true>: the planes hold the pre-normalisation tensor, y_a = f16(relu(fma(v, sc, sh))) is formed
    on load and is ZERO outside the image.  Against the float64 BatchNorm-on-load reference; gamma of both signs, one exactly 0, eps = 1e-3 (normal kind)."""
    c = dict(R.stats_case(name, exact), relu_in=0)
    s = _Sep(c, bn=c["bn"])
    out, u_dev, mean, var, _, _ = _stats_launch(s, c, True, name)
    _report(name, R.check_sep(c, u_dev, out, exact, bn=c["bn"]), "stats_bn")
    _report(name, R.check_stats(c, u_dev, mean, var), "stats_bn mean/var")
