"""Refuse before touching: the k = 3 entry points that zero a buffer before they launch (orcai_sepconv_planes_stats[_bn],
orcai_sepconv_planes_epi, orcai_h_sepconv_stats[_bn]) return ORCAI_E_UNSUPPORTED exactly where orcai_sepconv_route says "window", and
then leave `out`, `u_out` and `shards` untouched; where they accept, `out` equals the one-window kernel's (orcai_sepconv_tile_mode(0))
bit for bit.  One shape on each side of every boundary the route has (csrc/sep_route.h): the chunk limit, the LDS limit with the
entry's static surcharge, the strip rule, tile mode 0.  The boundary shapes are found on the host by scanning the query."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from half_fwd_ref import to_octet_planes  # noqa: E402

B, H, SENTINEL = 1, 2, -7.5
# entry -> (half, extras of orcai_sepconv_route)
ENTRIES = {"planes_stats": (0, 2), "planes_stats_bn": (0, 3), "planes_epi2": (0, 4), "planes_epi3": (0, 5), "h_stats": (1, 2), "h_stats_bn": (1, 3)}


def _last_accepted(lib, half, extras, Cin, Cout):
    """The first width W whose route is not window while W + 1's is (R = 1 planes of H rows, plane output, current tile mode)."""
    for W in range(1, 700):
        if lib.orcai_sepconv_route(half, Cin, Cout, H, W, 0, extras) != 0 and lib.orcai_sepconv_route(half, Cin, Cout, H, W + 1, 0, extras) == 0:
            return W
    return None


def _cases(lib, half, extras):
    """(tile mode, Cin, Cout, W) on each side of every boundary of this entry; asserts the figures today's formulas predict."""
    prev = lib.orcai_sepconv_tile_mode(1)
    try:
        w_chunk = _last_accepted(lib, half, extras, 16, 16)  # one output tile: never strips, small LDS: the 24-chunk limit
        w_lds = _last_accepted(lib, half, extras, 64, 64)    # four output tiles, 16 input quads: the LDS limit, if it comes first
        wide_strip = lib.orcai_sepconv_route(half, 30, 30, H, w_chunk + 5, 0, extras)
    finally:
        lib.orcai_sepconv_tile_mode(prev)
    assert w_chunk is not None and w_lds is not None and w_lds <= w_chunk
    cases = [(1, 16, 16, w_chunk), (1, 16, 16, w_chunk + 1)]
    if w_lds < w_chunk:  # (the f16 kernel's rows are half as wide: at <= 64 channels its LDS limit lies beyond the chunk limit)
        cases += [(1, 64, 64, w_lds), (1, 64, 64, w_lds + 1), (1, 16, 16, w_lds + 1)]
    if not half:
        assert w_chunk == 515
        if extras == 2:
            assert w_lds == 419
        # past the chunk limit only strips are left: two output tiles and <= 8 input quads, tile mode 1, not epi 3
        assert wide_strip == (0 if extras == 5 else 1)
    else:
        assert wide_strip == 0  # no strip kernel on the f16 path
    cases += [(1, 30, 30, w_chunk + 5), (1, 40, 30, w_chunk + 5), (1, 30, 33, w_chunk + 5), (2, 30, 30, w_chunk + 5), (2, 30, 30, 171)]
    cases += [(0, 16, 16, 64), (1, 16, 16, 64)]
    return cases


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.float16 else torch.int32 if t.dtype == torch.float32 else torch.int64)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _run(lib, N, entry, Cin, Cout, W, rng):
    """Runs `entry` under the current tile mode on sentinel-filled destinations; returns (rc, destinations, their sentinel copies, the
    one-window kernel's `out` on the same operands)."""
    half, _ = ENTRIES[entry]
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    ones, zeros = torch.ones(64, device="cuda"), torch.zeros(64, device="cuda")
    st = N.stream_ptr()
    WP, G = lib.orcai_padded_width(W, 3), 8 if half else 4
    CG, CGo = -(-Cin // G), -(-Cout // G)
    dt = torch.float16 if half else torch.float32
    x = rng.integers(-2, 3, size=(B, Cin, H, W)).astype(np.float32)
    dwk = rng.integers(-1, 2, size=(3, 3, Cin)).astype(np.float32)
    pw = rng.integers(-1, 2, size=(Cin, Cout)).astype(np.float32)
    if half:
        from orcai_amd.half import pack_depthwise_octets, pack_pointwise_fragments

        xin, dwd, pwd = dev(to_octet_planes(x.astype(np.float16), 3)), dev(pack_depthwise_octets(dwk[..., None])), dev(pack_pointwise_fragments(pw))
    else:
        xp = np.zeros((B, CG * 4, H + 2, WP), dtype=np.float32)
        xp[:, :Cin, 1 : 1 + H, :W] = x
        xin = dev(xp.reshape(B, CG, 4, H + 2, WP).transpose(0, 1, 3, 4, 2))
        dq = np.zeros((CG * 4, 9), dtype=np.float32)
        dq[:Cin] = dwk.transpose(2, 0, 1).reshape(Cin, 9)
        dwd, pwd = dev(dq.reshape(CG, 4, 9).transpose(0, 2, 1)), dev(pw)
    fill = lambda *s: torch.full(s, SENTINEL, dtype=dt, device="cuda")  # noqa: E731
    out, u, out_ref = fill(B, CGo, H + 2, WP, G), fill(B, CG, H + 2, WP, G), fill(B, CGo, H + 2, WP, G)
    shards = torch.full((8 * 16 * 32,), SENTINEL, dtype=torch.float64, device="cuda")
    dests = [out, u, shards]
    before = [t.clone() for t in dests]
    # BatchNorm folded on load with mean 0, variance 1, eps 0, gamma 1, beta 0 is exactly ReLU: the reference takes relu_in = 1
    relu_in = 1 if entry.endswith("_bn") else 0
    mode = lib.orcai_sepconv_tile_mode(0)
    try:
        if half:
            rc = lib.orcai_h_sepconv(N.ptr(xin), B, Cin, H, W, 3, 3, relu_in, N.ptr(dwd), N.ptr(pwd), N.ptr(ones), N.ptr(zeros), Cout, 0, 0, 0, 0, N.ptr(out_ref), None, st)
        else:
            rc = lib.orcai_sepconv_planes_u(N.ptr(xin), B, Cin, H, W, 3, 3, relu_in, N.ptr(dwd), N.ptr(pwd), N.ptr(ones), N.ptr(zeros), Cout, 0, 0, 0, 0, N.ptr(out_ref), None, st)
    finally:
        lib.orcai_sepconv_tile_mode(mode)
    assert rc == 0
    if entry == "planes_stats":
        rc = lib.orcai_sepconv_planes_stats(N.ptr(xin), B, Cin, H, W, 0, N.ptr(dwd), N.ptr(pwd), N.ptr(ones), N.ptr(zeros), Cout, N.ptr(out), N.ptr(u), N.ptr(shards), st)
    elif entry == "planes_stats_bn":
        rc = lib.orcai_sepconv_planes_stats_bn(N.ptr(xin), B, Cin, H, W, N.ptr(zeros), N.ptr(ones), N.ptr(ones), N.ptr(zeros), 0.0, N.ptr(dwd), N.ptr(pwd), N.ptr(ones), N.ptr(zeros),
                                               Cout, N.ptr(out), N.ptr(u), N.ptr(shards), st)
    elif entry in ("planes_epi2", "planes_epi3"):
        ref = torch.ones_like(out)  # epi 3 masks by ref > 0: all kept
        rc = lib.orcai_sepconv_planes_epi(N.ptr(xin), B, Cin, H, W, N.ptr(dwd), N.ptr(pwd), N.ptr(ones), N.ptr(zeros), Cout, N.ptr(out), int(entry[-1]), N.ptr(ref), N.ptr(zeros),
                                          N.ptr(ones), N.ptr(ones), N.ptr(zeros), 1e-3, 0, N.ptr(shards), st)
    elif entry == "h_stats":
        rc = lib.orcai_h_sepconv_stats(N.ptr(xin), B, Cin, H, W, 0, N.ptr(dwd), N.ptr(pwd), N.ptr(ones), N.ptr(zeros), Cout, N.ptr(out), N.ptr(u), N.ptr(shards), st)
    else:
        rc = lib.orcai_h_sepconv_stats_bn(N.ptr(xin), B, Cin, H, W, N.ptr(zeros), N.ptr(ones), N.ptr(ones), N.ptr(zeros), 0.0, N.ptr(dwd), N.ptr(pwd), N.ptr(ones), N.ptr(zeros), Cout,
                                          N.ptr(out), N.ptr(u), N.ptr(shards), st)
    torch.cuda.synchronize()
    return rc, dests, before, out_ref


@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_entry_refuses_exactly_where_the_route_is_window_and_touches_nothing(entry):
    from orcai_amd import _native as N

    lib = N.lib()
    half, extras = ENTRIES[entry]
    rng = np.random.default_rng(extras * 2 + half)
    outcomes = set()
    prev = lib.orcai_sepconv_tile_mode(-1)
    try:
        for mode, Cin, Cout, W in _cases(lib, half, extras):
            lib.orcai_sepconv_tile_mode(mode)
            route = lib.orcai_sepconv_route(half, Cin, Cout, H, W, 0, extras)
            assert route in (0, 1, 2)
            rc, dests, before, out_ref = _run(lib, N, entry, Cin, Cout, W, rng)
            what = (entry, mode, Cin, Cout, W, route, rc)
            outcomes.add(route)
            if route == 0:
                assert rc == N.E_UNSUPPORTED, what
                assert all(_same_bits(a, b) for a, b in zip(dests, before)), what
            else:
                assert rc == 0, what
                assert _same_bits(dests[0], out_ref), what
    finally:
        lib.orcai_sepconv_tile_mode(prev)
    assert outcomes == ({0, 2} if half or extras == 5 else {0, 1, 2})
