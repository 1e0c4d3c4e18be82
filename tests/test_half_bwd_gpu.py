"""The backward launchers of the f16 training path (orcai_amd/csrc/half_bwd.hip) one by one through the C ABI against float64
(tests/half_bwd_ref.py, itself checked on the CPU by tests/test_half_bwd_ref.py), and the f32 pooling backward on the same cases.

Inputs are f16-representable; every output buffer is pre-filled with a sentinel, so "not written" and "written as zero" differ: pads keep the
fill, the channels >= C of the last octet are zero at the image's pixels, one more image (or a guard) behind every buffer keeps the fill, and
accumulating outputs (dW, D) start from a non-zero constant.  Bounds are derived in half_bwd_ref.py from the kernels' expressions; every test
prints its largest error / bound (DESIGN.md records them)."""

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import half_bwd_ref as R  # noqa: E402

SENT = 30000.0  # a finite f16 (and f32) no result comes near
BITS16 = int(np.float16(SENT).view(np.uint16))
BITS32 = int(np.float32(SENT).view(np.uint32))
EPS = R.EPS


def _dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()  # a copy: the shared cases are read-only


def _oct(x, k):
    return _dev(R.to_octet_planes(np.asarray(x).astype(np.float16), k))


def _quad(x, k):
    return _dev(R.to_quad_planes(np.asarray(x).astype(np.float32), k))


def _filled(B, C, H, W, k, group=8):
    """B + 1 images of sentinel planes (octets of f16 or quads of f32): the kernel gets the first B."""
    Rr = k // 2
    return torch.full((B + 1, (C + group - 1) // group, H + 2 * Rr, R.padded_width(W, k), group), SENT, dtype=torch.float16 if group == 8 else torch.float32, device="cuda")


def _planes_out(t, B, C, H, W, k, tag, group=8, fill=None, written=True):
    """-> the real elements as float64 after the assertions on what may and must be written."""
    torch.cuda.synchronize()
    bits = t.cpu().numpy().view(np.uint16 if group == 8 else np.uint32)
    fill = (BITS16 if group == 8 else BITS32) if fill is None else fill
    if bits.shape[0] > B:
        assert (bits[B:] == fill).all(), f"{tag}: wrote behind the last image"
    valid = R.check_planes(bits[:B], C, H, W, k, fill, tag, group, written)
    return valid.view(np.float16 if group == 8 else np.float32).astype(np.float64)


def _report(name, case_id, worst):
    print(f"RATIO {name} {case_id} {worst:.4f}")


def _vec(a):
    return _dev(np.asarray(a, dtype=np.float32))


# ------------------------------------------------------------------------------------------------- pooling backward
POOL_IDS = [R.pool_case_id(c) for c in R.POOL_CASES]


def _pool_run(case, family, half):
    from orcai_amd import _native as N

    lib, st = N.lib(), N.stream_ptr()
    C, H, W, k = case
    B, G = R.POOL_B, 8 if half else 4
    c = R.pool_case(case, family)
    CG, Ho, Wo = (C + G - 1) // G, (H + 1) // 2, (W + 1) // 2
    planes = _oct if half else _quad
    dd, vv = planes(c["dout"], k), planes(c["v"], k)
    gd, md, vd = _vec(c["gamma"]), _vec(c["mean"]), _vec(c["var"])
    tag = f"{'h_' if half else ''}pool_bwd {R.pool_case_id(case)} {family}"
    bound = R.f32_chain_bound(c["S_dyx"], R.C_POOL_SUMS) + R.f64_sum_bound(c["S_dyx"])
    worst = 0.0
    for bias in (0, 1):
        dy = _filled(B, C, H, W, k, G)
        sums, dsum = torch.full((2 * G * CG + 4,), 5.0, dtype=torch.float64, device="cuda"), torch.full((G * CG + 4,), 5.0, dtype=torch.float64, device="cuda")
        dbias = torch.full((C + 1,), SENT, device="cuda")
        head = (N.ptr(dd), N.ptr(vv), B, C, H, W, k, N.ptr(dy), N.ptr(gd), N.ptr(md), N.ptr(vd), EPS, N.ptr(sums))
        if bias:
            fn = lib.orcai_h_pool_bwd_bn_bias if half else lib.orcai_pool_bwd_bn_bias
            N.check(fn(*head, N.ptr(dsum), N.ptr(dbias), st), tag)
        else:
            fn = lib.orcai_h_pool_bwd_bn if half else lib.orcai_pool_bwd_bn
            N.check(fn(*head, st), tag)
        got = _planes_out(dy, B, C, H, W, k, tag, G)
        R.check_equal(got, c["dy"], tag + " dy")
        s = sums.cpu().numpy()
        R.check_equal(s[:C], c["s_dy"], tag + " sum dy")
        assert (s[C : G * CG] == 0).all() and (s[G * CG + C : 2 * G * CG] == 0).all() and (s[2 * G * CG :] == 5.0).all(), tag
        worst = max(worst, R.check_within(s[G * CG : G * CG + C], c["s_dyx"], bound, tag + " sum dy xhat"))
        if bias:
            db = dbias.cpu().numpy()
            R.check_equal(db[:C], c["s_dout"], tag + " dbias")
            assert db[C] == np.float32(SENT) and (dsum.cpu().numpy()[G * CG :] == 5.0).all(), tag
    return worst


@pytest.mark.parametrize("family", R.POOL_FAMILIES)
@pytest.mark.parametrize("case", R.POOL_CASES, ids=POOL_IDS)
def test_h_pool_bwd_bn_chunks(case, family):
    """orcai_h_pool_bwd_bn and orcai_h_pool_bwd_bn_bias over several chunks of PB_ROWS pooled rows (the carry, the i0 - 1 pre-roll, idle lanes in the
    reduction, two workgroups at 33 x 171): dy bit-equal, sum dy and dbias exact, sum dy xhat within (34 + 5) u32 sum |dy xhat|."""
    _report("h_pool_bwd_bn", f"{R.pool_case_id(case)}-{family}", _pool_run(case, family, True))


@pytest.mark.parametrize("family", R.POOL_FAMILIES)
@pytest.mark.parametrize("case", R.POOL_CASES, ids=POOL_IDS)
def test_pool_bwd_bn_chunks_f32(case, family):
    """orcai_pool_bwd_bn and orcai_pool_bwd_bn_bias (quad planes) on the same cases: pool_bwd_kernel has the same chunk structure."""
    _report("pool_bwd_bn", f"{R.pool_case_id(case)}-{family}", _pool_run(case, family, False))


# ------------------------------------------------------------------------------------------------- orcai_h_bn_bwd_pointwise
def _sums_bounds(ref_b, ref_g, Sb, Sg):
    """dbeta: a float64 sum of f16 values stored as f32; dgamma: a float64 sum of exact products with an f32 xhat (N_DGAMMA u32), stored as f32."""
    return R.U32 * np.abs(ref_b) + R.f64_sum_bound(Sb), R.U32 * np.abs(ref_g) + R.N_DGAMMA * R.U32 * Sg + R.f64_sum_bound(Sg)


@pytest.mark.parametrize("case", R.PW_CASES, ids=[R.pw_case_id(c) for c in R.PW_CASES])
def test_h_bn_bwd_pointwise(case):
    """dbeta and dgamma against float64, dv per element within the f16-output bound (N_BN_BWD = 21 roundings on the size of the subtracted terms), du
    against the float64 contraction of the dv the kernel stored with the f16 weights; k = 5 / 7, sums handed in, W >= 64, dv aliasing dy."""
    from orcai_amd import _native as N
    from orcai_amd.half import pack_pointwise_fragments

    lib, st = N.lib(), N.stream_ptr()
    C, Cin, H, W, k, relu, ready, inplace = case
    B, CO = R.PW_B, (C + 7) // 8
    c = R.pw_case(case)
    tag = "h_bn_bwd_pointwise " + R.pw_case_id(case)
    dyd, vd = _oct(c["dy"], k), _oct(c["v"], k)
    w = _dev(pack_pointwise_fragments(c["wt"].astype(np.float32)))  # A fragments with k = conv-output channel, row = conv-input channel
    md, vard, gd, bd = _vec(c["mean"]), _vec(c["var"]), _vec(c["gamma"]), _vec(c["beta"])
    dv = dyd if inplace else _filled(B, C, H, W, k)
    du = _filled(B, Cin, H, W, k)
    scratch = np.full(16 * CO + 4, 5.0)
    if ready:  # as orcai_h_pool_bwd_bn lays them out: [2][8 CO]
        scratch[: 16 * CO] = 0.0
        scratch[:C], scratch[8 * CO : 8 * CO + C] = c["dbeta"], c["dgamma"]
    sd = _dev(scratch)
    dbeta, dgamma = torch.full((C + 1,), SENT, device="cuda"), torch.full((C + 1,), SENT, device="cuda")

    def call(C_=C, Cin_=Cin):
        return lib.orcai_h_bn_bwd_pointwise(N.ptr(dyd), N.ptr(vd), B, C_, H, W, k, N.ptr(md), N.ptr(vard), N.ptr(gd), N.ptr(bd), EPS, relu, N.ptr(sd), ready, N.ptr(dbeta),
                                            N.ptr(dgamma), N.ptr(w), Cin_, N.ptr(dv), N.ptr(du), st)

    N.check(call(), tag)
    got_dv = _planes_out(dv, B, C, H, W, k, tag + " dv", fill=0 if inplace else None, written=not inplace)
    got_du = _planes_out(du, B, Cin, H, W, k, tag + " du")
    db, dg = dbeta.cpu().numpy(), dgamma.cpu().numpy()
    assert db[C] == np.float32(SENT) and dg[C] == np.float32(SENT) and (sd.cpu().numpy()[16 * CO :] == 5.0).all(), tag
    bb, bg = _sums_bounds(c["dbeta"], c["dgamma"], c["Sb"], c["Sg"])
    r_b, r_g = R.check_within(db[:C], c["dbeta"], bb, tag + " dbeta"), R.check_within(dg[:C], c["dgamma"], bg, tag + " dgamma")
    if ready:
        assert np.array_equal(db[:C], c["dbeta"].astype(np.float32)) and np.array_equal(dg[:C], c["dgamma"].astype(np.float32)), tag
    r_v = R.check_within(got_dv, c["dv"], R.f16_out_bound(c["dv"], c["S"], R.N_BN_BWD), tag + " dv")
    want_du, S_du = R.du_ref(got_dv, c["wt"])
    r_u = R.check_within(got_du, want_du, R.f16_out_bound(want_du, S_du, R.mfma_sum_count(8 * CO)), tag + " du")
    _report("h_bn_bwd_pointwise", R.pw_case_id(case), max(r_b, r_g, r_v, r_u))
    print(f"  dbeta {r_b:.4f} dgamma {r_g:.4f} dv {r_v:.4f} du {r_u:.4f} gated {float(c['gated']):.5f}")
    # more than 64 channels on either side: refused with nothing touched
    before = [t.clone() for t in (dv, du, dbeta, dgamma, sd)]
    assert call(C_=65) == N.E_BADARG and call(Cin_=65) == N.E_BADARG
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip((dv, du, dbeta, dgamma, sd), before)), tag


# ------------------------------------------------------------------------------------------------- orcai_h_outer_reduce
@pytest.mark.parametrize("family", R.OUTER_FAMILIES)
@pytest.mark.parametrize("case", list(R.OUTER_CASES), ids=[R.outer_case_id(c) for c in R.OUTER_CASES])
def test_h_outer_reduce(case, family):
    """D += A (x) Bq over the pixels, on top of a non-zero start: small integers bit-equal to float64, N(0, 1) within the f32-chain bound
    (R.outer_chain); the grid-stride loop, the workspace-limited grid (nothing written behind the workspace), a_stride2 on a wide plane."""
    from orcai_amd import _native as N

    lib, st = N.lib(), N.stream_ptr()
    Ca, Cb, H, W, k, B, ws, s2 = case
    c, geo = R.outer_case(case, family), R.outer_geo(case)
    tag = f"h_outer_reduce {R.outer_case_id(case)} {family}"
    n = ws or R.OUTER_AMPLE
    ad, bd = _oct(c["a"], k), _oct(c["b"], k)
    wsd = torch.full((n + 4096,), SENT, device="cuda")
    start = 3.0 if family == "exact" else 0.5
    D = torch.full((Ca * Cb + 16,), start, device="cuda")
    N.check(lib.orcai_h_outer_reduce(N.ptr(ad), Ca, N.ptr(bd), Cb, B, H, W, k, s2, c["Ha"] if s2 else 0, c["Wa"] if s2 else 0, N.ptr(D), N.ptr(wsd), n, st), tag)
    torch.cuda.synchronize()
    assert bool((wsd[n:] == SENT).all()), f"{tag}: wrote behind the workspace"
    got = D.cpu().numpy().astype(np.float64)
    assert (got[Ca * Cb :] == start).all(), tag
    got = got[: Ca * Cb].reshape(Ca, Cb)
    if family == "exact":
        assert np.abs(c["S"]).max() + start < 2.0**24
        worst = R.check_equal(got, c["D"] + start, tag)
    else:
        worst = R.check_within(got, c["D"] + start, R.f32_chain_bound(c["S"] + start, R.outer_chain(geo)), tag)
    _report("h_outer_reduce", f"{R.outer_case_id(case)}-{family}", worst)


# ------------------------------------------------------------------------------------------------- BatchNorm statistics and apply
@pytest.mark.parametrize("case", list(R.STATS_CASES), ids=[f"C{c[0]}-{c[1]}x{c[2]}-k{c[3]}-B{c[4]}" for c in R.STATS_CASES])
def test_h_bn_planes_stats_exact(case):
    """Small integers: the sums are exact integers, so mean and variance equal float32 of the float64 result bit for bit, on the sharded route and on
    the plane >= 32768 route; orcai_h_planes_sum on the same planes with accumulate 0 and 1."""
    from orcai_amd import _native as N

    lib, st = N.lib(), N.stream_ptr()
    C, H, W, k, B = case
    CO = (C + 7) // 8
    v = R.ints_case((B, C, H, W), [C, H, W, k, B])
    vd = _oct(v, k)
    mean, var = torch.full((C + 1,), SENT, device="cuda"), torch.full((C + 1,), SENT, device="cuda")
    scratch = torch.full((16 * CO * 32 + 8,), 5.0, dtype=torch.float64, device="cuda")
    N.check(lib.orcai_h_bn_planes_stats(N.ptr(vd), B, C, H, W, k, N.ptr(scratch), N.ptr(mean), N.ptr(var), st), "h_bn_planes_stats")
    torch.cuda.synchronize()
    m, va = R.bn_stats_ref(v)
    assert np.array_equal(mean.cpu().numpy()[:C], m.astype(np.float32)) and np.array_equal(var.cpu().numpy()[:C], va.astype(np.float32))
    assert float(mean[C]) == SENT and float(var[C]) == SENT and bool((scratch[16 * CO * 32 :] == 5.0).all())
    want = R.planes_sum_ref(v)
    for accumulate in (0, 1):
        out = torch.full((C + 1,), 7.0, device="cuda")
        sc = torch.full((8 * CO + 4,), 5.0, dtype=torch.float64, device="cuda")
        N.check(lib.orcai_h_planes_sum(N.ptr(vd), B, C, H, W, k, N.ptr(sc), N.ptr(out), accumulate, st), "h_planes_sum")
        torch.cuda.synchronize()
        o = out.cpu().numpy().astype(np.float64)
        R.check_equal(o[:C], want + 7.0 * accumulate, f"h_planes_sum accumulate={accumulate}")
        assert o[C] == 7.0 and bool((sc[8 * CO :] == 5.0).all())


def test_h_bn_finish_sharded_by_hand():
    """orcai_h_bn_finish_sharded on 32 shards [CO][16] of integers laid out by hand (sum | sum of squares per octet), C = 13 of two octets."""
    from orcai_amd import _native as N

    lib = N.lib()
    C, B, H, W = 13, 2, 5, 13
    rng = np.random.default_rng(13)
    shards = np.zeros((32, 2, 16))
    shards[:, :, :8] = rng.integers(-50, 51, size=(32, 2, 8))
    shards[:, :, 8:] = rng.integers(1000, 2001, size=(32, 2, 8))
    mean, var = torch.full((C + 1,), SENT, device="cuda"), torch.full((C + 1,), SENT, device="cuda")
    sd = _dev(shards)
    N.check(lib.orcai_h_bn_finish_sharded(N.ptr(sd), B, C, H, W, N.ptr(mean), N.ptr(var), N.stream_ptr()), "h_bn_finish_sharded")
    torch.cuda.synchronize()
    m, va = R.shards_stats_ref(shards, C, B * H * W)
    assert np.array_equal(mean.cpu().numpy()[:C], m.astype(np.float32)) and np.array_equal(var.cpu().numpy()[:C], va.astype(np.float32))
    assert float(mean[C]) == SENT and float(var[C]) == SENT and (va > 0).all()


@pytest.mark.parametrize("case", R.APPLY_CASES, ids=[f"C{c[0]}-{c[1]}x{c[2]}-k{c[3]}-relu{c[4]}" for c in R.APPLY_CASES])
def test_h_bn_planes_apply(case):
    """y = [relu](v s + t) per element within the f16-output bound (N_BN_APPLY = 7 roundings on |v s| + |beta| + |mean s|), gamma of both signs."""
    from orcai_amd import _native as N

    lib = N.lib()
    C, H, W, k, relu = case
    B = R.APPLY_B
    rng = np.random.default_rng([C, H, W, k, relu])
    v = R.f16(2.0 * rng.standard_normal((B, C, H, W)))
    mean, var, gamma, beta = R._bn_vectors(rng, C)
    y = _filled(B, C, H, W, k)
    vd, md, vard, gd, bd = _oct(v, k), _vec(mean), _vec(var), _vec(gamma), _vec(beta)
    N.check(lib.orcai_h_bn_planes_apply(N.ptr(vd), B, C, H, W, k, N.ptr(md), N.ptr(vard), N.ptr(gd), N.ptr(bd), EPS, relu, N.ptr(y), N.stream_ptr()), "h_bn_planes_apply")
    got = _planes_out(y, B, C, H, W, k, "h_bn_planes_apply")
    want, S = R.bn_apply_ref(v, mean, var, gamma, beta, EPS, relu)
    assert (gamma < 0).any() and (gamma > 0).any() and (not relu or 0.1 < (want == 0).mean() < 0.9)
    _report("h_bn_planes_apply", f"C{C}-{H}x{W}-k{k}-relu{relu}", R.check_within(got, want, R.f16_out_bound(want, S, R.N_BN_APPLY), "h_bn_planes_apply"))


# ------------------------------------------------------------------------------------------------- orcai_h_conv0_bn_bwd, orcai_h_conv0_bn_bwd_ready
@pytest.mark.parametrize("case", R.CONV0_CASES, ids=[R.conv0_case_id(c) for c in R.CONV0_CASES])
def test_h_conv0_bn_bwd(case):
    """The entry conv's weight gradient with bn0 + ReLU backward on the fly, on top of a non-zero start, within the f32-chain bound (R.conv0_chain);
    dbeta and dgamma against float64; the _ready variant with the sums handed in; snippets further apart than H W with NaN between them; 400 x 171:
    a thread of the 256 x 256 grid takes a second pixel."""
    from orcai_amd import _native as N

    lib, st = N.lib(), N.stream_ptr()
    H, W, k, B, extra = case
    c = R.conv0_case(case)
    tag = "h_conv0_bn_bwd " + R.conv0_case_id(case)
    stride = H * W + extra
    xin = np.full(B * stride + 64, np.nan, dtype=np.float32)
    for b in range(B):
        xin[b * stride : b * stride + H * W] = c["x"][b].reshape(-1)
    xd, dyd, vd = _dev(xin), _oct(c["dy"], k), _oct(c["v"], k)
    md, vard, gd, bd = _vec(c["mean"]), _vec(c["var"]), _vec(c["gamma"]), _vec(c["beta"])
    start = 0.25
    bound = R.f32_chain_bound(c["T"] + start, R.conv0_chain(B, H, W))
    bb, bg = _sums_bounds(c["dbeta"], c["dgamma"], c["Sb"], c["Sg"])
    got = {}
    for ready in (0, 1):
        dW = torch.full((k * k * 16 + 16,), start, device="cuda")
        scratch = np.full(32 + 4, 5.0)
        if ready:
            scratch[:16], scratch[16:32] = c["dbeta"], c["dgamma"]
        sd = _dev(scratch)
        dbeta, dgamma = torch.full((17,), SENT, device="cuda"), torch.full((17,), SENT, device="cuda")
        fn = lib.orcai_h_conv0_bn_bwd_ready if ready else lib.orcai_h_conv0_bn_bwd
        N.check(fn(N.ptr(xd), stride, N.ptr(dyd), N.ptr(vd), B, H, W, k, N.ptr(md), N.ptr(vard), N.ptr(gd), N.ptr(bd), EPS, N.ptr(sd), N.ptr(dbeta), N.ptr(dgamma), N.ptr(dW), st),
                tag)
        torch.cuda.synchronize()
        w = dW.cpu().numpy().astype(np.float64)
        db, dg = dbeta.cpu().numpy(), dgamma.cpu().numpy()
        assert (w[k * k * 16 :] == start).all() and db[16] == np.float32(SENT) and dg[16] == np.float32(SENT) and (sd.cpu().numpy()[32:] == 5.0).all(), tag
        got[ready] = w[: k * k * 16].reshape(k * k, 16)
        r_w = R.check_within(got[ready], c["dW"] + start, bound, f"{tag} ready={ready} dW")
        r_b, r_g = R.check_within(db[:16], c["dbeta"], bb, tag + " dbeta"), R.check_within(dg[:16], c["dgamma"], bg, tag + " dgamma")
        if ready:
            assert np.array_equal(db[:16], c["dbeta"].astype(np.float32)) and np.array_equal(dg[:16], c["dgamma"].astype(np.float32)), tag
        _report("h_conv0_bn_bwd" + ("_ready" if ready else ""), R.conv0_case_id(case), max(r_w, r_b, r_g))
        print(f"  dW {r_w:.4f} dbeta {r_b:.4f} dgamma {r_g:.4f} gated {float(c['gated']):.5f}")
    R.check_within(got[1], got[0], 2 * bound, tag + " ready against not ready")


# ------------------------------------------------------------------------------------------------- orcai_h_feat_to_planes, orcai_h_planes_relu_bwd
@pytest.mark.parametrize("C,H,W,k,B", [(13, 5, 21, 3, 2), (30, 3, 65, 7, 1)])
def test_h_feat_to_planes_exact(C, H, W, k, B):
    """Keras Reshape layout f32 -> f16 octet planes: round to nearest even, bit for bit; C no multiple of 8; pads keep the fill."""
    from orcai_amd import _native as N

    rng = np.random.default_rng([C, H, W, k])
    f = (3.0 * rng.standard_normal((B, H, W * C))).astype(np.float32)
    out = _filled(B, C, H, W, k)
    fd = _dev(f)
    N.check(N.lib().orcai_h_feat_to_planes(N.ptr(fd), B, C, H, W, k, N.ptr(out), N.stream_ptr()), "h_feat_to_planes")
    got = _planes_out(out, B, C, H, W, k, "h_feat_to_planes")
    want = R.split_planes(R.feat_to_planes_ref(f, C, H, W, k), C, H, W, k)[0]
    R.check_equal(got, want, "h_feat_to_planes")
    assert (want.astype(np.float32) != f.reshape(B, H, W, C).transpose(0, 3, 1, 2)).mean() > 0.9  # the cast rounded


def test_h_planes_relu_bwd_exact():
    """dx = y > 0 ? dy : 0 on a whole buffer of 8 (3 * 256 + 5) halves (a partly filled last workgroup), zeros of both signs in y; n_halves & 7 != 0 is
    refused with nothing touched."""
    from orcai_amd import _native as N

    lib, st = N.lib(), N.stream_ptr()
    n = 8 * (3 * 256 + 5)
    rng = np.random.default_rng(5)
    dy = rng.standard_normal(n).astype(np.float16)
    y = rng.standard_normal(n).astype(np.float16)
    y[::7], y[3::11] = 0.0, -0.0
    dx = torch.full((n + 64,), SENT, dtype=torch.float16, device="cuda")
    dyd, yd = _dev(dy), _dev(y)
    N.check(lib.orcai_h_planes_relu_bwd(N.ptr(dyd), N.ptr(yd), n, N.ptr(dx), st), "h_planes_relu_bwd")
    torch.cuda.synchronize()
    got = dx.cpu().numpy()
    R.check_equal(got[:n], R.relu_bwd_ref(dy, y), "h_planes_relu_bwd")
    assert (got[n:].view(np.uint16) == BITS16).all()
    before = dx.clone()
    assert lib.orcai_h_planes_relu_bwd(N.ptr(dyd), N.ptr(yd), n - 4, N.ptr(dx), st) == N.E_BADARG
    torch.cuda.synchronize()
    assert torch.equal(dx, before)
