"""tests/half_fwd_ref.py on the CPU: the float64 references against torch float64, the layout helpers against each other, and the
exact-integer cases of tests/test_half_forward_gpu.py against the range in which f16 holds every integer."""

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import half_fwd_ref as R  # noqa: E402
from oracle.model_ref import same_pad  # noqa: E402

POOL_IDS = [R.pool_case_id(c) for c in R.POOL_CASES]


def _torch_pool_res_add(s, prev, wr, br, bn, eps):
    import torch.nn.functional as F

    x, pv = torch.from_numpy(s), torch.from_numpy(prev)
    if bn is not None:
        mean, var, gamma, beta = (torch.from_numpy(np.asarray(a, dtype=np.float64)) for a in bn)
        sc = gamma / torch.sqrt(var + eps)
        x = x * sc[None, :, None, None] + (beta - mean * sc)[None, :, None, None]
    _, pt, pb = same_pad(s.shape[2], 3, 2)
    _, pl, pr = same_pad(s.shape[3], 2, 2)
    pooled = F.max_pool2d(F.pad(x, (pl, pr, pt, pb), value=float("-inf")), (3, 2), 2)
    w = torch.from_numpy(np.asarray(wr, dtype=np.float64)).t()[:, :, None, None]  # [C][Cp][1][1]
    return (pooled + F.conv2d(pv[..., ::2, ::2], w, torch.from_numpy(np.asarray(br, dtype=np.float64)))).numpy()


@pytest.mark.parametrize("case", R.POOL_CASES, ids=POOL_IDS)
def test_pool_res_add_ref_equals_torch_float64(case):
    shape, B = case
    C, Cp, H, W, k = shape
    s, prev, wr, br, bn = R.pool_bn_case(shape, B)
    gamma = bn[2]
    assert (gamma < 0).any() and (gamma > 0).any() and gamma[C // 2] == 0.0 and gamma[C - 1] < 0 and C // 2 != C - 1
    for a in (s, prev, wr):  # what the kernel is given is what the reference sees
        assert np.array_equal(a, a.astype(np.float16).astype(np.float64))
    eps = R.pool_eps(shape)
    want, S = R.pool_res_add_ref(s, prev, wr, br, bn, eps)
    ref = _torch_pool_res_add(s, prev, wr, br, bn, eps)
    assert want.shape == ref.shape == (B, C, (H + 1) // 2, (W + 1) // 2)
    assert np.isfinite(want).all() and np.abs(want - ref).max() <= 1e-12
    assert S.shape == want.shape and (S >= np.abs(want) - 1e-12).all()  # the triangle inequality, term by term
    # the other eps gives another answer: a kernel that dropped or fixed it cannot pass
    other, _ = R.pool_res_add_ref(s, prev, wr, br, bn, 1e-3 if eps != 1e-3 else 0.0)
    assert np.abs(other - want).max() > 1e-3
    # without BatchNorm
    si, pi, wi, bi = R.pool_int_case(shape, B)
    wanti, Si = R.pool_res_add_ref(si, pi, wi, bi)
    assert np.abs(wanti - _torch_pool_res_add(si, pi, wi, bi, None, 0.0)).max() == 0.0


def test_pool_ref_applies_batchnorm_before_the_maximum():
    """One window, gamma < 0: the answer is BN(min), which max-then-BN gets wrong."""
    s = np.array([1.0, 5.0, -3.0, 2.0]).reshape(1, 1, 2, 2)
    prev, wr, br = np.zeros((1, 1, 2, 2)), np.zeros((1, 1)), np.zeros(1)
    bn = (np.array([1.0]), np.array([4.0]), np.array([-2.0]), np.array([0.5]))
    want, S = R.pool_res_add_ref(s, prev, wr, br, bn, eps=0.0)
    assert want.shape == (1, 1, 1, 1) and want[0, 0, 0, 0] == (-3.0 - 1.0) * -1.0 + 0.5
    assert S[0, 0, 0, 0] == 3.0 + 1.5  # |sc v_sel| + |sh|: v_sel = -3, sc = -1, sh = 0.5 + 1


@pytest.mark.parametrize("case", R.POOL_CASES, ids=POOL_IDS)
def test_pool_integer_cases_stay_exact_in_f16(case):
    shape, B = case
    s, prev, wr, br = R.pool_int_case(shape, B)
    want, S = R.pool_res_add_ref(s, prev, wr, br)
    assert np.array_equal(want, np.rint(want))
    assert S.max() < 1024, S.max()  # every partial sum in any order is below 2048 with a factor 2 to spare
    assert np.array_equal(want.astype(np.float16).astype(np.float64), want)
    for a in (s, prev, wr):
        assert np.array_equal(a.astype(np.float16).astype(np.float64), a)


@pytest.mark.parametrize("shape", list(R.GEMM_SHAPES), ids=lambda s: "x".join(map(str, s)))
def test_gemm_integer_cases_stay_exact(shape):
    M, N, K = shape
    rng, A, W, bias = R.gemm_int_case(shape)
    for act, sk in R.GEMM_EPILOGUES:
        scale, shift = R.gemm_epilogue(rng, N, sk, integers=True)
        for b in (bias, None):
            want, S = R.gemm_ref(A, W, b, scale, shift, act)
            assert np.array_equal(want, np.rint(want))
            bound = S if scale is None else np.abs(scale) * S + np.abs(shift)
            assert np.abs(want).max() <= bound.max() < 2048, bound.max()
        if scale is not None:
            assert (scale < 0).any() and (scale > 0).any() and (shift != 0).all()


def test_gemm_shapes_cover_every_axis_value():
    Ms, Ns, Ks = ({s[i] for s in R.GEMM_SHAPES} for i in range(3))
    assert Ms == {1, 5, 33, 70, 129} and Ns == {7, 17, 64, 65, 130} and Ks == {4, 12, 32, 36, 44, 60, 64, 100, 396}
    for M, N, K in R.GEMM_SHAPES:
        if K % 32:
            assert M % 16 and N % 16, (M, N, K)
    assert {K % 32 for _, _, K in R.GEMM_SHAPES} >= {4, 12, 28} and {K for _, _, K in R.GEMM_SHAPES if K % 8} == {4, 12, 36, 44, 60, 100, 396}


def test_gemm_ref_rounds_operands_to_nearest_even_and_nothing_else():
    rng, A, W, bias = R.gemm_float_case((33, 17, 100))
    scale, shift = R.gemm_epilogue(rng, 17, "pm", integers=False)
    assert (scale < 0).any() and (scale > 0).any()
    want, S = R.gemm_ref(A, W, bias, scale, shift, 1)
    a, w = torch.from_numpy(A).half().double(), torch.from_numpy(W).half().double()  # torch's cast is round to nearest even as well
    ref = torch.relu(a @ w + torch.from_numpy(bias).double()) * torch.from_numpy(scale).double() + torch.from_numpy(shift).double()
    assert np.abs(want - ref.numpy()).max() <= 1e-12
    assert np.abs(A.astype(np.float64) - a.numpy()).max() > 1e-5  # A is not f16-representable: the rounding is there to be seen
    # a tie: 1 + 2^-11 lies midway between the f16 neighbours 1 and 1 + 2^-10 and goes to the even one, 1; 1 + 3 * 2^-11 goes up to 1 + 2^-9
    tie = np.array([[1.0 + 2.0**-11, 1.0 + 3 * 2.0**-11]], dtype=np.float32)
    got, _ = R.gemm_ref(tie, np.eye(2, dtype=np.float32), None, None, None, 0)
    assert got.tolist() == [[1.0, 1.0 + 2.0**-9]]
    # the bound: (K + 8) 2^-23 S_epi, a thirtieth of ONE f16 rounding of a value of size S_epi at K = 100
    S_epi = np.abs(scale.astype(np.float64)) * S + np.abs(shift.astype(np.float64))
    assert np.array_equal(R.gemm_bound(S, 100, scale, shift), 108 * 2.0**-23 * S_epi) and np.array_equal(R.gemm_bound(S, 100, None, None), 108 * 2.0**-23 * S)
    assert 108 * 2.0**-23 < 2.0**-11 / 30
    no_bias, S0 = R.gemm_ref(A, W, None, None, None, 0)
    assert np.abs(no_bias - (a @ w).numpy()).max() <= 1e-12 and np.abs(S0 - (a.abs() @ w.abs()).numpy()).max() <= 1e-12


@pytest.mark.parametrize("C,H,W,k", [(30, 6, 11, 3), (7, 3, 33, 5), (64, 1, 86, 7), (17, 1, 2, 3)])
def test_octet_layout_round_trips(C, H, W, k):
    rng = np.random.default_rng(C + W)
    x = rng.standard_normal((2, C, H, W)).astype(np.float16)
    p = R.to_octet_planes(x, k)
    Rr = k // 2
    assert p.shape == (2, (C + 7) // 8, H + 2 * Rr, (W + Rr + 3) & ~3, 8) and p.dtype == np.float16
    back, pads = R.from_octet_planes(p, C, H, W, k)
    assert np.array_equal(back, x) and not pads.any()
    valid, zeros, outside = R.split_planes(p, C, H, W, k)
    assert np.array_equal(valid, x) and zeros.shape == (2, p.shape[1] * 8 - C, H, W) and not zeros.any() and not outside.any()
    # the three regions are disjoint and cover the planes
    assert valid.size + zeros.size + outside.size == p.size
    sent = np.full(p.shape, 3.0, dtype=np.float16)  # 1 at the image's pixels in every channel, 3 outside
    sent.transpose(0, 1, 4, 2, 3)[:, :, :, Rr : Rr + H, :W] = 1.0
    v3, z3, o3 = R.split_planes(sent, C, H, W, k)
    assert (v3 == 1.0).all() and (z3 == 1.0).all() and (o3 == 3.0).all()
    # quad planes (the f32 twin's layout)
    q = R.to_quad_planes(x.astype(np.float32), k)
    assert q.shape == (2, (C + 3) // 4, H + 2 * Rr, (W + Rr + 3) & ~3, 4)
    qb, qp = R.from_quad_planes(q, C, H, W, k)
    assert np.array_equal(qb, x.astype(np.float32)) and not qp.any()


def test_xpooled_layout():
    s = np.arange(2 * 9 * 3 * 5, dtype=np.float64).reshape(2, 9, 3, 5) - 100.0
    p = R.to_xpooled(s, fill=777.0)
    assert p.shape == (2, 2, 3, 4, 8) and p.dtype == np.float16
    full = p.transpose(0, 1, 4, 2, 3).reshape(2, 16, 3, 4)
    assert np.array_equal(full[:, :9, :, :2], np.maximum(s[..., 0:4:2], s[..., 1:4:2])) and np.array_equal(full[:, :9, :, 2], s[..., 4])
    assert (full[:, :9, :, 3] == 777.0).all() and not full[:, 9:].any()
