"""The four launchers of the ResNet1DConv head (ReduceFrequencyMean and Conv1D(num_labels, k, "same") + sigmoid, forward and backward),
called directly through the C ABI and compared with float64 numpy.

Tolerances: exact equality where the arithmetic is exact (one IEEE division; small integers); the worst-case summation bound
gamma_n = n u / (1 - n u), u = 2^-24, times the sum of the magnitudes of the terms, n = the number of roundings on the longest path;
and for the sigmoid outputs 2e-6, the bar tests/test_train_head_gpu.py states for f32 sigmoid outputs against float64 (the kernel's
__expf is approximate, so the summation bound alone does not cover it)."""

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

U = 2.0**-24


def gamma(n):
    return n * U / (1.0 - n * U)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---------------------------------------------------------------- ReduceFrequencyMean on the Keras Reshape layout (feature = x * C + c)
FREQ_SHAPES = [(1, 1, 1), (7, 3, 36), (300, 11, 36), (33, 22, 50)]


@pytest.mark.parametrize("M,W,C", FREQ_SHAPES)
def test_freq_mean_vs_float64(M, W, C):
    """out[m][c] = mean over x of feat[m][x*C + c].  W additions (the first onto 0 is exact) and one division: gamma_{W+1} mean|feat|."""
    from orcai_amd import _native as N

    feat = np.random.default_rng(M + W).standard_normal((M, W, C)).astype(np.float32)
    fd, out = _dev(feat.reshape(M, W * C)), torch.full((M, C), 777.0, dtype=torch.float32, device="cuda")
    N.check(N.lib().orcai_freq_mean(N.ptr(fd), M, W, C, N.ptr(out), N.stream_ptr()), "orcai_freq_mean")
    f64 = feat.astype(np.float64)
    err = np.abs(out.cpu().numpy().astype(np.float64) - f64.mean(axis=1))
    bound = gamma(W + 1) * np.abs(f64).mean(axis=1)
    assert float((err - bound).max()) <= 0.0, (float(err.max()), float(bound.min()))


@pytest.mark.parametrize("M,W,C", FREQ_SHAPES)
def test_freq_mean_bwd_is_one_division(M, W, C):
    """dfeat[m][x*C + c] = dfm[m][c] / W: one correctly rounded f32 division, equal to numpy's bit for bit."""
    from orcai_amd import _native as N

    dfm = np.random.default_rng(M + C).standard_normal((M, C)).astype(np.float32)
    dd, out = _dev(dfm), torch.full((M, W * C), 777.0, dtype=torch.float32, device="cuda")
    N.check(N.lib().orcai_freq_mean_bwd(N.ptr(dd), M, W, C, N.ptr(out), N.stream_ptr()), "orcai_freq_mean_bwd")
    want = np.broadcast_to((dfm / np.float32(W))[:, None, :], (M, W, C)).reshape(M, W * C)
    assert want.dtype == np.float32 and np.array_equal(out.cpu().numpy(), want)


def test_freq_mean_argument_checks():
    from orcai_amd import _native as N

    lib, st = N.lib(), N.stream_ptr()
    a, out = torch.ones(4, 6, device="cuda"), torch.full((4, 6), 777.0, device="cuda")
    for fn in (lib.orcai_freq_mean, lib.orcai_freq_mean_bwd):
        assert fn(None, 4, 2, 3, N.ptr(out), st) == N.E_BADARG and fn(N.ptr(a), 4, 2, 3, None, st) == N.E_BADARG
        assert fn(N.ptr(a), 0, 2, 3, N.ptr(out), st) == N.E_BADARG and fn(N.ptr(a), 4, 0, 3, N.ptr(out), st) == N.E_BADARG and fn(N.ptr(a), 4, 2, 0, N.ptr(out), st) == N.E_BADARG
    assert bool((out == 777.0).all())


# ---------------------------------------------------------------- Conv1D over time, "same" padding, sigmoid
# (B, T, C, K, L): T in {1, 2, 46} with T < K; K in {1, 3, 5} and the even K = 4, which pins the (K-1)/2 left and K/2 right padding the kernel
# states; L in {1, 7, 64}; C in {5, 36}.  K C L = 11520 weights and B T C = 8280 inputs span many 256-thread blocks of the backward kernels, T L = 2944
# outputs span six passes of the forward's 512 threads; B = 64 gives the weight gradient its 2944 terms of the batch-64 training step.
CONV_SHAPES = [
    (1, 1, 5, 1, 1),
    (2, 1, 5, 3, 7),
    (3, 2, 36, 5, 7),
    (2, 2, 5, 4, 64),
    (3, 46, 36, 3, 7),
    (2, 46, 36, 4, 7),
    (5, 46, 36, 5, 64),
    (3, 46, 5, 1, 1),
    (64, 46, 36, 5, 7),
]


def _windows(a, K):
    """a [B][T][X] -> [B][T][K][X]: element (b, t, k) = a[b][t + k - left], zero outside, left = (K - 1) // 2 (Keras "same": K // 2 on the right)."""
    left = (K - 1) // 2
    T = a.shape[1]
    ap = np.pad(a, ((0, 0), (left, K // 2), (0, 0)))
    return np.stack([ap[:, k : k + T] for k in range(K)], axis=2)


def _draw(rng, shape, ints, sparse=False):
    if not ints:
        return rng.standard_normal(shape).astype(np.float32)
    v = rng.integers(-1, 2, size=shape) * (rng.random(shape) < 0.3) if sparse else rng.integers(-2, 3, size=shape)
    return v.astype(np.float32)


def test_conv_shapes_cover_the_listed_sizes():
    assert {s[1] for s in CONV_SHAPES} == {1, 2, 46} and {s[3] for s in CONV_SHAPES} == {1, 3, 4, 5}
    assert {s[4] for s in CONV_SHAPES} == {1, 7, 64} and {s[2] for s in CONV_SHAPES} == {5, 36}
    assert any(T < K for _, T, _, K, _ in CONV_SHAPES)
    # the padding of an even kernel is asymmetric: one tap before, two after
    w = _windows(np.arange(1.0, 4.0).reshape(1, 3, 1), 4)[0, :, :, 0]
    assert np.array_equal(w, [[0, 1, 2, 3], [1, 2, 3, 0], [2, 3, 0, 0]])


@pytest.mark.parametrize("B,T,C,K,L", CONV_SHAPES)
def test_conv1d_sigmoid_vs_float64(B, T, C, K, L):
    """Probabilities against float64 at 2e-6.  The weights are scaled to a pre-activation of order 1, so no output saturates and a
    misplaced tap or a dropped boundary term moves the probability by orders of magnitude more than the bar."""
    from orcai_amd import _native as N

    rng = np.random.default_rng(B + T + C + K + L)
    x = rng.standard_normal((B, T, C)).astype(np.float32)
    w = (rng.standard_normal((K, C, L)) / np.sqrt(K * C)).astype(np.float32)
    bias = (0.5 * rng.standard_normal(L)).astype(np.float32)
    out = torch.full((B, T, L), 777.0, dtype=torch.float32, device="cuda")
    xd, wd, bd = _dev(x), _dev(w), _dev(bias)
    N.check(N.lib().orcai_conv1d_sigmoid(N.ptr(xd), N.ptr(wd), N.ptr(bd), B, T, C, K, L, N.ptr(out), N.stream_ptr()), "orcai_conv1d_sigmoid")
    z = np.einsum("btkc,kcl->btl", _windows(x.astype(np.float64), K), w.astype(np.float64)) + bias
    assert float(np.abs(z).max()) < 12.0  # far from saturation
    err = float(np.abs(out.cpu().numpy() - 1.0 / (1.0 + np.exp(-z))).max())
    assert err <= 2e-6, err


def test_conv1d_sigmoid_argument_checks():
    from orcai_amd import _native as N

    lib, st = N.lib(), N.stream_ptr()
    x, w, b = torch.ones(2, 3, 4, device="cuda"), torch.ones(3, 4, 5, device="cuda"), torch.ones(5, device="cuda")
    out = torch.full((2, 3, 5), 777.0, device="cuda")
    ok = [N.ptr(x), N.ptr(w), N.ptr(b), 2, 3, 4, 3, 5, N.ptr(out)]
    for i in (0, 1, 2, 8):
        assert lib.orcai_conv1d_sigmoid(*[None if j == i else v for j, v in enumerate(ok)], st) == N.E_BADARG
    for i in (3, 4, 5, 6, 7):
        assert lib.orcai_conv1d_sigmoid(*[0 if j == i else v for j, v in enumerate(ok)], st) == N.E_BADARG
    # the snippet is staged in LDS: T C floats beyond 64 KiB are refused (410 * 40 * 4 = 65600), before anything is read
    assert lib.orcai_conv1d_sigmoid(N.ptr(x), N.ptr(w), N.ptr(b), 2, 410, 40, 3, 5, N.ptr(out), st) == N.E_UNSUPPORTED
    assert bool((out == 777.0).all())


@pytest.mark.parametrize("ints", [False, True], ids=["float", "int"])
@pytest.mark.parametrize("B,T,C,K,L", CONV_SHAPES)
def test_conv1d_bwd_vs_float64(B, T, C, K, L, ints):
    """dW[k][c][l] += sum_{b,t} x[b][t+k-left][c] dz[b][t][l] onto a non-zero integer-valued dW (added to, not overwritten), and
    dx[b][t][c] = sum_{k,l} w[k][c][l] dz[b][t-k+left][l].
    float: dx is K L fused multiply-adds: gamma_{KL} sum|w||dz|; dW is at most B T fused multiply-adds, the add of the two partial sums and
    the add onto dW: gamma_{BT+2} (sum|x||dz| + |dW0|).
    int: small integers (dz sparse), every sum exact below 2^24: bit for bit."""
    from orcai_amd import _native as N

    rng = np.random.default_rng(B + T + C + K + L)
    x, w, dz = _draw(rng, (B, T, C), ints), _draw(rng, (K, C, L), ints), _draw(rng, (B, T, L), ints, sparse=True)
    dW0 = rng.integers(-8, 9, size=(K, C, L)).astype(np.float32)
    dW0[dW0 == 0] = 3.0
    xd, wd, zd, dW = _dev(x), _dev(w), _dev(dz), _dev(dW0)
    dx = torch.full((B, T, C), 777.0, dtype=torch.float32, device="cuda")
    N.check(N.lib().orcai_conv1d_bwd(N.ptr(xd), N.ptr(wd), N.ptr(zd), B, T, C, K, L, N.ptr(dW), N.ptr(dx), N.stream_ptr()), "orcai_conv1d_bwd")
    x64, w64, z64 = x.astype(np.float64), w.astype(np.float64), dz.astype(np.float64)
    ref_dW = dW0 + np.einsum("btkc,btl->kcl", _windows(x64, K), z64)
    mag_dW = np.abs(dW0) + np.einsum("btkc,btl->kcl", _windows(np.abs(x64), K), np.abs(z64))
    # dx[b][t][c] = sum_k w[k][c] . dz[b][t - k + left]: the windows of dz with the taps reversed (and the padding sides swapped with them)
    zwin = _windows(z64[:, ::-1], K)[:, ::-1]
    ref_dx = np.einsum("btkl,kcl->btc", zwin, w64)
    mag_dx = np.einsum("btkl,kcl->btc", np.abs(zwin), np.abs(w64))
    got_dW, got_dx = dW.cpu().numpy().astype(np.float64), dx.cpu().numpy().astype(np.float64)
    if ints:
        assert max(float(mag_dW.max()), float(mag_dx.max())) < 2.0**24
        assert np.array_equal(got_dW, ref_dW), float(np.abs(got_dW - ref_dW).max())
        assert np.array_equal(got_dx, ref_dx), float(np.abs(got_dx - ref_dx).max())
    else:
        e = np.abs(got_dW - ref_dW) - gamma(B * T + 2) * mag_dW
        assert float(e.max()) <= 0.0, ("dW", float(np.abs(got_dW - ref_dW).max()))
        e = np.abs(got_dx - ref_dx) - gamma(K * L) * mag_dx
        assert float(e.max()) <= 0.0, ("dx", float(np.abs(got_dx - ref_dx).max()))


def test_conv1d_bwd_reference_is_the_adjoint_of_the_forward_reference():
    """The two float64 references of this file agree with each other: <dz, conv(x, w)> = <dx(dz, w), x> = <dW(x, dz), w>, at an even and an odd K."""
    rng = np.random.default_rng(0)
    for K in (4, 5):
        x, w, dz = rng.standard_normal((2, 6, 3)), rng.standard_normal((K, 3, 2)), rng.standard_normal((2, 6, 2))
        z = np.einsum("btkc,kcl->btl", _windows(x, K), w)
        dW = np.einsum("btkc,btl->kcl", _windows(x, K), dz)
        dx = np.einsum("btkl,kcl->btc", _windows(dz[:, ::-1], K)[:, ::-1], w)
        s = float((z * dz).sum())
        assert abs(float((dW * w).sum()) - s) <= 1e-12 * abs(s) + 1e-12 and abs(float((dx * x).sum()) - s) <= 1e-12 * abs(s) + 1e-12


def test_conv1d_bwd_argument_checks():
    from orcai_amd import _native as N

    lib, st = N.lib(), N.stream_ptr()
    x, w, dz = torch.ones(2, 3, 4, device="cuda"), torch.ones(3, 4, 5, device="cuda"), torch.ones(2, 3, 5, device="cuda")
    dW, dx = torch.full((3, 4, 5), 777.0, device="cuda"), torch.full((2, 3, 4), 777.0, device="cuda")
    ok = [N.ptr(x), N.ptr(w), N.ptr(dz), 2, 3, 4, 3, 5, N.ptr(dW), N.ptr(dx)]
    for i in (0, 1, 2, 8, 9):
        assert lib.orcai_conv1d_bwd(*[None if j == i else v for j, v in enumerate(ok)], st) == N.E_BADARG
    for i in (3, 4, 5, 6, 7):
        assert lib.orcai_conv1d_bwd(*[0 if j == i else v for j, v in enumerate(ok)], st) == N.E_BADARG
    assert bool((dW == 777.0).all()) and bool((dx == 777.0).all())
