"""The references of tests/step_scalars_ref.py without a GPU: the dropout draw against two independent splitmix64 implementations, the masked loss
against the oracle (and where the two differ on purpose), its gradient against a central difference, Adam / EMA / L2 against their formulas, and
every error bound against a plain float32 evaluation of the same formula (a bound that float32 arithmetic itself cannot meet would be a wrong bound)."""

import math

import numpy as np
import pytest

import step_scalars_ref as S

M64 = (1 << 64) - 1


# ------------------------------------------------------------------------------------------------------------------------- dropout draw
def _keep_slow(seed, i, keep):
    """One element in pure Python integers."""
    z = (seed + 0x9E3779B97F4A7C15 * (i + 1)) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    z ^= z >> 31
    return np.float32(z >> 40) * np.float32(2.0**-24) < np.float32(keep)


@pytest.mark.parametrize("seed", [0, 1234, M64, 0xD1B54A32D192ED03])
@pytest.mark.parametrize("i0", [0, (1 << 32) - 500, (1 << 32) + 7, (1 << 40) + 1])
def test_splitmix_keep_equals_python_integers(seed, i0):
    """1000 indices from i0 on: below, across and above 2^32, where a 32-bit index would wrap."""
    for keep in (0.5, 0.7):
        got = S.splitmix_keep(seed, 1000, keep, i0=i0)
        assert got.dtype == np.bool_ and got.tolist() == [bool(_keep_slow(seed, i0 + j, keep)) for j in range(1000)]
    if i0 >= 1 << 32:  # the draw does change with the high half of the index
        assert not np.array_equal(S.splitmix_keep(seed, 1000, 0.5, i0=i0), S.splitmix_keep(seed, 1000, 0.5, i0=i0 & 0xFFFFFFFF))


def test_splitmix_keep_is_the_textbook_generator():
    """Element i for seed 0 is output i + 1 of splitmix64 started at state 0, in its usual stateful form (Steele, Lea, Flood 2014)."""
    state = 0
    outputs = []
    for _ in range(300):
        state = (state + 0x9E3779B97F4A7C15) & M64
        z = state
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
        outputs.append(z ^ (z >> 31))
    assert outputs[0] == 0xE220A8397B1DCDAF  # the published first output for seed 0
    for keep in (0.5, 0.7):
        assert S.splitmix_keep(0, 300, keep).tolist() == [(z >> 40) * 2.0**-24 < float(np.float32(keep)) for z in outputs]


def test_splitmix_keep_edges_and_dev_seed():
    assert S.splitmix_keep(99, 4096, 1.0).all() and not S.splitmix_keep(99, 4096, 0.0).any()
    assert abs(S.splitmix_keep(5, 1 << 16, 0.7).mean() - 0.7) < 0.01
    assert S.dev_seed(7, 0) == 7 and S.dev_seed(7, 1) == 7 + 0xD1B54A32D192ED03
    c = (1 << 33) + 5
    assert S.dev_seed(M64, c) == (M64 + c * 0xD1B54A32D192ED03) % (1 << 64) != S.dev_seed(M64, c & 0xFFFFFFFF)
    # one position further in the stream is another draw: an index off by one cannot pass for the right one
    assert not np.array_equal(S.splitmix_keep(3, 256, 0.5), S.splitmix_keep(3, 256, 0.5, i0=1))


# ------------------------------------------------------------------------------------------------------------------------- mask_scale
def test_mask_scale_witness_separates_one_rounding_from_two():
    """On the CPU: no f16 value at all separates the two at scale = float32(1 / 0.7), the scale of the trainer's default dropout, so there only the
    -0 product can show a tail contracted into one fused, single-rounding operation; at float32(1 / 0.6) S.MS_WITNESS does."""
    every = np.arange(0x0001, 0x7C00, dtype=np.uint16).view(np.float16)  # every positive finite f16 (the roundings are symmetric in sign)
    once, twice = S.once_and_twice(every, S.MS_SCALES[0])
    assert np.array_equal(once.view(np.uint16), twice.view(np.uint16))
    once, twice = S.once_and_twice(np.array([S.MS_WITNESS]), S.MS_SCALES[1])
    assert float(once[0]) == 2.005859375 and float(twice[0]) == 2.0078125
    for n in S.N_LIST:
        for last in (False, True):
            x, m = S.mask_scale_inputs(n, last)
            assert x.size == n and (x[n - 1], m[n - 1]) == ((S.MS_WITNESS, 1.0) if last else (np.float16(-1.5), 0.0))


# ------------------------------------------------------------------------------------------------------------------------- masked loss
def test_clip_bounds_are_the_float32_ones():
    assert float(S.BOUND_HI) == 1.0 - 2.0**-23 != 1.0 - 1e-7  # two float32 steps below 1
    assert float(S.BOUND_LO) != 1e-7 and abs(float(S.BOUND_LO) - 1e-7) < 1e-14


def test_bce_ref_is_the_oracle_away_from_saturation():
    from oracle.model_ref import masked_bce_ref, masked_binary_accuracy_ref

    p, y = S.bce_pool()
    p, y = p[:5000], y[:5000]
    assert float(p.min()) > 1e-7 and p.max() < S.BOUND_HI
    loss, count, correct, dz = S.bce_ref(p, y)
    assert count == int((y != -1).sum()) and 0.6 < count / 5000 < 0.8
    assert abs(loss / count - masked_bce_ref(y, p)) <= 1e-14 * loss / count
    assert correct / count == masked_binary_accuracy_ref(y, p)
    live = y != -1
    assert np.array_equal(dz == 0.0, ~live)
    # for labels in {0, 1} the gradient with respect to the logit simplifies to (q - t) / count
    assert np.abs(dz[live] - (p[live].astype(np.float64) - y[live]) / count).max() <= 1e-15 / count * 1e3
    lw, cw, kw, dzw = S.bce_ref(p, y, loss_weight=0.25, grad_scale=1024.0)
    assert (cw, kw) == (count, correct) and lw == 0.25 * loss and np.array_equal(dzw, dz * 256.0)


def test_bce_ref_saturated_probabilities():
    """0 and 1 cost 16.118 and 15.942 (the float32 clip), where the oracle's float64 clip gives 16.118 for both; the gradient is exactly zero at and
    outside the bounds and non-zero one float32 step inside."""
    from oracle.model_ref import masked_bce_ref

    f = np.float32
    assert S.bce_ref(f([0.0]), f([1.0]))[0] == -math.log(float(S.BOUND_LO)) and abs(S.bce_ref(f([0.0]), f([1.0]))[0] - 16.118) < 1e-3
    assert S.bce_ref(f([1.0]), f([0.0]))[0] == -math.log(2.0**-23) and abs(S.bce_ref(f([1.0]), f([0.0]))[0] - 15.942) < 1e-3
    assert abs(masked_bce_ref(f([0.0]), f([1.0])) - 16.118) < 1e-3  # the oracle: the same for both
    lo_in, hi_in = np.nextafter(S.BOUND_LO, f(1)), np.nextafter(S.BOUND_HI, f(0))
    for t in (0.0, 1.0):
        for p in (0.0, 1.0, S.BOUND_LO, S.BOUND_HI):
            assert S.bce_ref(f([p]), f([t]))[3][0] == 0.0
        for p in (lo_in, hi_in):
            assert S.bce_ref(f([p]), f([t]))[3][0] != 0.0
    assert S.bce_ref(f([0.3, 0.6]), f([-1.0, -1.0]))[:3] == (0.0, 0, 0)


def test_bce_ref_gradient_is_the_derivative_of_its_loss():
    """Central difference of loss_sum / count in the logit, in float64 (the float32 cast of p is bypassed by differencing the formula itself)."""
    rng = np.random.default_rng(3)
    z = rng.normal(0, 2, 40)
    t = rng.integers(0, 2, 40).astype(np.float64)
    t[::7] = -1.0  # an ordinary label under the custom mask value below
    loss = lambda zz: float(np.mean(-(t * np.log(1 / (1 + np.exp(-zz))) + (1 - t) * np.log(1 - 1 / (1 + np.exp(-zz))))))  # noqa: E731
    p64 = 1 / (1 + np.exp(-z))
    # bce_ref rounds p to float32 first: feed it float32 p and difference the loss around the logit of that p
    p32 = p64.astype(np.float32)
    z32 = np.log(p32.astype(np.float64) / (1 - p32.astype(np.float64)))
    dz = S.bce_ref(p32, t.astype(np.float32), mask_value=-2.0, loss_weight=3.0, grad_scale=2.0)[3]
    for i in range(40):
        e = np.zeros(40)
        e[i] = 1e-6
        fd = (loss(z32 + e) - loss(z32 - e)) / 2e-6 * 3.0 * 2.0
        assert abs(dz[i] - fd) <= 1e-8 * max(1.0, abs(fd)), (i, dz[i], fd)


def test_loss_bounds_stated_and_rigorous():
    """The stated bar charges an inexact 1.0f - q as one ulp of its logarithm.  That is not a worst-case bound where q is small (a single element
    shows it), which is why single saturated elements are held to the rigorous bound; the one-element case of the sweep has an exact 1.0f - q."""
    p, y = S.bce_pool()
    for n in S.BCE_N:
        stated, rigorous = S.bce_loss_bounds(p[:n], y[:n])
        assert 0.0 < stated and 0.0 < rigorous
        assert S.bce_loss_bounds(p[:n], y[:n], loss_weight=0.25) == (0.25 * stated, 0.25 * rigorous)
    stated, rigorous = S.bce_loss_bounds(p[:1], y[:1])
    assert stated == rigorous == S.LOGF_ULPS * S.U32 * math.log(4.0) + S.U64 * math.log(4.0)  # element 0: q = 0.75, t = 0
    stated, rigorous = S.bce_loss_bounds(np.float32([1e-3]), np.float32([0.0]))
    assert rigorous > stated
    # a float32 evaluation of the loss with a correctly rounded logarithm (error 0.5 ulp < LOGF_ULPS) lies within both
    for n in (257, 65537):
        q = np.clip(p[:n], S.BOUND_LO, S.BOUND_HI)
        t = y[:n].astype(np.float64)
        log32 = lambda a: np.log(a.astype(np.float64)).astype(np.float32).astype(np.float64)  # noqa: E731
        terms = np.where(y[:n] != -1, -(t * log32(q) + (1 - t) * log32(np.float32(1) - q)), 0.0)
        err = abs(math.fsum(terms) - S.bce_ref(p[:n], y[:n])[0])
        stated, rigorous = S.bce_loss_bounds(p[:n], y[:n])
        assert err <= rigorous and err <= stated


def test_grad_bound_holds_for_a_float32_evaluation():
    p, y = S.bce_pool()
    p, y = p[:70000], y[:70000]
    f = np.float32
    for lw, gs in ((None, 1.0), (0.25, 1024.0), (3.0, 1.0)):
        _, count, _, dz = S.bce_ref(p, y, loss_weight=lw, grad_scale=gs)
        g = (-y / p + (f(1) - y) / (f(1) - p)) * p * (f(1) - p) / f(count)
        if lw is not None:
            g = g * f(lw)
        g = np.where(y != -1, g * f(gs), f(0))
        assert g.dtype == np.float32
        excess = np.abs(g.astype(np.float64) - dz) - S.bce_grad_bound(p, y, loss_weight=lw, grad_scale=gs)
        assert excess.max() <= 0.0
        assert np.abs(g.astype(np.float64) - dz).max() > 0.0  # float32 is visible against the float64 reference: the bound is not vacuous


# ------------------------------------------------------------------------------------------------------------------------- Adam, EMA, L2
def _adam_inputs(n, seed=0):
    rng = np.random.default_rng(seed)
    w = rng.standard_normal(n).astype(np.float32)
    g = (rng.standard_normal(n) * 10.0 ** rng.integers(-6, 1, size=n)).astype(np.float32)
    m = (rng.standard_normal(n) * 10.0 ** rng.integers(-6, 1, size=n)).astype(np.float32)
    v = (rng.standard_normal(n) ** 2 * 10.0 ** rng.integers(-12, 1, size=n)).astype(np.float32) + np.float32(1e-30)
    return w, g, m, v


def test_adam_ref_is_the_oracle_step():
    from oracle.train_ref import adam_step_ref

    w, g, m, v = _adam_inputs(100)
    d = lambda a: a.astype(np.float64)  # noqa: E731
    f = lambda s: float(np.float32(s))  # noqa: E731
    for counter in (0, 1, 999):
        got = S.adam_ref(w, g, m, v, counter, 1e-4, gscale=1.0 / 3.0)
        want = adam_step_ref(d(w), d(g) * f(1.0 / 3.0), d(m), d(v), counter + 1, f(1e-4), f(0.9), f(0.999), f(1e-7))
        assert all(np.array_equal(a, b) for a, b in zip(got, want))
    # at t = 10^6 + 1 both powers underflow: alpha = lr exactly
    w1, m1, v1 = S.adam_ref(w, g, m, v, 10**6, 1e-4)
    assert f(0.999) ** (10**6 + 1) == 0.0 and f(0.9) ** (10**6 + 1) == 0.0
    assert np.array_equal(w1, d(w) - f(1e-4) * m1 / (np.sqrt(v1) + f(1e-7)))
    # the step number matters: t = counter would be another result
    assert not np.array_equal(S.adam_ref(w, g, m, v, 1, 1e-4)[0], S.adam_ref(w, g, m, v, 0, 1e-4)[0])


@pytest.mark.parametrize("gscale", [1.0, 1.0 / 1024.0, 1.0 / 3.0])
@pytest.mark.parametrize("counter", [0, 1, 999, 10**6])
def test_adam_bounds_hold_for_a_float32_evaluation_and_see_a_wrong_step(counter, gscale):
    f = np.float32
    w, g, m, v = _adam_inputs(70001, seed=counter % 7)
    lr, b1, b2, eps = f(1e-3), f(0.9), f(0.999), f(1e-7)
    t = counter + 1
    alpha = f(float(lr) * math.sqrt(1.0 - float(b2) ** t) / (1.0 - float(b1) ** t))
    gi = g * f(gscale)
    mi = m + (gi - m) * (f(1) - b1)
    vi = v + (gi * gi - v) * (f(1) - b2)
    wi = w - alpha * mi / (np.sqrt(vi) + eps)
    assert wi.dtype == mi.dtype == vi.dtype == np.float32
    ref = S.adam_ref(w, g, m, v, counter, lr, gscale=gscale)
    bounds = S.adam_bounds(w, g, m, v, counter, lr, gscale=gscale)
    for got, want, bound in zip((wi, mi, vi), ref, bounds):
        assert (np.abs(got.astype(np.float64) - want) - bound).max() <= 0.0
    if counter in (1, 999):  # t = counter instead of counter + 1 leaves the bound on w (at 10^6 alpha = lr either way; at 0 it divides by zero)
        a0 = f(float(lr) * math.sqrt(1.0 - float(b2) ** counter) / (1.0 - float(b1) ** counter))
        w_wrong = w - a0 * mi / (np.sqrt(vi) + eps)
        assert (np.abs(w_wrong.astype(np.float64) - ref[0]) - bounds[0]).max() > 0.0


def test_ema_and_l2_refs():
    rng = np.random.default_rng(1)
    mv, bt = rng.standard_normal(300).astype(np.float32), rng.standard_normal(300).astype(np.float32)
    mom = np.float32(0.99)
    ref = S.ema_ref(mv, bt, 0.99)
    assert np.array_equal(ref, mv.astype(np.float64) * float(mom) + bt.astype(np.float64) * (1.0 - float(mom)))
    got = mv * mom + bt * (np.float32(1) - mom)
    assert (np.abs(got.astype(np.float64) - ref) - S.ema_bound(mv, bt, 0.99)).max() <= 0.0
    w = rng.integers(-3, 4, 1000).astype(np.float32)
    assert S.l2_ref(w, 0.5) == 0.5 * float((w.astype(np.int64) ** 2).sum())
    assert S.l2_ref(np.float32([3.0]), 1e-3) == float(np.float32(1e-3)) * 9.0 != 1e-3 * 9.0
