"""Shared helpers of tests/test_step_scalars_ref.py and tests/test_step_scalars_gpu.py: plain numpy references of the small kernels that close a
training step (the dropout draw, the inputs of mask-and-scale, the masked loss and its gradient, Adam, the moving-average update, the L2 penalty) and the error bounds the GPU
tests hold those kernels to.  Nothing here touches a GPU.

Every bound is a worst-case rounding bound in the style of Higham's gamma_k = k u / (1 - k u), u = 2^-24: k counts the float32 roundings between
the inputs and one output, read off the kernel's source (the count is stated next to each bound); contraction into a fused multiply-add only
removes roundings.  The one constant that cannot be counted is the error of the device's logf (LOGF_ULPS, see there)."""

from __future__ import annotations

import functools
import math

import numpy as np

U32 = 2.0**-24  # unit roundoff of float32
U64 = 2.0**-53  # unit roundoff of float64

GOLDEN = 0x9E3779B97F4A7C15  # splitmix64's increment
MIX1, MIX2 = 0xBF58476D1CE4E5B9, 0x94D049BB133111EB
COUNTER_MUL = 0xD1B54A32D192ED03  # seed = seed_add + counter * COUNTER_MUL (orcai_dropout_mask_dev)
M64 = (1 << 64) - 1

# The float32 clip of MaskedBinaryCrossentropy: Keras clips the probabilities in the tensor's dtype, float32, so the bounds are the float32 values
# of 1e-7 and of 1 - 1e-7 (0.99999988... = 1 - 2^-23), not the float64 ones.
BOUND_LO = np.float32(1e-7)
BOUND_HI = np.float32(1) - np.float32(1e-7)

# Error of the device's logf in ulps, as the loss bound uses it.  The project cannot derive it and the device math library's documentation is not
# part of the tree, so it is 2 x the largest error torch.log (float32, on the GPU; not this project's code) shows against float64 on the clipped
# probabilities of the loss tests, and at least 2.  Measured on an MI355X over log q and log(1 - q) of the 196685 probabilities of bce_pool and the
# four values at and next to the clip bounds: 1.8691 ulp at most (at q = 0.032287043; 0.47 ulp on average), an ulp being the float32 spacing at
# the float64 logarithm.  Hence c = 2 x 1.8691.
LOGF_ULPS_MEASURED = 1.8691
LOGF_ULPS = max(2.0, 2.0 * LOGF_ULPS_MEASURED)  # 3.7382


def gamma(k: float, u: float = U32) -> float:
    return k * u / (1.0 - k * u)


# ------------------------------------------------------------------------------------------------------------------------- dropout draw
def dev_seed(seed_add: int, counter: int) -> int:
    return (seed_add + counter * COUNTER_MUL) & M64


def splitmix_keep(seed: int, n: int, keep: float, i0: int = 0) -> np.ndarray:
    """bool [n]: element i0 + j is kept iff u < float32(keep), u = float32(z >> 40) * 2^-24, z = splitmix64's output function applied to
    seed + GOLDEN * (i0 + j + 1) (all modulo 2^64; i0 + j may be 2^32 or more)."""
    with np.errstate(over="ignore"):
        i = np.uint64(i0 & M64) + np.arange(n, dtype=np.uint64) + np.uint64(1)
        z = np.uint64(seed & M64) + np.uint64(GOLDEN) * i
        z = (z ^ (z >> np.uint64(30))) * np.uint64(MIX1)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(MIX2)
        z = z ^ (z >> np.uint64(31))
    u = (z >> np.uint64(40)).astype(np.float32) * np.float32(2.0**-24)  # 24 bits: the conversion and the product are exact
    return u < np.float32(keep)


# ------------------------------------------------------------------------------------------------------------------------- mask_scale
N_LIST = (1, 7, 8, 9, 255, 256, 257, 2048 * 8 + 3)  # around the block of 256, the f16 lane of 8 (a tail of 1...7 elements), several blocks
MS_SCALES = (1.0 / 0.7, 1.0 / 0.6)
MS_WITNESS = np.float16(1.2041015625)  # times float32(1 / 0.6): 2.0078125 rounded to f32 and then to f16, 2.005859375 rounded once


def once_and_twice(x16, scale):
    """f16(x scale) with one rounding and with two (through float32); the product of an f16 and a float32 is exact in float64."""
    exact = x16.astype(np.float64) * np.float64(np.float32(scale))
    with np.errstate(over="ignore"):
        return exact.astype(np.float16), exact.astype(np.float32).astype(np.float16)


@functools.lru_cache(maxsize=None)
def mask_scale_inputs(n, witness_last):
    """x: standard normal; its last min(n, 8) elements (the f16 tail lane where there is one) are special: -0, +0, the largest f16 and its negative,
    a negative x under a zero mask (the product -0) and MS_WITNESS, whose scaled product rounds differently once and twice at scale 1 / 0.6.
    witness_last chooses which of the last two is the very last element, the only one at n = 1."""
    rng = np.random.default_rng(n)
    x = rng.standard_normal(n).astype(np.float16)
    m = (rng.random(n) < 0.7).astype(np.float16)
    special = [(-3.0, 1.0), (2.0, 0.0), (-65504.0, 1.0), (0.0, 1.0), (-0.0, 1.0), (65504.0, 1.0), (-1.5, 0.0), (float(MS_WITNESS), 1.0)]
    if not witness_last:
        special[-2:] = special[:-3:-1]
    k = min(n, 8)
    x[n - k :] = np.array([v for v, _ in special[-k:]], dtype=np.float16)
    m[n - k :] = np.array([v for _, v in special[-k:]], dtype=np.float16)
    x.setflags(write=False)
    m.setflags(write=False)
    return x, m


# ------------------------------------------------------------------------------------------------------------------------- masked loss
def _bce_parts(p, y, mask_value):
    p, y = np.asarray(p, dtype=np.float32).ravel(), np.asarray(y, dtype=np.float32).ravel()
    live = y != np.float32(mask_value)
    q = np.clip(p.astype(np.float64), np.float64(BOUND_LO), np.float64(BOUND_HI))
    t = y.astype(np.float64)
    with np.errstate(invalid="ignore"):
        la, lb = t * np.log(q), (1.0 - t) * np.log(1.0 - q)  # the two products of one loss term (t = 0 or 1 leaves one of them)
    return p, y, live, q, t, np.where(live, la, 0.0), np.where(live, lb, 0.0)


def bce_ref(p, y, mask_value=-1.0, loss_weight=None, grad_scale=1.0):
    """MaskedBinaryCrossentropy / MaskedBinaryAccuracy and the loss gradient in float64 from float32 p and y.

    Returns (loss_sum, count, correct, dz):
      loss_sum  loss_weight * sum over y != mask_value of -(t log q + (1 - t) log(1 - q)),  q = clip(p, BOUND_LO, BOUND_HI) widened to float64
      count     the number of elements with y != mask_value;  correct: those of them with (p > 0.5) == y
      dz        d(loss_weight * grad_scale * loss_sum / count) / d(logit), p = sigmoid(logit):
                (-t/q + (1-t)/(1-q)) q (1-q) / count * loss_weight * grad_scale where y != mask_value and BOUND_LO < p < BOUND_HI strictly,
                exactly 0 elsewhere (the clip has a zero derivative at and outside its bounds).

    Why the float32 clip: Keras clips in the tensor's dtype, so a probability of exactly 0 costs -log(float32(1e-7)) = 16.118 and one of exactly 1
    costs -log(1 - BOUND_HI) = -log(2^-23) = 15.942, where oracle.model_ref.masked_bce_ref (float64 bounds 1e-7 and 1 - 1e-7) gives 16.118 for
    both.  The two references differ for saturated probabilities only (p <= 1e-7 or p >= BOUND_HI); everywhere else they are the same function."""
    p, y, live, q, t, la, lb = _bce_parts(p, y, mask_value)
    lw = 1.0 if loss_weight is None else float(np.float32(loss_weight))
    gs = float(np.float32(grad_scale))
    count = int(live.sum())
    loss_sum = lw * math.fsum(-(la + lb))
    correct = int(((p > np.float32(0.5)).astype(np.float32) == y)[live].sum())
    inside = live & (p > BOUND_LO) & (p < BOUND_HI)
    dz = np.zeros(p.shape, dtype=np.float64)
    qi, ti = q[inside], t[inside]
    dz[inside] = (-ti / qi + (1.0 - ti) / (1.0 - qi)) * qi * (1.0 - qi) / max(count, 1) * lw * gs
    return loss_sum, count, correct, dz


def bce_loss_bounds(p, y, mask_value=-1.0, loss_weight=None, c_log=LOGF_ULPS):
    """(stated, rigorous): two bounds on |acc[0] - bce_ref's loss_sum| for bce_reduce_kernel.

    stated    sum of c u |log term| plus n 2^-53 times the sum of |log term|, c = c_log for log q and c_log + 1 for log(1 - q) where 1.0f - q
              is inexact (q < 0.5; at q >= 0.5 the subtraction is exact): the bar of the loss sweep.
    rigorous  the same with the rounding of 1.0f - q followed through the logarithm instead of being charged as one ulp of it:
              c_log u |log fl(1 - q)| + |log fl(1 - q) - log(1 - q)|, fl = rounding to float32.  Where q is small this exceeds the stated term
              (|log(1 - q)| ~ q, while fl(1 - q) is off by up to 2^-25), so `stated` is the tighter bar on a sum over many elements, whose
              subtraction errors do not all point one way, and no worst-case bound on one element: tests of single saturated elements use
              `rigorous`, which is one."""
    p, y, live, q, t, la, lb = _bce_parts(p, y, mask_value)
    lw = 1.0 if loss_weight is None else float(np.float32(loss_weight))
    one_minus_q32 = (np.float32(1) - q.astype(np.float32)).astype(np.float64)  # q is a float32 value: the cast is exact
    inexact = one_minus_q32 != 1.0 - q
    absa, absb = np.abs(la), np.abs(lb)
    total = math.fsum(absa + absb)
    double_part = p.size * U64 * total
    stated = U32 * math.fsum(c_log * absa + (c_log + inexact) * absb) + double_part
    with np.errstate(invalid="ignore", divide="ignore"):
        lb32 = np.where(live, np.abs(1.0 - t) * np.abs(np.log(one_minus_q32)), 0.0)
        shift = np.where(live, np.abs(1.0 - t) * np.abs(np.log(one_minus_q32) - np.log(1.0 - q)), 0.0)
    rigorous = U32 * c_log * math.fsum(absa + lb32) + math.fsum(shift) + double_part
    return lw * stated, lw * rigorous


# The loss sweep holds acc[0] to bce_loss_bounds' `stated` bound on the prefixes BCE_N of bce_pool.  That bar is the one the tests were asked
# to keep; it charges an inexact 1.0f - q as one ulp of its logarithm, which is no worst case (see bce_loss_bounds), so it is a bar that holds for
# this data, where the errors stay inside it (observed, not used as a bound: about a fifth of it on an MI355X), not for any data: after a change of the seed or
# of the distribution below, a sweep that misses it by a little need not mean a wrong kernel -- compare with `rigorous` before looking for one.
BCE_N = (1, 255, 256, 257, 65535, 65536, 65537, 3 * 65536 + 77)  # bce_reduce_kernel: 256 blocks of 256, a second pass from 65536 on


@functools.lru_cache(maxsize=None)
def bce_pool():
    """(p, y) float32 [max(BCE_N)], read-only; a loss test of n elements uses the first n.  p = sigmoid of N(0, 2.5^2) logits (about 1 in 10^9 of
    them would reach a clip bound: none does), y in {0, 1} with about 30 % replaced by the mask value -1 (but for ten
    elements at the boundaries of the sweep, which carry labels).  Element 0 is (0.75, 0): unmasked, and
    1.0f - 0.75f is exact, so the one-element case meets its bound by the error of logf alone."""
    rng = np.random.default_rng(20240)
    n = max(BCE_N)
    p = (1.0 / (1.0 + np.exp(-rng.normal(0.0, 2.5, n)))).astype(np.float32)
    y = rng.integers(0, 2, n).astype(np.float32)
    y[rng.random(n) < 0.3] = -1.0
    p[0], y[0] = 0.75, 0.0
    for i in (254, 255, 256, 257, 65534, 65535, 65536, 65537, n - 2, n - 1):  # unmasked on both sides of a block, of a pass, and at the end
        y[i] = i % 2
    p.setflags(write=False)
    y.setflags(write=False)
    return p, y


BCE_GRAD_K = 10


def bce_grad_bound(p, y, mask_value=-1.0, loss_weight=None, grad_scale=1.0):
    """Per element: gamma_10 (|t| (1 - q) + |1 - t| q) / count * loss_weight * grad_scale, the bound on |dz - bce_ref's dz| for bce_grad_kernel.
    For t in {0, 1} the magnitude is |dz| itself, t (1 - q) + (1 - t) q.  k = 10 float32 roundings at most, counted from the kernel:
    1.0f - q (it enters twice: in the divisor and in the factor, 2), the division of its term (1), the sum of the two terms (1), * q (1),
    * (1.0f - q) (1), the conversion of the count to float (1), / count (1), * loss_weight (1), * grad_scale (1)."""
    p, y, live, q, t, _, _ = _bce_parts(p, y, mask_value)
    lw = 1.0 if loss_weight is None else float(np.float32(loss_weight))
    count = max(int(live.sum()), 1)
    mag = (np.abs(t) * (1.0 - q) + np.abs(1.0 - t) * q) / count * lw * float(np.float32(grad_scale))
    return np.where(live, gamma(BCE_GRAD_K) * mag, 0.0)


# ------------------------------------------------------------------------------------------------------------------------- Adam, EMA, L2
def _f64(x):
    return np.asarray(x, dtype=np.float32).astype(np.float64)


def adam_ref(w, g, m, v, counter, lr, b1=0.9, b2=0.999, eps=1e-7, gscale=1.0):
    """oracle.train_ref.adam_step_ref on the float32 inputs widened to float64: g is multiplied by gscale in float64 first, t = counter + 1."""
    from oracle.train_ref import adam_step_ref

    f = lambda s: float(np.float32(s))  # noqa: E731
    return adam_step_ref(_f64(w), _f64(g) * f(gscale), _f64(m), _f64(v), int(counter) + 1, f(lr), f(b1), f(b2), f(eps))


def adam_bounds(w, g, m, v, counter, lr, b1=0.9, b2=0.999, eps=1e-7, gscale=1.0):
    """(bw, bm, bv): per-element bounds on |kernel - adam_ref| for adam_kernel / adam_dev_kernel, v >= 0.  With gi = g gscale, c1 = 1 - b1,
    c2 = 1 - b2, m' v' the reference's new moments, D = sqrt(v') + eps, A = alpha / D and U = A m' the reference's update:

      bm = gamma_5 (|m| + (|gi| + |m|) c1)        roundings: g * gscale, gi - m, 1.0f - b1, * c1, m + ...
      bv = gamma_7 (v + (gi^2 + v) c2)            roundings: gi twice in the square (2), gi * gi, ... - v, 1.0f - b2, * c2, v + ...
      bw = u (|w| + |U|) + A (bm + |m'| (gamma_8 + rv / 2)),   rv = gamma_8 (v + (gi^2 + v) c2) / v'
           the final subtraction (1); the update U inherits m's absolute error bm, and 6 relative roundings: alpha (its float64 evaluation
           and the rounding to float32: 2), sqrtf (1), + eps (1), alpha * m (1), / D (1); v's relative error rv enters through the square root,
           halved.  gamma_8 where 6 or 7 were counted leaves room for the second-order terms.
    Division and sqrtf are correctly rounded (hipcc's default for float32)."""
    f = lambda s: float(np.float32(s))  # noqa: E731
    w, g, m, v = _f64(w), _f64(g) * f(gscale), _f64(m), _f64(v)
    c1, c2, t = 1.0 - f(b1), 1.0 - f(b2), int(counter) + 1
    _, m1, v1 = adam_ref(w, g, m, v, counter, lr, b1, b2, eps, 1.0)
    alpha = f(lr) * math.sqrt(1.0 - f(b2) ** t) / (1.0 - f(b1) ** t)
    A = alpha / (np.sqrt(v1) + f(eps))
    magv = v + (g * g + v) * c2
    bm = gamma(5) * (np.abs(m) + (np.abs(g) + np.abs(m)) * c1)
    bv = gamma(7) * magv
    rv = gamma(8) * magv / v1
    bw = U32 * (np.abs(w) + A * np.abs(m1)) + A * (bm + np.abs(m1) * (gamma(8) + rv / 2.0))
    return bw, bm, bv


def ema_ref(moving, batch, momentum):
    mom = float(np.float32(momentum))
    return _f64(moving) * mom + _f64(batch) * (1.0 - mom)


def ema_bound(moving, batch, momentum):
    """gamma_3 (|moving| momentum + |batch| (1 - momentum)): at most three roundings reach either term (1.0f - momentum, its product, the sum)."""
    mom = float(np.float32(momentum))
    return gamma(3) * (np.abs(_f64(moving)) * mom + np.abs(_f64(batch)) * (1.0 - mom))


def l2_ref(w, lam):
    """float64(float32(lambda)) * sum w^2; the squares of float32 values are exact in float64 and math.fsum rounds their sum once."""
    return float(np.float64(np.float32(lam))) * math.fsum(_f64(w).ravel() ** 2)
