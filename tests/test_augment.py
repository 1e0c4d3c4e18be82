"""Training augmentation (orcai_amd/augment.py), the host side: parameter validation, the batch key, and the numpy twins plan_ref /
apply_ref that are the specification of the kernels in csrc/augment.hip.  No GPU."""

import numpy as np
import pytest

from orcai_amd import augment as A

H, W = 32, 5
FULL = {"time_masks": 2, "time_mask_rows": 6, "freq_masks": 2, "freq_mask_bins": 2, "level_shift": 0.1, "mix_probability": 0.25, "mask_value": 0.25,
        "mask_labels": True}


@pytest.mark.parametrize("spec, key", [
    ({"time_mask": 1}, "time_mask"),  # unknown key
    ({"time_masks": 9, "time_mask_rows": 4}, "time_masks"),  # out of range
    ({"time_masks": -1}, "time_masks"),
    ({"time_masks": 1, "time_mask_rows": H + 1}, "time_mask_rows"),
    ({"freq_masks": 9, "freq_mask_bins": 2}, "freq_masks"),
    ({"freq_masks": 1, "freq_mask_bins": W + 1}, "freq_mask_bins"),
    ({"level_shift": 1.5}, "level_shift"),
    ({"level_shift": -0.1}, "level_shift"),
    ({"mix_probability": 1.01}, "mix_probability"),
    ({"mix_probability": float("nan")}, "mix_probability"),
    ({"mask_value": float("inf")}, "mask_value"),
    ({"mask_labels": 1}, "mask_labels"),
    ({"time_masks": 2.0, "time_mask_rows": 4}, "time_masks"),  # a non-integer count
    ({"time_masks": 1.5, "time_mask_rows": 4}, "time_masks"),
    ({"freq_masks": True, "freq_mask_bins": 2}, "freq_masks"),
    ({"time_masks": 1, "time_mask_rows": 2.5}, "time_mask_rows"),
    ({"freq_masks": "2", "freq_mask_bins": 2}, "freq_masks"),
    ({"time_masks": 1}, "time_mask_rows"),  # masks asked for, of height 0
    ({"time_masks": 1, "time_mask_rows": 0}, "time_mask_rows"),
    ({"freq_masks": 3}, "freq_mask_bins"),
])
def test_validation_errors_name_the_key(spec, key):
    with pytest.raises(ValueError, match=key):
        A.validate(spec, H, W)


def test_validate_fills_defaults_and_leaves_the_spec_alone():
    assert A.validate(None, H, W) is None
    assert A.validate({}, H, W) == A.DEFAULTS
    spec = {"time_masks": 8, "time_mask_rows": H, "freq_masks": 8, "freq_mask_bins": W, "level_shift": 1, "mix_probability": 1, "mask_value": -3.5}
    before = dict(spec)
    out = A.validate(spec, H, W)
    assert spec == before and out["mask_labels"] is False and out["level_shift"] == 1.0 and out["time_masks"] == 8
    with pytest.raises(ValueError, match="augment"):
        A.validate([1, 2], H, W)


def test_train_and_hpsearch_reject_a_bad_spec_before_loading_anything(tmp_path):
    """The data directory holds nothing but the shapes file: reaching a dataset or a model would fail with another error."""
    import json

    from orcai_amd.hpsearch import hyperparameter_search
    from orcai_amd.io import read_json
    from orcai_amd.train import DEFAULT_ORCAI_PARAMETER, train

    (tmp_path / "dataset_shapes.json").write_text(json.dumps({"spectrogram": [32, 12, 1], "labels": [8, 3]}))
    p = read_json(DEFAULT_ORCAI_PARAMETER)
    p["model"]["augment"] = {"time_masks": 2, "time_mask_rows": 33}
    with pytest.raises(ValueError, match="time_mask_rows"):
        train(tmp_path, tmp_path / "out", p, verbosity=0)
    with pytest.raises(ValueError, match="time_mask_rows"):
        hyperparameter_search(tmp_path, tmp_path / "out", p, verbosity=0)


def test_augmented_without_a_spec_is_the_dataset_itself():
    ds = [(1, 2)]
    assert A.augmented(ds, None) is ds
    assert A.augmented(ds, None, seed=[12, 3], rank=1) is ds
    wrapped = A.augmented(ds, {}, seed=1)
    assert wrapped is not ds and len(wrapped) == 1 and wrapped.dataset is ds


def test_batch_key_separates_rank_epoch_and_batch():
    seed = [12, 1234]
    k = A.batch_key(seed, 0, 0, 0)
    assert 0 <= k < 2**64 and k == A.batch_key(seed, 0, 0, 0) == A.batch_key(list(seed), 0, 0, 0)
    keys = {A.batch_key(seed, r, e, i) for r in range(4) for e in range(6) for i in range(50)}
    assert len(keys) == 4 * 6 * 50
    assert A.batch_key([12, 1235], 0, 0, 0) != k
    # the Python-integer formula of the module docstring
    z = A.seed_word(seed)
    for v in (3, 5, 7):
        z = (z + 0x9E3779B97F4A7C15 * (v + 1)) % 2**64
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) % 2**64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) % 2**64
        z ^= z >> 31
    assert A.batch_key(seed, 3, 5, 7) == z


def test_draws_are_the_dropout_generator():
    """Draw j of snippet b against the finaliser of dropout_mask_kernel (train_head.hip) restated in Python integers."""
    key = A.batch_key([12, 1], 0, 2, 3)
    z = A._draws(key, 3)
    assert z.shape == (3, A.DRAWS) and z.dtype == np.uint64 and A.DRAWS >= 35
    for b, j in ((0, 0), (1, 7), (2, A.DRAWS - 1)):
        w = (key + 0x9E3779B97F4A7C15 * (b * A.DRAWS + j + 1)) % 2**64
        w = ((w ^ (w >> 30)) * 0xBF58476D1CE4E5B9) % 2**64
        w = ((w ^ (w >> 27)) * 0x94D049BB133111EB) % 2**64
        w ^= w >> 31
        assert int(z[b, j]) == w
        assert int(A._int_below(z[b : b + 1, j], 171)[0]) == ((w >> 32) * 171) >> 32
        assert float(A._uniform(z[b : b + 1, j])[0]) == (w >> 40) / 2.0**24


SEED = [12, 1234]  # [SEED_ID_AUGMENT, orcai_parameter["seed"]] of the train-workflow tests


def test_plan_ref_properties_over_4096_snippets():
    Hp, Wp, B = 736, 171, 64
    spec = {"time_masks": 3, "time_mask_rows": 40, "freq_masks": 2, "freq_mask_bins": 12, "level_shift": 0.1, "mix_probability": 0.25}
    plans = np.stack([A.plan_ref(A.batch_key(SEED, 0, e, i), B, Hp, Wp, spec) for e in range(4) for i in range(16)])
    assert plans.shape == (64, B, A.PLAN_WORDS) and plans.dtype == np.int32
    assert (plans[..., A.PLAN_N_TIME] == 3).all() and (plans[..., A.PLAN_N_FREQ] == 2).all()
    for word0, count, largest, extent in ((A.PLAN_TIME0, 3, 40, Hp), (A.PLAN_FREQ0, 2, 12, Wp)):
        pairs = plans[..., word0 : word0 + 2 * A.MAX_MASKS].reshape(64, B, A.MAX_MASKS, 2)
        start, height = pairs[..., 0], pairs[..., 1]
        assert (height >= 0).all() and (height[..., :count] <= largest).all() and (start >= 0).all() and (start + height <= extent).all()
        assert height[..., :count].max() == largest and height[..., :count].min() == 0  # both ends of the range are drawn
        assert (start[..., :count] + height[..., :count]).max() == extent and start[..., :count].min() == 0
        assert not pairs[:, :, count:].any()  # the pairs past the count are zero
    partner = plans[..., A.PLAN_PARTNER]
    b = np.arange(B)[None, :]
    mixed = partner >= 0
    assert ((partner == -1) | ((partner >= 0) & (partner < B) & (partner != b))).all()
    # 4096 Bernoulli(0.25) draws: sd = sqrt(4096 * 0.25 * 0.75) = 27.7 snippets; the bound is 5 sd around 1024
    n, p = mixed.size, 0.25
    assert n == 4096 and abs(int(mixed.sum()) - n * p) <= 5 * np.sqrt(n * p * (1 - p)), int(mixed.sum())
    assert len(np.unique(partner[mixed])) == B  # every snippet is somebody's partner over 1024 mixes
    shift = plans[..., A.PLAN_SHIFT].copy().view(np.float32)
    assert (np.abs(shift) <= np.float32(0.1)).all() and shift.min() < -0.09 and shift.max() > 0.09
    # same key, same plan; another rank, epoch or batch, another plan
    k = A.batch_key(SEED, 0, 1, 2)
    assert np.array_equal(A.plan_ref(k, B, Hp, Wp, spec), A.plan_ref(k, B, Hp, Wp, spec))
    for other in (A.batch_key(SEED, 1, 1, 2), A.batch_key(SEED, 0, 2, 2), A.batch_key(SEED, 0, 1, 3)):
        assert other != k and not np.array_equal(A.plan_ref(other, B, Hp, Wp, spec), A.plan_ref(k, B, Hp, Wp, spec))
    # a draw has a fixed slot: switching the masks off moves neither partner nor shift
    plain = A.plan_ref(k, B, Hp, Wp, {"level_shift": 0.1, "mix_probability": 0.25})
    assert np.array_equal(plain[:, :2], A.plan_ref(k, B, Hp, Wp, spec)[:, :2]) and not plain[:, 2:].any()
    # one snippet is never mixed
    assert A.plan_ref(k, 1, Hp, Wp, {"mix_probability": 1.0})[0, A.PLAN_PARTNER] == -1
    assert (A.plan_ref(k, 2, Hp, Wp, {"mix_probability": 1.0})[:, A.PLAN_PARTNER] == [1, 0]).all()


def _plan(B, partner=None, shift=None, time=(), freq=()):
    """A hand-made plan: the same (start, height) pairs for every snippet."""
    plan = np.zeros((B, A.PLAN_WORDS), dtype=np.int32)
    plan[:, A.PLAN_PARTNER] = -1 if partner is None else partner
    if shift is not None:
        plan[:, A.PLAN_SHIFT] = np.asarray(shift, dtype=np.float32).view(np.int32)
    plan[:, A.PLAN_N_TIME], plan[:, A.PLAN_N_FREQ] = len(time), len(freq)
    for k, (s, h) in enumerate(time):
        plan[:, A.PLAN_TIME0 + 2 * k : A.PLAN_TIME0 + 2 * k + 2] = (s, h)
    for k, (s, h) in enumerate(freq):
        plan[:, A.PLAN_FREQ0 + 2 * k : A.PLAN_FREQ0 + 2 * k + 2] = (s, h)
    return plan


def _xy(S=9, L=1, seed=0):
    rng = np.random.default_rng(seed)
    return rng.random((2, H, W), dtype=np.float32), rng.integers(-1, 2, (2, S, L)).astype(np.float32)


def test_apply_ref_label_truth_table():
    """All nine (own, partner) pairs of {0, 1, -1}: the first nine of the 8 x 2 label cells of snippet 0, mixed with snippet 1."""
    own = np.array([0, 0, 0, 1, 1, 1, -1, -1, -1], dtype=np.float32)
    other = np.array([0, 1, -1, 0, 1, -1, 0, 1, -1], dtype=np.float32)
    want = np.array([0, 1, -1, 1, 1, 1, -1, 1, -1], dtype=np.float32)
    x = np.random.default_rng(1).random((2, H, W), dtype=np.float32)
    y = np.zeros((2, 8, 2), dtype=np.float32)
    y[0].flat[:9], y[1].flat[:9] = own, other
    x_out, y_out = A.apply_ref(x, y, _plan(2, partner=[1, -1]), {"mix_probability": 1.0})
    assert np.array_equal(y_out[0].ravel()[:9], want) and not y_out[0].ravel()[9:].any()
    assert np.array_equal(y_out[1], y[1])  # snippet 1 is not mixed: unchanged
    assert np.array_equal(x_out[0], np.maximum(x[0], x[1])) and np.array_equal(x_out[1], x[1])


def test_apply_ref_mask_labels_needs_the_union_to_cover_a_step():
    x, y = _xy(S=8, L=3)
    y[:] = 1.0
    # step 2 = rows 8..11: rows 8, 9 from the first mask, 10, 11 from the second; step 5 = rows 20..23: the mask leaves row 23 out
    spec = {"time_masks": 3, "time_mask_rows": 8, "mask_labels": True, "mask_value": 0.25}
    plan = _plan(2, time=((6, 4), (10, 2), (19, 4)))
    x_out, y_out = A.apply_ref(x, y, plan, spec)
    want = np.ones((8, 3), dtype=np.float32)
    want[2] = -1.0
    assert np.array_equal(y_out[0], want) and np.array_equal(y_out[1], want)
    rows = np.zeros(H, dtype=bool)
    rows[6:12] = rows[19:23] = True
    assert (x_out[:, rows] == np.float32(0.25)).all() and np.array_equal(x_out[:, ~rows], x[:, ~rows])
    # neither mask alone covers the step, and without mask_labels the labels stay
    assert np.array_equal(A.apply_ref(x, y, _plan(2, time=((6, 4),)), spec)[1], y)
    assert np.array_equal(A.apply_ref(x, y, plan, {**spec, "mask_labels": False})[1], y)


def test_apply_ref_order_of_the_steps_and_frequency_masks():
    x, y = _xy(S=8, L=2)
    spec = {"freq_masks": 1, "freq_mask_bins": 2, "level_shift": 0.5, "mix_probability": 1.0, "mask_value": -2.0}
    shift = np.float32([0.4, -0.45])
    x_out, y_out = A.apply_ref(x, y, _plan(2, partner=[1, 0], shift=shift, freq=((3, 2),)), spec)
    mixed = np.maximum(x[0], x[1])
    for b in range(2):
        want = np.minimum(np.maximum(mixed + shift[b], np.float32(0)), np.float32(1))
        assert want.dtype == np.float32 and (want == 0).any() == (b == 1) and (want == 1).any() == (b == 0)  # both clamps are reached
        want[:, 3:5] = -2.0  # the mask value is written last: it is neither shifted nor clamped
        assert np.array_equal(x_out[b], want)


def test_apply_ref_with_everything_off_returns_the_input_bytes():
    x, y = _xy(S=8, L=3)
    x[0, 0, 0], x[0, 0, 1], x[1, 3, 2] = -0.0, 1.5, -7.0  # values a clamp or a max against +0 would change
    x0, y0 = x.copy(), y.copy()
    for spec in ({}, None, dict(A.DEFAULTS)):
        plan = A.plan_ref(A.batch_key(SEED, 0, 0, 0), 2, H, W, spec or {})
        x_out, y_out = A.apply_ref(x, y, plan, spec)
        assert x_out.tobytes() == x0.tobytes() and y_out.tobytes() == y0.tobytes()
        assert x_out is not x and x.tobytes() == x0.tobytes() and y.tobytes() == y0.tobytes()
    # level_shift == 0 skips the clamp even when the plan holds a shift
    x_out, _ = A.apply_ref(x, y, _plan(2, shift=[0.3, 0.3]), {})
    assert x_out.tobytes() == x0.tobytes()


def test_plan_ref_and_apply_ref_together():
    x, y = _xy(S=8, L=3, seed=5)
    plan = A.plan_ref(A.batch_key(SEED, 0, 0, 1), 2, H, W, FULL)
    x_out, y_out = A.apply_ref(x, y, plan, FULL)
    assert x_out.dtype == np.float32 and y_out.dtype == np.float32 and set(np.unique(y_out)) <= {-1.0, 0.0, 1.0}
    for b in range(2):
        rows, cols = A.mask_images(plan[b], H, W)
        assert (x_out[b][rows] == np.float32(0.25)).all() and (x_out[b][:, cols] == np.float32(0.25)).all()
        free = x_out[b][~rows][:, ~cols]
        assert (free >= 0).all() and (free <= 1).all()
    with pytest.raises(ValueError):
        A.apply_ref(x, y[:, :5], plan, FULL)  # 32 rows, 5 steps
