"""Training augmentation on the GPU (csrc/augment.hip) against its specification, the numpy twins plan_ref / apply_ref of
orcai_amd/augment.py.  Every comparison is bit for bit: the plan is integer arithmetic and one rounded product, the apply step a max, one add
and two clamps per element."""

import json
from pathlib import Path

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from orcai_amd import augment as A  # noqa: E402

ROOT = Path(__file__).resolve().parent.parent
SEED = [12, 1234]
SMALL = (5, 48, 19, 3, 4)  # B, H, W, S, L: an odd batch (partners wrap), H * W = 912 a multiple of 4, 16 rows per label step
FULL = {"time_masks": 3, "time_mask_rows": 20, "freq_masks": 2, "freq_mask_bins": 6, "level_shift": 0.2, "mix_probability": 0.6, "mask_value": 0.25,
        "mask_labels": True}


def _inputs(B, H, W, S, L, seed=0):
    """x in [0, 1); labels the way tests/test_datapath_gpu.py builds them: 0 / 1, a partially masked column and fully masked groups."""
    rng = np.random.default_rng(seed)
    x = rng.random((B, H, W), dtype=np.float32)
    y = (rng.random((B, S, L)) < 0.4).astype(np.float32)
    y[:, :, 1 % L][rng.random((B, S)) < 0.3] = -1.0
    y[B // 2, :, L - 1] = -1.0  # a -1 column
    y[0, S // 2, :] = -1.0  # a fully masked group
    return x, y


def _key_where(pred, B, H, W, spec, epoch=0):
    """The first batch key of the epoch whose REFERENCE plan has the property a case is about."""
    for i in range(256):
        k = A.batch_key(SEED, 0, epoch, i)
        if pred(A.plan_ref(k, B, H, W, spec)):
            return k
    raise AssertionError("no such plan among 256 keys")


def _device_plan(key, B, H, W, spec):
    from orcai_amd import _native as N

    s = A.validate(spec, H, W)
    plan = torch.full((B, A.PLAN_WORDS), -77, dtype=torch.int32, device="cuda")
    N.check(N.lib().orcai_augment_plan(key, B, H, W, s["time_masks"], s["time_mask_rows"], s["freq_masks"], s["freq_mask_bins"], s["level_shift"],
                                       s["mix_probability"], plan.data_ptr(), N.stream_ptr()), "orcai_augment_plan")
    return plan


def _device_apply(xt, yt, plan, spec):
    """The raw call on device tensors (xt may be a misaligned view); also checks that the inputs are left alone."""
    from orcai_amd import _native as N

    B, H, W = xt.shape
    S, L = yt.shape[1:]
    s = A.validate(spec, H, W)
    x0, y0 = xt.cpu().numpy().copy(), yt.cpu().numpy().copy()
    x_out, y_out = torch.full_like(xt, 9.0).contiguous(), torch.full_like(yt, 9.0).contiguous()
    flags = (A.FLAG_LEVEL_SHIFT if s["level_shift"] > 0 else 0) | (A.FLAG_MASK_LABELS if s["mask_labels"] else 0)
    N.check(N.lib().orcai_augment_apply(xt.data_ptr(), yt.data_ptr(), plan.data_ptr(), x_out.data_ptr(), y_out.data_ptr(), B, H, W, S, L, s["mask_value"], flags,
                                        N.stream_ptr()), "orcai_augment_apply")
    x_out, y_out = x_out.cpu().numpy(), y_out.cpu().numpy()
    assert xt.cpu().numpy().tobytes() == x0.tobytes() and yt.cpu().numpy().tobytes() == y0.tobytes()  # out of place
    return x_out, y_out


def _check(shape, spec, key, seed=0):
    B, H, W, S, L = shape
    x, y = _inputs(*shape, seed=seed)
    plan = _device_plan(key, B, H, W, spec)
    want_plan = A.plan_ref(key, B, H, W, spec)
    assert np.array_equal(plan.cpu().numpy(), want_plan)
    x_out, y_out = _device_apply(torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda(), plan, spec)
    want_x, want_y = A.apply_ref(x, y, want_plan, spec)
    assert x_out.tobytes() == want_x.tobytes(), int((x_out != want_x).sum())
    assert y_out.tobytes() == want_y.tobytes(), int((y_out != want_y).sum())
    return x, y, want_plan, want_x, want_y


@pytest.mark.parametrize("B", [1, 5, 64])
def test_plan_equals_plan_ref_word_for_word(B):
    H, W = 736, 171
    spec = {**FULL, "time_masks": 8, "time_mask_rows": 736, "freq_masks": 8, "freq_mask_bins": 171, "level_shift": 0.37, "mix_probability": 0.5}
    for key in (A.batch_key(SEED, 0, 0, 0), A.batch_key(SEED, 3, 17, 4021), 2**64 - 1):
        for s, h, w in ((spec, H, W), (FULL, 48, 19), ({}, 48, 19)):
            got = _device_plan(key, B, h, w, s).cpu().numpy()
            assert np.array_equal(got, A.plan_ref(key, B, h, w, s)), (B, key)


def test_apply_small_odd_batch_partners_wrap():
    B, H, W, S, L = SMALL
    key = _key_where(lambda p: ((p[:, 0] >= 0) & (p[:, 0] < np.arange(B))).any() and (p[:, 0] > np.arange(B)).any() and (p[:, 0] < 0).any(), B, H, W, FULL)
    x, y, plan, want_x, want_y = _check(SMALL, FULL, key)
    assert (want_x == np.float32(0.25)).any() and (want_y != y).any()  # the case is not a copy


def test_apply_one_snippet_is_never_mixed():
    spec = {**FULL, "mix_probability": 1.0}
    x, y, plan, want_x, want_y = _check((1,) + SMALL[1:], spec, A.batch_key(SEED, 0, 0, 1))
    assert plan[0, A.PLAN_PARTNER] == -1


def test_apply_production_shape():
    shape = (4, 736, 171, 46, 7)
    spec = {"time_masks": 8, "time_mask_rows": 40, "freq_masks": 2, "freq_mask_bins": 24, "level_shift": 0.1, "mix_probability": 0.6, "mask_value": 0.25,
            "mask_labels": True}
    factor = 16

    def covers_a_step(p):
        rows = A.mask_images(p[0], 736, 171)[0]
        return rows.reshape(46, factor).all(axis=1).any() and (p[:, 0] >= 0).any() and (p[:, 0] < 0).any()

    key = _key_where(covers_a_step, 4, 736, 171, spec)
    _check(shape, spec, key, seed=2)


OPTIONS = {
    "time": {"time_masks": 2, "time_mask_rows": 20},
    "freq": {"freq_masks": 2, "freq_mask_bins": 6},
    "shift": {"level_shift": 0.6},
    "mix": {"mix_probability": 0.6},
    "mask_labels": {"time_masks": 8, "time_mask_rows": 30, "mask_labels": True},
    "all": {"time_masks": 8, "time_mask_rows": 30, "freq_masks": 2, "freq_mask_bins": 6, "level_shift": 0.6, "mix_probability": 0.6, "mask_labels": True},
}


@pytest.mark.parametrize("name", list(OPTIONS))
def test_apply_each_option_alone_and_all_together(name):
    B, H, W, S, L = SMALL
    spec = {**OPTIONS[name], "mask_value": 0.25}
    x, y = _inputs(*SMALL)

    def shows_the_option(p):
        out_x, out_y = A.apply_ref(x, y, p, spec)
        if name in ("mask_labels", "all") and not ((out_y == -1) & (y != -1)).all(axis=2).any():
            return False  # a label step has to be covered by the union of the masks
        if name in ("shift", "all") and not ((out_x == 0).any() and (out_x == 1).any()):
            return False  # both clamps are reached
        if name in ("mix", "all") and not (p[:, 0] >= 0).any():
            return False
        return (out_x != x).any()

    _check(SMALL, spec, _key_where(shows_the_option, B, H, W, spec))


@pytest.mark.parametrize("shape", [SMALL, (3, 6, 5, 3, 2)], ids=["view_one_float_in", "size_not_a_multiple_of_4"])
def test_apply_scalar_route(shape):
    """x_in starts one float into a larger buffer (no 16-byte alignment anywhere); in the second shape H * W = 30, so the blocks of snippets 1 and 2 are
    misaligned even in an aligned buffer."""
    B, H, W, S, L = shape
    spec = {"time_masks": 2, "time_mask_rows": 3, "freq_masks": 1, "freq_mask_bins": 2, "level_shift": 0.2, "mix_probability": 0.6, "mask_value": 0.25}
    key = _key_where(lambda p: (p[:, 0] >= 0).any(), B, H, W, spec)
    x, y = _inputs(*shape, seed=3)
    plan = _device_plan(key, B, H, W, spec)
    want = A.apply_ref(x, y, A.plan_ref(key, B, H, W, spec), spec)
    for lead in (1, 0) if shape is not SMALL else (1,):
        buf = torch.zeros(x.size + 8, dtype=torch.float32, device="cuda")
        xt = buf[lead : lead + x.size].view(B, H, W)
        xt.copy_(torch.from_numpy(x))
        assert xt.is_contiguous() and xt.data_ptr() % 16 == 4 * lead
        x_out, y_out = _device_apply(xt, torch.from_numpy(y).cuda(), plan, spec)
        assert x_out.tobytes() == want[0].tobytes() and y_out.tobytes() == want[1].tobytes()
        assert not buf[:lead].any() and not buf[lead + x.size :].any()  # nothing written around the view


def test_labels_with_masked_columns_and_masked_groups():
    """Every (own, partner) pair of {0, 1, -1} occurs among the mixed snippets' labels, -1 columns and fully masked groups included."""
    shape = (8, 32, 12, 8, 5)
    B, H, W, S, L = shape
    spec = {"time_masks": 4, "time_mask_rows": 10, "mix_probability": 0.9, "mask_labels": True}
    x, y = _inputs(*shape, seed=4)

    def all_nine_pairs(p):
        pairs = {(a, b) for s in range(B) if p[s, 0] >= 0 for a, b in zip(y[s].ravel(), y[p[s, 0]].ravel())}
        return len(pairs) == 9

    key = _key_where(all_nine_pairs, B, H, W, spec)
    plan = _device_plan(key, B, H, W, spec)
    _, y_out = _device_apply(torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda(), plan, spec)
    want = A.apply_ref(x, y, A.plan_ref(key, B, H, W, spec), spec)[1]
    assert y_out.tobytes() == want.tobytes() and set(np.unique(y_out)) == {-1.0, 0.0, 1.0}


def test_invariants_defaults_copy_and_same_key_same_bytes():
    B, H, W, S, L = SMALL
    x, y = _inputs(*SMALL, seed=5)
    x[0, 0, :3] = (-0.0, 1.5, -7.0)  # values a clamp or a max against +0 would change
    xt, yt = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    key = A.batch_key(SEED, 0, 0, 0)
    for spec in ({}, dict(A.DEFAULTS)):
        x_out, y_out = _device_apply(xt, yt, _device_plan(key, B, H, W, spec), spec)
        assert x_out.tobytes() == x.tobytes() and y_out.tobytes() == y.tobytes()
    aug = A.Augmenter(FULL, SEED, rank=0)
    a, b = aug(xt, yt, 1, 2), aug(xt, yt, 1, 2)
    assert a[0].data_ptr() != xt.data_ptr() and a[0].cpu().numpy().tobytes() == b[0].cpu().numpy().tobytes() and torch.equal(a[1], b[1])
    assert xt.cpu().numpy().tobytes() == x.tobytes() and yt.cpu().numpy().tobytes() == y.tobytes()
    want = A.apply_ref(x, y, A.plan_ref(A.batch_key(SEED, 0, 1, 2), B, H, W, FULL), FULL)
    assert a[0].cpu().numpy().tobytes() == want[0].tobytes() and a[1].cpu().numpy().tobytes() == want[1].tobytes()
    c = aug(xt, yt, 1, 3)
    assert not torch.equal(c[0], a[0])  # another batch, other draws
    with pytest.raises(ValueError, match="time_mask_rows"):
        A.Augmenter({"time_masks": 1, "time_mask_rows": 49}, SEED)(xt, yt, 0, 0)


def test_error_codes_without_a_launch():
    from orcai_amd import _native as N

    lib, st = N.lib(), N.stream_ptr()
    B, H, W, S, L = SMALL
    x, y = (torch.from_numpy(a).cuda() for a in _inputs(*SMALL))
    plan = _device_plan(1, B, H, W, {})
    x_out, y_out = torch.full_like(x, 9.0), torch.full_like(y, 9.0)
    sentinel = torch.full((B, A.PLAN_WORDS), -77, dtype=torch.int32, device="cuda")
    p = [x.data_ptr(), y.data_ptr(), plan.data_ptr(), x_out.data_ptr(), y_out.data_ptr()]
    for i in range(5):  # a null pointer
        q = list(p)
        q[i] = None
        assert lib.orcai_augment_apply(*q, B, H, W, S, L, 0.0, 0, st) == N.E_BADARG
    assert lib.orcai_augment_apply(*p, B, H, W, 5, L, 0.0, 0, st) == N.E_BADARG  # 48 rows, 5 steps
    assert lib.orcai_augment_apply(*p, B, H, W, S, L, float("nan"), 0, st) == N.E_BADARG
    assert lib.orcai_augment_apply(*p, B, H, W, S, L, 0.0, 4, st) == N.E_BADARG  # an unknown flag
    assert lib.orcai_augment_apply(p[0], p[1], p[2], p[0], p[4], B, H, W, S, L, 0.0, 0, st) == N.E_BADARG  # in place
    assert lib.orcai_augment_apply(*p, B, A.MAX_H + 2, W, 2, L, 0.0, 0, st) == N.E_UNSUPPORTED  # past the LDS images
    assert lib.orcai_augment_apply(*p, B, H, A.MAX_W + 1, S, L, 0.0, 0, st) == N.E_UNSUPPORTED
    args = dict(B=B, H=H, W=W, time_masks=1, time_mask_rows=4, freq_masks=1, freq_mask_bins=4, level_shift=0.0, mix_probability=0.0)

    def plan_code(ptr=sentinel.data_ptr(), **over):
        a = {**args, **over}
        return lib.orcai_augment_plan(7, a["B"], a["H"], a["W"], a["time_masks"], a["time_mask_rows"], a["freq_masks"], a["freq_mask_bins"], a["level_shift"],
                                      a["mix_probability"], ptr, st)

    assert plan_code(ptr=None) == N.E_BADARG
    assert plan_code(time_masks=9) == N.E_UNSUPPORTED and plan_code(freq_masks=9) == N.E_UNSUPPORTED  # nine masks
    assert plan_code(H=A.MAX_H + 1) == N.E_UNSUPPORTED and plan_code(W=A.MAX_W + 1) == N.E_UNSUPPORTED
    assert plan_code(time_mask_rows=H + 1) == N.E_BADARG and plan_code(freq_mask_bins=-1) == N.E_BADARG and plan_code(B=0) == N.E_BADARG
    assert plan_code(level_shift=1.5) == N.E_BADARG and plan_code(mix_probability=float("nan")) == N.E_BADARG
    torch.cuda.synchronize()
    assert (x_out == 9.0).all() and (y_out == 9.0).all() and (sentinel == -77).all()  # nothing ran
    assert plan_code() == 0
    assert (sentinel.cpu().numpy() == A.plan_ref(7, B, H, W, {k: v for k, v in args.items() if k not in ("B", "H", "W")})).all()


def _recordings(tmp_path, n=2, W=20, L=4):
    rng = np.random.default_rng(0)
    dirs = []
    for r in range(n):
        d = tmp_path / f"rec{r}"
        (d / "spectrogram").mkdir(parents=True)
        (d / "labels").mkdir()
        T = 400 + 50 * r
        lab = (rng.random((T, L)) < 0.4).astype(np.float32)
        lab[:, r % L][rng.random(T) < 0.3] = -1.0
        lab[100:164, (r + 1) % L] = -1.0
        np.save(d / "spectrogram" / "spectrogram.npy", rng.random((T, W), dtype=np.float32))
        np.save(d / "labels" / "labels.npy", lab)
        dirs.append(d)
    return dirs


@pytest.mark.parametrize("kind", ["table", "materialised"])
def test_dataset_wrappers_follow_batch_key_over_two_epochs(tmp_path, kind):
    import pandas as pd

    from orcai_amd.datasets import SnippetDataset, SnippetTableDataset, make_synthetic_dataset

    if kind == "table":
        dirs = _recordings(tmp_path)
        rng = np.random.default_rng(1)
        recs = [str(dirs[int(rng.integers(2))]) for _ in range(19)]
        starts = [int(rng.integers(0, 400 - 64)) for _ in recs]
        table = pd.DataFrame({"recording_data_dir": recs, "row_start": starts, "row_stop": [s + 64 for s in starts]})
        make = lambda: SnippetTableDataset(table, 4, batch_size=6, shuffle=False)  # noqa: E731
        spec = {**FULL, "time_mask_rows": 30}
    else:
        make_synthetic_dataset(tmp_path / "ds", 19, seed=4, input_shape=(32, 12), out_steps=8, n_labels=3)
        make = lambda: SnippetDataset(tmp_path / "ds", 6, shuffle=False)  # noqa: E731
        spec = {**FULL, "time_mask_rows": 12}
    plain, ds = make(), make()
    wrapped = A.augmented(ds, spec, seed=SEED, rank=0)
    assert isinstance(wrapped, A.AugmentedDataset) and wrapped.dataset is ds and len(wrapped) == len(plain) == 3
    changed = 0
    for epoch in range(2):
        batches = list(wrapped)
        assert len(batches) == 3
        for i, ((xa, ya), (x, y)) in enumerate(zip(batches, plain)):
            x, y = x.cpu().numpy(), y.cpu().numpy()
            B, H, W = x.shape
            want = A.apply_ref(x, y, A.plan_ref(A.batch_key(SEED, 0, epoch, i), B, H, W, spec), spec)
            assert xa.cpu().numpy().tobytes() == want[0].tobytes() and ya.cpu().numpy().tobytes() == want[1].tobytes(), (epoch, i)
            changed += int((want[0] != x).any())
    assert changed == 6 and wrapped.epoch == 2


def _param(**model_over):
    from orcai_amd.io import read_json

    p = read_json(ROOT / "orcai_amd" / "defaults" / "default_orcai_parameter.json")
    p["calls"] = ["A", "B", "C"]
    p["seed"] = 1234
    p["model"].update({"filters": [10, 20], "lstm_units": 64, "batch_size": 8, "epochs": 2, "learning_rate": 3e-3, "dropout_rate": 0.2})  # the train-workflow test's model
    p["model"].update(model_over)
    return p


def _data(tmp_path, n_train=64, n_val=16):
    from orcai_amd.datasets import make_synthetic_dataset

    d = tmp_path / "data"
    d.mkdir()
    make_synthetic_dataset(d / "train_dataset", n_train, seed=4, input_shape=(32, 12), out_steps=8, n_labels=3)
    make_synthetic_dataset(d / "val_dataset", n_val, seed=5, input_shape=(32, 12), out_steps=8, n_labels=3)
    (d / "dataset_shapes.json").write_text(json.dumps({"spectrogram": [32, 12, 1], "labels": [8, 3]}))
    return d


SMALL_MODEL_AUGMENT = {"time_masks": 2, "time_mask_rows": 6, "freq_masks": 1, "freq_mask_bins": 3, "level_shift": 0.1, "mix_probability": 0.3, "mask_value": 0.0,
                       "mask_labels": True}


def test_train_end_to_end_with_every_option_on(tmp_path, monkeypatch):
    """8 steps per epoch on the replayed graph: the augmentation's launches run between replays, in the consumer's thread."""
    from orcai_amd.train import train
    from orcai_amd.training import Trainer

    calls = {"augment": 0, "graphed": 0}
    aug_call, graphed = A.Augmenter.__call__, Trainer.train_step_graphed

    def count_augment(self, *a, **k):
        calls["augment"] += 1
        return aug_call(self, *a, **k)

    def count_graphed(self, *a, **k):
        calls["graphed"] += 1
        return graphed(self, *a, **k)

    monkeypatch.setattr(A.Augmenter, "__call__", count_augment)
    monkeypatch.setattr(Trainer, "train_step_graphed", count_graphed)
    d = _data(tmp_path)
    out = tmp_path / "out"
    out.mkdir()
    p = _param(augment=dict(SMALL_MODEL_AUGMENT))
    train(d, out, p, verbosity=0)
    mdir = out / "orcai-v1"
    hist = json.loads((mdir / "training_history.json").read_text())
    assert len(hist["loss"]) == 2 and all(np.isfinite(v).all() for v in hist.values()), hist
    assert json.loads((mdir / "orcai_parameter.json").read_text())["model"]["augment"] == SMALL_MODEL_AUGMENT
    assert calls["graphed"] == 16 and calls["augment"] == 16  # every training batch, and only those: the 2 x 2 validation batches are not augmented


def test_hyperparameter_search_wraps_only_the_training_dataset(tmp_path, monkeypatch):
    """The search is stopped where the first trial's fit begins: what reaches it is the wrapper around the training dataset and the bare validation dataset."""
    import orcai_amd.hpsearch as HS
    from orcai_amd.datasets import SnippetDataset

    class Reached(Exception):
        pass

    class Model:
        class _loop:
            trainer = None

        def compile(self, **kw):
            pass

        def fit(self, train_ds, validation_data=None, **kw):
            raise Reached(train_ds, validation_data)

    monkeypatch.setattr(HS, "build_model", lambda *a, **k: Model())
    d = _data(tmp_path, n_train=16, n_val=8)
    hps = {"filters": {"set1": [10, 20]}, "lstm_units": [64], "dropout_rate": [0.0], "kernel_size": [3], "batch_size": [8]}
    with pytest.raises(Reached) as e:
        HS.hyperparameter_search(d, tmp_path / "hps_out", _param(augment=dict(SMALL_MODEL_AUGMENT)), hps, verbosity=0, max_epochs=3)
    train_ds, val_ds = e.value.args
    assert isinstance(train_ds, A.AugmentedDataset) and isinstance(train_ds.dataset, SnippetDataset) and train_ds.augmenter.spec == SMALL_MODEL_AUGMENT
    assert train_ds.augmenter.word == A.seed_word([12, 1234]) and len(train_ds) == 2
    assert type(val_ds) is SnippetDataset
    xa, ya = next(iter(train_ds))
    assert xa.is_cuda and tuple(xa.shape) == (8, 32, 12) and tuple(ya.shape) == (8, 8, 3)
    with pytest.raises(Reached) as e:
        HS.hyperparameter_search(d, tmp_path / "hps_out", _param(), hps, verbosity=0, max_epochs=3)
    assert type(e.value.args[0]) is SnippetDataset  # no augment key: the dataset as it is
