"""`orcai test` in one pass.

1. orcai_test_counts against device_tables.counts_from_arrays: both int64 arrays exactly equal.  Sizes follow test_tables.hip: 64 rows per wave
   (63 / 64 / 65), 256 rows per workgroup (255 / 256 / 257), more than 1024 tiles (a workgroup then takes two), L on both sides of the LDS
   histogram's limit of 16 labels (1, 7 | 33, 64).
2. End to end on a tiny seeded model and a list of three device batches: _test_model_on_dataset(device_tables=True) against device_tables=False.
"""

import json

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from pandas.testing import assert_frame_equal  # noqa: E402
from test_device_tables import random_case  # noqa: E402

from orcai_amd import _native as N  # noqa: E402
from orcai_amd.auxiliary import Messenger  # noqa: E402
from orcai_amd.device_tables import counts_from_arrays  # noqa: E402

GUARD = 0x5A5A5A5A5A5A5A5A  # in the words around conf and mis: the kernel must leave them alone
QUIET = Messenger(verbosity=0)


class Buffers:
    """[guard][conf L x 4][guard][mis 2 x (L+1) x (L+1) x L][guard] in one int64 device buffer, conf and mis zeroed by orcai_zero_fill."""

    def __init__(self, L):
        self.L, self.nc, self.nm = L, 4 * L, 2 * (L + 1) * (L + 1) * L
        self.buf = torch.full((self.nc + self.nm + 3,), GUARD, dtype=torch.int64, device="cuda")
        self.zero()

    def zero(self):
        for start, n in ((1, self.nc), (self.nc + 2, self.nm)):
            assert N.lib().orcai_zero_fill(self.buf.data_ptr() + 8 * start, 8 * n, N.stream_ptr()) == 0

    @property
    def conf(self):
        return self.buf.data_ptr() + 8

    @property
    def mis(self):
        return self.buf.data_ptr() + 8 * (self.nc + 2)

    def add(self, p, y):
        """p, y: f32 cuda tensors [M][L]."""
        N.check(N.lib().orcai_test_counts(N.ptr(p), N.ptr(y), p.shape[0], self.L, -1.0, self.conf, self.mis, N.stream_ptr()), "orcai_test_counts")

    def read(self):
        h = self.buf.cpu().numpy()
        assert h[0] == GUARD and h[self.nc + 1] == GUARD and h[-1] == GUARD
        L = self.L
        return h[1 : 1 + self.nc].reshape(L, 4).copy(), h[self.nc + 2 : -1].reshape(2, L + 1, L + 1, L).copy()


def device(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def pool(L, rows=1000):
    y, p = random_case(L, rows=rows, steps=1)
    return y.reshape(rows, L), p.reshape(rows, L)


@pytest.mark.parametrize("L", [1, 7, 33, 64])
def test_counts_equal_the_numpy_specification(L):
    y, p = pool(L)
    assert p[0, 0] == 0.5 and np.isnan(p[1, 0]) and (y == -1).any()
    if L > 1:
        assert ((y == 1).sum(axis=1) > 1).any() and ((p >= 0.5).sum(axis=1) == L).any()
    yd, pd_ = device(y), device(p)
    for M in (1, 63, 64, 65, 255, 256, 257, 1000):
        b = Buffers(L)
        b.add(pd_[:M], yd[:M])
        conf, mis = b.read()
        want_conf, want_mis = counts_from_arrays(y[:M], p[:M])
        assert np.array_equal(conf, want_conf), M
        assert np.array_equal(mis, want_mis), (M, np.argwhere(mis != want_mis)[:5])


def test_more_tiles_than_workgroups():
    """1026 tiles are more than the 1024 workgroups a launch of one tile each may have: 513 workgroups of two tiles, the last tile with one row."""
    L, M = 3, 1025 * 256 + 1
    y, p = pool(L)
    reps = -(-M // len(y))
    y, p = np.tile(y, (reps, 1))[:M], np.tile(p, (reps, 1))[:M]
    b = Buffers(L)
    b.add(device(p), device(y))
    conf, mis = b.read()
    want_conf, want_mis = counts_from_arrays(y, p)
    assert np.array_equal(conf, want_conf) and np.array_equal(mis, want_mis)


@pytest.mark.parametrize("L", [7, 64])
def test_hot_bin_holds_every_nolabel_row(L):
    M = 70000
    z = torch.zeros((M, L), dtype=torch.float32, device="cuda")
    b = Buffers(L)
    b.add(z, z)
    conf, mis = b.read()
    assert np.array_equal(conf, np.tile(np.array([M, 0, 0, 0]), (L, 1)))
    want = np.zeros_like(mis)
    want[:, L, L, 0] = M
    assert np.array_equal(mis, want)


@pytest.mark.parametrize("L", [7, 33])
def test_calls_accumulate_and_repeat_bit_for_bit(L):
    y, p = pool(L)
    yd, pd_ = device(y), device(p)
    whole = Buffers(L)
    whole.add(pd_, yd)
    halves = Buffers(L)
    halves.add(pd_[:437], yd[:437])
    halves.add(pd_[437:], yd[437:])
    first = whole.buf.cpu().numpy()
    assert np.array_equal(halves.buf.cpu().numpy(), first)
    whole.zero()
    whole.add(pd_, yd)
    assert whole.buf.cpu().numpy().tobytes() == first.tobytes()
    want_conf, want_mis = counts_from_arrays(y, p)
    conf, mis = whole.read()
    assert np.array_equal(conf, want_conf) and np.array_equal(mis, want_mis)


def test_argument_checks():
    L, M = 7, 100
    lib, st = N.lib(), N.stream_ptr()
    z = torch.zeros((M, L), dtype=torch.float32, device="cuda")
    b = Buffers(L)
    good = dict(p=z.data_ptr(), y=z.data_ptr(), M=M, L=L, mask=-1.0, conf=b.conf, mis=b.mis, stream=st)
    for change in ({"L": 0}, {"L": 65}, {"L": -1}, {"M": 0}, {"M": -5}, {"p": None}, {"y": None}, {"conf": None}, {"mis": None}):
        assert lib.orcai_test_counts(*{**good, **change}.values()) == N.E_BADARG, change
    assert lib.orcai_test_counts(*{**good, "M": 2**60}.values()) == N.E_UNSUPPORTED  # 2^32 workgroups of 2^20 tiles: refused before any launch
    torch.cuda.synchronize()
    conf, mis = b.read()
    assert not conf.any() and not mis.any()  # nothing was launched
    assert lib.orcai_test_counts(*good.values()) == 0
    conf, mis = b.read()
    assert conf[:, 0].tolist() == [M] * L and mis[0, L, L, 0] == M and mis.sum() == 2 * M


# ---------------------------------------------------------------- end to end
def tiny_model(kind):
    from orcai_amd.architectures import ResNet1DConv, ResNetLSTM

    if kind == "ResNet1DConv":
        return ResNet1DConv((32, 12, 1), 3, [10, 20], 3, 0.0, seed=3)
    return ResNetLSTM((32, 12, 1), 3, [10, 20], 3, 0.0, 64, seed=3)


def batches(model, n=3, B=16, seed=5):
    """A plain list of device batches (both passes of the flag-off route then see the same batches): noise spectrograms; labels mostly 0 with single
    labels, some double labels and masked elements."""
    rng = np.random.default_rng(seed)
    H, W = model.input_hw
    out = []
    for _ in range(n):
        x = rng.standard_normal((B, H, W)).astype(np.float32)
        y = (rng.random((B, model.out_steps, model.num_labels)) < 0.25).astype(np.float32)
        y[rng.random(y.shape) < 0.1] = -1
        out.append((device(x), device(y)))
    return out


@pytest.mark.parametrize("kind", ["ResNetLSTM", "ResNet1DConv"])
def test_one_pass_equals_the_two_pass_route(kind, tmp_path, capsys):
    """Tables: exact.  MBA: equal (its sums are integers).  loss: orcai_masked_bce's bce_reduce_kernel adds its per-workgroup f64 sums with atomics, so
    it is NOT order-independent once a batch fills more than one workgroup (here 16 * 8 * 3 = 384 elements: two); the two routes therefore agree to
    1e-9 relative, the float64 reordering bound for these sizes, and not necessarily to the bit."""
    from orcai_amd.test import _save_test_results, _test_model_on_dataset

    model = tiny_model(kind)
    data = batches(model)
    names = ["A", "B", "C"]
    host = _test_model_on_dataset(model, data, names, "test_data", QUIET)
    dev = _test_model_on_dataset(model, data, names, "test_data", QUIET, device_tables=True)
    capsys.readouterr()
    assert set(dev) == set(host) and dev["dataset"] == host["dataset"]
    assert host["confusion_table"]["Total"].sum() > 0 and host["confusion_table"][["TP", "FP"]].to_numpy().sum() > 0  # the model predicts something
    assert_frame_equal(dev["confusion_table"], host["confusion_table"], check_exact=True)
    assert list(dev["misclassification_tables"]) == list(host["misclassification_tables"])
    for key, table in host["misclassification_tables"].items():
        assert_frame_equal(dev["misclassification_tables"][key], table, check_exact=True)
    assert set(dev["data_metrics"]) == set(host["data_metrics"])
    assert dev["data_metrics"]["MBA"] == host["data_metrics"]["MBA"]
    print("loss", repr(dev["data_metrics"]["loss"]), repr(host["data_metrics"]["loss"]))
    assert abs(dev["data_metrics"]["loss"] - host["data_metrics"]["loss"]) <= 1e-9 * abs(host["data_metrics"]["loss"])
    # the files: the three tables byte for byte; the metrics file holds the loss, which may differ in its last bits (above)
    _save_test_results(host, tmp_path / "host", QUIET)
    _save_test_results(dev, tmp_path / "dev", QUIET)
    files = sorted(f.name for f in (tmp_path / "host").iterdir())
    assert len(files) == 4 and files == sorted(f.name for f in (tmp_path / "dev").iterdir())
    for f in files:
        if f.endswith(".csv"):
            assert (tmp_path / "dev" / f).read_bytes() == (tmp_path / "host" / f).read_bytes(), f
        else:
            got, want = (json.loads((tmp_path / d / f).read_text()) for d in ("dev", "host"))
            assert got["MBA"] == want["MBA"] and abs(got["loss"] - want["loss"]) <= 1e-9 * abs(want["loss"]) and set(got) == set(want)


def test_host_batches_are_refused_by_name():
    from orcai_amd.test import _test_model_on_dataset

    model = tiny_model("ResNetLSTM")
    data = [(x.cpu(), y.cpu()) for x, y in batches(model, n=1)]
    with pytest.raises(ValueError, match="--device-tables"):
        _test_model_on_dataset(model, data, ["A", "B", "C"], "test_data", QUIET, device_tables=True)
