"""Per-label decision thresholds on the GPU.  Everything compared is integers, strings or file bytes: every comparison is exact.

1. orcai_threshold_counts against threshold_sweep.hist_from_arrays.  Sizes follow test_tables.hip: one wave (63 / 65 rows), one workgroup (257 rows),
   more than one label tile (17 labels at T = 200: tiles of 16; 64 labels at T = 1024: tiles of 7), the largest table, 4099 rows = 17 row tiles.
2. orcai_extract_labels_per_label against orcai_extract_labels (equal thresholds: equal bytes) and against the host route (unequal thresholds).
3. End to end: `orcai test` with the sweep on both routes, `orcai predict` with a thresholds file on both routes.
"""

import json

import numpy as np
import pandas as pd
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from test_device_labels import DELTA_T, TPO, same  # noqa: E402

from orcai_amd import _native as N  # noqa: E402
from orcai_amd import device_labels as D  # noqa: E402
from orcai_amd import predict as P  # noqa: E402
from orcai_amd import threshold_sweep as W  # noqa: E402
from orcai_amd.auxiliary import Messenger  # noqa: E402

GUARD = 0x5A5A5A5A5A5A5A5A  # in the words around hist: the kernel must leave them alone
SENTINEL = -77
QUIET = Messenger(verbosity=0)
CALLS = ["BR", "BUZZ", "HERDING", "PHS", "SS", "TAILSLAP", "WHISTLE"]
SHAPES = [(1, 1, 1), (63, 7, 2), (65, 7, 200), (257, 17, 200), (1000, 64, 1024), (4099, 16, 33)]


def device(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def table_for(T):
    """f32 [T], strictly ascending: the Keras table where it has inner entries, else T evenly spaced values inside (0, 1)."""
    return W.keras_thresholds(T) if T >= 100 else np.linspace(0, 1, T + 2)[1:-1].astype(np.float32)


def sweep_case(M, L, T, seed=0):
    """(y, p, t): a quarter of the probabilities exactly on table entries, some one ulp either side of an entry, zeros, ones and NaNs; labels 0 / 1
    with masked elements and labels of 0.5; for L > 1 the last column all masked, for L > 2 column 1 of one class only."""
    rng = np.random.default_rng(1000 * M + 10 * L + seed)
    t = table_for(T)
    p = rng.random((M, L)).astype(np.float32)
    kind = rng.random((M, L))
    entry = t[rng.integers(0, T, (M, L))]
    p = np.where(kind < 0.25, entry, p)
    p = np.where((kind >= 0.25) & (kind < 0.30), np.nextafter(entry, np.float32(-1)), p)
    p = np.where((kind >= 0.30) & (kind < 0.35), np.nextafter(entry, np.float32(2)), p)
    p = np.where((kind >= 0.35) & (kind < 0.38), np.float32(0), p)
    p = np.where((kind >= 0.38) & (kind < 0.41), np.float32(1), p)
    p = np.where((kind >= 0.41) & (kind < 0.44), np.float32(np.nan), p).astype(np.float32)
    y = (rng.random((M, L)) < 0.3).astype(np.float32)
    other = rng.random((M, L))
    y[other < 0.1] = -1
    y[(other >= 0.1) & (other < 0.15)] = 0.5
    if L > 1:
        y[:, L - 1] = -1
    if L > 2:
        y[:, 1] = np.where(y[:, 1] == 1, 0, y[:, 1])
    return y, p, t


class Hist:
    """[guard][hist L x 2 x (T + 1)][guard] in one int64 device buffer, hist zeroed by orcai_zero_fill."""

    def __init__(self, L, t):
        self.L, self.T, self.n = L, len(t), L * 2 * (len(t) + 1)
        self.table = device(t)
        self.buf = torch.full((self.n + 2,), GUARD, dtype=torch.int64, device="cuda")
        self.zero()

    def zero(self):
        assert N.lib().orcai_zero_fill(self.hist, 8 * self.n, N.stream_ptr()) == 0

    @property
    def hist(self):
        return self.buf.data_ptr() + 8

    def add(self, p, y):
        """p, y: f32 cuda tensors [M][L]."""
        N.check(N.lib().orcai_threshold_counts(N.ptr(p), N.ptr(y), p.shape[0], self.L, -1.0, N.ptr(self.table), self.T, self.hist, N.stream_ptr()),
                "orcai_threshold_counts")

    def read(self):
        h = self.buf.cpu().numpy()
        assert h[0] == GUARD and h[-1] == GUARD
        return h[1:-1].reshape(self.L, 2, self.T + 1).copy()


# ------------------------------------------------------------------ 1. orcai_threshold_counts
@pytest.mark.parametrize("M,L,T", SHAPES)
def test_counts_equal_the_numpy_specification(M, L, T):
    y, p, t = sweep_case(M, L, T)
    if M >= 63:
        assert np.isin(p, t).mean() > 0.15 and np.isnan(p).any() and (p == 0).any() and (p == 1).any() and (y == -1).any() and (y == 0.5).any()
        assert (y[:, L - 1] == -1).all() and not (y[:, 1] == 1).any() and (y[:, 1] == 0).any() and (y[:, 0] == 1).any()
        k = (p[:, :, None] > t).sum(axis=2)
        on = np.isin(p, t)
        assert (np.take(t, np.minimum(k[on], T - 1)) == p[on]).all()  # a probability on an entry lies below it: k is the entry's own index
    b = Hist(L, t)
    b.add(device(p), device(y))
    got, want = b.read(), W.hist_from_arrays(y, p, t, -1.0)
    assert got.dtype == want.dtype == np.int64 and np.array_equal(got, want), np.argwhere(got != want)[:5]
    assert want.sum() == ((y == 0) | (y == 1)).sum()
    if L > 1 and M >= 63:
        assert not got[L - 1].any() and not got[1, 1].any() and got[1, 0].sum() > 0


def test_calls_accumulate_and_repeat_bit_for_bit():
    M, L, T = 257, 17, 200
    y, p, t = sweep_case(M, L, T, seed=1)
    yd, pd_ = device(y), device(p)
    whole = Hist(L, t)
    whole.add(pd_, yd)
    halves = Hist(L, t)
    halves.add(pd_[:101], yd[:101])
    halves.add(pd_[101:], yd[101:])
    first = whole.buf.cpu().numpy()
    assert np.array_equal(halves.buf.cpu().numpy(), first)
    whole.zero()
    whole.add(pd_, yd)
    assert whole.buf.cpu().numpy().tobytes() == first.tobytes()
    whole.add(pd_, yd)
    assert np.array_equal(whole.read(), 2 * W.hist_from_arrays(y, p, t, -1.0))


def test_refusals_leave_hist_alone():
    M, L, T = 100, 7, 200
    lib, st = N.lib(), N.stream_ptr()
    z = torch.zeros((M, L), dtype=torch.float32, device="cuda")
    b = Hist(L, table_for(T))
    good = dict(p=z.data_ptr(), y=z.data_ptr(), M=M, L=L, mask=-1.0, thresholds=N.ptr(b.table), T=T, hist=b.hist, stream=st)
    for change in ({"p": None}, {"y": None}, {"thresholds": None}, {"hist": None}, {"M": 0}, {"M": -5}, {"L": 0}, {"L": 65}, {"L": -1}, {"T": 0}, {"T": 1025},
                   {"T": -1}):
        assert lib.orcai_threshold_counts(*{**good, **change}.values()) == N.E_BADARG, change
    assert lib.orcai_threshold_counts(*{**good, "M": 2**60}.values()) == N.E_UNSUPPORTED  # 2^32 row workgroups: refused before any launch
    torch.cuda.synchronize()
    assert not b.read().any()
    assert lib.orcai_threshold_counts(*good.values()) == 0
    hist = b.read()
    assert hist[:, 0, 1].tolist() == [M] * L and hist.sum() == M * L  # p = 0 lies above the table's first entry, -1e-7, alone


def test_the_device_accumulator_is_the_kernel():
    M, L, T = 300, 7, 50
    y, p, t = sweep_case(M, L, T, seed=2)
    counts = W.ThresholdCounts(L, t, torch.device("cuda", torch.cuda.current_device()))
    counts.add(device(p[:128].reshape(2, 64, L)), device(y[:128].reshape(2, 64, L)))
    counts.add(device(p[128:]), device(y[128:]))
    assert np.array_equal(counts.result(), W.hist_from_arrays(y, p, t, -1.0))
    with pytest.raises(ValueError, match="ascend"):
        W.ThresholdCounts(L, t[::-1], "cuda")


# ------------------------------------------------------------------ 2. orcai_extract_labels_per_label
def extract(agg, cnt, table, rank, limits=None, thresholds=None):
    """One call of the scalar entry point with 0.5 (thresholds None) or of the per-label one: (runs as the device holds them, offsets)."""
    S, L = agg.shape
    R = len(table)
    cap = L * ((S + 1) // 2) + R
    a, c = device(agg), device(cnt)
    t = torch.tensor(table, dtype=torch.int64, device="cuda")
    rk = device(np.asarray(rank, dtype=np.int32))
    lim = None if limits is None else device(np.asarray(limits, dtype=np.float64))
    runs = torch.full((cap + 2, 4), SENTINEL, dtype=torch.int32, device="cuda")
    offsets = torch.full((R + 1,), SENTINEL, dtype=torch.int64, device="cuda")
    lib = N.lib()
    nbytes = lib.orcai_extract_labels_workspace_bytes(L, R, S)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    tail = (N.ptr(rk), None if lim is None else N.ptr(lim), DELTA_T, TPO, N.ptr(runs), cap, N.ptr(offsets), N.ptr(ws), nbytes, N.stream_ptr())
    if thresholds is None:
        N.check(lib.orcai_extract_labels(N.ptr(a), N.ptr(c), L, N.ptr(t), R, S, 0.5, *tail), "orcai_extract_labels")
    else:
        th = device(np.asarray(thresholds, dtype=np.float64))
        N.check(lib.orcai_extract_labels_per_label(N.ptr(a), N.ptr(c), L, N.ptr(t), R, S, N.ptr(th), *tail), "orcai_extract_labels_per_label")
    torch.cuda.synchronize()
    return runs.cpu().numpy(), offsets.cpu().numpy()


def ragged_case(seed=4):
    """Two recordings of 150 and 211 rows, L = 7: blocks of three equal rows with some NaNs.  Recording 0 has the maximum count 2, recording 1 the
    maximum 1, so the two divide their thresholds differently."""
    rng = np.random.default_rng(seed)
    sizes = [150, 211]
    table = [(0, 0, sizes[0], 0), (0, 0, sizes[1], sizes[0])]
    S = sum(sizes)
    agg = np.repeat(rng.random((S // 3 + 1, 7)), 3, axis=0)[:S]
    agg[rng.random(agg.shape) < 0.02] = np.nan
    cnt = np.full(S, 2.0)
    cnt[:4] = 1.0
    cnt[sizes[0] :] = 1.0
    cnt[S - 2 :] = 0.0  # zero-count steps behind the last snippet
    return agg, cnt, table


@pytest.mark.parametrize("with_limits", [False, True])
def test_equal_thresholds_write_the_scalar_calls_bytes(with_limits):
    agg, cnt, table = ragged_case()
    agg[40:43, 2] = 0.25  # exactly at 0.5 / 2 and at 0.5 / 1
    agg[200:203, 5] = 0.5
    rank = D.label_rank(CALLS, "*")
    limits = D.resolve_limits(CALLS, "*", {"default": [0.1, 0.3], "BR": [None, 0.2]}) if with_limits else None
    scalar = extract(agg, cnt, table, rank, limits)
    per_label = extract(agg, cnt, table, rank, limits, thresholds=[0.5] * 7)
    assert scalar[1][-1] > 50 and scalar[1][1] > 0
    assert per_label[0].tobytes() == scalar[0].tobytes() and per_label[1].tobytes() == scalar[1].tobytes()
    if with_limits:
        assert {0, 1, 2} <= set(int(v) for v in scalar[0][: scalar[1][-1], 3])


def test_unequal_thresholds_equal_the_host_route():
    agg, cnt, table = ragged_case(seed=6)
    thresholds = [0.1, 0.9, 0.5, 0.3, 2.5, 0.0, 0.65]
    for (_, _, S, row), m in zip(table, (2.0, 1.0)):  # probabilities exactly at thresholds[l] / max(cnt) of their recording, and one ulp above
        for l in (1, 3, 6):
            agg[row + 30 : row + 48, l] = 0.0
            agg[row + 33 : row + 36, l] = thresholds[l] / m
            agg[row + 39 : row + 42, l] = np.nextafter(thresholds[l] / m, 2.0)
    rank = D.label_rank(CALLS, "*")
    runs, offsets = extract(agg, cnt, table, rank, thresholds=thresholds)
    assert (runs[offsets[-1] :] == SENTINEL).all()
    total = 0
    for r, (_, _, S, row) in enumerate(table):
        frame, _, _ = D.labels_frame(runs[offsets[r] : offsets[r + 1]], CALLS, "*", TPO, False)
        with np.errstate(invalid="ignore"):
            starts, stops, names = P.compute_binary_predictions(agg[row : row + S], cnt[row : row + S], CALLS, threshold=thresholds)
        want = P.compute_labels(starts, stops, names, TPO, "*")
        assert same(frame, want), r
        for l in (1, 3, 6):
            mine = frame[frame["label"] == CALLS[l] + "*"]
            assert ((mine["start"] == 39 * TPO) & (mine["stop"] == 41 * TPO)).any() and not ((mine["start"] <= 34 * TPO) & (mine["stop"] >= 34 * TPO)).any()
        assert "SS*" not in set(frame["label"]) and (frame["label"] == "TAILSLAP*").sum() >= 1
        total += len(frame)
    assert total > 50
    scalar, _ = extract(agg, cnt, table, rank)
    assert scalar.tobytes() != runs.tobytes()
    # the Python half: the same rows through extract_labels_device
    pending = D.extract_labels_device(device(agg), device(cnt), torch.tensor(table, dtype=torch.int64, device="cuda"), 2, CALLS, "*", TPO, DELTA_T, thresholds=thresholds)
    for r, rows in enumerate(pending.runs()):
        assert np.array_equal(rows, runs[offsets[r] : offsets[r + 1]])
    assert lib_refuses_null_thresholds()


def lib_refuses_null_thresholds():
    z = torch.zeros(64, dtype=torch.float64, device="cuda")
    return N.lib().orcai_extract_labels_per_label(N.ptr(z), N.ptr(z), 1, N.ptr(z), 1, 8, None, N.ptr(z), None, DELTA_T, TPO, N.ptr(z), 1, N.ptr(z), N.ptr(z), 512,
                                                  N.stream_ptr()) == N.E_BADARG


# ------------------------------------------------------------------ 3. end to end
def test_orcai_test_writes_the_same_sweep_on_both_routes(tmp_path, capsys):
    """24 synthetic snippets of the small model of test_device_tables_gpu in batches of 8, not shuffled: both routes and both passes of the host route
    see the same batches.  A batch has 8 * 8 * 3 = 192 elements, one workgroup of orcai_masked_bce: the loss is the same sum on every run, so the
    metrics file is compared byte for byte as well."""
    from orcai_amd.architectures import ResNetLSTM
    from orcai_amd.datasets import SnippetDataset, make_synthetic_dataset
    from orcai_amd.test import _save_test_results, _test_model_on_dataset

    model = ResNetLSTM((32, 12, 1), 3, [10, 20], 3, 0.0, 64, seed=3)
    make_synthetic_dataset(tmp_path / "data", 24, seed=4, input_shape=(32, 12), out_steps=8, n_labels=3)
    names = ["A", "B", "C"]
    files = {}
    for key, flags in {"host": {}, "host_sweep": {"threshold_sweep": True}, "dev": {"device_tables": True},
                       "dev_sweep": {"device_tables": True, "threshold_sweep": True}, "dev_sweep_17": {"device_tables": True, "threshold_sweep": True, "num_thresholds": 17}}.items():
        data = SnippetDataset(tmp_path / "data", 8, seed=1, shuffle=False)
        results = _test_model_on_dataset(model, data, names, "test_data", QUIET, **flags)
        assert ("threshold_sweep" in results) == ("threshold_sweep" in flags)
        _save_test_results(results, tmp_path / key, QUIET)
        files[key] = {f.name: f.read_bytes() for f in sorted((tmp_path / key).iterdir())}
    capsys.readouterr()
    new = ["test_data_auc.json", "test_data_threshold_sweep.csv", "test_data_thresholds.json"]
    assert len(files["host"]) == 4 and sorted(set(files["host_sweep"]) - set(files["host"])) == new
    for route in ("host", "dev"):  # every file of the run without the flag, byte for byte
        assert sorted(files[route + "_sweep"]) == sorted(list(files[route]) + new)
        for name, data in files[route].items():
            assert files[route + "_sweep"][name] == data, (route, name)
    for name in new:  # the three new files: the same on both routes
        assert files["dev_sweep"][name] == files["host_sweep"][name], name
    sweep = pd.read_csv(tmp_path / "dev_sweep" / "test_data_threshold_sweep.csv")
    assert len(sweep) == 3 * 200 and (sweep["TP"] + sweep["FN"]).nunique() <= 3 and sweep["TP"].sum() > 0 and sweep["FP"].sum() > 0
    assert len(pd.read_csv(tmp_path / "dev_sweep_17" / "test_data_threshold_sweep.csv")) == 3 * 17
    thresholds = json.loads(files["dev_sweep"]["test_data_thresholds.json"])
    auc = json.loads(files["dev_sweep"]["test_data_auc.json"])
    assert list(thresholds) == names and list(auc["ROC_AUC"]) == names and 0.0 <= auc["MAUC"] <= 1.0


@pytest.fixture(scope="module")
def recording(tmp_path_factory):
    """(model directory, folder with a.wav and b.wav, the averaged probabilities of a.wav [S][7])."""
    from test_predict_e2e_gpu import _model_dir

    from orcai_amd import wavio
    from orcai_amd.synthetic import synth_recording

    base = tmp_path_factory.mktemp("thresholds")
    model_dir, _ = _model_dir(base)
    clips = base / "clips"
    clips.mkdir()
    wavio.write_wav_pcm16(clips / "a.wav", synth_recording(8.0, 48000, seed=34), 48000)
    wavio.write_wav_pcm16(clips / "b.wav", synth_recording(5.0, 48000, seed=33), 48000)
    out = base / "plain"
    out.mkdir()
    P.predict(clips / "a.wav", model_dir=model_dir, output_path=out / "a.txt", save_probabilities=True, verbosity=0)
    probabilities = pd.read_csv(out / "a_probabilities.csv.gz", index_col="time", float_precision="round_trip")
    assert list(probabilities.columns) == CALLS
    return model_dir, clips, out, probabilities.to_numpy()


def chosen_thresholds(prob):
    """{label: threshold} for six of the seven labels (WHISTLE keeps 0.5).  a.wav has three overlapping snippets, so the maximum count is 2 and label l
    is cut at thresholds[l] / 2.  BR: if every row is above 0.25 -- one run over the whole recording at 0.5 -- a threshold no probability reaches
    (no run), otherwise one below every probability (one run over the whole recording): its intervals differ from those at 0.5 either way.  The
    others: twice the middle between the column's extremes, and for PHS twice a probability of the column itself (a row exactly at the cut)."""
    out = {"BR": 3.0 if prob[:, 0].min() > 0.25 else -1.0}
    for l in range(1, 6):
        out[CALLS[l]] = float(prob[:, l].min() + prob[:, l].max())
    out["PHS"] = float(2.0 * np.sort(prob[:, 3])[len(prob) // 2])
    return out


def test_predict_with_thresholds_on_both_routes(tmp_path, recording):
    model_dir, clips, plain, prob = recording
    want = (plain / "a.txt").read_bytes()

    def run(name, **flags):
        P.predict(clips / "a.wav", model_dir=model_dir, output_path=tmp_path / name, verbosity=0, **flags)
        return (tmp_path / name).read_bytes()

    assert run("half_host.txt", thresholds={c: 0.5 for c in CALLS}) == want
    assert run("half_dev.txt", thresholds={c: 0.5 for c in CALLS}, device_labels=True) == want
    path = tmp_path / "thresholds.json"
    path.write_text(json.dumps(chosen_thresholds(prob)))
    host, dev = run("host.txt", thresholds=path), run("dev.txt", thresholds=path, device_labels=True)
    assert dev == host and host != want

    def intervals(data, label):
        return [line for line in data.decode().splitlines()[1:] if line.endswith("\t" + label + "*")]

    assert intervals(host, "BR") != intervals(want, "BR") and intervals(host, "WHISTLE") == intervals(want, "WHISTLE")


@pytest.mark.parametrize("batch_frames", [0, 3000])
def test_predict_table_with_thresholds(tmp_path, recording, batch_frames):
    model_dir, clips, _, prob = recording
    pd.DataFrame({"recording": ["a", "b"], "base_dir_recording": [str(clips)] * 2, "rel_recording_path": ["a.wav", "b.wav"], "channel": [1, 1]}).to_csv(
        tmp_path / "table.csv", index=False)
    thresholds = chosen_thresholds(prob)
    got = {}
    for flag in (False, True):
        folder = tmp_path / str(flag)
        folder.mkdir()
        P.predict(tmp_path / "table.csv", model_dir=model_dir, output_path=folder, verbosity=0, batch_frames=batch_frames, device_labels=flag, thresholds=thresholds)
        got[flag] = {f.name: f.read_bytes() for f in sorted(folder.iterdir())}
    assert len(got[False]) == 2 and got[True] == got[False]
    P.predict(clips / "a.wav", model_dir=model_dir, output_path=tmp_path / "one.txt", verbosity=0, thresholds=thresholds)
    assert got[False]["a_model_predicted.txt"] == (tmp_path / "one.txt").read_bytes()
