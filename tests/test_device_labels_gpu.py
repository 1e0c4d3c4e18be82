"""Label extraction on the GPU.  Everything compared is integers or strings, so every comparison is exact.

1. orcai_extract_labels on crafted agg / cnt against the host route (compute_binary_predictions + compute_labels + filter_predictions, through
   test_device_labels.host_route) per recording: DataFrame.equals, equal columns, equal too-short / too-long counts; and its raw rows against the
   contract restated in numpy (test_device_labels.contract), label indices and statuses included.  Sizes follow labels.hip: 256 rows per
   workgroup (255 / 256 / 257), 64 row tiles = 16384 rows per scan pass (three passes and a remainder: 49741 rows).
2. End to end, on the model directory and the clips of test_predict_batch_gpu: predict(device_labels=True) writes the bytes predict() writes, on
   every route; predict_wavs(device_labels=True) returns predict_wav's triples; without save_probabilities no S x L doubles reach the host.
"""

import numpy as np
import pandas as pd
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from test_device_labels import DELTA_T, QUIET, TPO, contract, host_route, same  # noqa: E402
from test_predict_batch_gpu import _clips, content  # noqa: E402
from test_predict_e2e_gpu import _model_dir  # noqa: E402
from test_wav_decode import riff  # noqa: E402

from orcai_amd import _native as N  # noqa: E402
from orcai_amd import device_labels as D  # noqa: E402
from orcai_amd import predict as P  # noqa: E402

SENTINEL = -77
ROW_TILE, SCAN_TILE = 256, 64  # labels.hip


def names_for(L):
    """L distinct names whose string order is not the index order."""
    return [f"n{(i * 37 + 5) % 64:02d}" for i in range(L)]


def extract(agg, cnt, table, rank, limits=None, capacity=None, guard_rows=2):
    """One call: (runs int32 [capacity + guard_rows][4] as the device holds them, offsets int64 [R + 1])."""
    S, L = agg.shape
    R = len(table)
    cap = L * ((S + 1) // 2) + R if capacity is None else capacity
    a, c = torch.from_numpy(np.ascontiguousarray(agg)).cuda(), torch.from_numpy(np.ascontiguousarray(cnt)).cuda()
    t = torch.tensor(table, dtype=torch.int64, device="cuda")
    rk = torch.from_numpy(np.asarray(rank, dtype=np.int32)).cuda()
    lim = None if limits is None else torch.from_numpy(np.ascontiguousarray(limits, dtype=np.float64)).cuda()
    runs = torch.full((cap + guard_rows, 4), SENTINEL, dtype=torch.int32, device="cuda")
    offsets = torch.full((R + 1,), SENTINEL, dtype=torch.int64, device="cuda")
    lib = N.lib()
    nbytes = lib.orcai_extract_labels_workspace_bytes(L, R, S)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    N.check(lib.orcai_extract_labels(N.ptr(a), N.ptr(c), L, N.ptr(t), R, S, 0.5, N.ptr(rk), None if lim is None else N.ptr(lim), DELTA_T, TPO, N.ptr(runs), cap,
                                     N.ptr(offsets), N.ptr(ws), nbytes, N.stream_ptr()), "orcai_extract_labels")
    torch.cuda.synchronize()
    return runs.cpu().numpy(), offsets.cpu().numpy()


def host_or_empty(agg, cnt, calls, suffix, limits):
    if len(cnt) == 0:
        frame = P.compute_labels([], [], [], TPO, suffix)
        return (frame if limits is None else P.filter_predictions(frame, DELTA_T, limits, suffix, msgr=QUIET)), 0, 0
    return host_route(agg, cnt, calls, suffix, limits)


def check(agg, cnt, table, calls, suffix="*", limits=None):
    """The kernel against the host route per recording and against the contract row by row; returns the number of runs."""
    rank = D.label_rank(calls, suffix)
    lim = None if limits is None else D.resolve_limits(calls, suffix, limits)
    runs, offsets = extract(agg, cnt, table, rank, lim)
    total = int(offsets[-1])
    want_runs, want_offsets = contract(agg, cnt, table, 0.5, rank, lim, DELTA_T, TPO)
    assert np.array_equal(offsets, want_offsets), (offsets, want_offsets)
    assert np.array_equal(runs[:total], want_runs)
    assert (runs[total:] == SENTINEL).all()
    for r, (_, _, S, row) in enumerate(table):
        frame, n_short, n_long = D.labels_frame(runs[offsets[r] : offsets[r + 1]], calls, suffix, TPO, limits is not None)
        want, w_short, w_long = host_or_empty(agg[row : row + S], cnt[row : row + S], calls, suffix, limits)
        assert same(frame, want) and (n_short, n_long) == (w_short, w_long), (r, S, row)
    return total


def one(S):
    return [(0, 0, S, 0)]


def counts(S):
    c = np.full(S, 2.0)
    c[0] = 1.0  # the first rows of a recording are covered once; the maximum, 2, sets the threshold 0.25
    return c


def patterns(S, L, seed):
    rng = np.random.default_rng(seed)
    rows, cols = np.arange(S)[:, None], np.arange(L)[None, :]
    hi, z = 0.9, np.zeros((S, L))
    out = {"zeros": z.copy(), "ones": z + hi, "1010": np.where(rows % 2 == 0, hi, 0.0) + z, "0101": np.where(rows % 2 == 1, hi, 0.0) + z,
           "run at row 0": np.where(rows < 3, hi, 0.0) + z, "run to the last row": np.where(rows >= S - 2, hi, 0.0) + z,
           "single rows": np.where((rows + cols) % 3 == 0, hi, 0.0), "staggered edges": np.where((rows + cols) % 7 < 1 + cols % 5, hi, 0.0),
           "at the threshold": np.where(rng.random((S, L)) < 0.5, 0.25, np.nextafter(0.25, 1.0)),
           "random 0.3": np.where(rng.random((S, L)) < 0.3, hi, 0.1), "random 0.9": np.where(rng.random((S, L)) < 0.9, hi, 0.1)}
    nan = out["random 0.9"].copy()
    nan[rng.random((S, L)) < 0.2] = np.nan
    out["nan"] = nan
    return out


# ------------------------------------------------------------------ 1. the kernel
@pytest.mark.parametrize("L", [1, 7, 33, 64])
def test_patterns_equal_the_host_route(L):
    calls = names_for(L)
    for S in (1, 2, 63, 64, 65, ROW_TILE - 1, ROW_TILE, ROW_TILE + 1):
        for name, agg in patterns(S, L, seed=1000 * L + S).items():
            total = check(agg, counts(S), one(S), calls)
            if name in ("1010", "0101"):
                assert total == L * ((S + (name == "1010")) // 2)  # the capacity bound: ceil(S / 2) runs per column
            if name in ("zeros",):
                assert total == 0
            if name == "ones":
                assert total == L
            if name == "at the threshold" and S > 8:
                assert 0 < total  # the values one ulp above are ones, the equal ones are not (checked by the comparison above)


def test_three_scan_passes_and_a_remainder():
    """49741 rows = 3 * 16384 + 2 * 256 + 77: one run as long as the recording, one column alternating every row, a run across every row-tile
    edge and one across every scan-pass edge, random columns."""
    S, L = 3 * SCAN_TILE * ROW_TILE + 2 * ROW_TILE + 77, 7
    rng = np.random.default_rng(7)
    agg = np.where(rng.random((S, L)) < 0.3, 0.9, 0.1)
    agg[:, 0] = 0.9
    agg[:, 1] = np.where(np.arange(S) % 2 == 0, 0.9, 0.0)
    agg[:, 2] = 0.0
    edges = np.arange(ROW_TILE, S, ROW_TILE)
    agg[edges - 1, 2] = agg[edges, 2] = 0.9
    agg[:, 3] = np.where(rng.random(S) < 0.9, 0.9, 0.1)
    agg[:, 4] = 0.0
    for e in range(SCAN_TILE * ROW_TILE, S, SCAN_TILE * ROW_TILE):
        agg[e - 300 : e + 300, 4] = 0.9
    total = check(agg, counts(S), one(S), names_for(L))
    assert total > 20000


def test_all_64_columns_alternating_fill_the_capacity_bound():
    S, L = 2 * ROW_TILE + 3, 64
    agg = np.where(np.arange(S)[:, None] % 2 == 0, 0.9, 0.0) + np.zeros((S, L))
    assert check(agg, counts(S), one(S), names_for(L)) == L * ((S + 1) // 2)


@pytest.mark.parametrize("R", [1, 3, 17])
def test_ragged_recordings(R):
    sizes = {1: [46], 3: [46, 0, 1], 17: [46, 1, 0, 0, 69, 300, 1, 46, 2, 0, 257, 46, 63, 1, 1, 256, 0]}[R]
    L = 7
    table, row = [], 0
    for S in sizes:
        table.append((0, 0, S, row))
        row += S
    rng = np.random.default_rng(R)
    agg = np.where(rng.random((row, L)) < 0.5, 0.9, 0.1)
    cnt = np.full(row, 2.0)
    for (_, _, S, r0) in table:  # a one in the last row of every recording and in the first of the next, in every column: two runs
        if S > 0:
            agg[r0] = agg[r0 + S - 1] = 0.9
    if R == 17:  # values of 0.3 where one recording's maximum count is 1 (threshold 0.5: no ones) and its neighbour's is 2 (0.25: all ones)
        (_, _, Sa, ra), (_, _, Sb, rb) = table[0], table[7]
        agg[ra : ra + Sa] = 0.3
        cnt[ra : ra + Sa] = 1.0
        agg[rb : rb + Sb] = 0.3
        cnt[rb + Sb - 1] = 0.0  # a zero-count step behind the last snippet
        cnt[table[1][3]] = 0.0  # a one-row recording without cover: no runs
    check(agg, cnt, table, names_for(L))
    runs, offsets = extract(agg, cnt, table, D.label_rank(names_for(L), "*"))
    if R == 17:
        assert offsets[1] - offsets[0] == 0 and offsets[8] - offsets[7] == L and offsets[2] - offsets[1] == 0
    assert all(offsets[r + 1] == offsets[r] for r, S in enumerate(sizes) if S == 0)


def test_order_of_equal_starts_equal_intervals_and_duplicate_names():
    calls = ["b", "a", "b", "B", "a", "c"]
    S = 40
    agg = np.zeros((S, len(calls)))
    agg[3:9, 0] = agg[3:6, 1] = agg[3:9, 2] = agg[3:6, 3] = agg[3:9, 4] = agg[3:4, 5] = 0.9  # one start, three stops, equal intervals across labels
    agg[20:22] = 0.9  # six equal intervals
    agg[39, ::2] = 0.9
    for suffix in ("*", "~", None):
        assert check(agg, counts(S), one(S), calls, suffix=suffix) == 15
    rank = D.label_rank(calls, "*")
    runs, offsets = extract(agg, counts(S), one(S), rank)
    assert [int(v) for v in runs[:6, 2]] == [5, 3, 1, 4, 0, 2]  # stop 3 (c), stop 5 (B, a), stop 8 (a, b, b): the duplicates in index order
    assert [int(v) for v in runs[6:12, 2]] == [3, 1, 4, 0, 2, 5]  # "B*" < "a*" = "a*" < "b*" = "b*" < "c*"


def test_duration_filter_with_durations_equal_to_the_limits():
    calls = ["a", "b", "c", "d"]
    S = 300
    agg = np.zeros((S, 4))
    row = 1
    for length in list(range(1, 12)) * 3:  # stop - start = 0 .. 10 rows
        agg[row : row + length, :] = 0.9
        row += length + 1
    assert row < S

    def seconds(rows):
        return ((rows) * 16) * DELTA_T  # the expression of the kernel and of the host: equality occurs

    limits = {"a": [seconds(2), seconds(4)], "b": [None, seconds(7)], "default": [seconds(5), None], "d": [seconds(3), seconds(3)]}
    lim = D.resolve_limits(calls, "*", limits)
    assert check(agg, counts(S), one(S), calls, limits=limits) == 4 * 33
    runs, _ = extract(agg, counts(S), one(S), D.label_rank(calls, "*"), lim)
    runs = runs[: 4 * 33]
    length = runs[:, 1] - runs[:, 0]
    for label, (lo, hi) in enumerate([(2, 4), (0, 7), (5, 10**9), (3, 3)]):
        mine = runs[:, 2] == label
        assert np.array_equal(runs[mine, 3], np.where(length[mine] < lo, 1, np.where(length[mine] > hi, 2, 0)))  # the limits themselves are kept
    assert {0, 1, 2} == set(int(v) for v in runs[:, 3])
    check(agg, counts(S), one(S), calls, limits={"a": [seconds(2), None]})  # no default: the others are 0 .. inf
    check(agg, counts(S), one(S), calls, suffix="~", limits=limits)


def test_overflow_counts_every_run_and_stores_only_capacity():
    S, L = 65, 7
    agg = np.where(np.arange(S)[:, None] % 2 == 0, 0.9, 0.0) + np.zeros((S, L))
    rank = D.label_rank(names_for(L), "*")
    full, offsets = extract(agg, counts(S), one(S), rank)
    assert offsets[-1] == 7 * 33
    for capacity in (100, 1, 0):
        runs, offsets = extract(agg, counts(S), one(S), rank, capacity=capacity, guard_rows=8)
        assert offsets[-1] == 7 * 33 and offsets[0] == 0
        assert np.array_equal(runs[:capacity], full[:capacity]) and (runs[capacity:] == SENTINEL).all()


def test_two_launches_write_the_same_bytes():
    S, L = 3 * ROW_TILE + 9, 33
    agg = patterns(S, L, seed=3)["nan"]
    rank = D.label_rank(names_for(L), "*")
    lim = D.resolve_limits(names_for(L), "*", {"default": [0.01, 0.05]})
    a, b = extract(agg, counts(S), one(S), rank, lim), extract(agg, counts(S), one(S), rank, lim)
    assert a[1][-1] > 1000 and a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


def test_refusals_launch_nothing():
    S, L, R = 65, 7, 1
    dev = lambda x: torch.from_numpy(x).cuda()  # noqa: E731
    agg, cnt = dev(np.full((S, L), 0.9)), dev(counts(S))
    table = torch.tensor(one(S), dtype=torch.int64, device="cuda")
    rank = dev(np.arange(L, dtype=np.int32))
    runs = torch.full((L * 33 + 2, 4), SENTINEL, dtype=torch.int32, device="cuda")
    offsets = torch.full((R + 1,), SENTINEL, dtype=torch.int64, device="cuda")
    lib = N.lib()
    need = lib.orcai_extract_labels_workspace_bytes(L, R, S)
    assert need > 0 and lib.orcai_extract_labels_workspace_bytes(0, R, S) == 0 and lib.orcai_extract_labels_workspace_bytes(65, R, S) == 0
    ws = torch.full((need,), 0x5A, dtype=torch.uint8, device="cuda")
    good = dict(agg=N.ptr(agg), cnt=N.ptr(cnt), L=L, table=N.ptr(table), R=R, S_total=S, threshold=0.5, label_rank=N.ptr(rank), limits=None, frame_seconds=DELTA_T,
                tpo=TPO, runs=N.ptr(runs), capacity=L * 33 + 1, offsets=N.ptr(offsets), workspace=N.ptr(ws), workspace_bytes=need, stream=N.stream_ptr())
    bad = {f"null {k}": {k: None} for k in ("agg", "cnt", "table", "label_rank", "runs", "offsets", "workspace")}
    bad.update({"L = 0": {"L": 0}, "L = 65": {"L": 65}, "R = 0": {"R": 0}, "S_total = 0": {"S_total": 0}, "capacity < 0": {"capacity": -1}, "tpo = 0": {"tpo": 0},
                "small workspace": {"workspace_bytes": need - 1}})
    for name, change in bad.items():
        assert lib.orcai_extract_labels(*{**good, **change}.values()) == N.E_BADARG, name
    # a grid of 2^31 row tiles: refused before the (never this large) workspace is touched
    assert lib.orcai_extract_labels(*{**good, "S_total": 2**39 + 1, "workspace_bytes": 2**62}.values()) == N.E_UNSUPPORTED
    torch.cuda.synchronize()
    assert bool((runs == SENTINEL).all()) and bool((offsets == SENTINEL).all()) and bool((ws == 0x5A).all())
    assert lib.orcai_extract_labels(*good.values()) == 0  # and the good call runs
    torch.cuda.synchronize()
    assert int(offsets[1]) == L


def test_more_runs_than_the_eager_copy(monkeypatch):
    """extract_labels_device: the runs past EAGER_RUNS come in the second copy; per recording the host route's tables."""
    monkeypatch.setattr(D, "EAGER_RUNS", 16)
    L, sizes = 7, [46, 0, 69, 1]
    calls = names_for(L)
    table, row = [], 0
    for S in sizes:
        table.append((0, 0, S, row))
        row += S
    agg = patterns(row, L, seed=11)["random 0.3"]
    cnt = np.full(row, 2.0)
    limits = {"default": [0.05, 0.2]}  # a row is 16 * DELTA_T = 0.085 s: single rows are too short, four rows and more too long
    for lim in (None, limits):
        pending = D.extract_labels_device(torch.from_numpy(agg).cuda(), torch.from_numpy(cnt).cuda(), torch.tensor(table, dtype=torch.int64, device="cuda"), len(table),
                                          calls, "*", TPO, DELTA_T, call_duration_limits=lim)
        got = pending.results()
        assert sum(len(f) + a + b for f, a, b in got) > 100
        for (_, _, S, r0), (frame, n_short, n_long) in zip(table, got):
            want, w_short, w_long = host_or_empty(agg[r0 : r0 + S], cnt[r0 : r0 + S], calls, "*", lim)
            assert same(frame, want) and (n_short, n_long) == (w_short, w_long)


# ------------------------------------------------------------------ 2. end to end
def _durations(results):
    return np.concatenate([((r[0]["stop"] - r[0]["start"]) * r[2]).to_numpy(dtype=np.float64) for r in results if isinstance(r, tuple)] or [np.zeros(0)])


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    """(model directory, clip paths, duration limits).  The output bias of the test's own copy of the seeded weights is moved until the clips hold
    at least ten intervals of more than one duration; the limits then drop the ones shorter than the mean."""
    from orcai_amd.io import load_orcai_model

    base = tmp_path_factory.mktemp("device_labels")
    source, _ = _model_dir(base)
    paths = _clips(base / "clips")
    weights = dict(np.load(source / "orcai-v1.weights.npz"))
    for k, shift in enumerate((0.0, -0.5, 0.5, -1.0, 1.0, -1.5, 1.5, -2.0, 2.0, -3.0, 3.0)):
        d = base / f"shift{k}" / "model"
        d.mkdir(parents=True)
        for n in ("orcai_parameter.json", "model_shape.json"):
            (d / n).write_text((source / n).read_text())
        np.savez(d / "orcai-v1.weights.npz", **{**weights, "dense2/bias": weights["dense2/bias"] + np.float32(shift)})
        model, param, shape = load_orcai_model(d)
        seconds = _durations(P.predict_wavs([(p, 1) for p in paths], model, param, shape))
        if len(seconds) >= 10 and len(np.unique(seconds)) > 1:
            mean = float(np.mean(seconds))  # above the shortest interval, whatever the distribution
            return d, paths, {"default": [mean, None], "BR": [mean, max(mean, float(np.max(seconds)) / 2)]}
    pytest.fail("no output bias gives the clips ten intervals")


def _lines(data: bytes) -> int:
    return len(data.decode().strip().split("\n")) - 1


def _files(folder, skip=()):
    return {f.name: content(f) for f in sorted(folder.iterdir()) if f.suffix != ".wav" and f.name not in skip}


def _compare_routes(run, make_folder, limits):
    """run(folder, **flags) writes its files into folder.  Per limits: the host route with probabilities once; the device route with and without."""
    found = kept = 0
    for lim in (None, limits):
        ref = make_folder()
        run(ref, call_duration_limits=lim, save_probabilities=True, device_labels=False)
        want = _files(ref)
        assert any(n.endswith(".gz") for n in want) and any(n.endswith(".txt") for n in want)
        dev = make_folder()
        run(dev, call_duration_limits=lim, save_probabilities=True, device_labels=True)
        assert _files(dev) == want
        dev = make_folder()
        run(dev, call_duration_limits=lim, save_probabilities=False, device_labels=True)
        assert _files(dev) == {n: b for n, b in want.items() if n.endswith(".txt")}
        n = sum(_lines(b) for name, b in want.items() if name.endswith(".txt"))
        found, kept = (n, kept) if lim is None else (found, n)
    return found, kept


def _folders(tmp_path, link=None):
    made = []

    def make():
        folder = tmp_path / f"run{len(made)}"
        folder.mkdir()
        made.append(folder)
        if link is not None:
            (folder / link.name).write_bytes(link.read_bytes())
        return folder

    return make


def test_predict_one_wav_writes_the_same_files(tmp_path, setup):
    model_dir, paths, limits = setup

    def run(folder, **flags):
        P.predict(folder / "a.wav", model_dir=model_dir, verbosity=0, **flags)

    found, kept = _compare_routes(run, _folders(tmp_path, link=paths[0]), limits)
    assert found >= 1


@pytest.mark.parametrize("batch_frames", [0, 3000])
def test_predict_table_writes_the_same_files(tmp_path, setup, batch_frames):
    model_dir, paths, limits = setup
    names = ["a", "b", "d", "e", "c", "missing"]  # c is shorter than one snippet, the last file does not exist: both are logged and skipped
    pd.DataFrame({"recording": names, "base_dir_recording": [str(paths[0].parent)] * len(names), "rel_recording_path": [f"{n}.wav" for n in names[:5]] + ["nope.wav"],
                  "channel": [1] * len(names)}).to_csv(tmp_path / "table.csv", index=False)

    def run(folder, **flags):
        P.predict(tmp_path / "table.csv", model_dir=model_dir, output_path=folder, verbosity=0, batch_frames=batch_frames, **flags)

    found, kept = _compare_routes(run, _folders(tmp_path), limits)
    assert found >= 10 and kept < found  # ten intervals compared, and the limits drop at least one


def test_predict_all_channels_writes_the_same_files(tmp_path, setup):
    from orcai_amd.synthetic import synth_recording

    model_dir, _, limits = setup
    rate = 22050
    pcm = np.stack([synth_recording(8.0, rate, seed=40 + c) for c in range(3)]).astype(np.int32)
    payload = np.ascontiguousarray(pcm.T << 8).view(np.uint8).reshape(-1, 4)[:, :3].tobytes()
    wav = tmp_path / "array.wav"
    wav.write_bytes(riff("S24", 3, rate, payload))

    def run(folder, **flags):
        P.predict(folder / "array.wav", channel="all", model_dir=model_dir, verbosity=0, **flags)

    found, _ = _compare_routes(run, _folders(tmp_path, link=wav), limits)
    assert found >= 3


def test_predict_wavs_returns_predict_wavs_triples(setup):
    from orcai_amd.io import load_orcai_model

    model_dir, paths, _ = setup
    model, param, shape = load_orcai_model(model_dir)
    got = P.predict_wavs([(p, 1) for p in paths], model, param, shape, device_labels=True)
    again = P.predict_wavs([(p, 1) for p in paths], model, param, shape, device_labels=True, max_frames=4000)
    for i, p in enumerate(paths):
        if i == 2:
            assert isinstance(got[i], ValueError) and "recording too short" in str(got[i])
            continue
        labels, agg, delta_t = P.predict_wav(p, 1, model, param, shape)
        one_dev = P.predict_wav(p, 1, model, param, shape, device_labels=True)
        for triple in (got[i], again[i], one_dev):
            assert same(triple[0], labels) and triple[1].dtype == np.float64 and np.array_equal(triple[1], agg) and triple[2] == delta_t


def test_the_probabilities_stay_on_the_device(tmp_path, setup, monkeypatch):
    """A spy on every device-to-host tensor copy: with device_labels=True and save_probabilities=False no f64 buffer of S x L values (or more) reaches
    the host; the same spy sees that buffer on the host route."""
    model_dir, paths, limits = setup
    S, L = 2250 // 16, 7  # the 12 s clip: 2251 spectrogram frames
    seen = []
    copy_, cpu, to = torch.Tensor.copy_, torch.Tensor.cpu, torch.Tensor.to

    def spy_copy(self, src, *a, **k):
        if isinstance(src, torch.Tensor) and src.is_cuda and not self.is_cuda:
            seen.append((src.dtype, src.numel()))
        return copy_(self, src, *a, **k)

    def spy_cpu(self, *a, **k):
        if self.is_cuda:
            seen.append((self.dtype, self.numel()))
        return cpu(self, *a, **k)

    def spy_to(self, *a, **k):
        out = to(self, *a, **k)
        if self.is_cuda and not out.is_cuda:
            seen.append((self.dtype, self.numel()))
        return out

    monkeypatch.setattr(torch.Tensor, "copy_", spy_copy)
    monkeypatch.setattr(torch.Tensor, "cpu", spy_cpu)
    monkeypatch.setattr(torch.Tensor, "to", spy_to)
    big = {}
    for flag in (False, True):
        folder = tmp_path / str(flag)
        folder.mkdir()
        (folder / "a.wav").write_bytes(paths[0].read_bytes())
        seen.clear()
        P.predict(folder / "a.wav", model_dir=model_dir, verbosity=0, call_duration_limits=limits, device_labels=flag)
        big[flag] = [n for dtype, n in seen if dtype == torch.float64 and n >= S * L]
    assert big[False] and not big[True], big
    assert content(tmp_path / "True" / "a_c1_orcai-v1_predicted.txt") == content(tmp_path / "False" / "a_c1_orcai-v1_predicted.txt")
