"""orcai_interval_scores on the GPU.  Everything compared is bytes: the kernel's 24 bytes per run against the host twin's three fields.

1. The kernel behind each of the three extraction calls, on the same device buffers, at the sizes at which labels.hip can go wrong: 256 rows per tile
   (255 / 256 / 257 / 513), a run from the last row of a tile to the first row of the next but one, one run over 128 tiles (more than the 16 lanes of
   a run, more than a wave), the capacity bound, three recordings off the tile edges with one without rows, a NaN in a merged gap; two calls; the
   refusals; the second copy of extract_labels_device.
2. predict(scores=True) end to end on tiny synthetic recordings with seeded untrained weights: the score file is the same bytes with device_labels
   and without, the label file is the file written without the option, with duration limits the score file has exactly the kept lines.
"""

import numpy as np
import pandas as pd
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from test_interval_scores import scored_contract  # noqa: E402
from test_label_refine import DELTA_T, TPO, names_for, smoothed  # noqa: E402
from test_predict_batch_gpu import _clips, content  # noqa: E402
from test_predict_e2e_gpu import _model_dir  # noqa: E402
from test_wav_decode import riff  # noqa: E402

from orcai_amd import _native as N  # noqa: E402
from orcai_amd import device_labels as D  # noqa: E402
from orcai_amd import predict as P  # noqa: E402
from orcai_amd import scores as Z  # noqa: E402

SENTINEL = -77
ROW_TILE = 256  # labels.hip


def dev(x, dtype):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=dtype)).cuda()


def extract_and_score(agg, cnt, table, call="per_label", t_lo=None, t_hi=None, gaps=None, eager_runs=0, repeat=1, guard_rows=2):
    """One extraction call (`call`: scalar / per_label / refined) and `repeat` scoring calls behind it on the same buffers.  Returns (runs int32
    [total][4], offsets int64 [R + 1], [per scoring call (scores int64 [capacity + guard_rows][3], eager int64 [eager_runs + guard_rows][3])])."""
    S, L = agg.shape
    R = len(table)
    cap = L * ((S + 1) // 2) + R
    t_lo = np.full(L, 0.5) if t_lo is None else t_lo
    a, c, t = dev(agg, np.float64), dev(cnt, np.float64), torch.tensor(table, dtype=torch.int64, device="cuda")
    rk, lo = dev(D.label_rank(names_for(L), "*"), np.int32), dev(t_lo, np.float64)
    runs = torch.full((cap + guard_rows, 4), SENTINEL, dtype=torch.int32, device="cuda")
    offsets = torch.full((R + 1,), SENTINEL, dtype=torch.int64, device="cuda")
    lib = N.lib()
    nbytes = (lib.orcai_extract_labels_refined_workspace_bytes if call == "refined" else lib.orcai_extract_labels_workspace_bytes)(L, R, S)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    tail = (N.ptr(rk), None, DELTA_T, TPO, N.ptr(runs), cap, N.ptr(offsets), N.ptr(ws), nbytes, N.stream_ptr())
    if call == "refined":
        hi, g = dev(t_lo if t_hi is None else t_hi, np.float64), dev(np.zeros(L) if gaps is None else gaps, np.int32)
        N.check(lib.orcai_extract_labels_refined(N.ptr(a), N.ptr(c), L, N.ptr(t), R, S, N.ptr(lo), N.ptr(hi), N.ptr(g), *tail), "orcai_extract_labels_refined")
    elif call == "per_label":
        N.check(lib.orcai_extract_labels_per_label(N.ptr(a), N.ptr(c), L, N.ptr(t), R, S, N.ptr(lo), *tail), "orcai_extract_labels_per_label")
    else:
        N.check(lib.orcai_extract_labels(N.ptr(a), N.ptr(c), L, N.ptr(t), R, S, float(t_lo[0]), *tail), "orcai_extract_labels")
    sbytes = lib.orcai_interval_scores_workspace_bytes(L, R, S)
    assert sbytes > 0
    outs = []
    for _ in range(repeat):
        sws = torch.empty(sbytes, dtype=torch.uint8, device="cuda")
        scores = torch.full((cap + guard_rows, 3), SENTINEL, dtype=torch.int64, device="cuda")
        eager = torch.full((eager_runs + guard_rows, 3), SENTINEL, dtype=torch.int64, device="cuda")
        N.check(lib.orcai_interval_scores(N.ptr(a), L, N.ptr(t), R, S, N.ptr(runs), N.ptr(offsets), cap, N.ptr(scores), N.ptr(eager) if eager_runs else None,
                                          eager_runs, N.ptr(sws), sbytes, N.stream_ptr()), "orcai_interval_scores")
        outs.append((scores, eager))
    torch.cuda.synchronize()
    offsets = offsets.cpu().numpy()
    return runs.cpu().numpy()[: int(offsets[-1])], offsets, [(s.cpu().numpy(), e.cpu().numpy()) for s, e in outs]


def check(agg, cnt, table, **kwargs):
    """The kernel's rows against the host twin on the runs the extraction call found, every byte of the output buffer; returns (runs, words)."""
    runs, offsets, [(scores, _)] = extract_and_score(agg, cnt, table, **kwargs)
    total = len(runs)
    want = scored_contract(agg, table, runs, offsets)
    assert scores[:total].tobytes() == want.tobytes(), np.argwhere(scores[:total] != want)[:5]
    assert (scores[total:] == SENTINEL).all()
    return runs, want


def one(S):
    return [(0, 0, S, 0)]


def noise(S, L, seed):
    """Smoothed noise in [0, 1.2] with NaN sprinkled in and per-label thresholds; the count's maximum is 1."""
    rng = np.random.default_rng(seed)
    agg = 1.2 * smoothed(S, L, seed, width=min(5, S))
    agg[rng.random((S, L)) < 0.01] = np.nan
    return agg, 0.6 + 0.05 * rng.random(L), rng


# ------------------------------------------------------------------ 1. the kernel
@pytest.mark.parametrize("S", [ROW_TILE - 1, ROW_TILE, ROW_TILE + 1, 2 * ROW_TILE + 1])
def test_rows_around_the_tile_edge(S):
    agg, t_lo, _ = noise(S, 7, seed=S)
    runs, _ = check(agg, np.ones(S), one(S), t_lo=t_lo)
    assert len(runs) > 20
    whole = np.full((S, 3), 0.75)  # one run per column over every row: whole tiles and the remainder
    whole[S // 2, 0] = whole[S - 1, 1] = whole[0, 2] = 0.9
    runs, words = check(whole, np.ones(S), one(S))
    assert runs[:, :2].tolist() == [[0, S - 1]] * 3 and sorted(words[:, 2].tolist()) == [0, S // 2, S - 1]


def test_a_run_from_the_last_row_of_a_tile_to_the_first_row_of_the_next_but_one():
    S = 3 * ROW_TILE
    agg = np.zeros((S, 4))
    agg[ROW_TILE - 1 : 2 * ROW_TILE + 1, 0] = 0.6  # head of one row, one whole tile, tail of one row
    agg[2 * ROW_TILE, 0] = 0.8  # the maximum in the tail
    agg[ROW_TILE - 1 : 2 * ROW_TILE + 1, 1] = 0.6
    agg[ROW_TILE - 1, 1] = agg[ROW_TILE + 7, 1] = agg[2 * ROW_TILE, 1] = 0.8  # equal maxima in head, tile and tail: the head's row
    agg[ROW_TILE : 2 * ROW_TILE, 2] = 0.6  # exactly one tile
    agg[ROW_TILE + 100, 2] = agg[ROW_TILE + 200, 2] = 0.7
    agg[ROW_TILE - 2 : ROW_TILE + 2, 3] = 0.6  # across the edge without a whole tile
    agg[ROW_TILE, 3] = 0.7
    runs, words = check(agg, np.ones(S), one(S))
    got = {int(l): (int(s), int(e), int(row)) for (s, e, l, _), row in zip(runs.tolist(), words[:, 2].tolist())}
    assert got == {0: (ROW_TILE - 1, 2 * ROW_TILE, 2 * ROW_TILE), 1: (ROW_TILE - 1, 2 * ROW_TILE, ROW_TILE - 1), 2: (ROW_TILE, 2 * ROW_TILE - 1, ROW_TILE + 100),
                   3: (ROW_TILE - 2, ROW_TILE + 1, ROW_TILE)}


def test_one_run_over_128_tiles():
    S = 2 * 64 * ROW_TILE + 3
    rng = np.random.default_rng(8)
    agg = 0.6 + 0.3 * rng.random((S, 2))
    agg[[70 * ROW_TILE + 5, 3 * ROW_TILE + 9, 100 * ROW_TILE], 0] = 0.95  # equal maxima in three tiles: the lowest row
    agg[S - 1, 1] = 0.99
    runs, words = check(agg, np.ones(S), one(S))
    assert runs[:, :3].tolist() == [[0, S - 1, 0], [0, S - 1, 1]] and words[:, 2].tolist() == [3 * ROW_TILE + 9, S - 1]
    ones = np.ones((S, 2))
    _, words = check(ones, np.ones(S), one(S))
    assert words[:, 1].tolist() == [S * 2**32] * 2 and words[:, 2].tolist() == [0, 0]


@pytest.mark.parametrize("L", [1, 7, 64])
def test_smoothed_noise_behind_each_extraction_call(L):
    S = 3000
    agg, t_lo, rng = noise(S, L, seed=50 + L)
    cnt = np.ones(S)
    plain, _ = check(agg, cnt, one(S), call="per_label", t_lo=t_lo)
    scalar, _ = check(agg, cnt, one(S), call="scalar", t_lo=np.full(L, 0.6))
    refined, _ = check(agg, cnt, one(S), call="refined", t_lo=t_lo, t_hi=t_lo + 0.1 * rng.random(L), gaps=rng.integers(1, 6, L))
    assert len(plain) > 20 * L and len(scalar) > 20 * L and 5 * L < len(refined) < len(plain)
    nan_in_gap = sum(bool(np.isnan(agg[s : e + 1, l]).any()) for s, e, l, _ in refined.tolist())
    assert nan_in_gap >= 1 or L == 1  # a merged run holds a NaN row (test_a_nan_row_in_a_merged_gap crafts one)


def test_a_nan_row_in_a_merged_gap():
    text = "..XnX...XnnX" + "." * 300 + "XnX"
    agg = np.array([{".": 0.1, "X": 0.9, "n": np.nan}[c] for c in text])[:, None]
    S = len(text)
    runs, words = check(agg, np.ones(S), one(S), call="refined", t_hi=np.array([0.8]), gaps=np.array([2]))
    assert runs[:, :2].tolist() == [[2, 4], [8, 11], [312, 314]] and words[:, 2].tolist() == [2, 8, 312]
    assert words[:, 1].tolist() == [2 * int(Z.q32(np.array([0.9]))[0])] * 3  # the NaN rows add nothing to the sum


def test_every_column_alternating_fills_the_capacity_bound():
    S, L = 4 * ROW_TILE + 1, 64
    agg = np.where(np.arange(S)[:, None] % 2 == 0, 0.9, 0.0) + 0.001 * np.arange(L)[None, :]
    runs, _ = check(agg, np.ones(S), one(S))
    assert len(runs) == L * ((S + 1) // 2)  # capacity less the one slot per recording
    merged, words = check(agg, np.ones(S), one(S), call="refined", gaps=np.ones(L))  # the same with a gap of one row: one run per column
    assert len(merged) == L and (merged[:, 1] == S - 1).all() and (words[:, 2] == 0).all()


def test_three_recordings_off_the_tile_edges_and_one_without_rows():
    sizes, L = [300, 0, 215, 700], 7
    table, row = [], 0
    for S in sizes:
        table.append((0, 0, S, row))
        row += S
    agg, t_lo, rng = noise(row, L, seed=5)
    cnt = np.full(row, 2.0)
    cnt[300:515] = 1.0  # the third recording's own maximum: its cut is twice the others'
    agg[:2] = 0.9
    for r0 in (300, 515):  # a run on either side of every recording edge
        agg[r0 - 2 : r0 + 2] = 0.9
    runs, words = check(agg, cnt, table, call="refined", t_lo=t_lo, t_hi=t_lo + 0.1, gaps=rng.integers(0, 6, L))
    assert len(runs) > 30 and (words[:, 2] >= runs[:, 0]).all() and (words[:, 2] <= runs[:, 1]).all()  # rows counted inside the recording
    many = [(0, 0, 1, i) for i in range(40)] + [(0, 0, row - 40, 40)]  # one-row recordings: the search in offsets
    check(agg, cnt, many, t_lo=t_lo)
    huge, _ = check(agg, cnt, table, call="refined", t_lo=t_lo, t_hi=t_lo, gaps=np.full(L, 2**31 - 1))  # one run per column and recording
    assert len(huge) == 3 * L


def test_two_calls_write_the_same_bytes_and_the_eager_rows_are_a_copy():
    S, L, E = 3 * ROW_TILE + 9, 33, 40
    agg, t_lo, _ = noise(S, L, seed=3)
    runs, offsets, [(s1, e1), (s2, e2)] = extract_and_score(agg, np.ones(S), one(S), t_lo=t_lo, eager_runs=E, repeat=2)
    assert len(runs) > 100 and s1.tobytes() == s2.tobytes() and e1.tobytes() == e2.tobytes()
    assert s1[: len(runs)].tobytes() == scored_contract(agg, one(S), runs, offsets).tobytes()
    assert e1[:E].tobytes() == s1[:E].tobytes() and (e1[E:] == SENTINEL).all()
    few, _, [(s3, e3)] = extract_and_score(agg[:40], np.ones(40), one(40), t_lo=t_lo, eager_runs=4096)  # fewer runs than eager rows
    assert 0 < len(few) < 4096 and e3[: len(few)].tobytes() == s3[: len(few)].tobytes() and (e3[len(few) :] == SENTINEL).all()


def test_refusals_launch_nothing():
    S, L, R = 65, 7, 1
    cap = L * 33 + 1
    agg = dev(np.full((S, L), 0.9), np.float64)
    table = torch.tensor(one(S), dtype=torch.int64, device="cuda")
    runs = torch.zeros((cap, 4), dtype=torch.int32, device="cuda")
    runs[:L, 1] = S - 1
    runs[:L, 2] = torch.arange(L, dtype=torch.int32, device="cuda")
    offsets = torch.tensor([0, L], dtype=torch.int64, device="cuda")
    scores = torch.full((cap + 1, 3), SENTINEL, dtype=torch.int64, device="cuda")
    eager = torch.full((8, 3), SENTINEL, dtype=torch.int64, device="cuda")
    lib = N.lib()
    size = lib.orcai_interval_scores_workspace_bytes
    need = size(L, R, S)
    assert need > 0 and size(0, R, S) == 0 and size(65, R, S) == 0 and size(L, 0, S) == 0 and size(L, R, 0) == 0 and size(L, R, 2**31) == 0
    assert size(L, R, 2**31 - 1) > 0
    ws = torch.full((need,), 0x5A, dtype=torch.uint8, device="cuda")
    good = dict(agg=N.ptr(agg), L=L, table=N.ptr(table), R=R, S_total=S, runs=N.ptr(runs), offsets=N.ptr(offsets), capacity=cap, scores=N.ptr(scores),
                eager=N.ptr(eager), eager_runs=4, workspace=N.ptr(ws), workspace_bytes=need, stream=N.stream_ptr())
    bad = {f"null {k}": {k: None} for k in ("agg", "table", "runs", "offsets", "scores", "workspace")}
    bad.update({"L = 0": {"L": 0}, "L = 65": {"L": 65}, "R = 0": {"R": 0}, "S_total = 0": {"S_total": 0}, "capacity < 0": {"capacity": -1},
                "eager_runs < 0": {"eager_runs": -1}, "small workspace": {"workspace_bytes": need - 1}, "misaligned runs": {"runs": N.ptr(runs) + 4},
                "misaligned scores": {"scores": N.ptr(scores) + 4}, "misaligned eager": {"eager": N.ptr(eager) + 4},
                "misaligned workspace": {"workspace": N.ptr(ws) + 16}})
    for name, change in bad.items():
        assert lib.orcai_interval_scores(*{**good, **change}.values()) == N.E_BADARG, name
    for rows in (2**31, 2**39 + 1):  # refused before the (never this large) workspace is touched
        assert lib.orcai_interval_scores(*{**good, "S_total": rows, "workspace_bytes": 2**62}.values()) == N.E_UNSUPPORTED
    torch.cuda.synchronize()
    assert bool((scores == SENTINEL).all()) and bool((eager == SENTINEL).all()) and bool((ws == 0x5A).all())
    assert lib.orcai_interval_scores(*good.values()) == 0  # and the good call runs
    torch.cuda.synchronize()
    got = scores.cpu().numpy()
    assert got[:L, 0].view(np.float64).tolist() == [0.9] * L and got[:L, 2].tolist() == [0] * L and (got[L:] == SENTINEL).all()
    assert eager.cpu().numpy()[:4].tobytes() == got[:4].tobytes() and bool((eager[4:] == SENTINEL).all())


def test_extract_labels_device_scores_and_the_second_copy(monkeypatch):
    """extract_labels_device(scores=True): the rows past EAGER_RUNS come in the second copy; per recording the host route's columns, kept rows under
    duration limits with their own scores; without the option the calls made today."""
    L, sizes = 7, [46, 0, 69, 1]
    calls = names_for(L)
    table, row = [], 0
    for S in sizes:
        table.append((0, 0, S, row))
        row += S
    agg, t_lo, rng = noise(row, L, seed=11)
    cnt = np.ones(row)
    limits = {"default": [0.05, 0.2]}  # a row is 16 * DELTA_T = 0.085 s: single rows are too short, four rows and more too long
    called = []
    real = N.lib

    class Spy:
        def __getattr__(self, name):
            called.append(name)
            return getattr(real(), name)

    monkeypatch.setattr(D.N, "lib", lambda: Spy())
    args = (torch.from_numpy(agg).cuda(), torch.from_numpy(cnt).cuda(), torch.tensor(table, dtype=torch.int64, device="cuda"), len(table), calls, "*", TPO, DELTA_T)
    D.extract_labels_device(*args, thresholds=t_lo).results()
    assert called == ["orcai_extract_labels_workspace_bytes", "orcai_extract_labels_per_label"]
    for eager_runs in (16, 4096):
        monkeypatch.setattr(D, "EAGER_RUNS", eager_runs)
        for lim in (None, limits):
            for refine in ({}, {"high_thresholds": t_lo + 0.05, "gap_rows": np.full(L, 2)}):
                called.clear()
                got = D.extract_labels_device(*args, thresholds=t_lo, call_duration_limits=lim, scores=True, **refine).results()
                assert called[-2:] == ["orcai_interval_scores_workspace_bytes", "orcai_interval_scores"] and len(called) == 4
                plain = D.extract_labels_device(*args, thresholds=t_lo, call_duration_limits=lim, **refine).results()
                assert sum(len(f) + a + b for f, a, b in got) > 20  # more than the 16 eager runs
                for (_, _, S, r0), (frame, n_short, n_long), (want, w_short, w_long) in zip(table, got, plain):
                    assert (n_short, n_long) == (w_short, w_long) and frame.drop(columns=Z.SCORE_COLUMNS).equals(want)
                    scored = Z.add_scores(want[["start", "stop", "label"]], agg[r0 : r0 + S], calls, "*", TPO)
                    assert frame[Z.SCORE_COLUMNS].equals(scored[Z.SCORE_COLUMNS])
                    assert [frame[c].dtype for c in Z.SCORE_COLUMNS] == [np.float64, np.int64, np.float64]


# ------------------------------------------------------------------ 2. end to end
@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    """(model directory, clip paths, options, duration limits).  The thresholds are quantiles of the 12 s clip's own averaged probabilities (times its
    maximum count of 2: the cut is threshold / max(count)), so about half of its rows are above the low one and a fifth above the high one."""
    from orcai_amd.io import load_orcai_model

    base = tmp_path_factory.mktemp("interval_scores")
    model_dir, _ = _model_dir(base)
    paths = _clips(base / "clips")
    model, param, shape = load_orcai_model(model_dir)
    _, agg, delta_t = P.predict_wav(paths[0], 1, model, param, shape)
    calls = param["calls"]
    low = {c: float(2 * np.quantile(agg[:, i], 0.5)) for i, c in enumerate(calls)}
    high = {c: float(2 * np.quantile(agg[:, i], 0.8)) for i, c in enumerate(calls)}
    step = TPO * float(delta_t)
    limits = {"default": [2.5 * step, 30 * step]}
    return model_dir, paths, {"thresholds": low, "high_thresholds": high, "merge_gap": 2.001 * step}, limits


def _files(folder, suffix):
    return {f.name: content(f) for f in sorted(folder.iterdir()) if f.name.endswith(suffix)}


def _routes(run, make_folder, options, limits):
    """run(folder, **flags) writes into folder.  Per set of options: the files without scores, then with scores on the host and on the device."""
    lines = {}
    for name, flags in (("plain", {"thresholds": options["thresholds"]}), ("refined", options), ("limits", {**options, "call_duration_limits": limits})):
        off, host, device = make_folder(), make_folder(), make_folder()
        run(off, **flags)
        run(host, scores=True, **flags)
        run(device, scores=True, device_labels=True, **flags)
        labels = _files(off, ".txt")
        assert labels and not _files(off, "_scores.csv")
        assert _files(host, ".txt") == labels and _files(device, ".txt") == labels  # the label file is the file written without the option
        want = _files(host, "_scores.csv")
        assert _files(device, "_scores.csv") == want and len(want) == len(labels)
        for label_name, label_bytes in labels.items():
            score_lines = want[label_name[: -len(".txt")] + "_scores.csv"].decode().split("\n")
            label_lines = label_bytes.decode().split("\n")
            assert score_lines[0] == "start\tstop\tlabel\tpeak_time\tpeak\tmean" and len(score_lines) == len(label_lines)
            for score_line, label_line in zip(score_lines[1:-1], label_lines[1:-1]):
                cells = score_line.split("\t")
                assert "\t".join(cells[:3]) == label_line and float(cells[0]) <= float(cells[3]) <= float(cells[1])
                assert 0.0 < float(cells[5]) <= float(cells[4]) <= 1.0
        lines[name] = sum(len(b.decode().split("\n")) - 2 for b in want.values())
        for f in host.iterdir():
            if f.suffix == ".txt":
                f.unlink()
        with pytest.raises(FileExistsError):  # the label files are gone, the score files are not: the overwrite check covers them
            run(host, scores=True, **flags)
    assert lines["plain"] > lines["refined"] > lines["limits"] > 0  # with duration limits: exactly the kept lines (compared line by line above), and fewer
    return lines


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


def test_predict_one_wav(tmp_path, setup):
    model_dir, paths, options, limits = setup

    def run(folder, **flags):
        P.predict(folder / "a.wav", model_dir=model_dir, verbosity=0, **flags)

    _routes(run, _folders(tmp_path, link=paths[0]), options, limits)


@pytest.mark.parametrize("batch_frames", [0, 3000])
def test_predict_table(tmp_path, setup, batch_frames):
    model_dir, paths, options, limits = setup
    names = ["a", "b", "d", "e"]
    pd.DataFrame({"recording": names, "base_dir_recording": [str(paths[0].parent)] * len(names), "rel_recording_path": [f"{n}.wav" for n in names],
                  "channel": [1] * len(names)}).to_csv(tmp_path / "table.csv", index=False)

    def run(folder, **flags):
        before = set(folder.iterdir())
        P.predict(tmp_path / "table.csv", model_dir=model_dir, output_path=folder, verbosity=0, batch_frames=batch_frames, **flags)
        if before and set(folder.iterdir()) == before:  # table mode logs a recording's error and goes on: nothing new was written
            raise FileExistsError(folder)

    _routes(run, _folders(tmp_path), options, limits)


def test_predict_all_channels(tmp_path, setup):
    from orcai_amd.synthetic import synth_recording

    model_dir, _, options, limits = setup
    rate = 22050
    pcm = np.stack([synth_recording(8.0, rate, seed=40 + c) for c in range(3)]).astype(np.int32)
    payload = np.ascontiguousarray(pcm.T << 8).view(np.uint8).reshape(-1, 4)[:, :3].tobytes()
    wav = tmp_path / "array.wav"
    wav.write_bytes(riff("S24", 3, rate, payload))

    def run(folder, **flags):
        P.predict(folder / "array.wav", channel="all", model_dir=model_dir, verbosity=0, **flags)

    _routes(run, _folders(tmp_path, link=wav), options, limits)


def test_predict_wavs_returns_the_columns(setup):
    from orcai_amd.io import load_orcai_model

    model_dir, paths, options, _ = setup
    model, param, shape = load_orcai_model(model_dir)
    items = [(p, 1) for p in paths]
    plain = P.predict_wavs(items, model, param, shape, **options)
    host = P.predict_wavs(items, model, param, shape, scores=True, **options)
    device = P.predict_wavs(items, model, param, shape, scores=True, device_labels=True, **options)
    single = P.predict_wav(paths[0], 1, model, param, shape, scores=True, device_labels=True, **options)[0]
    assert single.equals(host[0][0]) and len(single) > 5
    for a, b, c in zip(plain, host, device):
        if isinstance(a, Exception):
            assert isinstance(b, Exception) and isinstance(c, Exception)
            continue
        assert b[0].equals(c[0]) and b[0][["start", "stop", "label"]].equals(a[0]) and list(b[0].columns) == ["start", "stop", "label"] + Z.SCORE_COLUMNS
