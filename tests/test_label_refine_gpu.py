"""orcai_extract_labels_refined on the GPU.  Everything compared is integers or file bytes, so every comparison is exact.

1. The kernel against the numpy contract (test_label_refine.refined_contract: compute_binary_predictions per recording, ordered and judged as the
   header states), byte for byte, at the sizes at which labels.hip can go wrong: 256 rows per workgroup (255 / 256 / 257), 64 row tiles = 16384 rows
   per scan pass (16384 + 300), 64 candidates per keep word, three recordings whose edges are off the tile edges and one without rows; the five
   worst cases of the design at those sizes; the identity against orcai_extract_labels_per_label on the same buffers; two calls; the refusals.
2. End to end on tiny synthetic recordings with seeded untrained weights: thresholds and gap from the recording's own probability quantiles, so the
   refined file differs from the unrefined one; with --device-labels and without the files are the same bytes on every route.
"""

import numpy as np
import pandas as pd
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from test_label_refine import DELTA_T, TPO, names_for, refined_contract, smoothed  # noqa: E402
from test_predict_batch_gpu import _clips, content  # noqa: E402
from test_predict_e2e_gpu import _model_dir  # noqa: E402
from test_wav_decode import riff  # noqa: E402

from orcai_amd import _native as N  # noqa: E402
from orcai_amd import device_labels as D  # noqa: E402
from orcai_amd import predict as P  # noqa: E402

SENTINEL = -77
ROW_TILE, SCAN_TILE = 256, 64  # labels.hip
EDGE = ROW_TILE * SCAN_TILE  # 16384: the scan's carry
BIG = EDGE + 300


def dev(x, dtype):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=dtype)).cuda()


def extract(agg, cnt, table, rank, t_lo, t_hi=None, gaps=None, limits=None, guard_rows=2):
    """One call: (runs int32 [capacity + guard_rows][4] as the device holds them, offsets int64 [R + 1]).  t_hi and gaps None: the per-label call."""
    S, L = agg.shape
    R = len(table)
    cap = L * ((S + 1) // 2) + R
    a, c, t = dev(agg, np.float64), dev(cnt, np.float64), torch.tensor(table, dtype=torch.int64, device="cuda")
    rk, lo = dev(rank, np.int32), dev(t_lo, np.float64)
    lim = None if limits is None else dev(limits, np.float64)
    runs = torch.full((cap + guard_rows, 4), SENTINEL, dtype=torch.int32, device="cuda")
    offsets = torch.full((R + 1,), SENTINEL, dtype=torch.int64, device="cuda")
    lib = N.lib()
    refined = t_hi is not None
    nbytes = (lib.orcai_extract_labels_refined_workspace_bytes if refined else lib.orcai_extract_labels_workspace_bytes)(L, R, S)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    tail = (N.ptr(rk), None if lim is None else N.ptr(lim), DELTA_T, TPO, N.ptr(runs), cap, N.ptr(offsets), N.ptr(ws), nbytes, N.stream_ptr())
    if refined:
        hi, g = dev(t_hi, np.float64), dev(gaps, np.int32)
        N.check(lib.orcai_extract_labels_refined(N.ptr(a), N.ptr(c), L, N.ptr(t), R, S, N.ptr(lo), N.ptr(hi), N.ptr(g), *tail), "orcai_extract_labels_refined")
    else:
        N.check(lib.orcai_extract_labels_per_label(N.ptr(a), N.ptr(c), L, N.ptr(t), R, S, N.ptr(lo), *tail), "orcai_extract_labels_per_label")
    torch.cuda.synchronize()
    return runs.cpu().numpy(), offsets.cpu().numpy()


def check(agg, cnt, table, t_lo, t_hi, gaps, limits=None):
    """The kernel against the contract, every byte of the output buffers; returns the runs found."""
    L = agg.shape[1]
    rank = D.label_rank(names_for(L), "*")
    runs, offsets = extract(agg, cnt, table, rank, t_lo, t_hi, gaps, limits)
    want_runs, want_offsets = refined_contract(agg, cnt, table, t_lo, t_hi, gaps, rank, limits, DELTA_T, TPO)
    assert np.array_equal(offsets, want_offsets), (offsets, want_offsets)
    total = int(offsets[-1])
    assert runs[:total].tobytes() == want_runs.tobytes()
    assert (runs[total:] == SENTINEL).all()
    return runs[:total]


def one(S):
    return [(0, 0, S, 0)]


def counts(S):
    c = np.full(S, 2.0)
    c[0] = 1.0  # the maximum, 2, halves every threshold
    return c


def noise_case(S, L, seed):
    rng = np.random.default_rng(seed)
    agg = smoothed(S, L, seed, width=min(5, S))
    agg[rng.random((S, L)) < 0.01] = np.nan
    t_lo = 2 * (0.5 + 0.05 * rng.random(L))
    return agg, t_lo, t_lo + 2 * 0.12 * rng.random(L), rng.integers(0, 6, L)


LIMITS = np.array([[3 * TPO * DELTA_T, 12 * TPO * DELTA_T]] * 64)  # too short below 3 rows, too long above 12: merging moves runs between the three


# ------------------------------------------------------------------ 1. the kernel
@pytest.mark.parametrize("L", [1, 7, 64])
def test_smoothed_noise_equals_the_contract(L):
    changed = 0
    for S in (1, 2, ROW_TILE - 1, ROW_TILE, ROW_TILE + 1, BIG):
        agg, t_lo, t_hi, gaps = noise_case(S, L, seed=1000 * L + S)
        refined = check(agg, counts(S), one(S), t_lo, t_hi, gaps, LIMITS[:L])
        plain = check(agg, counts(S), one(S), t_lo, t_lo, np.zeros(L, dtype=np.int32), LIMITS[:L])
        changed += len(plain) - len(refined)
        if S == BIG:
            assert len(refined) > 50 * L and {0, 1, 2} <= set(refined[:, 3].tolist())
            check(agg, counts(S), one(S), t_lo, t_hi, np.zeros(L, dtype=np.int32))  # hysteresis alone
            check(agg, counts(S), one(S), t_lo, t_lo, gaps)  # merging alone
    assert changed > 50 * L  # refinement removes runs: the comparison above is not one of equal inputs


def test_three_recordings_off_the_tile_edges_and_one_without_rows():
    sizes, L = [300, 0, 215, 700], 7
    table, row = [], 0
    for S in sizes:
        table.append((0, 0, S, row))
        row += S
    agg, t_lo, t_hi, gaps = noise_case(row, L, seed=5)
    cnt = np.full(row, 2.0)
    cnt[300:515] = 1.0  # the third recording's own maximum: its cut is twice the others'
    agg[:2] = 1.5
    for r0 in (300, 515):  # a kept run on either side of every recording edge, one row apart
        agg[r0 - 2 : r0 + 2] = 1.5
    found = check(agg, cnt, table, t_lo, t_hi, gaps, LIMITS[:L])
    assert len(found) > 30
    huge = check(agg, cnt, table, t_lo, t_hi, np.full(L, 2**31 - 1, dtype=np.int32))  # worst case 3: one run per column PER RECORDING
    assert len(huge) == 3 * L and huge[:, 0].tolist().count(0) == 3 * L
    many = [(0, 0, 1, i) for i in range(40)] + [(0, 0, row - 40, 40)]  # R > 1 with one-row recordings: every candidate list entry is a recording
    check(agg, cnt, many, t_lo, t_hi, gaps)


def test_worst_case_1_one_run_as_long_as_the_recording():
    """Column 0: low everywhere, high only in the last row (kept).  Column 1: the same without a high row (dropped).  Column 2: high only in row 0."""
    agg = np.full((BIG, 3), 0.6)
    agg[-1, 0] = agg[0, 2] = 0.9
    runs = check(agg, np.ones(BIG), one(BIG), [0.5] * 3, [0.8] * 3, [0, 7, 7])
    assert runs.tolist() == [[0, BIG - 1, 0, 0], [0, BIG - 1, 2, 0]]


@pytest.mark.parametrize("L", [1, 64])
def test_worst_cases_2_and_4_alternating_columns_become_one_run_each(L):
    for S in (ROW_TILE + 1, BIG):
        agg = np.where(np.arange(S)[:, None] % 2 == 0, 0.9, 0.0) + np.zeros((S, L))
        runs = check(agg, np.ones(S), one(S), [0.5] * L, [0.8] * L, [1] * L)
        assert len(runs) == L and (runs[:, 0] == 0).all() and (runs[:, 1] == (S - 1) // 2 * 2).all()
        if L == 64:  # every second column keeps gap 0: S / 2 runs beside the merged ones, in the order of the label file
            runs = check(agg, np.ones(S), one(S), [0.5] * L, [0.8] * L, [1, 0] * 32)
            assert len(runs) == 32 + 32 * ((S + 1) // 2)


def test_worst_case_5_chains_and_candidates_across_the_tile_and_scan_edges():
    S, L = BIG, 6
    agg = np.zeros((S, L))
    for e in (ROW_TILE, 2 * ROW_TILE, EDGE):
        agg[e - 1, 0] = agg[e + 1, 0] = 0.9  # two kept runs, the gap row is the first of the tile: joined at g = 1
        agg[e - 3 : e, 1] = agg[e + 2 : e + 4, 1] = 0.9  # a gap of 2 rows across the edge: not joined at g = 1
        agg[e - 5 : e + 5, 2] = 0.6  # a candidate across the edge whose only high row is the first of the tile
        agg[e, 2] = 0.9
        agg[e - 5 : e + 5, 3] = 0.6  # the same without a high row: dropped, and it lies in the gap of two kept runs that are joined over it
        agg[e - 9 : e - 7, 3] = agg[e + 7 : e + 9, 3] = 0.9
    agg[::3, 4] = 0.9  # a chain from the first row to the last over every edge
    agg[EDGE - 70 * 3 : EDGE + 70 * 3 : 3, 5] = 0.9  # more than 64 candidates (a keep word) on either side of the scan edge, all one chain
    agg[EDGE + 70 * 3 + 40, 5] = 0.9
    runs = check(agg, np.ones(S), one(S), [0.5] * L, [0.8] * L, [1, 1, 0, 16, 2, 2])
    per_column = [runs[runs[:, 2] == l][:, :2].tolist() for l in range(L)]
    assert per_column[0] == [[e - 1, e + 1] for e in (ROW_TILE, 2 * ROW_TILE, EDGE)]
    assert per_column[1] == sorted([[e - 3, e - 1] for e in (ROW_TILE, 2 * ROW_TILE, EDGE)] + [[e + 2, e + 3] for e in (ROW_TILE, 2 * ROW_TILE, EDGE)])
    assert per_column[2] == [[e - 5, e + 4] for e in (ROW_TILE, 2 * ROW_TILE, EDGE)]
    assert per_column[3] == [[e - 9, e + 8] for e in (ROW_TILE, 2 * ROW_TILE, EDGE)]
    assert per_column[4] == [[0, (S - 1) // 3 * 3]]
    assert per_column[5] == [[EDGE - 210, EDGE + 207], [EDGE + 250, EDGE + 250]]


@pytest.mark.parametrize("L", [1, 7, 64])
def test_identity_writes_the_bytes_of_the_per_label_call(L):
    """high == low and every gap 0, on the same buffers: runs, offsets and the untouched tail."""
    for S in (ROW_TILE + 1, BIG):
        agg, t_lo, _, _ = noise_case(S, L, seed=77 + L)
        rank = D.label_rank(names_for(L), "*")
        plain = extract(agg, counts(S), one(S), rank, t_lo, limits=LIMITS[:L])
        same = extract(agg, counts(S), one(S), rank, t_lo, t_lo, np.zeros(L, dtype=np.int32), limits=LIMITS[:L])
        assert plain[1][-1] > 10 and plain[0].tobytes() == same[0].tobytes() and plain[1].tobytes() == same[1].tobytes()


def test_two_calls_write_the_same_bytes():
    S, L = 3 * ROW_TILE + 9, 33
    agg, t_lo, t_hi, gaps = noise_case(S, L, seed=3)
    rank = D.label_rank(names_for(L), "*")
    a, b = (extract(agg, counts(S), one(S), rank, t_lo, t_hi, gaps, LIMITS[:L]) for _ in range(2))
    assert a[1][-1] > 100 and a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


def test_refusals_launch_nothing():
    S, L, R = 65, 7, 1
    agg, cnt = dev(np.full((S, L), 0.9), np.float64), dev(counts(S), np.float64)
    table = torch.tensor(one(S), dtype=torch.int64, device="cuda")
    rank, lo, hi, gaps = dev(np.arange(L), np.int32), dev([0.5] * L, np.float64), dev([0.6] * L, np.float64), dev([0] * L, np.int32)
    runs = torch.full((L * 33 + 2, 4), SENTINEL, dtype=torch.int32, device="cuda")
    offsets = torch.full((R + 1,), SENTINEL, dtype=torch.int64, device="cuda")
    lib = N.lib()
    size = lib.orcai_extract_labels_refined_workspace_bytes
    need = size(L, R, S)
    assert need > lib.orcai_extract_labels_workspace_bytes(L, R, S) > 0
    assert size(0, R, S) == 0 and size(65, R, S) == 0 and size(L, 0, S) == 0 and size(L, R, 0) == 0 and size(L, R, 2**31) == 0 and size(L, R, 2**31 - 1) > 0
    ws = torch.full((need,), 0x5A, dtype=torch.uint8, device="cuda")
    good = dict(agg=N.ptr(agg), cnt=N.ptr(cnt), L=L, table=N.ptr(table), R=R, S_total=S, thresholds=N.ptr(lo), high_thresholds=N.ptr(hi), gap_rows=N.ptr(gaps),
                label_rank=N.ptr(rank), limits=None, frame_seconds=DELTA_T, tpo=TPO, runs=N.ptr(runs), capacity=L * 33 + 1, offsets=N.ptr(offsets),
                workspace=N.ptr(ws), workspace_bytes=need, stream=N.stream_ptr())
    bad = {f"null {k}": {k: None} for k in ("agg", "cnt", "table", "label_rank", "runs", "offsets", "workspace", "thresholds", "high_thresholds", "gap_rows")}
    bad.update({"L = 0": {"L": 0}, "L = 65": {"L": 65}, "R = 0": {"R": 0}, "S_total = 0": {"S_total": 0}, "capacity < 0": {"capacity": -1}, "tpo = 0": {"tpo": 0},
                "small workspace": {"workspace_bytes": need - 1}, "misaligned runs": {"runs": N.ptr(runs) + 4}, "misaligned workspace": {"workspace": N.ptr(ws) + 16}})
    for name, change in bad.items():
        assert lib.orcai_extract_labels_refined(*{**good, **change}.values()) == N.E_BADARG, name
    for rows in (2**31, 2**39 + 1):  # candidate rows are int32: refused before the (never this large) workspace is touched
        assert lib.orcai_extract_labels_refined(*{**good, "S_total": rows, "workspace_bytes": 2**62}.values()) == N.E_UNSUPPORTED
    torch.cuda.synchronize()
    assert bool((runs == SENTINEL).all()) and bool((offsets == SENTINEL).all()) and bool((ws == 0x5A).all())
    assert lib.orcai_extract_labels_refined(*good.values()) == 0  # and the good call runs
    torch.cuda.synchronize()
    assert int(offsets[1]) == L


def test_extract_labels_device_takes_the_refined_call_only_when_asked(monkeypatch):
    L, S = 7, 600
    agg, t_lo, t_hi, gaps = noise_case(S, L, seed=9)
    calls, cnt = names_for(L), counts(S)
    called = []
    real = N.lib

    class Spy:
        def __getattr__(self, name):
            called.append(name)
            return getattr(real(), name)

    monkeypatch.setattr(D.N, "lib", lambda: Spy())
    args = (torch.from_numpy(agg).cuda(), torch.from_numpy(cnt).cuda(), torch.tensor(one(S), dtype=torch.int64, device="cuda"), 1, calls, "*", TPO, DELTA_T)
    rank = D.label_rank(calls, "*")

    def frame(t_hi_, gaps_):
        runs, _ = refined_contract(agg, cnt, one(S), t_lo, t_hi_, gaps_, rank, None, DELTA_T, TPO)
        return D.labels_frame(runs, calls, "*", TPO, False)[0]

    plain = D.extract_labels_device(*args, thresholds=t_lo).results()[0][0]
    assert called == ["orcai_extract_labels_workspace_bytes", "orcai_extract_labels_per_label"] and plain.equals(frame(t_lo, [0] * L))
    called.clear()
    D.extract_labels_device(*args).results()
    assert called == ["orcai_extract_labels_workspace_bytes", "orcai_extract_labels"]
    for kwargs, want in (({"high_thresholds": t_hi, "gap_rows": gaps}, frame(t_hi, gaps)), ({"high_thresholds": t_hi}, frame(t_hi, [0] * L)),
                         ({"gap_rows": gaps}, frame(t_lo, gaps))):
        called.clear()
        got = D.extract_labels_device(*args, thresholds=t_lo, **kwargs).results()[0][0]
        assert called == ["orcai_extract_labels_refined_workspace_bytes", "orcai_extract_labels_refined"]
        assert got.equals(want) and len(got) < len(plain)


# ------------------------------------------------------------------ 2. end to end
@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    """(model directory, clip paths, options).  The thresholds are quantiles of the 12 s clip's own averaged probabilities (times its maximum count
    of 2: the cut is threshold / max(count)), so about half of its rows are above the low one and a fifth above the high one."""
    from orcai_amd.io import load_orcai_model

    base = tmp_path_factory.mktemp("label_refine")
    model_dir, _ = _model_dir(base)
    paths = _clips(base / "clips")
    model, param, shape = load_orcai_model(model_dir)
    _, agg, delta_t = P.predict_wav(paths[0], 1, model, param, shape)
    calls = param["calls"]
    low = {c: float(2 * np.quantile(agg[:, i], 0.5)) for i, c in enumerate(calls)}
    high = {c: float(2 * np.quantile(agg[:, i], 0.8)) for i, c in enumerate(calls)}
    step = TPO * float(delta_t)
    gap = {c: (1 + i % 3) * step * 1.001 for i, c in enumerate(calls)}  # 1 to 3 output steps
    limits = {"default": [2.5 * step, 30 * step]}
    return model_dir, paths, {"thresholds": low, "high_thresholds": high, "merge_gap": gap}, limits


def _files(folder):
    return {f.name: content(f) for f in sorted(folder.iterdir()) if f.suffix == ".txt"}


def _routes(run, make_folder, options, limits):
    """run(folder, **flags) writes into folder.  The unrefined files once; refined on the host and on the device, with duration limits and without."""
    plain = make_folder()
    run(plain, thresholds=options["thresholds"])
    unrefined = _files(plain)
    assert unrefined
    identity = make_folder()  # the refined code with high = low and no gap: the parent's files
    run(identity, thresholds=options["thresholds"], high_thresholds=options["thresholds"], merge_gap=0.0, device_labels=True)
    assert _files(identity) == unrefined
    for lim in (None, limits):
        host, device = make_folder(), make_folder()
        run(host, call_duration_limits=lim, **options)
        run(device, call_duration_limits=lim, device_labels=True, **options)
        want = _files(host)
        assert _files(device) == want and want.keys() == unrefined.keys()
        if lim is None:
            assert want != unrefined  # refinement really changes the files
            assert sum(b.count(b"\n") for b in want.values()) < sum(b.count(b"\n") for b in unrefined.values())
    return want


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
        P.predict(tmp_path / "table.csv", model_dir=model_dir, output_path=folder, verbosity=0, batch_frames=batch_frames, **flags)

    assert len(_routes(run, _folders(tmp_path), options, limits)) == 4


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

    assert len(_routes(run, _folders(tmp_path, link=wav), options, limits)) == 3
