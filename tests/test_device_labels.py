"""The host half of the device label extraction, without a GPU: the label order and the duration limits are resolved as the host route
resolves them per interval, and the DataFrame assembled from the kernel's output contract -- restated here in numpy (`contract`) -- equals the
host route's (compute_binary_predictions + compute_labels + filter_predictions) exactly: DataFrame.equals, equal column lists, equal counts."""

import json

import numpy as np
import pandas as pd
import pytest

from orcai_amd import _native as N
from orcai_amd import device_labels as D
from orcai_amd import predict as P
from orcai_amd.auxiliary import Messenger

CALLS = ["BR", "BUZZ", "HERDING", "PHS", "SS", "TAILSLAP", "WHISTLE"]
QUIET = Messenger(verbosity=0)
DELTA_T = 256 / 48000
TPO = 16


def contract(agg, cnt, table, threshold, rank, limits, frame_seconds, tpo):
    """orcai_extract_labels as include/orcai_hip.h states it: (runs int32 [n][4], offsets int64 [R + 1])."""
    runs, offsets = [], [0]
    for _, _, S, row in table:
        found = []
        c = cnt[row : row + S]
        if S > 0 and (np.isnan(c).any() or c.max() != 0):
            thr = np.float64(threshold) / c.max()
            b = (agg[row : row + S] > thr).astype(np.int8)  # strict; NaN compares false
            for l in range(agg.shape[1]):
                d = np.diff(b[:, l], prepend=0, append=0)
                found += [(int(s), int(e), l) for s, e in zip(np.where(d == 1)[0], np.where(d == -1)[0] - 1)]
        found.sort(key=lambda t: (t[0], t[1], int(rank[t[2]]), t[2]))
        for s, e, l in found:
            status = 0
            if limits is not None:
                d = np.float64((e - s) * tpo) * np.float64(frame_seconds)
                status = 1 if d < limits[l, 0] else 2 if d > limits[l, 1] else 0
            runs.append((s, e, l, status))
        offsets.append(len(runs))
    return np.array(runs, dtype=np.int32).reshape(-1, 4), np.array(offsets, dtype=np.int64)


def host_route(agg, cnt, calls, suffix, limits=None, delta_t=DELTA_T, tpo=TPO):
    """(table, n_too_short, n_too_long) of the existing host route; with limits the table is what filter_predictions returns."""
    with np.errstate(divide="ignore", invalid="ignore"):
        s, e, n = P.compute_binary_predictions(agg, cnt, calls, threshold=0.5)
    frame = P.compute_labels(s, e, n, tpo, suffix)
    if limits is None:
        return frame, 0, 0
    kept = P.filter_predictions(frame, delta_t=delta_t, call_duration_limits=limits, label_suffix=suffix, msgr=QUIET)
    ok = frame["duration_ok"] if len(frame) else pd.Series([], dtype=object)
    return kept, int((ok == "too short").sum()), int((ok == "too long").sum())


def same(a: pd.DataFrame, b: pd.DataFrame) -> bool:
    return a.equals(b) and list(a.columns) == list(b.columns) and list(a.dtypes) == list(b.dtypes) and a.index.equals(b.index)


def test_symbols_are_bound():
    assert len(N._SIGNATURES["orcai_extract_labels"][1]) == 17 and N._SIGNATURES["orcai_extract_labels_workspace_bytes"][1] == [N.C.c_int, N.C.c_int, N.c_i64]


@pytest.mark.parametrize("calls,suffix", [(["A", "AB"], "~"), (["A", "AB"], "*"), (["AB", "A"], "~"), (["b", "a", "b", "B", "a"], "*"), (CALLS, None), (CALLS, ""),
                                          (["x*", "x", "x*y"], "*")])
def test_label_rank_is_the_stable_string_order_of_the_suffixed_names(calls, suffix):
    rank = D.label_rank(calls, suffix)
    assert rank.dtype == np.int32 and sorted(rank) == list(range(len(calls)))
    # one interval per label, all at the same start and stop, through the host's own sort
    frame = P.compute_labels([3] * len(calls), [5] * len(calls), list(calls), TPO, suffix)
    names = D.suffixed_names(calls, suffix)
    by_rank = [names[i] for i in np.argsort(rank, kind="stable")]
    assert list(frame["label"]) == by_rank
    for i in range(len(calls)):  # duplicates keep the label index order
        for j in range(i + 1, len(calls)):
            if names[i] == names[j]:
                assert rank[i] < rank[j]
    if calls == ["A", "AB"]:
        assert list(rank) == ([1, 0] if suffix == "~" else [0, 1])  # "AB~" < "A~", but "A*" < "AB*"


LIMIT_CASES = [
    {"BR": [0.1, 0.5], "default": [0.05, None], "SS": [None, 0.2]},
    {"BR": [None, None], "WHISTLE": [0.3, 1.0]},  # no default: the others are 0 .. inf
    {"default": [0.25, 0.75]},
    {},
]


@pytest.mark.parametrize("limits", LIMIT_CASES)
@pytest.mark.parametrize("suffix", ["*", "~", "", None, "S"])
def test_limits_resolve_as_check_duration_looks_them_up(limits, suffix):
    got = D.resolve_limits(CALLS, suffix, limits)
    assert got.shape == (7, 2) and got.dtype == np.float64
    for i, name in enumerate(D.suffixed_names(CALLS, suffix)):
        for frames in (0, 1, 9, 10, 37, 38, 56, 57, 93, 94, 140, 141, 187, 188, 10**6):  # around 0.05, 0.2, 0.3, 0.5, 0.75, 1.0 s
            verdict = P._check_duration(pd.Series({"label": name, "duration": frames}), limits, DELTA_T, suffix if suffix is not None else "None")
            d = np.float64(frames) * DELTA_T
            mine = "too short" if d < got[i, 0] else "too long" if d > got[i, 1] else "keep"
            assert mine == verdict, (name, frames, got[i])
    assert np.array_equal(D.resolve_limits(["SS"], "S", {"": [1, 2], "default": [3, 4]}), [[1.0, 2.0]])  # every occurrence of the suffix goes


def test_limits_from_a_json_file(tmp_path):
    path = tmp_path / "limits.json"
    path.write_text(json.dumps(LIMIT_CASES[0]))
    assert np.array_equal(D.resolve_limits(CALLS, "*", path), D.resolve_limits(CALLS, "*", LIMIT_CASES[0]))
    assert np.array_equal(D.resolve_limits(CALLS, "*", P.DEFAULT_CALL_DURATION_LIMITS).shape, (7, 2))


@pytest.fixture(scope="module")
def golden(golden_dir):
    g = np.load(golden_dir / "labels_crafted.npz")
    return g["aggregated"], g["overlap_count"]


def _frames(agg, cnt, table, calls, suffix, limits):
    lim = None if limits is None else D.resolve_limits(calls, suffix, limits)
    runs, offsets = contract(agg, cnt, table, 0.5, D.label_rank(calls, suffix), lim, DELTA_T, TPO)
    return [D.labels_frame(runs[offsets[r] : offsets[r + 1]], calls, suffix, TPO, limits is not None) for r in range(len(table))]


@pytest.mark.parametrize("limits", [None] + LIMIT_CASES)
@pytest.mark.parametrize("suffix", ["*", "~", "", None])
def test_frame_from_the_contract_equals_the_host_route_on_the_golden_matrix(golden, suffix, limits):
    agg, cnt = golden
    (frame, n_short, n_long), = _frames(agg, cnt, [(0, 0, len(cnt), 0)], CALLS, suffix, limits)
    want, w_short, w_long = host_route(agg, cnt, CALLS, suffix, limits)
    assert same(frame, want) and (n_short, n_long) == (w_short, w_long)
    assert len(want) + n_short + n_long >= 5
    if limits == LIMIT_CASES[0]:
        assert n_short > 0 and n_long > 0


def test_ragged_random_matrix_with_duplicate_names_and_equal_keys():
    rng = np.random.default_rng(5)
    calls = ["b", "a", "b", "B", "a"]
    sizes = [46, 0, 1, 69, 46, 0]
    table, row = [], 0
    for S in sizes:
        table.append((0, 0, S, row))
        row += S
    agg = np.repeat(rng.random((row // 3 + 1, 5)), 3, axis=0)[:row]  # runs of three rows: equal starts and stops across labels
    agg[rng.random(agg.shape) < 0.02] = np.nan
    cnt = np.full(row, 2.0)
    cnt[46:47] = 1.0  # the one-row recording: threshold 0.5
    for limits in (None, {"a": [0.05, 0.2], "default": [None, 0.1]}):
        frames = _frames(agg, cnt, table, calls, "*", limits)
        for (_, _, S, r0), (frame, n_short, n_long) in zip(table, frames):
            if S == 0:
                want, w = (P.compute_labels([], [], [], TPO, "*"), (0, 0))
                if limits is not None:
                    want = P.filter_predictions(want, DELTA_T, limits, "*", msgr=QUIET)
            else:
                want, *w = host_route(agg[r0 : r0 + S], cnt[r0 : r0 + S], calls, "*", limits)
            assert same(frame, want) and (n_short, n_long) == tuple(w), (S, r0)
    assert sum(len(f[0]) for f in _frames(agg, cnt, table, calls, "*", None)) > 40


def test_empty_input_gives_the_host_routes_empty_tables():
    agg, cnt = np.zeros((46, 7)), np.full(46, 2.0)
    for limits in (None, LIMIT_CASES[0]):
        (frame, n_short, n_long), = _frames(agg, cnt, [(0, 0, 46, 0)], CALLS, "*", limits)
        want, w_short, w_long = host_route(agg, cnt, CALLS, "*", limits)
        assert len(frame) == 0 and same(frame, want) and (n_short, n_long) == (0, 0) == (w_short, w_long)


def test_cli_has_the_flag():
    from click.testing import CliRunner

    from orcai_amd.cli import cli

    out = CliRunner().invoke(cli, ["predict", "--help"]).output
    assert "--device-labels" in out
    import inspect

    assert inspect.signature(P.predict).parameters["device_labels"].default is False
    assert inspect.signature(P.predict_wavs).parameters["device_labels"].default is False
