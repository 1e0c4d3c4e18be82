"""A score for every detected interval, without a GPU.

The host twin (orcai_amd/scores.py: column operations) against `oracle`, a deliberately slow restatement: a Python loop per interval with max, the first
index that attains it, and math.fsum of the clamped rows.  peak and peak_frame must be equal; the mean may differ from the exact one by 2**-32 (2**-33
is the contract's bound on the fixed-point mean, the rest covers the final f64 division and fsum's own rounding).  `scored_contract` -- the three fields
orcai_interval_scores writes, from the host twin -- is shared with test_interval_scores_gpu.
"""

import inspect
import math

import numpy as np
import pandas as pd
import pytest
from test_label_refine import CALLS, DELTA_T, TPO, host, names_for, refined_contract, smoothed

from orcai_amd import predict as P
from orcai_amd import scores as Z
from orcai_amd.device_labels import label_rank, labels_frame

MEAN_BOUND = 2.0**-32


def oracle(agg, start_row, stop_row, label):
    """(peak, peak_row, exact mean of the clamped rows) of one interval.  A loop over its rows, on purpose."""
    rows = [float(agg[s, label]) for s in range(start_row, stop_row + 1)]
    seen = [v for v in rows if not math.isnan(v)]
    peak = max(seen)
    peak_row = start_row + rows.index(peak)
    clamped = [0.0 if math.isnan(v) else min(max(v, 0.0), 1.0) for v in rows]
    return peak, peak_row, math.fsum(clamped) / len(rows)


def scored_contract(agg, table, runs, offsets):
    """orcai_interval_scores' output for the runs of an extraction call: int64 words [n][3] = {peak bits, sum_q32 bits, peak_row}."""
    out = np.zeros((len(runs), 3), dtype=np.int64)
    for r, (_, _, S, row) in enumerate(table):
        a, b = int(offsets[r]), int(offsets[r + 1])
        peak, sums, rows = Z.interval_scores(agg[row : row + S], runs[a:b, 0], runs[a:b, 1], runs[a:b, 2])
        out[a:b, 0], out[a:b, 1], out[a:b, 2] = peak.view(np.int64), sums.view(np.int64), rows
    return out


def check_against_oracle(agg, runs):
    """The twin against the oracle for runs int [n][>=3] = {start_row, stop_row, label} of one recording; returns the score columns."""
    peak, sums, rows = Z.interval_scores(agg, runs[:, 0], runs[:, 1], runs[:, 2])
    assert peak.dtype == np.float64 and sums.dtype == np.uint64 and rows.dtype == np.int64
    n_rows = runs[:, 1].astype(np.int64) - runs[:, 0] + 1
    columns = Z.score_columns(peak, sums, rows, n_rows, TPO)
    for i, (s, e, l) in enumerate(runs[:, :3].tolist()):
        want_peak, want_row, want_mean = oracle(agg, s, e, l)
        assert columns["peak"][i] == want_peak and columns["peak_frame"][i] == want_row * TPO, (i, s, e, l)
        assert abs(columns["mean"][i] - want_mean) <= MEAN_BOUND, (i, columns["mean"][i], want_mean)
        assert int(sums[i]) == sum(int(q) for q in Z.q32(agg[s : e + 1, l]))  # Python integers: no wrap, no order
    return columns


def noise_runs(S, L, seed, gaps=None):
    """Smoothed noise scaled into [0, 1.2] (so some rows clamp), NaN sprinkled in, and the runs the refined contract finds in it."""
    rng = np.random.default_rng(seed)
    agg = 1.2 * smoothed(S, L, seed)
    agg[rng.random((S, L)) < 0.01] = np.nan
    cnt = np.ones(S)
    t_lo = 0.6 + 0.05 * rng.random(L)
    t_hi = t_lo + 0.1 * rng.random(L)
    gaps = rng.integers(0, 6, L) if gaps is None else gaps
    runs, _ = refined_contract(agg, cnt, [(0, 0, S, 0)], t_lo, t_hi, gaps, label_rank(names_for(L), "*"), None, DELTA_T, TPO)
    return agg, runs


# ------------------------------------------------------------------ the twin against the oracle
@pytest.mark.parametrize("L,seed", [(1, 21), (7, 22), (64, 23)])
def test_smoothed_noise_equals_the_oracle(L, seed):
    agg, runs = noise_runs(700, L, seed)
    assert len(runs) > 5 * L
    nan_inside = sum(bool(np.isnan(agg[s : e + 1, l]).any()) for s, e, l, _ in runs.tolist())
    clamped = sum(bool((agg[s : e + 1, l] > 1).any()) for s, e, l, _ in runs.tolist())
    assert nan_inside >= 1 and clamped >= 1, (nan_inside, clamped)  # a seed that shows neither fails
    columns = check_against_oracle(agg, runs)
    assert columns["peak"].dtype == np.float64 and columns["peak_frame"].dtype == np.int64 and columns["mean"].dtype == np.float64


def test_equal_maxima_go_to_the_earlier_row():
    agg = np.array([0.1, 0.7, 0.9, 0.3, 0.9, 0.9, 0.2, 0.9])[:, None]
    runs = np.array([[0, 7, 0], [3, 7, 0], [5, 6, 0], [0, 1, 0], [6, 6, 0]])
    peak, _, rows = Z.interval_scores(agg, runs[:, 0], runs[:, 1], runs[:, 2])
    assert rows.tolist() == [2, 4, 5, 1, 6] and peak.tolist() == [0.9, 0.9, 0.9, 0.7, 0.2]
    check_against_oracle(agg, runs)


def test_values_of_exactly_zero_and_one_and_outside():
    agg = np.array([[0.0, 1.0, 1.0], [1.0, 1.0, -0.5], [0.0, 1.0, 1.5], [2.0**-33, 1.0, 0.25]])
    runs = np.array([[0, 3, 0], [0, 3, 1], [0, 3, 2], [0, 0, 0], [3, 3, 0]])
    peak, sums, rows = Z.interval_scores(agg, runs[:, 0], runs[:, 1], runs[:, 2])
    assert peak.tolist() == [1.0, 1.0, 1.5, 0.0, 2.0**-33] and rows.tolist() == [1, 0, 2, 0, 3]  # the peak is the value itself, unclamped
    assert sums.tolist() == [2**32, 4 * 2**32, 2**32 + 2**32 + 2**30, 0, 0]  # 2**-33 * 2**32 = 0.5 rounds to the even 0; -0.5 -> 0, 1.5 -> 1
    assert Z.q32(np.array([1.5 * 2.0**-32, 2.5 * 2.0**-32, np.nan, -1.0, 7.0])).tolist() == [2, 2, 0, 0, 2**32]  # round-half-even
    check_against_oracle(agg, runs)


def test_a_nan_inside_a_merged_gap_is_skipped_and_counts_as_a_row():
    text = "..XnX...XnnX"
    agg = np.array([{".": 0.1, "X": 0.9, "n": np.nan}[c] for c in text])[:, None]
    assert host(agg, np.ones(len(text)), ["a"], [0.5], [0.8], [2]) == [(2, 4, 0), (8, 11, 0)]
    runs = np.array([[2, 4, 0], [8, 11, 0]])
    columns = check_against_oracle(agg, runs)
    assert columns["peak"].tolist() == [0.9, 0.9] and columns["peak_frame"].tolist() == [2 * TPO, 8 * TPO]
    assert abs(columns["mean"][0] - 0.6) <= MEAN_BOUND and abs(columns["mean"][1] - 0.45) <= MEAN_BOUND  # the NaN rows are rows of the interval
    only_nan = Z.interval_scores(agg, [3], [3], [0])  # no extraction call produces it; the contract stays defined
    assert np.isnan(only_nan[0][0]) and only_nan[1].tolist() == [0] and only_nan[2].tolist() == [-1]


def test_an_empty_table_keeps_the_dtypes():
    peak, sums, rows = Z.interval_scores(np.zeros((5, 2)), [], [], [])
    assert (peak.dtype, sums.dtype, rows.dtype) == (np.float64, np.uint64, np.int64) and len(peak) == len(sums) == len(rows) == 0
    empty = P.compute_labels([], [], [], TPO, "*")
    got = Z.add_scores(empty, np.zeros((5, 2)), ["a", "b"], "*", TPO)
    assert list(got.columns) == ["start", "stop", "label", "peak", "peak_frame", "mean"] and len(got) == 0
    assert got["peak"].dtype == np.float64 and got["peak_frame"].dtype == np.int64 and got["mean"].dtype == np.float64
    assert got[["start", "stop", "label"]].equals(empty) and list(empty.columns) == ["start", "stop", "label"]  # the input is not touched
    frame, _, _ = labels_frame(np.zeros((0, 4), dtype=np.int32), ["a", "b"], "*", TPO, False, scores=np.zeros((0, 3), dtype=np.int64))
    assert list(frame.columns) == list(got.columns) and [frame[c].dtype for c in Z.SCORE_COLUMNS] == [got[c].dtype for c in Z.SCORE_COLUMNS]


def test_the_refined_contract_with_gaps_three_recordings():
    sizes, L = [300, 0, 215, 700], 7
    table, row = [], 0
    for S in sizes:
        table.append((0, 0, S, row))
        row += S
    rng = np.random.default_rng(31)
    agg = smoothed(row, L, 31)
    agg[rng.random((row, L)) < 0.01] = np.nan
    t_lo = 0.5 + 0.05 * rng.random(L)
    runs, offsets = refined_contract(agg, np.ones(row), table, t_lo, t_lo + 0.1 * rng.random(L), rng.integers(1, 6, L), label_rank(names_for(L), "*"), None,
                                     DELTA_T, TPO)
    words = scored_contract(agg, table, runs, offsets)
    assert len(runs) > 30 and offsets[1] == offsets[2]
    for r, (_, _, S, first) in enumerate(table):
        a, b = int(offsets[r]), int(offsets[r + 1])
        columns = check_against_oracle(agg[first : first + S], runs[a:b])
        assert columns["peak"].to_numpy().tobytes() == words[a:b, 0].tobytes() and (columns["peak_frame"] == words[a:b, 2] * TPO).all()


def test_a_run_of_two_to_the_twenty_ones_sums_to_two_to_the_fifty_two():
    S = 2**20
    agg = np.ones((S + 2, 1))
    agg[0] = agg[-1] = 0.25
    peak, sums, rows = Z.interval_scores(agg, [1, 0], [S, S + 1], [0, 0])
    assert int(sums[0]) == 2**52 and int(sums[1]) == 2**52 + 2**31 and rows.tolist() == [1, 1] and peak.tolist() == [1.0, 1.0]
    assert Z.score_columns(peak, sums, rows, np.array([S, S + 2]), TPO)["mean"][0] == 1.0


def test_wrapped_prefix_sums_still_give_exact_differences():
    """2**33 rows of ones would wrap the uint64 prefix; the same arithmetic on a prefix that starts near 2**64 shows the difference survives."""
    q = Z.q32(np.ones(8))
    prefix = np.cumsum(np.concatenate([[np.uint64(2**64 - 3 * 2**32)], q]).astype(np.uint64))
    assert int(prefix[-1]) == 5 * 2**32 and int((prefix[8:] - prefix[:1])[0]) == 8 * 2**32


# ------------------------------------------------------------------ tables and files
def test_add_scores_and_the_duration_filter_keep_every_row_its_own_scores():
    agg, runs = noise_runs(400, 7, 41)
    frame = labels_frame(runs, CALLS, "*", TPO, False)[0]
    scored = Z.add_scores(frame, agg, CALLS, "*", TPO)
    assert scored[["start", "stop", "label"]].equals(frame) and list(frame.columns) == ["start", "stop", "label"]
    words = scored_contract(agg, [(0, 0, 400, 0)], runs, [0, len(runs)])
    device = labels_frame(runs, CALLS, "*", TPO, False, scores=words)[0]
    assert device.equals(scored)  # the device route's frame from the same three fields
    limits = {"default": [3 * TPO * DELTA_T, 12 * TPO * DELTA_T]}
    kept = P.filter_predictions(scored.copy(), DELTA_T, limits, verbosity=0)
    assert 0 < len(kept) < len(scored) and kept[Z.SCORE_COLUMNS].equals(scored.loc[kept.index, Z.SCORE_COLUMNS])
    assert kept[["start", "stop", "label"]].equals(P.filter_predictions(frame.copy(), DELTA_T, limits, verbosity=0)[["start", "stop", "label"]])


def test_the_score_file_and_the_label_file(tmp_path):
    agg, runs = noise_runs(400, 7, 42)
    scored = Z.add_scores(labels_frame(runs, CALLS, "*", TPO, False)[0], agg, CALLS, "*", TPO)
    plain, with_scores = tmp_path / "plain_predicted.txt", tmp_path / "rec_predicted.txt"
    P.save_predictions(scored[["start", "stop", "label"]], plain, DELTA_T)
    P._save_recording((scored, agg, DELTA_T), with_scores, {"calls": CALLS}, scores=True)
    assert with_scores.read_bytes() == plain.read_bytes()  # three columns, the same bytes
    lines = (tmp_path / "rec_predicted_scores.csv").read_text().split("\n")
    assert lines[0].split("\t") == ["start", "stop", "label", "peak_time", "peak", "mean"] and lines[-1] == "" and len(lines) == len(scored) + 2
    labels = plain.read_text().split("\n")
    for line, label_line, (_, row) in zip(lines[1:-1], labels[1:-1], scored.iterrows()):
        cells = line.split("\t")
        assert "\t".join(cells[:3]) == label_line
        assert float(cells[3]) == round(row["peak_frame"] * DELTA_T, 4) and float(cells[4]) == round(row["peak"], 6) and float(cells[5]) == round(row["mean"], 6)
        assert float(cells[0]) <= float(cells[3]) <= float(cells[1])
    P._save_recording((scored, agg, DELTA_T), tmp_path / "off_predicted.txt", {"calls": CALLS})
    assert not (tmp_path / "off_predicted_scores.csv").exists()


def test_the_overwrite_check_covers_the_score_file(tmp_path):
    wav = tmp_path / "a.wav"
    param = {"name": "m"}
    out = P._checked_output_path(wav, 1, param, "default", False, scores=True)
    assert out == tmp_path / "a_c1_m_predicted.txt"
    (tmp_path / "a_c1_m_predicted_scores.csv").write_text("")
    assert P._checked_output_path(wav, 1, param, "default", False) == out  # without the option the file is nobody's business
    with pytest.raises(FileExistsError, match="_scores.csv"):
        P._checked_output_path(wav, 1, param, "default", False, scores=True)
    assert P._checked_output_path(wav, 1, param, "default", True, scores=True) == out


# ------------------------------------------------------------------ the option
def test_cli_and_label_spec_carry_the_option(tmp_path, monkeypatch):
    from click.testing import CliRunner

    from orcai_amd.cli import cli

    assert "--scores" in CliRunner().invoke(cli, ["predict", "--help"]).output
    for f in (P.predict, P.predict_wav, P.predict_wavs, P.label_spec):
        assert inspect.signature(f).parameters["scores"].default is False
    assert P.label_spec({"calls": CALLS})["scores"] is False and P.label_spec({"calls": CALLS}, scores=True)["scores"] is True
    seen = {}
    monkeypatch.setattr(P, "predict", lambda **kwargs: seen.update(kwargs))
    wav = tmp_path / "a.wav"
    wav.write_bytes(b"")
    assert CliRunner().invoke(cli, ["predict", str(wav), "--scores", "-v", "0"]).exit_code == 0 and seen["scores"] is True
    seen.clear()
    assert CliRunner().invoke(cli, ["predict", str(wav), "-v", "0"]).exit_code == 0 and seen["scores"] is False


def test_the_host_route_adds_the_columns_only_when_asked():
    agg, _ = noise_runs(300, 7, 43)
    agg = np.nan_to_num(agg, nan=0.0)
    state = {"pending": (agg, np.ones(300)), "delta_t": DELTA_T, "orcai_parameter": {"calls": CALLS, "model": {"filters": [1, 2, 3, 4]}}}
    plain, _, _ = P.predict_wav_finish(state)
    scored, _, _ = P.predict_wav_finish(state, scores=True)
    assert list(plain.columns) == ["start", "stop", "label"] and len(plain) > 10
    assert list(scored.columns) == ["start", "stop", "label"] + Z.SCORE_COLUMNS and scored[["start", "stop", "label"]].equals(plain)
    rows = pd.DataFrame({"s": scored["start"] // TPO, "e": scored["stop"] // TPO, "l": [CALLS.index(n[:-1]) for n in scored["label"]]}).to_numpy()
    columns = check_against_oracle(agg, rows)
    assert columns.equals(scored[Z.SCORE_COLUMNS].reset_index(drop=True))
