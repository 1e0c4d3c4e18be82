"""Hysteresis thresholds and gap merging in label extraction, without a GPU.

The numpy contract behind compute_binary_predictions(high_threshold=, merge_gap_rows=) against `naive`, a deliberately slow restatement: Python loops
over the rows build the candidates, look for a hi row in each, and walk the chains.  Hand-written cases for every clause, seeded smoothed noise for
L in {1, 7, 64} (with the phenomena asserted on the naive result, so a seed that shows nothing fails), the seconds-to-steps conversion, the
resolver's errors, the CLI, and the defaults.  `refined_contract` -- orcai_extract_labels_refined's output, from the host route -- is shared with
test_label_refine_gpu.
"""

import inspect
import json

import numpy as np
import pandas as pd
import pytest

from orcai_amd import predict as P
from orcai_amd import refine as F
from orcai_amd import threshold_sweep as W

CALLS = ["BR", "BUZZ", "HERDING", "PHS", "SS", "TAILSLAP", "WHISTLE"]
DELTA_T = 256 / 48000
TPO = 16


def names_for(L):
    return [f"n{(i * 37 + 5) % 64:02d}" for i in range(L)]


def naive(agg, cnt, t_lo, t_hi, gaps):
    """One recording: ([(start, stop, label)] label by label, {"dropped", "longest_chain", "untouched"}).  Loops over rows, on purpose."""
    S, L = agg.shape
    out, stats = [], {"dropped": 0, "longest_chain": 0, "untouched": 0}
    if S == 0:
        return out, stats
    top = np.max(cnt)
    if top == 0:
        return out, stats
    for l in range(L):
        lo = [bool(agg[s, l] > np.float64(t_lo[l]) / top) for s in range(S)]
        hi = [bool(agg[s, l] > np.float64(t_hi[l]) / top) for s in range(S)]
        candidates, s = [], 0
        while s < S:
            if not lo[s]:
                s += 1
                continue
            e = s
            while e + 1 < S and lo[e + 1]:
                e += 1
            keep = False
            for i in range(s, e + 1):
                keep = keep or (lo[i] and hi[i])
            candidates.append((s, e, keep))
            s = e + 1
        kept = [(s, e) for s, e, keep in candidates if keep]
        stats["dropped"] += len(candidates) - len(kept)
        i = 0
        while i < len(kept):
            start, stop = kept[i]
            j = i
            while j + 1 < len(kept) and kept[j + 1][0] - stop - 1 <= gaps[l]:
                j += 1
                stop = kept[j][1]
            out.append((start, stop, l))
            stats["longest_chain"] = max(stats["longest_chain"], j - i + 1)
            stats["untouched"] += j == i
            i = j + 1
    return out, stats


def host(agg, cnt, calls, t_lo, t_hi=None, gaps=None):
    """compute_binary_predictions' answer as [(start, stop, label index)]."""
    with np.errstate(divide="ignore", invalid="ignore"):
        starts, stops, names = P.compute_binary_predictions(agg, cnt, calls, threshold=t_lo, high_threshold=t_hi, merge_gap_rows=gaps)
    assert len(set(calls)) == len(calls)
    return [(int(s), int(e), calls.index(n)) for s, e, n in zip(starts, stops, names)]


def refined_contract(agg, cnt, table, t_lo, t_hi, gaps, rank, limits, frame_seconds, tpo):
    """orcai_extract_labels_refined as include/orcai_hip.h states it, from the host route per recording: (runs int32 [n][4], offsets int64 [R + 1])."""
    calls = [str(i) for i in range(agg.shape[1])]
    runs, offsets = [], [0]
    for _, _, S, row in table:
        found = host(agg[row : row + S], cnt[row : row + S], calls, t_lo, t_hi, gaps) if S > 0 else []
        found.sort(key=lambda t: (t[0], t[1], int(rank[t[2]]), t[2]))
        for s, e, l in found:
            status = 0
            if limits is not None:
                d = np.float64((e - s) * tpo) * np.float64(frame_seconds)
                status = 1 if d < limits[l, 0] else 2 if d > limits[l, 1] else 0
            runs.append((s, e, l, status))
        offsets.append(len(runs))
    return np.array(runs, dtype=np.int32).reshape(-1, 4), np.array(offsets, dtype=np.int64)


def column(text):
    """One column from a string: '.' below both thresholds, 'o' between them, 'X' above both, 'n' NaN.  Thresholds 0.5 / 0.8 at a count of 1."""
    return np.array([{".": 0.1, "o": 0.6, "X": 0.9, "n": np.nan}[c] for c in text], dtype=np.float64)[:, None]


def runs_of(text, gap=0, t_lo=0.5, t_hi=0.8, cnt=None):
    agg = column(text)
    cnt = np.ones(len(text)) if cnt is None else cnt
    got = host(agg, cnt, ["a"], [t_lo], [t_hi], [gap])
    assert got == naive(agg, cnt, [t_lo], [t_hi], [gap])[0]
    return [(s, e) for s, e, _ in got]


# ------------------------------------------------------------------ hand-written cases
def test_hysteresis_keeps_a_candidate_iff_it_reaches_the_high_threshold():
    assert runs_of("..ooo..oXo..X..o.") == [(7, 9), (12, 12)]
    assert runs_of("ooooooooX") == [(0, 8)] and runs_of("Xoooooooo") == [(0, 8)]  # the only hi row at either end
    assert runs_of("ooooooooo") == [] and runs_of(".........") == []
    assert runs_of("X") == [(0, 0)] and runs_of("o") == [] and runs_of(".") == []


def test_equal_thresholds_make_hysteresis_the_identity():
    text = "..ooo..oXo..X..o."
    assert runs_of(text, t_hi=0.5) == [(2, 4), (7, 9), (12, 12), (15, 15)]
    agg = column(text)
    assert host(agg, np.ones(len(text)), ["a"], [0.5], [0.5], [0]) == host(agg, np.ones(len(text)), ["a"], [0.5])


def test_high_counts_only_where_low_is_set():
    """t_hi below t_lo (the resolver refuses it; the contract stays defined): hi rows outside a candidate keep nothing and start nothing."""
    assert runs_of("..ooo..X.", t_lo=0.8, t_hi=0.5) == [(7, 7)]


def test_a_gap_of_exactly_g_is_bridged_and_g_plus_one_is_not():
    assert runs_of("X..X...X", gap=2) == [(0, 3), (7, 7)]
    assert runs_of("X..X...X", gap=3) == [(0, 7)]
    assert runs_of("X..X...X", gap=1) == [(0, 0), (3, 3), (7, 7)]
    assert runs_of("X.X", gap=1) == [(0, 2)]


def test_a_gap_of_zero_is_the_identity():
    assert runs_of("X.X..XX.X", gap=0) == [(0, 0), (2, 2), (5, 6), (8, 8)]
    agg = column("X.X..XoX.o")
    assert host(agg, np.ones(10), ["a"], [0.5], None, [0]) == host(agg, np.ones(10), ["a"], [0.5])


def test_joining_is_transitive():
    assert runs_of("X.X.X.X.X.X", gap=1) == [(0, 10)]
    assert runs_of("X.X.X..X.X", gap=1) == [(0, 4), (7, 9)]


def test_a_dropped_candidate_inside_a_bridged_gap_does_not_prevent_the_join():
    assert runs_of("XX.oo.XX", gap=4) == [(0, 7)]
    assert runs_of("XX.oo.XX", gap=3) == [(0, 1), (6, 7)]  # the gap is measured between the KEPT runs: 4 rows
    assert runs_of("XX.oo.XX", gap=4, t_hi=0.5) == [(0, 7)]
    assert runs_of("oo.XX.oo", gap=4) == [(3, 4)]  # dropped candidates are not revived by a neighbour


def test_nan_rows_are_below_both_thresholds():
    assert runs_of("XnX", gap=0) == [(0, 0), (2, 2)] and runs_of("XnX", gap=1) == [(0, 2)]
    assert runs_of("onX") == [(2, 2)] and runs_of("nnn") == []


def test_a_zero_or_nan_count_maximum_gives_no_runs():
    assert runs_of("XXoX", cnt=np.zeros(4)) == []
    assert runs_of("XXoX", t_lo=-1.0, t_hi=-1.0, cnt=np.zeros(4)) == []  # -1 / 0 = -inf would make everything a one
    assert runs_of("XXoX", cnt=np.array([1.0, np.nan, 1.0, 1.0])) == []
    assert runs_of("X.oX", cnt=np.array([1.0, 0.0, 2.0, 1.0])) == [(0, 0), (2, 3)]  # only the maximum counts: cut at 0.25 / 0.4, 0.6 is a hi row too
    assert host(np.zeros((0, 1)), np.zeros(0), ["a"], [0.5], [0.8], [1]) == []


def test_runs_of_different_recordings_are_never_joined():
    """The contract works per recording; the last run of one and the first of the next stay apart whatever the gap."""
    text = "X.XX" + "X.X"
    agg, cnt = column(text), np.ones(7)
    table = [(0, 0, 4, 0), (0, 0, 0, 4), (0, 0, 3, 4)]
    runs, offsets = refined_contract(agg, cnt, table, [0.5], [0.8], [100], [0], None, DELTA_T, TPO)
    assert offsets.tolist() == [0, 1, 1, 2] and runs.tolist() == [[0, 3, 0, 0], [0, 2, 0, 0]]
    want = []
    for _, _, S, row in table:
        want += [(s, e) for s, e, _ in naive(agg[row : row + S], cnt[row : row + S], [0.5], [0.8], [100])[0]]
    assert want == [(0, 3), (0, 2)]


def test_labels_have_their_own_thresholds_and_gaps():
    agg = np.hstack([column("X.X..oXo"), column("X.X..oXo"), column("X.X..oXo")])
    got = host(agg, np.ones(8), ["a", "b", "c"], [0.5, 0.5, 0.7], [0.5, 0.95, 0.8], [1, 5, 10])
    assert got == [(0, 2, 0), (5, 7, 0), (0, 6, 2)] == naive(agg, np.ones(8), [0.5, 0.5, 0.7], [0.5, 0.95, 0.8], [1, 5, 10])[0]
    scalar = host(agg, np.ones(8), ["a", "b", "c"], 0.5, 0.8, 2)  # scalars stand for every label
    assert scalar == host(agg, np.ones(8), ["a", "b", "c"], [0.5] * 3, [0.8] * 3, [2] * 3) == [(0, 7, l) for l in range(3)]
    with pytest.raises(ValueError, match="one per label"):
        P.compute_binary_predictions(agg, np.ones(8), ["a", "b", "c"], 0.5, high_threshold=[0.8, 0.8])
    with pytest.raises(ValueError, match="one per label"):
        P.compute_binary_predictions(agg, np.ones(8), ["a", "b", "c"], 0.5, merge_gap_rows=[1, 2, 3, 4])


# ------------------------------------------------------------------ seeded smoothed noise
def smoothed(S, L, seed, width=5):
    """Box-smoothed uniform noise in [0, 1], scaled by the count's maximum of 2 as the overlap average leaves it: runs are several rows long."""
    rng = np.random.default_rng(seed)
    raw = rng.random((S + width - 1, L))
    box = np.cumsum(np.vstack([np.zeros((1, L)), raw]), axis=0)
    return (box[width:] - box[:-width]) / width


@pytest.mark.parametrize("L,seed", [(1, 11), (7, 12), (64, 13)])
def test_smoothed_noise_equals_the_naive_restatement(L, seed):
    S = 700
    rng = np.random.default_rng(seed + 100)
    agg = smoothed(S, L, seed)
    agg[rng.random((S, L)) < 0.01] = np.nan
    cnt = np.full(S, 2.0)
    cnt[0] = 1.0
    t_lo = 2 * (0.5 + 0.05 * rng.random(L))  # against agg itself: the cut is t / max(cnt)
    t_hi = t_lo + 2 * 0.12 * rng.random(L)
    gaps = rng.integers(0, 6, L)
    gaps[0] = 3
    calls = names_for(L)
    want, stats = naive(agg, cnt, t_lo, t_hi, gaps)
    assert stats["dropped"] >= 1 and stats["longest_chain"] >= 3 and stats["untouched"] >= 1, stats
    assert host(agg, cnt, calls, t_lo, t_hi, gaps) == want
    assert host(agg, cnt, calls, t_lo, t_hi, None) == naive(agg, cnt, t_lo, t_hi, [0] * L)[0]
    assert host(agg, cnt, calls, t_lo, None, gaps) == naive(agg, cnt, t_lo, t_lo, gaps)[0]
    unrefined = host(agg, cnt, calls, t_lo)
    assert unrefined == naive(agg, cnt, t_lo, t_lo, [0] * L)[0] and len(unrefined) > len(want)


# ------------------------------------------------------------------ seconds to output steps
def test_gap_rows_is_the_floor_of_seconds_over_the_step():
    step = TPO * DELTA_T
    got = F.gap_rows([0.0, step * 0.999, step, 2.5 * step, 1e30, np.inf], TPO, DELTA_T)
    assert got.dtype == np.int32 and got.tolist() == [0, 0, 1, 2, 2**31 - 1, 2**31 - 1]
    for seconds in (0.05, 0.1, 0.25, 1.0, 3.3):
        assert int(F.gap_rows(seconds, TPO, DELTA_T)) == int(np.floor(seconds / (TPO * DELTA_T)))
    assert F.gap_rows([0.3, 0.3], 16, 0.005).shape == (2,) and F.gap_rows(0.3, 16, 0.005).shape == ()


# ------------------------------------------------------------------ the resolver
def test_resolve_refinement(tmp_path):
    assert W.resolve_refinement(None, None, None, CALLS) is None
    assert W.resolve_refinement(None, None, [0.3] * 7, CALLS) is None
    assert W.resolve_refinement(0.8, None, None, CALLS) == {"high": [0.8] * 7, "gap_seconds": [0.0] * 7}
    assert W.resolve_refinement("0.8", "0.25", None, CALLS) == {"high": [0.8] * 7, "gap_seconds": [0.25] * 7}
    low = [0.5, 0.5, 0.5, 0.5, 0.25, 0.5, 0.9]
    got = W.resolve_refinement({"SS": 0.4, "BR": 1}, {"BUZZ": 0.1}, low, CALLS)
    assert got == {"high": [1.0, 0.5, 0.5, 0.5, 0.4, 0.5, 0.9], "gap_seconds": [0.0, 0.1, 0.0, 0.0, 0.0, 0.0, 0.0]}  # not named: high = threshold, gap 0
    path = tmp_path / "gap.json"
    path.write_text(json.dumps({"WHISTLE": 0.5}))
    assert W.resolve_refinement(None, path, None, CALLS)["gap_seconds"][6] == 0.5 == W.resolve_refinement(None, str(path), None, CALLS)["gap_seconds"][6]
    assert W.resolve_refinement(None, path, None, CALLS)["high"] == [0.5] * 7


def test_resolve_refinement_errors():
    with pytest.raises(ValueError, match="CLICK"):
        W.resolve_refinement({"CLICK": 0.9}, None, None, CALLS)
    with pytest.raises(ValueError, match="CLICK"):
        W.resolve_refinement(None, {"BR": 0.1, "CLICK": 0.1}, None, CALLS)
    with pytest.raises(ValueError, match="negative"):
        W.resolve_refinement(None, -0.1, None, CALLS)
    with pytest.raises(ValueError, match="negative"):
        W.resolve_refinement(None, {"SS": -1}, None, CALLS)
    with pytest.raises(ValueError, match="below its threshold"):
        W.resolve_refinement(0.4, None, None, CALLS)
    with pytest.raises(ValueError, match="WHISTLE"):  # after --thresholds is applied
        W.resolve_refinement(0.8, None, [0.5] * 6 + [0.9], CALLS)
    with pytest.raises(ValueError, match="below its threshold"):
        W.resolve_refinement({"BR": float("nan")}, None, None, CALLS)
    assert W.resolve_refinement(0.5, 0.0, None, CALLS) == {"high": [0.5] * 7, "gap_seconds": [0.0] * 7}  # equality and a zero gap are fine


def test_predict_rejects_bad_options_before_the_model_is_loaded(tmp_path, monkeypatch):
    def no_model(*a, **k):
        raise AssertionError("the model was loaded")

    monkeypatch.setattr(P, "load_orcai_model", no_model)
    wav = tmp_path / "a.wav"
    wav.write_bytes(b"")
    for bad, match in (({"high_thresholds": {"CLICK": 0.9}}, "CLICK"), ({"merge_gap": -1}, "negative"), ({"high_thresholds": 0.4}, "below"),
                       ({"high_thresholds": 0.6, "thresholds": {"BR": 0.7}}, "BR")):
        with pytest.raises(ValueError, match=match):
            P.predict(wav, verbosity=0, **bad)
    with pytest.raises(AssertionError, match="the model was loaded"):
        P.predict(wav, verbosity=0, high_thresholds=0.6, merge_gap={"BR": 0.2})


# ------------------------------------------------------------------ the command line
def test_cli_predict_hands_the_options_on(tmp_path, monkeypatch):
    from click.testing import CliRunner

    from orcai_amd.cli import cli

    out = CliRunner().invoke(cli, ["predict", "--help"]).output
    assert "--high-thresholds" in out and "--merge-gap" in out
    for f in (P.predict, P.predict_wav, P.predict_wavs):
        assert inspect.signature(f).parameters["high_thresholds"].default is None and inspect.signature(f).parameters["merge_gap"].default is None
    seen = {}
    monkeypatch.setattr(P, "predict", lambda **kwargs: seen.update(kwargs))
    wav = tmp_path / "a.wav"
    wav.write_bytes(b"")
    gaps = tmp_path / "gaps.json"
    gaps.write_text(json.dumps({"BR": 0.2}))
    result = CliRunner().invoke(cli, ["predict", str(wav), "--high-thresholds", "0.7", "--merge-gap", str(gaps), "-v", "0"])
    assert result.exit_code == 0, result.output
    assert seen["high_thresholds"] == "0.7" and seen["merge_gap"] == str(gaps)
    assert W.resolve_refinement(seen["high_thresholds"], seen["merge_gap"], None, CALLS) == {"high": [0.7] * 7, "gap_seconds": [0.2] + [0.0] * 6}
    seen.clear()
    assert CliRunner().invoke(cli, ["predict", str(wav), "-v", "0"]).exit_code == 0
    assert seen["high_thresholds"] is None and seen["merge_gap"] is None


# ------------------------------------------------------------------ defaults
def test_without_the_options_the_lists_are_todays():
    agg = smoothed(400, 7, seed=3)
    cnt = np.full(400, 2.0)
    for threshold in (0.5, [1.0, 0.9, 1.1, 1.0, 1.0, 0.8, 1.2]):
        starts, stops, names = P.compute_binary_predictions(agg, cnt, CALLS, threshold=threshold)
        binary = (agg > np.asarray(threshold) / np.max(cnt)).astype(int)  # predict.py:298-317
        w_starts, w_stops, w_names = [], [], []
        for i, name in enumerate(CALLS):
            if binary[:, i].sum() > 0:
                d = np.diff(binary[:, i], prepend=0, append=0)
                w_starts += list(np.where(d == 1)[0])
                w_stops += list(np.where(d == -1)[0] - 1)
                w_names += [name] * int((d == 1).sum())
        assert len(starts) > 20 and (starts, stops, names) == (w_starts, w_stops, w_names)
        same = P.compute_binary_predictions(agg, cnt, CALLS, threshold=threshold, high_threshold=threshold, merge_gap_rows=0)
        assert same == (starts, stops, names)
        assert all(type(a) is type(b) for a, b in zip(same[0] + same[1], starts + stops))
    params = inspect.signature(P.compute_binary_predictions).parameters
    assert params["high_threshold"].default is None and params["merge_gap_rows"].default is None
    assert P.label_spec({"calls": CALLS})["refine"] is None
