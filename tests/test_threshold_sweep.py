"""orcai_amd/threshold_sweep.py without a GPU: the threshold table, the histogram that is the written specification of
orcai_threshold_counts, the sweep table, the areas under the curves and the recommended thresholds made from it; and the per-label thresholds of the
host route of `orcai predict`.  Counts are compared exactly."""

import inspect
import json

import numpy as np
import pytest

from orcai_amd import _native as N
from orcai_amd import predict as P
from orcai_amd import threshold_sweep as W
from orcai_amd.device_tables import counts_from_arrays

CALLS = ["BR", "BUZZ", "HERDING", "PHS", "SS", "TAILSLAP", "WHISTLE"]


def test_keras_thresholds_is_the_table_of_keras_auc():
    t = W.keras_thresholds(200)
    assert t.dtype == np.float32 and t.shape == (200,) and (np.diff(t) > 0).all()
    assert t[0] < 0 and t[-1] > 1
    # [0 - 1e-7] + [(i + 1) / (T - 1) for i in range(T - 2)] + [1 + 1e-7]: entry j (0 < j < T - 1) is j / (T - 1)
    assert t[1] == np.float32(1 / 199) and t[100] == np.float32(100 / 199) and t[101] == np.float32(101 / 199) and t[198] == np.float32(198 / 199)
    assert t[0] == np.float32(-1e-7) and t[199] == np.float32(1 + 1e-7)
    assert len(W.keras_thresholds(2)) == 2 and len(W.keras_thresholds(1024)) == 1024
    for bad in (1, 0, 1025):
        with pytest.raises(ValueError):
            W.keras_thresholds(bad)


def seeded_case(L=7, rows=4000, seed=3):
    rng = np.random.default_rng(seed)
    y = (rng.random((rows, L)) < 0.3).astype(np.float32)
    p = rng.random((rows, L)).astype(np.float32)
    y[rng.random((rows, L)) < 0.15] = -1
    p[rng.random((rows, L)) < 0.1] = 0.5
    p[rng.random((rows, L)) < 0.05] = np.nextafter(np.float32(0.5), np.float32(0))
    p[rng.random((rows, L)) < 0.03] = np.nan
    return y, p


def test_one_threshold_below_a_half_gives_the_confusion_counts():
    """The table [nextafter(0.5f, 0)] makes p > t the same as p >= 0.5f: the sweep's one row per label is orcai_test_counts' conf."""
    y, p = seeded_case()
    assert (p == 0.5).sum() > 100 and np.isnan(p).sum() > 100 and (y == -1).sum() > 100 and (p == np.nextafter(np.float32(0.5), np.float32(0))).sum() > 100
    t = np.array([np.nextafter(np.float32(0.5), np.float32(0))], dtype=np.float32)
    hist = W.hist_from_arrays(y, p, t, -1.0)
    assert hist.shape == (7, 2, 2) and hist.dtype == np.int64
    sweep = W.sweep_from_hist(hist, t, CALLS)
    conf, _ = counts_from_arrays(y, p)
    assert list(sweep["label"]) == CALLS
    assert np.array_equal(sweep[["TN", "FP", "FN", "TP"]].to_numpy(), conf)
    assert sweep["TP"].dtype == np.int64 and sweep["precision"].dtype == np.float64


def test_hist_counts_what_the_contract_counts():
    t = np.array([0.25, 0.5, 0.75], dtype=np.float32)
    p = np.array([[0.25], [0.5], [np.nextafter(np.float32(0.5), np.float32(1))], [0.0], [1.0], [np.nan], [0.9], [0.9], [0.6]], dtype=np.float32)
    y = np.array([[1], [1], [1], [0], [0], [1], [-1], [0.5], [0]], dtype=np.float32)
    hist = W.hist_from_arrays(y, p, t, -1.0)
    # class 1: 0.25 -> k 0, 0.5 -> k 1, just above 0.5 -> k 2, NaN -> k 0; class 0: 0 -> k 0, 1 -> k 3, 0.6 -> k 2; the masked and the 0.5 label: nowhere
    assert hist.tolist() == [[[1, 0, 1, 1], [2, 1, 1, 0]]]
    assert W.hist_from_arrays(y.reshape(3, 3, 1), p.reshape(3, 3, 1), t, -1.0).tolist() == hist.tolist()
    sweep = W.sweep_from_hist(hist, t, ["x"])
    assert sweep["TP"].tolist() == [2, 1, 0] and sweep["FP"].tolist() == [2, 2, 1] and sweep["FN"].tolist() == [2, 3, 4] and sweep["TN"].tolist() == [1, 1, 2]
    assert sweep["precision"].tolist() == [0.5, 1 / 3, 0.0] and sweep["recall"].tolist() == [0.5, 0.25, 0.0] and sweep["FPR"].tolist() == [2 / 3, 2 / 3, 1 / 3]
    assert sweep["F1"].tolist() == [4 / 8, 2 / 7, 0.0]


def hist_at(T, entries, L=1):
    """hist [L][2][T + 1] with hist[l][c][k] = n for (l, c, k, n) in entries."""
    hist = np.zeros((L, 2, T + 1), dtype=np.int64)
    for l, c, k, n in entries:
        hist[l, c, k] = n
    return hist


def test_auc_on_hand_made_histograms():
    T = 200
    # perfectly separated: every negative below threshold 50, every positive above threshold 150
    sep = W.auc_from_hist(hist_at(T, [(0, 0, 10, 30), (0, 0, 50, 5), (0, 1, 151, 7), (0, 1, 190, 2)]))
    assert sep["ROC_AUC"][0] == 1.0 and sep["PR_AUC"][0] == 1.0 and sep["MAUC"] == 1.0
    # both classes with the same distribution: half of each class at k = 50, half at k = 150.  The curve has three distinct points, (1, 1) for the
    # thresholds j < 50, (1/2, 1/2) for 50 <= j < 150 and (0, 0) from j = 150 on; its two trapezoids are 1/2 * 3/4 and 1/2 * 1/4: exactly 1/2.
    same = W.auc_from_hist(hist_at(T, [(0, 0, 50, 8), (0, 0, 150, 8), (0, 1, 50, 3), (0, 1, 150, 3)]))
    assert same["ROC_AUC"][0] == 0.5 and same["MAUC"] == 0.5
    # unequal parts, the same in both classes: the points are (1, 1), (1/4, 1/4), (0, 0): 3/4 * 5/8 + 1/4 * 1/8 = 1/2 again
    skew = W.auc_from_hist(hist_at(T, [(0, 0, 50, 9), (0, 0, 150, 3), (0, 1, 50, 6), (0, 1, 150, 2)]))
    assert skew["ROC_AUC"][0] == 0.5
    # no positives: recall is 0 / 0 = 0 at every threshold; no negatives: FPR is 0 everywhere
    for empty in (hist_at(T, [(0, 0, 20, 5), (0, 0, 120, 5)]), hist_at(T, [])):
        auc = W.auc_from_hist(empty)
        assert auc["ROC_AUC"][0] == 0.0 and auc["PR_AUC"][0] == 0.0 and auc["MAUC"] == 0.0
    auc = W.auc_from_hist(hist_at(T, [(0, 1, 20, 5)]))
    assert auc["ROC_AUC"][0] == 0.0 and auc["PR_AUC"][0] == 1.0 and auc["MAUC"] == 0.0  # whatever is predicted is a positive: precision 1
    # a curve by hand: negatives 4 at k = 10, 4 at k = 100; positives 2 at k = 100, 6 at k = 180.  Points (FPR, recall): (1, 1) for j < 10,
    # (1/2, 1) for 10 <= j < 100, (0, 3/4) for 100 <= j < 180, (0, 0) after: area = 1/2 * 1 + 1/2 * (1 + 3/4) / 2 = 15/16
    hand = hist_at(T, [(0, 0, 10, 4), (0, 0, 100, 4), (0, 1, 100, 2), (0, 1, 180, 6)])
    assert W.auc_from_hist(hand)["ROC_AUC"][0] == 15 / 16
    # MAUC: the ROC AUC of the labels' histograms added together
    three = np.concatenate([hand, hist_at(T, [(0, 0, 50, 9), (0, 0, 150, 3), (0, 1, 50, 6), (0, 1, 150, 2)]), hist_at(T, [(0, 0, 20, 5)])])
    auc = W.auc_from_hist(three)
    assert auc["ROC_AUC"].tolist() == [15 / 16, 0.5, 0.0] and auc["ROC_AUC"].shape == auc["PR_AUC"].shape == (3,)
    assert auc["MAUC"] == W.auc_from_hist(three.sum(axis=0, keepdims=True))["ROC_AUC"][0] and 0.5 < auc["MAUC"] < 15 / 16
    assert not np.isnan(auc["PR_AUC"]).any() and 0.5 < auc["PR_AUC"][0] <= 1.0


def test_pr_auc_is_the_closed_form_of_the_interpolated_curve():
    """Two thresholds apart: TP 8 -> 6 while FP 4 -> 0.  Between them precision = TP / (TP + FP) with FP = 2 (TP - 6): the integral over recall
    TP / 8 of TP / (3 TP - 12) from TP = 6 to 8 is (1 / 8) (2 / 3 + (4 / 3) ln 2); the stretch from (6, 0) to (0, 0) has precision 1: 6 / 8."""
    T = 3
    hist = hist_at(T, [(0, 0, 1, 4), (0, 1, 1, 2), (0, 1, 2, 6)])  # thresholds 0, 1, 2: TP 8, 6, 0; FP 4, 0, 0
    want = (2 / 3 + 4 / 3 * np.log(2)) / 8 + 6 / 8
    assert abs(W.auc_from_hist(hist)["PR_AUC"][0] - want) < 1e-15


def test_recommend_thresholds():
    t = W.keras_thresholds(200)
    # a planted optimum: negatives below threshold 120, positives above, except a few positives low and a few negatives high
    planted = hist_at(200, [(0, 0, 60, 50), (0, 0, 140, 3), (0, 1, 121, 40), (0, 1, 30, 4)])
    sweep = W.sweep_from_hist(planted, t, ["a"])
    f1 = sweep["F1"].to_numpy()
    assert np.argmax(f1) == 60 and (f1[60:121] == f1[60]).all() and f1[59] < f1[60] and f1[121] < f1[120]  # F1 is maximal for 60 <= j <= 120
    # the tie rule: nearest to 0.5 among j = 60 .. 120 is j = 99 or 100 (|99/199 - 1/2| = |100/199 - 1/2| in exact arithmetic): the nearer in
    # float64 of the two float32 entries, the lower one if they are equally near
    d99, d100 = abs(float(t[99]) - 0.5), abs(float(t[100]) - 0.5)
    want = float(t[99]) if d99 <= d100 else float(t[100])
    assert W.recommend_thresholds(sweep) == {"a": want}
    # a tie between two thresholds equally far from 0.5 takes the lower one; one far from 0.5 loses to one near it
    tie = W.sweep_from_hist(hist_at(3, [(0, 0, 0, 5), (0, 1, 3, 5)]), np.array([0.25, 0.5, 0.75], dtype=np.float32), ["a"])
    assert tie["F1"].tolist() == [1.0, 1.0, 1.0] and W.recommend_thresholds(tie) == {"a": 0.5}
    tie = W.sweep_from_hist(hist_at(2, [(0, 0, 0, 5), (0, 1, 2, 5)]), np.array([0.25, 0.75], dtype=np.float32), ["a"])
    assert W.recommend_thresholds(tie) == {"a": 0.25}
    tie = W.sweep_from_hist(hist_at(3, [(0, 0, 0, 5), (0, 1, 3, 5)]), np.array([0.125, 0.25, 0.875], dtype=np.float32), ["a"])
    assert W.recommend_thresholds(tie) == {"a": 0.25}
    # several labels, in order; a label without a positive keeps 0.5
    both = np.concatenate([planted, hist_at(200, [(0, 0, 60, 50)]), hist_at(200, [(0, 0, 20, 10), (0, 1, 31, 10)])])
    got = W.recommend_thresholds(W.sweep_from_hist(both, t, ["a", "none", "low"]))
    assert list(got) == ["a", "none", "low"] and got["a"] == want and got["none"] == 0.5 and float(t[20]) <= got["low"] <= float(t[30])
    assert all(type(v) is float for v in got.values()) and json.loads(json.dumps(got)) == got


def test_report_is_what_orcai_test_writes():
    y, p = seeded_case()
    t = W.keras_thresholds(50)
    report = W.report_from_hist(W.hist_from_arrays(y, p, t, -1.0), t, CALLS)
    assert list(report) == ["sweep", "auc", "thresholds"] and len(report["sweep"]) == 7 * 50
    assert list(report["sweep"].columns) == ["label", "threshold", "TP", "FP", "FN", "TN", "precision", "recall", "F1", "FPR"]
    assert list(report["auc"]) == ["ROC_AUC", "PR_AUC", "MAUC"] and list(report["auc"]["ROC_AUC"]) == CALLS and list(report["thresholds"]) == CALLS
    assert abs(report["auc"]["MAUC"] - 0.5) < 0.05  # the seeded probabilities know nothing of the labels
    json.dumps(report["auc"]), json.dumps(report["thresholds"])
    first = report["sweep"].iloc[0]  # at the first threshold (below 0) every counted element with a number is predicted; the NaNs are not
    counted = (y[:, 0] != -1)
    assert first["TP"] + first["FP"] == (counted & ~np.isnan(p[:, 0])).sum() and first["TP"] + first["FP"] + first["FN"] + first["TN"] == counted.sum()


def _aggregate(S=120, L=7, seed=2):
    rng = np.random.default_rng(seed)
    cnt = np.full(S, 2.0)
    cnt[:5] = 1.0
    agg = np.repeat(rng.random((S // 4, L)), 4, axis=0)
    return agg, cnt


def test_compute_binary_predictions_takes_one_threshold_per_label():
    agg, cnt = _aggregate()
    for value in (0.5, 0.3):
        assert P.compute_binary_predictions(agg, cnt, CALLS, threshold=[value] * 7) == P.compute_binary_predictions(agg, cnt, CALLS, threshold=value)
        assert P.compute_binary_predictions(agg, cnt, CALLS, threshold=np.full(7, value)) == P.compute_binary_predictions(agg, cnt, CALLS, threshold=value)
    thresholds = [0.1, 0.9, 0.5, 0.3, 2.5, 0.0, 0.65]
    agg[10:14, 3] = thresholds[3] / 2.0  # exactly at thresholds[l] / max(count): not a one
    agg[16:28, 3] = 0.0
    agg[20:24, 3] = np.nextafter(thresholds[3] / 2.0, 1.0)  # one ulp above: a one
    starts, stops, names = P.compute_binary_predictions(agg, cnt, CALLS, threshold=thresholds)
    want = []
    for l, name in enumerate(CALLS):  # the per-column statement
        b = np.concatenate([[0], (agg[:, l] > thresholds[l] / np.max(cnt)).astype(int), [0]])
        d = np.diff(b)
        want += [(int(s), int(e), name) for s, e in zip(np.where(d == 1)[0], np.where(d == -1)[0] - 1)]
    assert [(int(s), int(e), n) for s, e, n in zip(starts, stops, names)] == want
    assert ("PHS" in names) and (20, 23, "PHS") in want and not any(s <= 10 <= e and n == "PHS" for s, e, n in want) and "SS" not in names
    assert starts != P.compute_binary_predictions(agg, cnt, CALLS, threshold=0.5)[0]
    with pytest.raises(ValueError, match="one threshold per label"):
        P.compute_binary_predictions(agg, cnt, CALLS, threshold=[0.5] * 6)


def test_resolve_thresholds(tmp_path):
    assert W.resolve_thresholds(None, CALLS) is None
    assert W.resolve_thresholds({}, CALLS) == [0.5] * 7
    assert W.resolve_thresholds({"SS": 0.25, "BR": 1}, CALLS) == [1.0, 0.5, 0.5, 0.5, 0.25, 0.5, 0.5]
    path = tmp_path / "thresholds.json"
    path.write_text(json.dumps({"WHISTLE": 0.125}))
    assert W.resolve_thresholds(path, CALLS) == [0.5] * 6 + [0.125] and W.resolve_thresholds(str(path), CALLS) == [0.5] * 6 + [0.125]
    with pytest.raises(ValueError, match="CLICK, ss"):
        W.resolve_thresholds({"ss": 0.1, "BR": 0.2, "CLICK": 0.3}, CALLS)


def test_predict_rejects_unknown_labels_before_touching_a_device(tmp_path, monkeypatch):
    def no_model(*a, **k):
        raise AssertionError("the model was loaded")

    monkeypatch.setattr(P, "load_orcai_model", no_model)
    wav = tmp_path / "a.wav"
    wav.write_bytes(b"")
    path = tmp_path / "thresholds.json"
    path.write_text(json.dumps({"BR": 0.3, "CLICK": 0.3}))
    for thresholds in ({"CLICK": 0.3}, path):
        with pytest.raises(ValueError, match="CLICK"):
            P.predict(wav, verbosity=0, thresholds=thresholds)
    with pytest.raises(AssertionError, match="the model was loaded"):  # known labels pass the check
        P.predict(wav, verbosity=0, thresholds={"BR": 0.3})


def test_symbols_are_declared_and_bound():
    header = (N.LIB_PATH.parent.parent / "include" / "orcai_hip.h").read_text()
    assert ("int orcai_threshold_counts(const float* p, const float* y, int64_t M, int L, float mask_value, const float* thresholds, int T, int64_t* hist,\n"
            "                           void* stream);") in header
    assert len(N._SIGNATURES["orcai_threshold_counts"][1]) == 9
    per_label, scalar = N._SIGNATURES["orcai_extract_labels_per_label"][1], N._SIGNATURES["orcai_extract_labels"][1]
    assert len(per_label) == 17 and per_label[6] is N.C.c_void_p and scalar[6] is N.C.c_double and per_label[:6] + per_label[7:] == scalar[:6] + scalar[7:]
    assert N.lib().orcai_threshold_counts is not None and N.lib().orcai_extract_labels_per_label is not None


def test_cli_and_signatures_have_the_flags():
    from click.testing import CliRunner

    from orcai_amd.cli import cli
    from orcai_amd.test import _test_model_on_dataset, test_model

    out = CliRunner().invoke(cli, ["test", "--help"]).output
    assert "--threshold-sweep" in out and "--num-thresholds" in out
    assert "--thresholds" in CliRunner().invoke(cli, ["predict", "--help"]).output
    for f in (test_model, _test_model_on_dataset):
        assert inspect.signature(f).parameters["threshold_sweep"].default is False and inspect.signature(f).parameters["num_thresholds"].default == 200
    for f in (P.predict, P.predict_wav, P.predict_wavs):
        assert inspect.signature(f).parameters["thresholds"].default is None
