"""Per-label decision thresholds: the host half of orcai_threshold_counts.

The kernel (csrc/test_tables.hip) reduces every batch of probabilities and labels to one integer array and adds it to the batches before it:

  hist  int64 [L][2][T + 1]: per label l and class c (the label value, 0 or 1; masked and other values are not counted) how many elements have a
        probability above exactly k of the T thresholds, at index [l][c][k].  The comparison is the strict f32 `p > thresholds[j]`; a NaN is above
        nothing (k = 0).

`hist_from_arrays` is the same arithmetic in numpy -- the written specification and the reference of the tests.  Everything else here is formed from
hist on the host in float64: the sweep table (TP / FP / FN / TN and the ratios at every threshold), the areas under the ROC and the PR curve per label
and pooled (the reference's MaskedAUC, architectures.py:289-304, as a report of `orcai test` rather than a training metric), and the threshold of
maximal F1 per label that `orcai predict --thresholds` takes.  `ThresholdCounts` is the device-side accumulator of one dataset.
"""

from __future__ import annotations

import numpy as np
import pandas as pd

from orcai_amd.auxiliary import MASK_VALUE

DEFAULT_THRESHOLD = 0.5  # what every label is cut at without a thresholds file
KERAS_EPSILON = 1e-7  # keras.backend.epsilon()


def keras_thresholds(T: int = 200) -> np.ndarray:
    """f32 [T]: the table of keras.metrics.AUC(num_thresholds=T): -epsilon, then i / (T - 1) for i = 1 .. T - 2, then 1 + epsilon, rounded to float32.
    Strictly ascending; the first entry is below every probability and the last above every one."""
    T = int(T)
    if not 2 <= T <= 1024:
        raise ValueError(f"num_thresholds must be 2..1024 (orcai_threshold_counts takes tables of up to 1024 entries), got {T}")
    return np.array([0.0 - KERAS_EPSILON] + [(i + 1) * 1.0 / (T - 1) for i in range(T - 2)] + [1.0 + KERAS_EPSILON], dtype=np.float32)


def hist_from_arrays(y_true, y_pred, thresholds, mask_value=MASK_VALUE) -> np.ndarray:
    """hist int64 [L][2][T + 1] of labels y_true and probabilities y_pred, [..., L] each, as include/orcai_hip.h states it for
    orcai_threshold_counts: k = the number of j with p > thresholds[j], in float32."""
    y = np.asarray(y_true, dtype=np.float32)
    L = y.shape[-1]
    y = y.reshape(-1, L)
    p = np.asarray(y_pred, dtype=np.float32).reshape(-1, L)
    t = np.asarray(thresholds, dtype=np.float32).reshape(-1)
    T = len(t)
    k = np.zeros(p.shape, dtype=np.int64)
    with np.errstate(invalid="ignore"):
        for j in range(T):
            k += p > t[j]  # NaN: False
    counted = (y != np.float32(mask_value)) & ((y == 0) | (y == 1))
    c = (y == 1).astype(np.int64)
    index = (np.arange(L, dtype=np.int64)[None, :] * 2 + c) * (T + 1) + k
    return np.bincount(index[counted], minlength=L * 2 * (T + 1)).astype(np.int64).reshape(L, 2, T + 1)


def _div_no_nan(a, b):
    """a / b in float64, 0 where b is 0 (tf.math.divide_no_nan)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    out = np.zeros(np.broadcast(a, b).shape, dtype=np.float64)
    np.divide(a, b, out=out, where=b != 0)
    return out


def _curve_counts(hist: np.ndarray):
    """(TP, FP, FN, TN) int64 [..., T] from hist [..., 2, T + 1]: predicted positive at threshold j is k >= j + 1."""
    hist = np.asarray(hist, dtype=np.int64)
    above = np.cumsum(hist[..., ::-1], axis=-1)[..., ::-1]  # above[k] = the sum over k' >= k
    tp, fp = above[..., 1, 1:], above[..., 0, 1:]
    return tp, fp, above[..., 1, :1] - tp, above[..., 0, :1] - fp


def sweep_from_hist(hist: np.ndarray, thresholds, label_names: list[str]) -> pd.DataFrame:
    """One row per (label, threshold), labels in the order given and thresholds ascending: label, threshold, the integer TP / FP / FN / TN of
    `p > threshold` over the label's counted elements, and precision, recall, F1 and FPR in float64 with 0 / 0 = 0."""
    hist = np.asarray(hist)
    t = np.asarray(thresholds, dtype=np.float32).reshape(-1)
    L, T = len(label_names), len(t)
    assert hist.shape == (L, 2, T + 1), hist.shape
    tp, fp, fn, tn = (a.reshape(-1) for a in _curve_counts(hist))
    return pd.DataFrame({"label": np.repeat(np.array(list(label_names), dtype=object), T), "threshold": np.tile(t.astype(np.float64), L),
                         "TP": tp, "FP": fp, "FN": fn, "TN": tn, "precision": _div_no_nan(tp, tp + fp), "recall": _div_no_nan(tp, tp + fn),
                         "F1": _div_no_nan(2 * tp, 2 * tp + fp + fn), "FPR": _div_no_nan(fp, fp + tn)})


def _roc_auc(tp, fp, fn, tn) -> np.ndarray:
    """keras.metrics.AUC(curve="ROC", summation_method="interpolation"): the trapezoid of recall over FPR across the threshold table."""
    x, y = _div_no_nan(fp, fp + tn), _div_no_nan(tp, tp + fn)
    return np.sum((x[..., :-1] - x[..., 1:]) * (y[..., :-1] + y[..., 1:]) / 2.0, axis=-1)


def _pr_auc(tp, fp, fn) -> np.ndarray:
    """keras.metrics.AUC(curve="PR", summation_method="interpolation") (AUC.interpolate_pr_auc: Davis & Goadrich 2006, the precision between two
    thresholds interpolated along a straight line in (TP, TP + FP) and integrated over recall in closed form)."""
    tp, fp, fn = (np.asarray(a, dtype=np.float64) for a in (tp, fp, fn))
    pos = tp + fp
    dtp = tp[..., :-1] - tp[..., 1:]
    slope = _div_no_nan(dtp, np.maximum(pos[..., :-1] - pos[..., 1:], 0))
    intercept = tp[..., 1:] - slope * pos[..., 1:]
    both = (pos[..., :-1] > 0) & (pos[..., 1:] > 0)
    ratio = np.where(both, _div_no_nan(pos[..., :-1], np.maximum(pos[..., 1:], 0)), 1.0)
    return np.sum(_div_no_nan(slope * (dtp + intercept * np.log(ratio)), np.maximum(tp[..., 1:] + fn[..., 1:], 0)), axis=-1)


def auc_from_hist(hist: np.ndarray) -> dict:
    """{"ROC_AUC": f64 [L], "PR_AUC": f64 [L], "MAUC": float} from hist int64 [L][2][T + 1].

    MAUC is the ROC AUC of the histograms of all labels added together: what the reference's MaskedAUC computes with the defaults of
    keras.metrics.AUC (multi_label=False pools every unmasked element of every label; the trapezoid of recall over FPR across the table).  Keras
    accumulates its four counts and evaluates the curve in float32; here the counts are exact integers and the curve is evaluated in float64, so the
    figures agree with Keras to float32 precision, not to the bit.  A label without positives (or without negatives) has the area 0, not NaN."""
    hist = np.asarray(hist, dtype=np.int64)
    assert hist.ndim == 3 and hist.shape[1] == 2 and hist.shape[2] >= 3, hist.shape
    tp, fp, fn, tn = _curve_counts(hist)
    return {"ROC_AUC": _roc_auc(tp, fp, fn, tn), "PR_AUC": _pr_auc(tp, fp, fn), "MAUC": float(_roc_auc(*_curve_counts(hist.sum(axis=0))))}


def recommend_thresholds(sweep: pd.DataFrame) -> dict:
    """{label: threshold}: per label of a sweep_from_hist table the threshold of maximal F1; among equal F1 the threshold nearest to 0.5, then the
    lower one.  A label without a single positive keeps 0.5."""
    out = {}
    for label, rows in sweep.groupby("label", sort=False):
        if int(rows["TP"].iloc[0] + rows["FN"].iloc[0]) == 0:
            out[label] = DEFAULT_THRESHOLD
            continue
        t, f1 = rows["threshold"].to_numpy(), rows["F1"].to_numpy()
        tied = t[f1 == f1.max()]
        best = sorted(tied, key=lambda v: (abs(v - DEFAULT_THRESHOLD), v))[0]
        out[label] = float(best)
    return out


def resolve_thresholds(thresholds, calls: list[str]) -> list[float] | None:
    """The L thresholds of `orcai predict --thresholds` in the order of `calls`, from a dict {label: threshold} or the path of a thresholds.json;
    None stays None.  Labels the dict does not name keep 0.5; labels it names that the model does not know raise ValueError."""
    if thresholds is None:
        return None
    if not isinstance(thresholds, dict):
        from orcai_amd.io import read_json

        thresholds = read_json(thresholds)
    unknown = sorted(str(k) for k in thresholds if k not in calls)
    if unknown:
        raise ValueError(f"thresholds name labels the model does not have: {', '.join(unknown)} (its labels: {', '.join(calls)})")
    return [float(thresholds.get(call, DEFAULT_THRESHOLD)) for call in calls]


def _label_values(value, calls: list[str], what: str) -> dict:
    """{label: float} from a number (every label), a dict {label: value} or the path of such a JSON file; a label the model does not have raises."""
    if isinstance(value, str):
        try:
            value = float(value)
        except ValueError:
            pass
    if isinstance(value, (int, float, np.integer, np.floating)) and not isinstance(value, bool):
        return {call: float(value) for call in calls}
    if not isinstance(value, dict):
        from orcai_amd.io import read_json

        value = read_json(value)
    if not isinstance(value, dict):
        return _label_values(value, calls, what)  # a JSON file holding one number
    unknown = sorted(str(k) for k in value if k not in calls)
    if unknown:
        raise ValueError(f"{what} name labels the model does not have: {', '.join(unknown)} (its labels: {', '.join(calls)})")
    return {k: float(v) for k, v in value.items()}


def resolve_refinement(high_thresholds, merge_gap, thresholds: list[float] | None, calls: list[str]) -> dict | None:
    """`orcai predict --high-thresholds --merge-gap` in the order of `calls`: {"high": L floats, "gap_seconds": L floats}, or None when neither is
    given.  Each is a number (all labels), a dict {label: value} or the path of such a JSON file; `thresholds` is resolve_thresholds' answer (None:
    0.5 everywhere).  Labels not named get high = their threshold and gap 0.  Raises ValueError for a label the model does not have, a gap that is
    not >= 0 and a high threshold that is not >= the label's threshold."""
    if high_thresholds is None and merge_gap is None:
        return None
    low = [DEFAULT_THRESHOLD] * len(calls) if thresholds is None else [float(t) for t in thresholds]
    named_high = {} if high_thresholds is None else _label_values(high_thresholds, calls, "high thresholds")
    named_gap = {} if merge_gap is None else _label_values(merge_gap, calls, "merge gaps")
    high = [named_high.get(call, t) for call, t in zip(calls, low)]
    gap = [named_gap.get(call, 0.0) for call in calls]
    for call, t, h, g in zip(calls, low, high, gap):
        if not h >= t:
            raise ValueError(f"high threshold of {call} ({h}) is below its threshold ({t})")
        if not g >= 0:
            raise ValueError(f"merge gap of {call} ({g}) is negative")
    return {"high": high, "gap_seconds": gap}


def report_from_hist(hist: np.ndarray, thresholds, label_names: list[str]) -> dict:
    """What `orcai test --threshold-sweep` writes for one dataset: {"sweep": DataFrame, "auc": {...}, "thresholds": {label: threshold}}."""
    sweep = sweep_from_hist(hist, thresholds, label_names)
    auc = auc_from_hist(hist)
    return {"sweep": sweep,
            "auc": {"ROC_AUC": {name: float(v) for name, v in zip(label_names, auc["ROC_AUC"])},
                    "PR_AUC": {name: float(v) for name, v in zip(label_names, auc["PR_AUC"])}, "MAUC": auc["MAUC"]},
            "thresholds": recommend_thresholds(sweep)}


class ThresholdCounts:
    """hist of one dataset on the device: zeroed once (the table goes to the device then), `add` queues orcai_threshold_counts for one batch on the
    current stream (no copy, no synchronisation), `result` copies hist back in one synchronising transfer."""

    def __init__(self, num_labels: int, thresholds, device):
        import torch

        from orcai_amd import _native as N

        t = np.ascontiguousarray(thresholds, dtype=np.float32).reshape(-1)
        if not 1 <= num_labels <= 64 or not 1 <= len(t) <= 1024:
            raise ValueError(f"orcai_threshold_counts takes 1..64 labels and 1..1024 thresholds, got {num_labels} and {len(t)}")
        if not (np.diff(t) > 0).all():
            raise ValueError("ThresholdCounts: the thresholds must ascend strictly")
        self.L, self.T, self.thresholds = int(num_labels), len(t), t
        self._table = torch.from_numpy(t).to(device)
        self._buf = torch.empty(self.L * 2 * (self.T + 1), dtype=torch.int64, device=device)
        N.check(N.lib().orcai_zero_fill(N.ptr(self._buf), 8 * self._buf.numel(), N.stream_ptr()), "orcai_zero_fill")

    def add(self, probs, labels, mask_value: float = MASK_VALUE) -> None:
        """probs, labels: contiguous float32 cuda tensors [..., L] of one shape."""
        import torch

        from orcai_amd import _native as N

        for name, t in (("probs", probs), ("labels", labels)):
            if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
                raise ValueError(f"ThresholdCounts.add: {name} must be a contiguous float32 cuda tensor")
        if probs.shape != labels.shape or probs.shape[-1] != self.L or probs.device != self._buf.device:
            raise ValueError(f"ThresholdCounts.add: probs {tuple(probs.shape)} and labels {tuple(labels.shape)} must be one shape [..., {self.L}] on {self._buf.device}")
        N.check(N.lib().orcai_threshold_counts(N.ptr(probs), N.ptr(labels), probs.numel() // self.L, self.L, float(mask_value), N.ptr(self._table), self.T,
                                               N.ptr(self._buf), N.stream_ptr()), "orcai_threshold_counts")

    def result(self) -> np.ndarray:
        """hist int64 [L][2][T + 1] on the host."""
        return self._buf.cpu().numpy().reshape(self.L, 2, self.T + 1)
