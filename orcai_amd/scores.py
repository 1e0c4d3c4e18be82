"""A score for every detected interval: the host twin of orcai_interval_scores, and the columns both routes hand to the files.

The contract (include/orcai_hip.h states the same one).  For an interval of label l over output rows start_row .. stop_row inclusive of one
recording, with p[s] = agg[s][l] (for a merged interval the rows of its gaps count):

  peak      the largest p[s] as the f64 it is; NaN rows are skipped (a gap row may be NaN, a start row never is: NaN is above no threshold).
  peak_row  the lowest row that attains peak: ties go to the earlier row.
  sum_q32   the sum of q[s] = rint(min(max(p[s], 0), 1) * 2**32) (round-half-even, NaN gives 0) as an unsigned 64-bit integer.  The scaling by a power of
            two and the rint are exact, integer addition is associative: numpy's cumsum and the GPU's tree give the same bits.  Differences of wrapped
            unsigned prefix sums are still exact, and an interval of fewer than 2**31 rows sums to less than 2**63.
  mean      sum_q32 / (n_rows * 2**32), formed here in f64 for both routes (`score_columns`): within 2**-33 of the exact mean of the clamped rows.

Column operations only: one uint64 cumsum for the sums, maximum.reduceat / minimum.reduceat over the intervals for the peaks; nothing runs per row.
"""

from __future__ import annotations

import numpy as np
import pandas as pd

Q32 = 4294967296.0  # 2**32
SCORE_COLUMNS = ["peak", "peak_frame", "mean"]


def q32(p: np.ndarray) -> np.ndarray:
    """uint64 q[s] of the contract, elementwise."""
    with np.errstate(invalid="ignore"):
        q = np.rint(np.clip(np.asarray(p, dtype=np.float64), 0.0, 1.0) * Q32)
    q[np.isnan(q)] = 0.0
    return q.astype(np.uint64)


def interval_scores(aggregated_predictions: np.ndarray, start_rows, stop_rows, labels) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(peak f64 [n], sum_q32 uint64 [n], peak_row int64 [n]) -- the three fields orcai_interval_scores writes -- for n intervals of one recording:
    rows start_rows[i] .. stop_rows[i] inclusive of column labels[i] of aggregated_predictions f64 [S][L].  The intervals may come in any order and
    may overlap.  An interval whose rows are all NaN: peak NaN, peak_row -1."""
    agg = np.asarray(aggregated_predictions, dtype=np.float64)
    start = np.asarray(start_rows, dtype=np.int64).reshape(-1)
    stop = np.asarray(stop_rows, dtype=np.int64).reshape(-1)
    label = np.asarray(labels, dtype=np.int64).reshape(-1)
    n = len(start)
    if n == 0:
        return np.zeros(0, dtype=np.float64), np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=np.int64)
    S, L = agg.shape
    if (start < 0).any() or (stop >= S).any() or (stop < start).any() or (label < 0).any() or (label >= L).any():
        raise ValueError("interval_scores: an interval outside the averaged probabilities")
    flat = np.ascontiguousarray(agg.T).reshape(-1)  # label-major: an interval is a contiguous stretch
    first, behind = label * S + start, label * S + stop + 1
    prefix = np.zeros(L * S + 1, dtype=np.uint64)
    np.cumsum(q32(flat), out=prefix[1:])  # wraps modulo 2**64; the differences below do not care
    sums = prefix[behind] - prefix[first]
    # reduceat over the index pairs (first, behind): every even segment is an interval, the odd ones (what lies between two pairs) are thrown away
    pairs = np.stack([first, behind], axis=1).reshape(-1)
    values = np.append(np.where(np.isnan(flat), -np.inf, flat), -np.inf)  # one element behind the end: `behind` may point there
    top = np.maximum.reduceat(values, pairs)[::2]
    lengths = behind - first
    rows = np.repeat(first - np.cumsum(lengths) + lengths, lengths) + np.arange(int(lengths.sum()))  # the flat rows of all intervals, one after another
    attains = (flat[rows] == np.repeat(top, lengths)) & ~np.isnan(flat[rows])
    where = np.where(attains, rows, np.iinfo(np.int64).max)
    at = np.minimum.reduceat(where, np.cumsum(lengths) - lengths)  # the lowest row that attains the maximum
    found = at != np.iinfo(np.int64).max
    peak = np.full(n, np.nan)
    peak[found] = flat[at[found]]
    return peak, sums, np.where(found, at - label * S, -1)


def score_columns(peak: np.ndarray, sum_q32: np.ndarray, peak_row: np.ndarray, n_rows: np.ndarray, time_steps_per_output_step: int) -> pd.DataFrame:
    """The three columns of a scored label table from the three fields of either route: peak (f64), peak_frame (int64, peak_row * tpo: the unit of
    start / stop) and mean (f64).  The ONE place the mean is formed."""
    mean = np.asarray(sum_q32, dtype=np.uint64).astype(np.float64) / (np.asarray(n_rows, dtype=np.int64).astype(np.float64) * Q32)
    return pd.DataFrame({"peak": np.asarray(peak, dtype=np.float64), "peak_frame": np.asarray(peak_row, dtype=np.int64) * int(time_steps_per_output_step),
                         "mean": mean})


def add_scores(predicted_labels: pd.DataFrame, aggregated_predictions: np.ndarray, calls, label_suffix: str | None,
               time_steps_per_output_step: int) -> pd.DataFrame:
    """compute_labels' table (start, stop in frames, label with its suffix, sorted) with the three score columns, from the host's averaged
    probabilities.  Label names are looked up in the suffixed `calls`; of two equal names the first column is taken."""
    from orcai_amd.device_labels import suffixed_names

    tpo = int(time_steps_per_output_step)
    column = {}
    for i, name in enumerate(suffixed_names(calls, label_suffix)):
        column.setdefault(name, i)
    start = predicted_labels["start"].to_numpy(dtype=np.int64) // tpo
    stop = predicted_labels["stop"].to_numpy(dtype=np.int64) // tpo
    label = np.array([column[name] for name in predicted_labels["label"]], dtype=np.int64)
    peak, sums, rows = interval_scores(aggregated_predictions, start, stop, label)
    columns = score_columns(peak, sums, rows, stop - start + 1, tpo)
    out = predicted_labels.copy()
    for name in SCORE_COLUMNS:
        out[name] = columns[name].to_numpy()
    return out
