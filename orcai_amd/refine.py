"""Hysteresis thresholds and gap merging in label extraction: the host half.

The contract, per recording and label l, on the recording's own rows:
  lo[s] = agg[s][l] > t_lo[l] / max(cnt),  hi[s] = lo[s] and agg[s][l] > t_hi[l] / max(cnt)   (strict, NaN false)
  1. candidates are the maximal stretches of lo;  2. a candidate is kept iff one of its rows has hi set;
  3. kept runs are joined while next.start - prev.stop - 1 <= g[l], transitively, whatever dropped candidates lie in the gap.
`refined_runs` is that contract for one column in numpy column operations -- a cumulative sum and two comparisons, nothing per interval; the kernel
(orcai_extract_labels_refined, csrc/labels.hip) implements the same one.  `gap_rows` is the ONE place the public gap, in seconds, becomes output
steps; the host route and the device route both call it.
"""

from __future__ import annotations

import numpy as np

from orcai_amd.auxiliary import find_consecutive_ones

INT32_MAX = 2**31 - 1


def gap_rows(seconds, time_steps_per_output_step: int, delta_t: float) -> np.ndarray:
    """int32, of the shape of `seconds`: floor(seconds / (time_steps_per_output_step * delta_t)) in float64, clipped to int32."""
    with np.errstate(divide="ignore", invalid="ignore"):
        rows = np.floor(np.asarray(seconds, dtype=np.float64) / (time_steps_per_output_step * np.float64(delta_t)))
    return np.clip(np.nan_to_num(rows, nan=0.0, posinf=INT32_MAX), 0, INT32_MAX).astype(np.int32)


def refined_runs(lo: np.ndarray, hi: np.ndarray, gap: int) -> tuple[np.ndarray, np.ndarray]:
    """(starts, inclusive stops) of one column of one recording: lo, hi are its boolean masks, gap the largest number of rows bridged."""
    lo = np.asarray(lo, dtype=bool)
    starts, stops = find_consecutive_ones(lo.astype(int))
    if len(starts) == 0:
        return starts, stops
    seen = np.concatenate([[0], np.cumsum(lo & np.asarray(hi, dtype=bool))])  # hi rows before row s, counted only where lo is set
    keep = seen[stops + 1] > seen[starts]
    starts, stops = starts[keep], stops[keep]
    if gap > 0 and len(starts) > 1:
        apart = starts[1:] - stops[:-1] - 1 > gap  # between neighbours: True where the chain breaks
        starts, stops = starts[np.concatenate([[True], apart])], stops[np.concatenate([apart, [True]])]
    return starts, stops


def per_label(value, L: int, what: str, dtype) -> np.ndarray:
    """A scalar, or one value per label, as an array of L."""
    out = np.asarray(value, dtype=dtype)
    if out.ndim == 0:
        return np.full(L, out, dtype=dtype)
    if out.shape != (L,):
        raise ValueError(f"{what}: one per label wanted ({L}), got shape {out.shape}")
    return out
