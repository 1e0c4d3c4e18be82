"""Label extraction on the GPU: the host half of orcai_extract_labels.

The kernel (csrc/labels.hip) thresholds the averaged probabilities, finds the runs of ones per label, orders them as the label file orders them and
judges each against the duration limits; it hands back four integers per run.  What is left here is resolved ONCE per call, not per interval: the
string order of the label names (`label_rank`), the {min, max} limits per label (`resolve_limits`, _check_duration's lookup), and wrapping the
integer columns in the DataFrame the host route (predict.compute_labels, predict.filter_predictions) builds.
"""

from __future__ import annotations


import numpy as np
import pandas as pd
import torch

from orcai_amd import _native as N

EAGER_RUNS = 4096  # runs that travel to the host with the offsets in the one eager copy (64 KiB); a recording-hour of orca calls is a few thousand
STATUS_NAMES = np.array(["keep", "too short", "too long"], dtype=object)  # _check_duration's verdicts, by the kernel's status


def suffixed_names(calls, label_suffix: str | None) -> list[str]:
    """The label column's strings (compute_labels)."""
    if (label_suffix is not None) & (label_suffix != ""):
        return [label + label_suffix for label in calls]
    return list(calls)


def label_rank(calls, label_suffix: str | None) -> np.ndarray:
    """int32 [L]: the position of every label in the stable string sort of the suffixed names -- the third key of compute_labels'
    sort_values(by=["start", "stop", "label"]).  Equal names get consecutive ranks in label index order, which is the order the stable sort leaves
    them in (the table is built label by label)."""
    names = suffixed_names(calls, label_suffix)
    rank = np.empty(len(names), dtype=np.int32)
    rank[sorted(range(len(names)), key=lambda i: names[i])] = np.arange(len(names), dtype=np.int32)
    return rank


def resolve_limits(calls, label_suffix: str | None, call_duration_limits) -> np.ndarray:
    """f64 [L][2] = {min, max} seconds per label, as _check_duration finds them for a row of that label: the suffixed name with every occurrence of
    the suffix removed is looked up, else "default", else (0, inf); None is 0 / inf."""
    if not isinstance(call_duration_limits, dict):
        from orcai_amd.io import read_json

        call_duration_limits = read_json(call_duration_limits)
    out = np.empty((len(calls), 2), dtype=np.float64)
    for i, name in enumerate(suffixed_names(calls, label_suffix)):
        label = name.replace(f"{label_suffix}", "")
        if label in call_duration_limits:
            lo, hi = call_duration_limits[label]
        elif "default" in call_duration_limits:
            lo, hi = call_duration_limits["default"]
        else:
            lo, hi = 0, np.inf
        out[i] = (0 if lo is None else lo, np.inf if hi is None else hi)
    return out


def labels_frame(runs: np.ndarray, calls, label_suffix: str | None, time_steps_per_output_step: int, filtered: bool, scores: np.ndarray | None = None):
    """(predicted_labels, n_too_short, n_too_long) from the kernel's rows of one recording, int32 [n][4] = {start_row, stop_row, label, status} in
    file order.  filtered=False: compute_labels' table.  filtered=True: what filter_predictions returns for that table (the kept rows under their
    original index, with `duration` and `duration_ok`).  scores (int64 [n][3], orcai_interval_scores' rows {peak, sum_q32, peak_row} as raw words):
    three more columns, peak / peak_frame / mean (scores.score_columns), every kept row with its own.  Column arithmetic only; nothing runs per
    interval."""
    from orcai_amd.predict import compute_labels

    if scores is not None:
        from orcai_amd.scores import SCORE_COLUMNS, score_columns

        words = np.ascontiguousarray(scores, dtype=np.int64).reshape(-1, 3)
        n_rows = runs[:, 1].astype(np.int64) - runs[:, 0].astype(np.int64) + 1
        columns = score_columns(words[:, 0].view(np.float64), words[:, 1].view(np.uint64), words[:, 2], n_rows, time_steps_per_output_step)
    if len(runs) == 0:  # the empty table's dtypes are those of empty lists: let the host route make it
        frame = compute_labels([], [], [], time_steps_per_output_step, label_suffix)
        if scores is not None:
            for name in SCORE_COLUMNS:
                frame[name] = columns[name].to_numpy()
        if filtered:
            frame["duration"] = frame["stop"] - frame["start"]
            frame["duration_ok"] = []
        return frame, 0, 0
    runs = runs.astype(np.int64)
    names = np.array(suffixed_names(calls, label_suffix), dtype=object)
    frame = pd.DataFrame({"start": runs[:, 0] * time_steps_per_output_step, "stop": runs[:, 1] * time_steps_per_output_step, "label": names[runs[:, 2]]})
    if scores is not None:
        for name in SCORE_COLUMNS:
            frame[name] = columns[name].to_numpy()
    if not filtered:
        return frame, 0, 0
    status = runs[:, 3]
    frame["duration"] = frame["stop"] - frame["start"]
    frame["duration_ok"] = STATUS_NAMES[status]
    return frame[status == 0], int((status == 1).sum()), int((status == 2).sum())


_constants = {}  # (device, names, suffix, limits) -> (label_rank, limits) on the device


def _device_constants(device, calls, label_suffix, call_duration_limits):
    limits = None if call_duration_limits is None else resolve_limits(calls, label_suffix, call_duration_limits)
    key = (str(device), tuple(calls), label_suffix, None if limits is None else limits.tobytes())
    if key not in _constants:
        if len(_constants) > 64:
            _constants.clear()
        rank = torch.from_numpy(label_rank(calls, label_suffix)).to(device)
        _constants[key] = (rank, None if limits is None else torch.from_numpy(limits).to(device))
    return _constants[key]


def _device_thresholds(device, thresholds, L: int, dtype=np.float64, what: str = "thresholds") -> torch.Tensor:
    """f64 [L] (or `dtype`) on the device, uploaded once per (device, values)."""
    values = np.ascontiguousarray(thresholds, dtype=dtype).reshape(-1)
    if len(values) != L:
        raise ValueError(f"{what}: one per label wanted ({L}), got {len(values)}")
    key = (str(device), what, values.tobytes())
    if key not in _constants:
        if len(_constants) > 64:
            _constants.clear()
        _constants[key] = torch.from_numpy(values).to(device)
    return _constants[key]


class PendingLabels:
    """The label intervals of one recording, or of every recording of a batch, on their way from the GPU to pinned host memory.  `results()` waits
    for the copy (an event on the launch stream, not a device-wide synchronisation) and returns, per recording, (predicted_labels, n_too_short,
    n_too_long) -- labels_frame's triple."""

    def __init__(self, R, calls, label_suffix, tpo, filtered, host=None, device=None, header=0, event=None, keep=(), scores=None, front=0):
        self._R, self._calls, self._suffix, self._tpo, self.filtered = R, calls, label_suffix, tpo, filtered
        self._host, self._device, self._header, self._event, self._keep = host, device, header, event, keep
        self._scores, self._front = scores, front  # the device's int64 [capacity][3] of orcai_interval_scores (None: not asked for); the int32 words
        self.scored = scores is not None           # of the eager score rows in front of the offsets in `host` / `device`
        self._results = None

    def _fetch(self):
        """(per recording the kernel's rows int32 [n_r][4], per recording the score rows int64 [n_r][3] or None)."""
        if self._host is None:  # nothing was launched: recordings without output rows
            none = np.zeros((0, 3), dtype=np.int64) if self.scored else None
            return [np.zeros((0, 4), dtype=np.int32) for _ in range(self._R)], [none] * self._R
        if self._event is not None:
            self._event.synchronize()
            self._event = None
        host = self._host.numpy()
        front = self._front
        offsets = host[front : front + 2 * (self._R + 1)].view(np.int64)
        total = int(offsets[self._R])
        rows = host[front + self._header :].reshape(-1, 4)
        scores = host[: front // 6 * 6].view(np.int64).reshape(-1, 3) if self.scored else None
        if total > len(rows):  # more runs than travelled with the offsets: one more copy, of exactly the rest
            rest = self._device[front + self._header + 4 * len(rows) : front + self._header + 4 * total]
            if self.scored:  # the rest of the 24-byte rows behind the rest of the runs, in the same copy
                both = torch.cat([rest, self._scores[len(rows) : total].reshape(-1).view(torch.int32)]).cpu().numpy()
                rest, more = both[: 4 * (total - len(rows))], both[4 * (total - len(rows)) :].view(np.int64).reshape(-1, 3)
                scores = np.concatenate([scores, more])
            else:
                rest = rest.cpu().numpy()
            rows = np.concatenate([rows, rest.reshape(-1, 4)])
        self._keep = ()
        cut = [(int(offsets[r]), int(offsets[r + 1])) for r in range(self._R)]
        return [rows[a:b] for a, b in cut], [scores[a:b] if self.scored else None for a, b in cut]

    def runs(self) -> list[np.ndarray]:
        """Per recording the kernel's rows, int32 [n_r][4]."""
        return self._fetch()[0]

    def results(self) -> list[tuple[pd.DataFrame, int, int]]:
        if self._results is None:
            self._results = [labels_frame(rows, self._calls, self._suffix, self._tpo, self.filtered, scores=scores) for rows, scores in zip(*self._fetch())]
            self._host = self._device = self._scores = None
        return self._results


def extract_labels_device(agg_dev: torch.Tensor, cnt_dev: torch.Tensor, table_dev: torch.Tensor, R: int, calls, label_suffix: str | None,
                          time_steps_per_output_step: int, delta_t: float, call_duration_limits=None, threshold: float = 0.5,
                          thresholds=None, high_thresholds=None, gap_rows=None, scores: bool = False) -> PendingLabels:
    """Queue orcai_extract_labels on the current stream for the averaged probabilities agg_dev f64 [S_total][L] / cnt_dev f64 [S_total] of the R
    recordings of table_dev (int64 [R][4] on the device, orcai_overlap_average_ragged's table; one recording: [[0, n, S, 0]]), and the copy of its
    result to pinned memory behind one event.  call_duration_limits (a dict or a JSON path) makes the kernel judge every interval as
    filter_predictions does with delta_t seconds per frame.  thresholds (L floats, one per label): orcai_extract_labels_per_label in place of the
    scalar `threshold`.  high_thresholds (L floats) and gap_rows (L ints, output steps; refine.gap_rows): hysteresis and gap merging, DESIGN 4.15 --
    orcai_extract_labels_refined when either is given (the other: high = the threshold, gap 0), the calls above untouched when neither is.

    What travels to the host: the R + 1 offsets and the first EAGER_RUNS runs, in ONE copy whose size does not depend on S_total or L.  The device
    buffer holds the kernel's capacity bound (L * ceil(S_total / 2) + R runs, the size of agg itself), so nothing is ever dropped; when more than
    EAGER_RUNS runs were found, results() fetches exactly the remaining ones in a second copy.  The bytes copied are 16 per run found.

    scores=True: orcai_interval_scores is queued behind the extraction call, whichever of the three it was, and results() returns
    frames with the columns peak, peak_frame and mean.  Its 24-byte rows of the first EAGER_RUNS runs lie in FRONT of the offsets in the same
    buffer and ride in the same eager copy (40 bytes per run then); the rest come with the second copy.  scores=False makes exactly the calls
    made without the option."""
    S_total, L = int(agg_dev.shape[0]), int(agg_dev.shape[1])
    filtered = call_duration_limits is not None
    if S_total < 1:
        return PendingLabels(R, calls, label_suffix, time_steps_per_output_step, filtered, scores=True if scores else None)
    lib = N.lib()
    rank, limits = _device_constants(agg_dev.device, calls, label_suffix, call_duration_limits)
    capacity = L * ((S_total + 1) // 2) + R
    header = -(-2 * (R + 1) // 4) * 4  # int32 words in front of the runs: the int64 offsets, padded to 16 bytes
    front = -(-6 * min(capacity, EAGER_RUNS) // 4) * 4 if scores else 0  # int32 words in front of the offsets: the eager score rows, padded to 16 bytes
    out = torch.empty(front + header + 4 * capacity, dtype=torch.int32, device=agg_dev.device)
    refined = high_thresholds is not None or gap_rows is not None
    ws_bytes = int((lib.orcai_extract_labels_refined_workspace_bytes if refined else lib.orcai_extract_labels_workspace_bytes)(L, R, S_total))
    if refined and ws_bytes == 0:
        raise ValueError(f"label extraction: {S_total} output rows, {L} labels, {R} recordings is outside what the kernel takes")
    workspace = torch.empty(ws_bytes, dtype=torch.uint8, device=agg_dev.device)
    tail = (N.ptr(rank), None if limits is None else N.ptr(limits), float(delta_t), int(time_steps_per_output_step), out.data_ptr() + 4 * (front + header),
            capacity, out.data_ptr() + 4 * front, workspace.data_ptr(), ws_bytes, N.stream_ptr())
    per_label = None
    if refined:
        per_label = _device_thresholds(agg_dev.device, np.full(L, float(threshold)) if thresholds is None else thresholds, L)
        high = per_label if high_thresholds is None else _device_thresholds(agg_dev.device, high_thresholds, L, what="high_thresholds")
        gaps = _device_thresholds(agg_dev.device, np.zeros(L) if gap_rows is None else gap_rows, L, dtype=np.int32, what="gap_rows")
        N.check(lib.orcai_extract_labels_refined(N.ptr(agg_dev), N.ptr(cnt_dev), L, N.ptr(table_dev), R, S_total, N.ptr(per_label), N.ptr(high), N.ptr(gaps), *tail),
                "orcai_extract_labels_refined")
        per_label = (per_label, high, gaps)
    elif thresholds is None:
        N.check(lib.orcai_extract_labels(N.ptr(agg_dev), N.ptr(cnt_dev), L, N.ptr(table_dev), R, S_total, float(threshold), *tail), "orcai_extract_labels")
    else:
        per_label = _device_thresholds(agg_dev.device, thresholds, L)
        N.check(lib.orcai_extract_labels_per_label(N.ptr(agg_dev), N.ptr(cnt_dev), L, N.ptr(table_dev), R, S_total, N.ptr(per_label), *tail),
                "orcai_extract_labels_per_label")
    all_scores = score_ws = None
    if scores:
        score_bytes = int(lib.orcai_interval_scores_workspace_bytes(L, R, S_total))
        if score_bytes == 0:
            raise ValueError(f"interval scores: {S_total} output rows, {L} labels, {R} recordings is outside what the kernel takes")
        all_scores = torch.empty((capacity, 3), dtype=torch.int64, device=agg_dev.device)
        score_ws = torch.empty(score_bytes, dtype=torch.uint8, device=agg_dev.device)
        N.check(lib.orcai_interval_scores(N.ptr(agg_dev), L, N.ptr(table_dev), R, S_total, out.data_ptr() + 4 * (front + header), out.data_ptr() + 4 * front,
                                          capacity, all_scores.data_ptr(), out.data_ptr(), front // 6, score_ws.data_ptr(), score_bytes, N.stream_ptr()),
                "orcai_interval_scores")
    eager = front + header + 4 * min(capacity, EAGER_RUNS)
    host = torch.empty(eager, dtype=torch.int32, pin_memory=True)
    host.copy_(out[:eager], non_blocking=True)
    event = torch.cuda.Event()
    event.record()
    return PendingLabels(R, calls, label_suffix, time_steps_per_output_step, filtered, host=host, device=out, header=header, event=event,
                         keep=(agg_dev, cnt_dev, table_dev, workspace, rank, limits, per_label, score_ws), scores=all_scores, front=front)
