"""Inference driver.  Same names, arguments, return types, output files and error behaviour as the
reference's ``src/orcAI/predict.py``; the arithmetic (front end, snippet forward passes, overlap average)
runs in HIP kernels.  Label extraction (thresholding an [S,7] matrix, run detection, sorting, TSV) is the
reference's thin host logic restated with numpy/pandas.  With ``device_labels=True`` the threshold, the run detection, the sort and the duration
filter run in one more kernel call (orcai_extract_labels, device_labels.py) and the host wraps its integer columns in the same DataFrame.
"""

from __future__ import annotations

from importlib.resources import files
from pathlib import Path

import numpy as np
import pandas as pd
import torch
from tqdm import tqdm

from orcai_amd import _native as N
from orcai_amd.auxiliary import Messenger, find_consecutive_ones
from orcai_amd.io import load_orcai_model, read_json
from orcai_amd.spectrogram import make_spectrogram, make_spectrogram_device

DEFAULT_MODEL_DIR = files("orcai_amd.models").joinpath("orcai-V1")
DEFAULT_CALL_DURATION_LIMITS = files("orcai_amd.defaults").joinpath("default_call_duration_limits.json")


def _check_duration(calls: pd.Series, call_duration_limits: dict, delta_t: float, label_suffix: str = "*") -> str:
    """predict.py:14-66."""
    label = calls["label"].replace(f"{label_suffix}", "")
    if label in call_duration_limits:
        min_duration, max_duration = call_duration_limits[label]
    elif "default" in call_duration_limits:
        min_duration, max_duration = call_duration_limits["default"]
    else:
        min_duration, max_duration = 0, np.inf
    if min_duration is None:
        min_duration = 0
    if max_duration is None:
        max_duration = np.inf
    if calls["duration"] * delta_t < min_duration:
        return "too short"
    if calls["duration"] * delta_t > max_duration:
        return "too long"
    return "keep"


def filter_predictions(predicted_labels: pd.DataFrame, delta_t: float, call_duration_limits: (Path | str) | dict = DEFAULT_CALL_DURATION_LIMITS,
                       label_suffix: str = "*", verbosity: int = 2, msgr: Messenger | None = None) -> pd.DataFrame:
    """Drop predicted calls whose duration is outside the per-label limits (predict.py:69-159)."""
    if msgr is None:
        msgr = Messenger(verbosity=verbosity, title="Filtering predictions")
    msgr.part("Filtering predictions")
    predicted_labels["duration"] = predicted_labels["stop"] - predicted_labels["start"]
    if not isinstance(call_duration_limits, dict):
        call_duration_limits = read_json(call_duration_limits)
    msgr.part("Filtering calls based on duration")
    if len(predicted_labels) == 0:
        predicted_labels["duration_ok"] = []
        return predicted_labels
    predicted_labels["duration_ok"] = predicted_labels.apply(lambda x: _check_duration(x, call_duration_limits, delta_t, label_suffix), axis=1)
    n_long = int((predicted_labels["duration_ok"] == "too long").sum())
    n_short = int((predicted_labels["duration_ok"] == "too short").sum())
    msgr.info(f"Discarding {n_long + n_short} calls based on duration (too short: {n_short}, too long: {n_long})")
    kept = predicted_labels[predicted_labels["duration_ok"] == "keep"]
    msgr.success("Filtering predictions finished.")
    return kept


def filter_predictions_file(predicted_labels: Path | str, output_file: Path | str = "default", overwrite: bool = False,
                            call_duration_limits: (Path | str) | dict = DEFAULT_CALL_DURATION_LIMITS, label_suffix: str = "*", verbosity: int = 2,
                            msgr: Messenger | None = None):
    """predict.py:162-232."""
    if msgr is None:
        msgr = Messenger(verbosity=verbosity, title="Filtering predictions file")
    if output_file == "default":
        output_file = Path(predicted_labels).with_name(Path(predicted_labels).stem + "_filtered.txt")
    else:
        output_file = Path(output_file)
    msgr.info(f"Output file: {output_file}")
    if output_file.exists() and not overwrite:
        raise FileExistsError(f"Annotation file already exists: {output_file}")
    table = pd.read_csv(predicted_labels, sep="\t", encoding="utf-8")
    kept = filter_predictions(table, delta_t=1, call_duration_limits=call_duration_limits, label_suffix=label_suffix, verbosity=verbosity, msgr=msgr)
    save_predictions(kept, output_file, delta_t=1, msgr=msgr)


class PendingAggregate:
    """Averaged probabilities of one recording, or of every recording of a batch, on their way from the GPU to pinned host memory.  `result()` waits
    for the copy (an event on the launch stream, not a device-wide synchronisation) and returns the two host arrays; for a batch (`slices` =
    [(first output row, rows)] per recording) `results()` returns one (aggregated, count) pair per recording, views of the one host buffer."""

    def __init__(self, agg_host: torch.Tensor, cnt_host: torch.Tensor, event, keep=(), slices=None, labels=None):
        self._agg, self._cnt, self._event, self._keep, self._slices = agg_host, cnt_host, event, keep, slices
        self.labels = labels  # device_labels.PendingLabels of the same recordings, or None; with labels the probabilities may stay on the device

    def result(self) -> tuple[np.ndarray, np.ndarray]:
        if self._agg is None:  # device labels, and nobody asked for the probabilities: they were not copied
            return None, None
        if self._event is not None:
            self._event.synchronize()
            self._event, self._keep = None, ()
        return self._agg.numpy(), self._cnt.numpy()

    def results(self) -> list[tuple[np.ndarray, np.ndarray]]:
        agg, cnt = self.result()
        if agg is None:
            return [(None, None)] * (len(self._slices) if self._slices is not None else 1)
        slices = self._slices if self._slices is not None else [(0, len(cnt))]
        return [(agg[row : row + rows], cnt[row : row + rows]) for row, rows in slices]


def label_spec(orcai_parameter: dict, label_suffix: str = "*", call_duration_limits=None, probabilities: bool = True, thresholds=None,
               refine=None, scores: bool = False) -> dict:
    """What the launch half needs to queue orcai_extract_labels behind the overlap average (device_labels=...): the label names, the suffix, the
    duration limits the kernel is to judge by (None: no filter), whether the averaged probabilities are still wanted on the host, and the per-label
    thresholds (L floats; None: 0.5 for every label through the scalar entry point).  refine (threshold_sweep.resolve_refinement's dict, or None):
    the high thresholds and the merge gaps in seconds, for orcai_extract_labels_refined.  scores: orcai_interval_scores behind the extraction call
    (DESIGN 4.16)."""
    return {"calls": orcai_parameter["calls"], "label_suffix": label_suffix, "call_duration_limits": call_duration_limits, "probabilities": probabilities,
            "thresholds": thresholds, "refine": refine, "scores": bool(scores)}


def _queue_labels(spec: dict, agg: torch.Tensor, cnt: torch.Tensor, table: torch.Tensor, R: int, n_filters: int, delta_t: float):
    from orcai_amd.device_labels import extract_labels_device

    return extract_labels_device(agg, cnt, table, R, spec["calls"], spec["label_suffix"], 2**n_filters, delta_t, call_duration_limits=spec["call_duration_limits"],
                                 thresholds=spec.get("thresholds"), **_refine_arguments(spec.get("refine"), 2**n_filters, delta_t, "high_thresholds", "gap_rows"),
                                 **({"scores": True} if spec.get("scores") else {}))


def _refine_arguments(refine: dict | None, time_steps_per_output_step: int, delta_t: float, high_name: str, gap_name: str) -> dict:
    """The two keyword arguments of either route for a resolved refinement (none for None): the high thresholds, and the gaps in output steps."""
    if refine is None:
        return {}
    from orcai_amd.refine import gap_rows

    return {high_name: refine["high"], gap_name: gap_rows(refine["gap_seconds"], time_steps_per_output_step, delta_t)}


def aggregate_predictions_device(predictions: torch.Tensor, n_frames: int, snippet_length: int, n_filters: int, wait: bool = True,
                                 device_labels: dict | None = None, delta_t: float = 0.0):
    """Overlap-average of per-snippet predictions on the GPU (predict.py:276-293).
    predictions: f32 cuda [n, P, L].  Returns host (f64 [n_frames // 2**n_filters, L], f64 [...]); with wait=False a PendingAggregate
    whose copy to (pinned) host memory is still in flight, so that the caller can queue the next recording's GPU work first.
    device_labels (a label_spec, with wait=False): orcai_extract_labels is queued behind the average and the PendingAggregate carries its
    PendingLabels; the probabilities are copied only if the spec wants them."""
    lib = N.lib()
    tpo = 2**n_filters
    shift = snippet_length // 2
    P = snippet_length // tpo
    S = n_frames // tpo
    n, L = int(predictions.shape[0]), int(predictions.shape[2])
    agg = torch.empty((S, L), dtype=torch.float64, device=predictions.device)
    cnt = torch.empty((S,), dtype=torch.float64, device=predictions.device)
    if S > 0:
        pred = predictions.contiguous()
        N.check(lib.orcai_overlap_average(pred.data_ptr() if n > 0 else agg.data_ptr(), n, P, L, shift // tpo, S, N.ptr(agg), N.ptr(cnt), N.stream_ptr()),
                "orcai_overlap_average")
    if wait:
        return agg.cpu().numpy(), cnt.cpu().numpy()
    labels = None
    if device_labels is not None:
        table = torch.tensor([[0, n, S, 0]], dtype=torch.int64).pin_memory().to(predictions.device, non_blocking=True)
        labels = _queue_labels(device_labels, agg, cnt, table, 1, n_filters, delta_t)
        if not device_labels["probabilities"]:
            return PendingAggregate(None, None, None, labels=labels)
    agg_host = torch.empty((S, L), dtype=torch.float64, pin_memory=True)
    cnt_host = torch.empty((S,), dtype=torch.float64, pin_memory=True)
    agg_host.copy_(agg, non_blocking=True)
    cnt_host.copy_(cnt, non_blocking=True)
    event = torch.cuda.Event()
    event.record()
    return PendingAggregate(agg_host, cnt_host, event, keep=(agg, cnt, predictions), labels=labels)


def aggregate_batch_device(predictions: torch.Tensor, layout, snippet_length: int, n_filters: int, device_labels: dict | None = None,
                           delta_t: float = 0.0) -> PendingAggregate:
    """aggregate_predictions_device for every recording of a batch (batch.Batch) in one launch of orcai_overlap_average_ragged; the averaged
    probabilities and counts of the whole batch go to the host in ONE pinned copy behind one event.  predictions: f32 cuda [layout.n_total, P, L]
    (model.predict_batch).  Per recording the same bits as aggregate_predictions_device on its own snippets.  device_labels: as there, one
    orcai_extract_labels over the whole batch."""
    tpo = 2**n_filters
    P = snippet_length // tpo
    step = (snippet_length // 2) // tpo
    L = int(predictions.shape[2])
    S = layout.out_rows
    pred = predictions.contiguous()
    table = torch.tensor(layout.table, dtype=torch.int64).pin_memory().to(pred.device, non_blocking=True)
    both = torch.empty(S * (L + 1), dtype=torch.float64, device=pred.device)  # agg [S][L], then cnt [S]
    N.check(N.lib().orcai_overlap_average_ragged(N.ptr(pred), P, L, step, N.ptr(table), len(layout.table), S, both.data_ptr(), both[S * L :].data_ptr(),
                                                 N.stream_ptr()), "orcai_overlap_average_ragged")
    slices = [(row, rows) for _, _, rows, row in layout.table]
    labels = None
    if device_labels is not None:
        labels = _queue_labels(device_labels, both[: S * L].view(S, L), both[S * L :], table, len(layout.table), n_filters, delta_t)
        if not device_labels["probabilities"]:
            return PendingAggregate(None, None, None, slices=slices, labels=labels)
    host = torch.empty(S * (L + 1), dtype=torch.float64, pin_memory=True)
    host.copy_(both, non_blocking=True)
    event = torch.cuda.Event()
    event.record()
    return PendingAggregate(host[: S * L].view(S, L), host[S * L :], event, keep=(both, table, pred), slices=slices, labels=labels)


def compute_aggregated_predictions(recording_path: Path, spectrogram, model, orcai_parameter: dict, shape: dict,
                                   msgr: Messenger = Messenger(verbosity=0), progressbar: tqdm = None, wait: bool = True,
                                   device_labels: dict | None = None, delta_t: float = 0.0):
    """Slice into 50 %-overlapping snippets, predict, overlap-average (predict.py:235-295).

    ``model`` may be any object with ``.predict(ndarray[n,L,F,1], verbose=int) -> ndarray[n,P,labels]`` (the
    reference's duck-typed boundary).  A native ResNetLSTM is run without materialising the snippets; a
    ``spectrogram`` that already lives on the GPU (torch tensor) is used in place.  wait=False returns a PendingAggregate (the
    device-to-host copy of the averaged probabilities still in flight) instead of the two host arrays; device_labels / delta_t: see
    aggregate_predictions_device.
    """
    snippet_length = shape["input_shape"][0]
    shift = snippet_length // 2
    n_filters = len(orcai_parameter["model"]["filters"])
    n_frames = int(spectrogram.shape[0])
    num_snippets = (n_frames - snippet_length) // shift + 1
    if num_snippets <= 0:
        # predict.py:244-268 is unguarded here: the empty snippet array reaches model.predict and Keras raises on its shape.
        # Same outcome (an exception, caught per recording in table mode, predict.py:752-755), with a usable message.
        raise ValueError(f"recording too short: {n_frames} spectrogram frames, one snippet needs {snippet_length}")
    msgr.info(f"slicing into {num_snippets} snippets for prediction")
    msgr.info("Prediction of snippets")
    native = hasattr(model, "predict_spectrogram")
    if native:
        spec_dev = spectrogram if isinstance(spectrogram, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(spectrogram, dtype=np.float32)).cuda()
        # inside a process group the snippets of this recording are split into contiguous per-rank blocks and all-gathered
        predictions = model.predict_spectrogram(spec_dev.contiguous(), shard=bool(orcai_parameter.get("shard_snippets", False)))
    else:
        spec_host = spectrogram.cpu().numpy() if isinstance(spectrogram, torch.Tensor) else spectrogram
        snippets = np.array([spec_host[i * shift : i * shift + snippet_length] for i in range(num_snippets)])
        snippets = snippets[..., np.newaxis]
        predictions = torch.from_numpy(np.asarray(model.predict(snippets, verbose=0 if msgr.verbosity < 2 else 1), dtype=np.float32)).cuda()
    msgr.info("Aggregating predictions")
    if progressbar:
        progressbar.set_description(f"{recording_path.stem} - Aggregating predictions")
        progressbar.refresh()
    if predictions.shape[0] == 0:
        predictions = predictions.reshape(0, snippet_length // 2**n_filters, shape["num_labels"])
    return aggregate_predictions_device(predictions, n_frames, snippet_length, n_filters, wait=wait, device_labels=None if wait else device_labels,
                                        delta_t=delta_t)


def compute_binary_predictions(aggregated_predictions: np.ndarray, overlap_count: np.ndarray, calls: list[str], threshold=0.5, high_threshold=None,
                               merge_gap_rows=None):
    """predict.py:298-317.  threshold: a float, or a sequence of one threshold per label (column l is cut at threshold[l] / max(count)).
    high_threshold (>= threshold) and merge_gap_rows (output steps), each a scalar or one per label: hysteresis and gap merging, refine.py's contract.
    A stretch above `threshold` counts only if it reaches high_threshold somewhere, and kept stretches of one label at most merge_gap_rows apart are
    one interval.  Neither given: the reference's cut, untouched."""
    if not np.isscalar(threshold):
        threshold = np.asarray(threshold, dtype=np.float64)
        if threshold.shape != (len(calls),):
            raise ValueError(f"compute_binary_predictions: one threshold per label wanted ({len(calls)}), got shape {threshold.shape}")
    if high_threshold is not None or merge_gap_rows is not None:
        return _refined_binary_predictions(aggregated_predictions, overlap_count, calls, threshold, high_threshold, merge_gap_rows)
    adjusted_threshold = threshold / np.max(overlap_count)
    binary_prediction = (aggregated_predictions > adjusted_threshold).astype(int)
    row_starts, row_stops, label_names = [], [], []
    for i, label_name in enumerate(calls):
        if binary_prediction[:, i].sum() > 0:  # == the reference's builtin sum(), vectorised
            row_start, row_stop = find_consecutive_ones(binary_prediction[:, i])
            row_starts += list(row_start)
            row_stops += list(row_stop)
            label_names += [label_name] * len(row_start)
    return row_starts, row_stops, label_names


def _refined_binary_predictions(aggregated_predictions, overlap_count, calls, threshold, high_threshold, merge_gap_rows):
    """compute_binary_predictions with hysteresis and gap merging: numpy column operations per label (refine.refined_runs)."""
    from orcai_amd.refine import per_label, refined_runs

    L = len(calls)
    low = per_label(threshold, L, "compute_binary_predictions: threshold", np.float64)
    high = low if high_threshold is None else per_label(high_threshold, L, "compute_binary_predictions: high_threshold", np.float64)
    gaps = per_label(0 if merge_gap_rows is None else merge_gap_rows, L, "compute_binary_predictions: merge_gap_rows", np.int64)
    row_starts, row_stops, label_names = [], [], []
    if len(overlap_count) == 0:
        return row_starts, row_stops, label_names
    top = np.max(overlap_count)
    with np.errstate(divide="ignore", invalid="ignore"):  # a zero maximum: +inf (or NaN for a zero threshold), nothing is above it
        lo = aggregated_predictions > low / top
        hi = aggregated_predictions > high / top
    if top == 0:
        lo[:] = False
    for i, label_name in enumerate(calls):
        if lo[:, i].any():
            row_start, row_stop = refined_runs(lo[:, i], hi[:, i], int(gaps[i]))
            row_starts += list(row_start)
            row_stops += list(row_stop)
            label_names += [label_name] * len(row_start)
    return row_starts, row_stops, label_names


def compute_labels(row_starts, row_stops, label_names, time_steps_per_output_step: int, label_suffix: str | None) -> pd.DataFrame:
    """predict.py:320-340."""
    if (label_suffix is not None) & (label_suffix != ""):
        label_names = [label + label_suffix for label in label_names]
    return (
        pd.DataFrame({"start": np.asarray(row_starts) * time_steps_per_output_step, "stop": np.asarray(row_stops) * time_steps_per_output_step,
                      "label": label_names})
        .sort_values(by=["start", "stop", "label"])
        .reset_index(drop=True)
    )


def _convert_times_to_seconds(predicted_labels: pd.DataFrame, delta_t: float) -> pd.DataFrame:
    """predict.py:343-364."""
    predicted_labels = predicted_labels.copy()
    predicted_labels["start"] = predicted_labels["start"] * delta_t
    predicted_labels["stop"] = predicted_labels["stop"] * delta_t
    return predicted_labels


def _mel_width_hint(orcai_parameter: dict) -> str:
    """Tail of the width error when the mel front end is on: the width is then n_mels, not the freq_range crop."""
    mel = orcai_parameter["spectrogram"].get("mel")
    if mel is None:
        return ""
    return f": spectrogram parameter mel is set, so the width is mel.n_mels = {mel.get('n_mels')}; the model must have been trained at that width"


def predict_wav_launch(recording_path: Path | str, channel: int, model, orcai_parameter: dict, shape: dict, msgr: Messenger = Messenger(verbosity=0),
                       progressbar: tqdm = None, device_labels: dict | None = None) -> dict:
    """First half of predict_wav: spectrogram, snippets through the model and the overlap average are QUEUED on the GPU, the averaged
    probabilities are on their way to pinned host memory.  The returned state goes to predict_wav_finish; in table mode the next
    recording is launched in between, so the host half of one recording runs beside the GPU half of the next.  device_labels (a label_spec; ignored
    for a model without the native path): the label extraction is queued on the GPU as well."""
    recording_path = Path(recording_path)
    if progressbar:
        progressbar.set_description(f"{recording_path.stem}: Generating spectrogram")
        progressbar.refresh()
    native = hasattr(model, "predict_spectrogram")
    if native:
        spectrogram, _, times = make_spectrogram_device(recording_path, channel, orcai_parameter, msgr)
    else:
        spectrogram, _, times = make_spectrogram(recording_path, channel, orcai_parameter, msgr=msgr)
    delta_t = times[1] - times[0]
    if spectrogram.shape[1] != shape["input_shape"][1]:
        raise ValueError(f"Spectrogram shape ({spectrogram.shape[1]}) for {recording_path.stem} not equal to input shape ({shape['input_shape'][1]})"
                         + _mel_width_hint(orcai_parameter))
    msgr.part(f"Prediction of annotations for wav_file: {recording_path.stem}")
    if progressbar:
        progressbar.set_description(f"{recording_path.stem} - Predicting annotations")
        progressbar.refresh()
    pending = compute_aggregated_predictions(recording_path=recording_path, spectrogram=spectrogram, model=model, orcai_parameter=orcai_parameter, shape=shape,
                                             msgr=msgr, progressbar=progressbar, wait=not native, device_labels=device_labels, delta_t=delta_t)
    return {"pending": pending, "delta_t": delta_t, "orcai_parameter": orcai_parameter}


def predict_wav_finish(state: dict, label_suffix: str = "*", msgr: Messenger = Messenger(verbosity=0), thresholds=None, refine=None,
                       scores: bool = False):
    """Second half of predict_wav (host): threshold, runs of ones, label table (predict.py:298-340).  thresholds: one per label (L floats) in place
    of 0.5 on the host route; refine: resolve_refinement's dict, hysteresis and gap merging on the host route.  Labels that came from the device
    were cut by the thresholds and the refinement of their label_spec.  scores: the columns peak, peak_frame and mean on the host route
    (scores.add_scores); labels from the device carry them when their label_spec asked for them."""
    pending, orcai_parameter = state["pending"], state["orcai_parameter"]
    aggregated_predictions, overlap_count = pending.result() if isinstance(pending, PendingAggregate) else pending
    device_result = state.get("device_labels_result")
    if device_result is None and isinstance(pending, PendingAggregate) and pending.labels is not None:
        device_result = pending.labels.results()[0]
    if device_result is not None:
        return _finish_device_labels(device_result, pending.labels if isinstance(pending, PendingAggregate) else state["device_labels"],
                                     aggregated_predictions, state["delta_t"], msgr)
    time_steps_per_output_step = 2 ** len(orcai_parameter["model"]["filters"])
    row_starts, row_stops, label_names = compute_binary_predictions(aggregated_predictions=aggregated_predictions, overlap_count=overlap_count,
                                                                    calls=orcai_parameter["calls"],
                                                                    threshold=0.5 if thresholds is None else thresholds,
                                                                    **_refine_arguments(refine, time_steps_per_output_step, state["delta_t"],
                                                                                        "high_threshold", "merge_gap_rows"))
    msgr.info("converting binary predictions into start and stop frames")
    predicted_labels = compute_labels(row_starts, row_stops, label_names, time_steps_per_output_step=time_steps_per_output_step, label_suffix=label_suffix)
    if scores:
        from orcai_amd.scores import add_scores

        predicted_labels = add_scores(predicted_labels, aggregated_predictions, orcai_parameter["calls"], label_suffix, time_steps_per_output_step)
    msgr.info(f"found {len(predicted_labels)} acoustic signals")
    msgr.success("Prediction finished.")
    return predicted_labels, aggregated_predictions, state["delta_t"]


def _finish_device_labels(device_result: tuple, labels, aggregated_predictions, delta_t: float, msgr: Messenger):
    """predict_wav_finish for a recording whose labels came from orcai_extract_labels.  With duration limits the table is already the filtered one
    and carries the kernel's counts in .attrs["duration_filter"], which _save_recording reports in place of calling filter_predictions."""
    predicted_labels, n_short, n_long = device_result
    found = len(predicted_labels) + n_short + n_long
    if labels.filtered:
        predicted_labels.attrs["duration_filter"] = {"found": found, "too_short": n_short, "too_long": n_long}
    msgr.info(f"found {found} acoustic signals")
    msgr.success("Prediction finished.")
    return predicted_labels, aggregated_predictions, delta_t


def predict_wav(recording_path: Path | str, channel: int, model, orcai_parameter: dict, shape: dict, label_suffix: str = "*",
                msgr: Messenger = Messenger(verbosity=0), progressbar: tqdm = None, device_labels: bool = False, thresholds=None,
                high_thresholds=None, merge_gap=None, scores: bool = False):
    """(predicted_labels DataFrame, aggregated_predictions ndarray, delta_t) for one wav file (predict.py:367-471).  device_labels=True: the label
    table comes from orcai_extract_labels (the same table).  thresholds: a dict {label: threshold} or the path of a thresholds.json.
    high_thresholds, merge_gap (seconds): a number, a dict {label: value} or the path of such a JSON file, as for predict().  scores=True: the table
    has three more columns, peak (f64), peak_frame (in the unit of start / stop) and mean (f64) of every interval."""
    from orcai_amd.threshold_sweep import resolve_refinement, resolve_thresholds

    thresholds = resolve_thresholds(thresholds, orcai_parameter["calls"])
    refine = resolve_refinement(high_thresholds, merge_gap, thresholds, orcai_parameter["calls"])
    state = predict_wav_launch(recording_path, channel, model, orcai_parameter, shape, msgr=msgr, progressbar=progressbar,
                               device_labels=label_spec(orcai_parameter, label_suffix, thresholds=thresholds, refine=refine, scores=scores) if device_labels else None)
    return predict_wav_finish(state, label_suffix=label_suffix, msgr=msgr, thresholds=thresholds, refine=refine, scores=scores)


def _too_short(n_frames: int, snippet_length: int) -> ValueError:
    return ValueError(f"recording too short: {n_frames} spectrogram frames, one snippet needs {snippet_length}")


def _launch_batches(sources, model, orcai_parameter: dict, shape: dict, max_frames: int, msgr: Messenger = Messenger(verbosity=0),
                    device_labels: dict | None = None):
    """The GPU half of several recordings per detector pass (batch.py), as a generator of batch states.  sources: an iterable of (key, thunk),
    thunk() -> the recording's f32 cuda samples at the model's sampling rate (spectrogram.load_wav), called one by one as the batches fill.  A
    batch closes before the recording that would take its buffer past max_frames spectrogram frames; a state is yielded once the work of its batch is
    QUEUED: the front end of every recording into its rows of the batch buffer, one forward pass, one orcai_overlap_average_ragged, one copy to
    pinned memory.  state["members"] = [(key, delta_t)] in buffer order, state["failed"] = [(key, exception)]: the recordings met since the last
    state that raised (thunk errors, a spectrogram of the wrong width, too short for one snippet) and are in no batch.
    device_labels (a label_spec): one orcai_extract_labels per batch behind the average."""
    from orcai_amd import frontend as fe
    from orcai_amd.batch import Grouper, layout as batch_layout

    sp = orcai_parameter["spectrogram"]
    H, W = shape["input_shape"][0], shape["input_shape"][1]
    n_filters = len(orcai_parameter["model"]["filters"])
    grouper = Grouper(H, max_frames)
    members, failed = [], []  # members: (key, pcm, T, delta_t)

    def queue():
        state = {"members": [(key, delta_t) for key, _, _, delta_t in members], "failed": list(failed), "pending": None, "orcai_parameter": orcai_parameter}
        if members:
            lay = batch_layout([T for _, _, T, _ in members], H, 2**n_filters)
            buf = model.batch_buffer(lay)
            front = fe.get_frontend()
            for (_, pcm, T, _), o in zip(members, lay.offsets):
                front.make_spectrogram(pcm, sp, out=buf[o : o + T])
            predictions, _ = model.predict_batch(buf, lay)
            state["pending"] = aggregate_batch_device(predictions, lay, H, n_filters, device_labels=device_labels, delta_t=members[0][3])
            state["junk_snippets"], state["snippets"] = lay.junk, lay.n_total
            msgr.info(f"batch of {len(members)} recordings: {lay.n_total} snippets in one pass ({lay.junk} of them between recordings)")
        members.clear()
        failed.clear()
        grouper.close()
        return state

    for key, thunk in sources:
        try:
            pcm = thunk()
            T, K = fe.get_frontend().spectrogram_shape(pcm.numel(), sp)
            times = fe.frames_to_time(min(T, 2), sp["sampling_rate"], sp["n_overlap"])
            delta_t = times[1] - times[0]
            if K != W:
                raise ValueError(f"Spectrogram shape ({K}) for {getattr(key, 'stem', key)} not equal to input shape ({W})" + _mel_width_hint(orcai_parameter))
            if T < H:
                raise _too_short(T, H)
        except Exception as e:  # this recording alone; the batch goes on
            failed.append((key, e))
            continue
        if not grouper.fits(T):
            yield queue()
        grouper.add(T)
        members.append((key, pcm, T, delta_t))
    if members or failed:
        yield queue()


def _finish_batch(state: dict, label_suffix: str = "*", msgr: Messenger = Messenger(verbosity=0), thresholds=None, refine=None, scores: bool = False) -> list:
    """The host half of one batch state: [(key, predict_wav's triple or the exception the recording raised)], the failed ones first."""
    out = list(state["failed"])
    if state["pending"] is not None:
        labels = state["pending"].labels
        label_results = labels.results() if labels is not None else [None] * len(state["members"])
        for (key, delta_t), pair, device_result in zip(state["members"], state["pending"].results(), label_results):
            out.append((key, predict_wav_finish({"pending": pair, "delta_t": delta_t, "orcai_parameter": state["orcai_parameter"],
                                                 "device_labels_result": device_result, "device_labels": labels}, label_suffix=label_suffix, msgr=msgr,
                                                thresholds=thresholds, refine=refine, scores=scores)))
    return out


def _run_batches(states, finish) -> None:
    """One batch deep: the GPU half of batch b + 1 is queued (the next state is drawn from the generator) before finish(state of batch b) runs."""
    in_flight = None
    for state in states:
        if in_flight is not None:
            finish(in_flight)
        in_flight = state
    if in_flight is not None:
        finish(in_flight)


def predict_wavs_launch(items, model, orcai_parameter: dict, shape: dict, max_frames: int | None = None, msgr: Messenger = Messenger(verbosity=0),
                        device_labels: dict | None = None):
    """First half of predict_wavs: a generator of batch states (_launch_batches) whose keys are the indices into `items`."""
    from orcai_amd.batch import DEFAULT_MAX_FRAMES
    from orcai_amd.spectrogram import load_wav

    sr = orcai_parameter["spectrogram"]["sampling_rate"]
    sources = ((i, lambda path=path, channel=channel: load_wav(Path(path), sr, channel, msgr)) for i, (path, channel) in enumerate(items))
    return _launch_batches(sources, model, orcai_parameter, shape, DEFAULT_MAX_FRAMES if max_frames is None else max_frames, msgr=msgr,
                           device_labels=device_labels)


def predict_wavs_finish(state: dict, label_suffix: str = "*", msgr: Messenger = Messenger(verbosity=0), thresholds=None, refine=None,
                        scores: bool = False) -> list:
    """Second half (host): [(index into items, (predicted_labels, aggregated_predictions, delta_t) or the exception that item raised)]."""
    return _finish_batch(state, label_suffix=label_suffix, msgr=msgr, thresholds=thresholds, refine=refine, scores=scores)


def predict_wavs(items, model, orcai_parameter: dict, shape: dict, label_suffix: str = "*", max_frames: int | None = None,
                 msgr: Messenger = Messenger(verbosity=0), device_labels: bool = False, thresholds=None, high_thresholds=None, merge_gap=None,
                 scores: bool = False) -> list:
    """predict_wav for every (path, channel) of `items`, several recordings per detector pass: batches of at most max_frames spectrogram frames
    (batch.DEFAULT_MAX_FRAMES: an hour's worth) go through ONE forward pass and ONE overlap average, the host half of a batch runs beside the GPU
    half of the next.  Returns, per item, what predict_wav returns for it -- the same label table, the same f64 probabilities, the same delta_t --
    or the exception it raised (a missing file, a recording shorter than one snippet); the other items are unaffected.
    A model without the native batch path (the reference's duck-typed ``.predict`` boundary) runs item by item.
    device_labels=True: the label tables of a batch come from one orcai_extract_labels (the same tables).  thresholds, high_thresholds, merge_gap,
    scores: as for predict_wav."""
    from orcai_amd.threshold_sweep import resolve_refinement, resolve_thresholds

    thresholds = resolve_thresholds(thresholds, orcai_parameter["calls"])
    refine = resolve_refinement(high_thresholds, merge_gap, thresholds, orcai_parameter["calls"])
    listed = None if thresholds is None else dict(zip(orcai_parameter["calls"], thresholds))
    items = list(items)
    results = [None] * len(items)
    if not hasattr(model, "predict_batch"):
        for i, (path, channel) in enumerate(items):
            try:
                results[i] = predict_wav(path, channel, model, orcai_parameter, shape, label_suffix=label_suffix, msgr=msgr, device_labels=device_labels,
                                         thresholds=listed, high_thresholds=high_thresholds, merge_gap=merge_gap, scores=scores)
            except Exception as e:
                results[i] = e
        return results

    def finish(state):
        for i, result in predict_wavs_finish(state, label_suffix=label_suffix, msgr=msgr, thresholds=thresholds, refine=refine, scores=scores):
            results[i] = result

    _run_batches(predict_wavs_launch(items, model, orcai_parameter, shape, max_frames=max_frames, msgr=msgr,
                                     device_labels=label_spec(orcai_parameter, label_suffix, thresholds=thresholds, refine=refine, scores=scores)
                                     if device_labels else None),
                 finish)
    return results


def save_predictions(predicted_labels: pd.DataFrame, output_path: Path | str, delta_t: float, msgr: Messenger = Messenger(verbosity=0)) -> None:
    """Tab-separated start/stop/label with header, seconds rounded to 4 places (predict.py:474-499)."""
    predicted_labels = _convert_times_to_seconds(predicted_labels, delta_t)
    predicted_labels[["start", "stop", "label"]].round(4).to_csv(output_path, sep="\t", index=False)
    msgr.info(f"Predictions saved to {output_path}")


def save_prediction_scores(predicted_labels: pd.DataFrame, output_path: Path | str, delta_t: float, msgr: Messenger = Messenger(verbosity=0)) -> None:
    """save_predictions' sibling for a scored table: <stem>_scores.csv next to the label file, one line per line of the label file in
    its order.  Tab-separated start / stop / label / peak_time / peak / mean with header; times in seconds rounded to 4 places as save_predictions
    rounds them, peak and mean rounded to 6."""
    output_path = Path(output_path)
    scores_path = output_path.with_name(f"{output_path.stem}_scores.csv")
    seconds = {name: np.round(predicted_labels[column].to_numpy() * delta_t, 4) for name, column in (("start", "start"), ("stop", "stop"), ("peak_time", "peak_frame"))}
    pd.DataFrame({"start": seconds["start"], "stop": seconds["stop"], "label": predicted_labels["label"].to_numpy(), "peak_time": seconds["peak_time"],
                  "peak": np.round(predicted_labels["peak"].to_numpy(), 6), "mean": np.round(predicted_labels["mean"].to_numpy(), 6)}).to_csv(
        scores_path, sep="\t", index=False)
    msgr.info(f"Interval scores saved to {scores_path}")


def save_prediction_probabilities(aggregated_predictions: np.ndarray, orcai_parameter: dict, delta_t: float, output_path: Path | str,
                                  msgr: Messenger = Messenger(verbosity=0)) -> None:
    """predict.py:502-531."""
    output_path = Path(output_path)
    predictions_path = output_path.with_name(f"{output_path.stem}_probabilities.csv.gz")
    pd.DataFrame(aggregated_predictions, columns=orcai_parameter["calls"], index=delta_t * range(len(aggregated_predictions))).to_csv(
        predictions_path, index_label="time", compression="gzip")
    msgr.info(f"Prediction probabilities saved to {predictions_path}")


def _checked_output_path(recording_path: Path, channel: int, orcai_parameter: dict, output_path: Path | str = "default", overwrite: bool = False,
                         msgr: Messenger = Messenger(verbosity=0), scores: bool = False):
    """predict.py:534-575: the output path of one recording and the overwrite check.  scores: the check covers <stem>_scores.csv as well."""
    if output_path is not None:
        if output_path == "default":
            filename = f"{recording_path.stem}_c{channel}_{orcai_parameter['name']}_predicted.txt"
            output_path = recording_path.with_name(filename)
        else:
            output_path = Path(output_path)
        msgr.info(f"Output file: {output_path}")
        if output_path.exists():
            if overwrite:
                msgr.warning(f"Output file {output_path} already exists. Overwriting.")
            else:
                raise FileExistsError(f"Annotation file already exists: {output_path}")
        scores_path = output_path.with_name(f"{output_path.stem}_scores.csv")
        if scores and scores_path.exists():
            if overwrite:
                msgr.warning(f"Output file {scores_path} already exists. Overwriting.")
            else:
                raise FileExistsError(f"Score file already exists: {scores_path}")
    return output_path


def _launch_recording(recording_path: Path | str, channel: int, model, orcai_parameter: dict, shape: dict, output_path: Path | str = "default",
                      overwrite: bool = False, msgr: Messenger = Messenger(verbosity=0), progressbar: tqdm = None, device_labels: dict | None = None,
                      scores: bool = False) -> dict:
    """predict.py:534-575: output path and overwrite check, then the GPU half of the recording (queued, not waited for)."""
    recording_path = Path(recording_path)
    output_path = _checked_output_path(recording_path, channel, orcai_parameter, output_path, overwrite, msgr, scores=scores)
    state = predict_wav_launch(recording_path=recording_path, channel=channel, model=model, orcai_parameter=orcai_parameter, shape=shape, msgr=msgr,
                               progressbar=progressbar, device_labels=device_labels)
    state["output_path"] = output_path
    return state


def _save_recording(result: tuple, output_path, orcai_parameter: dict, save_probabilities: bool = False, call_duration_limits: (Path | str) | dict = None,
                    label_suffix: str = "*", msgr: Messenger = Messenger(verbosity=0), scores: bool = False) -> None:
    """predict.py:576-632 after the labels: optional duration filter, files.  scores: the score file of the (filtered) table beside the label file."""
    predicted_labels, aggregated_predictions, delta_t = result
    counts = predicted_labels.attrs.get("duration_filter")
    if counts is not None:  # device labels: the kernel judged every interval, the table is the filtered one
        msgr.part("Filtering predictions")
        msgr.part("Filtering calls based on duration")
        if counts["found"] > 0:
            msgr.info(f"Discarding {counts['too_long'] + counts['too_short']} calls based on duration (too short: {counts['too_short']}, too long: {counts['too_long']})")
            msgr.success("Filtering predictions finished.")
    elif call_duration_limits is not None:
        predicted_labels = filter_predictions(predicted_labels, delta_t=delta_t, call_duration_limits=call_duration_limits, label_suffix=label_suffix, msgr=msgr)
    save_predictions(predicted_labels=predicted_labels, output_path=output_path, delta_t=delta_t, msgr=msgr)
    if scores and output_path is not None:
        save_prediction_scores(predicted_labels=predicted_labels, output_path=output_path, delta_t=delta_t, msgr=msgr)
    if save_probabilities:
        save_prediction_probabilities(aggregated_predictions=aggregated_predictions, orcai_parameter=orcai_parameter, delta_t=delta_t, output_path=output_path, msgr=msgr)


def _finish_recording(state: dict, save_probabilities: bool = False, call_duration_limits: (Path | str) | dict = None, label_suffix: str = "*",
                      msgr: Messenger = Messenger(verbosity=0), thresholds=None, refine=None, scores: bool = False) -> None:
    """predict.py:576-632: the host half -- labels, optional duration filter, files."""
    result = predict_wav_finish(state, label_suffix=label_suffix, msgr=msgr, thresholds=thresholds, refine=refine, scores=scores)
    _save_recording(result, state["output_path"], state["orcai_parameter"], save_probabilities=save_probabilities, call_duration_limits=call_duration_limits,
                    label_suffix=label_suffix, msgr=msgr, scores=scores)


def _predict_and_save(recording_path: Path | str, channel: int, model, orcai_parameter: dict, shape: dict, output_path: Path | str = "default",
                      overwrite: bool = False, save_probabilities: bool = False, call_duration_limits: (Path | str) | dict = None,
                      label_suffix: str = "*", msgr: Messenger = Messenger(verbosity=0), progressbar: tqdm = None, device_labels: dict | None = None,
                      thresholds=None, refine=None, scores: bool = False) -> None:
    """predict.py:534-632."""
    state = _launch_recording(recording_path, channel, model, orcai_parameter, shape, output_path=output_path, overwrite=overwrite, msgr=msgr,
                              progressbar=progressbar, device_labels=device_labels, scores=scores)
    _finish_recording(state, save_probabilities=save_probabilities, call_duration_limits=call_duration_limits, label_suffix=label_suffix, msgr=msgr,
                      thresholds=thresholds, refine=refine, scores=scores)


def _predict_all_channels(recording_path: Path, model, orcai_parameter: dict, shape: dict, output_path: Path | str = "default", overwrite: bool = False,
                          save_probabilities: bool = False, call_duration_limits: (Path | str) | dict = None, label_suffix: str = "*",
                          msgr: Messenger = Messenger(verbosity=0), device_labels: dict | None = None, thresholds=None, refine=None,
                          scores: bool = False) -> None:
    """predict(channel="all"): one read and one upload of the file, every channel decoded by orcai_pcm_decode_planar, the channels as ONE batch through
    the detector.  One output file per channel, under the name -- and with the bytes -- predict(channel=c) gives it."""
    from orcai_amd.spectrogram import load_wav_all

    if output_path is not None and output_path != "default":
        raise ValueError("channel='all' writes one file per channel next to the recording: output_path must be 'default' (or None)")
    pcms = load_wav_all(recording_path, orcai_parameter["spectrogram"]["sampling_rate"], msgr)
    paths = {c: _checked_output_path(recording_path, c, orcai_parameter, output_path, overwrite, msgr, scores=scores) for c in range(1, len(pcms) + 1)}
    sources = ((c, lambda pcm=pcm: pcm) for c, pcm in enumerate(pcms, start=1))
    errors = []

    def finish(state):
        for c, result in _finish_batch(state, label_suffix=label_suffix, msgr=msgr, thresholds=thresholds, refine=refine, scores=scores):
            if isinstance(result, Exception):
                errors.append(result)
                continue
            _save_recording(result, paths[c], orcai_parameter, save_probabilities=save_probabilities, call_duration_limits=call_duration_limits,
                            label_suffix=label_suffix, msgr=msgr, scores=scores)

    total = sum(int(pcm.numel()) for pcm in pcms) // orcai_parameter["spectrogram"]["n_overlap"] + (shape["input_shape"][0] + 1) * len(pcms)
    _run_batches(_launch_batches(sources, model, orcai_parameter, shape, max_frames=total, msgr=msgr, device_labels=device_labels), finish)  # max_frames: all channels in one batch
    if errors:
        raise errors[0]  # every channel has the same length: the single-channel call's error


def _predict_table_batched(recording_table: pd.DataFrame, model, orcai_parameter: dict, shape: dict, batch_frames: int, overwrite: bool,
                           save_probabilities: bool, call_duration_limits, label_suffix: str, msgr: Messenger, progressbar: tqdm,
                           device_labels: dict | None = None, thresholds=None, refine=None, scores: bool = False) -> None:
    """Table mode with batch_frames > 0: the rows of the table in order, grouped into detector passes of at most batch_frames spectrogram frames.
    Per recording the output path, the overwrite check, the files and the error line are those of the one-by-one loop; one batch deep, so the host
    half of a batch (labels, files) runs beside the GPU half of the next."""
    from orcai_amd.spectrogram import load_wav

    quiet = Messenger(verbosity=0)
    sr = orcai_parameter["spectrogram"]["sampling_rate"]
    outputs = {}

    def error(i, e):
        msgr.error(f"Error predicting {recording_table.loc[i, 'recording']}: {e.args[0] if e.args else e}")  # predict.py:752-755: log and continue

    def sources():
        for i in progressbar:
            path = Path(recording_table.loc[i, "base_dir_recording"]).joinpath(recording_table.loc[i, "rel_recording_path"])
            channel = recording_table.loc[i, "channel"]
            try:
                outputs[i] = _checked_output_path(path, channel, orcai_parameter, recording_table.loc[i, "output_path"], overwrite, quiet, scores=scores)
            except Exception as e:
                error(i, e)
                continue
            yield i, lambda path=path, channel=channel: load_wav(path, sr, channel, quiet)

    def finish(state):
        for i, result in _finish_batch(state, label_suffix=label_suffix, msgr=quiet, thresholds=thresholds, refine=refine, scores=scores):
            try:
                if isinstance(result, Exception):
                    raise result
                _save_recording(result, outputs[i], orcai_parameter, save_probabilities=save_probabilities, call_duration_limits=call_duration_limits,
                                label_suffix=label_suffix, msgr=quiet, scores=scores)
            except Exception as e:
                error(i, e)

    _run_batches(_launch_batches(sources(), model, orcai_parameter, shape, batch_frames, msgr=quiet, device_labels=device_labels), finish)


def predict(recording_path: str | Path, channel: int | str = 1, model_dir: str | Path = DEFAULT_MODEL_DIR, output_path: str | Path = "default",
            overwrite: bool = False, save_probabilities: bool = False, base_dir_recording: str | Path | None = None,
            call_duration_limits: str | Path | None = None, label_suffix: str = "*", verbosity: int = 2, msgr: Messenger | None = None,
            batch_frames: int = 0, device_labels: bool = False, thresholds: str | Path | dict | None = None,
            high_thresholds: float | str | Path | dict | None = None, merge_gap: float | str | Path | dict | None = None, scores: bool = False) -> None:
    """Predict calls in a wav file or in every recording of a recording-table CSV (predict.py:635-757).
    channel="all" (a wav file): every channel of the file from one read of its bytes, one output file per channel.
    batch_frames > 0 (a table): consecutive recordings go through the detector in batches of at most batch_frames spectrogram frames
    (predict_wavs' path: many short clips fill the GPU that one of them cannot); 0, the default, is one detector pass per recording.  The files
    are the same bytes either way.
    device_labels=True: threshold, run detection, sort and duration filter of every route run on the GPU (orcai_extract_labels) and only the
    intervals found come back; without save_probabilities the averaged probabilities never leave the device.  The files are the same bytes.
    Ignored for a model without the native path.
    thresholds: a dict {label: threshold} or the path of such a JSON file (the thresholds.json of ``orcai test --threshold-sweep``): label l is cut at
    thresholds[l] in place of 0.5 on every route, with device_labels or without.  Labels it does not name keep 0.5; a label the model does not have
    raises ValueError before the model is loaded.
    high_thresholds, merge_gap: hysteresis and gap merging, each a number for all labels, a dict {label: value} or the path of such a
    JSON file.  A stretch above its label's threshold is an interval only if it reaches the label's high threshold somewhere, and kept intervals of
    one label at most merge_gap seconds apart are written as one.  Labels not named keep high = threshold and gap 0; both off (None) is the cut above
    alone, through the calls made without them.  An unknown label, a negative gap or a high threshold below the label's threshold raises ValueError
    before the model is loaded.  Every route, with device_labels (orcai_extract_labels_refined) or without: the same bytes.
    scores=True: next to every label file, which stays byte for byte the file written without the option, <stem>_scores.csv with one
    line per line of the label file: start, stop, label, peak_time, peak and mean -- the largest averaged probability of the interval, where it is
    attained, and the interval's mean probability (the rows of merged gaps count).  Every route; with device_labels the scores come from
    orcai_interval_scores and the file is the same bytes.  The overwrite check covers the score file."""
    if msgr is None:
        msgr = Messenger(verbosity=verbosity, title="Predicting calls")
    model_dir = Path(model_dir)
    recording_path = Path(recording_path)
    refine = None
    if thresholds is not None or high_thresholds is not None or merge_gap is not None:
        from orcai_amd.threshold_sweep import resolve_refinement, resolve_thresholds

        calls = read_json(model_dir.joinpath("orcai_parameter.json"))["calls"]
        thresholds = resolve_thresholds(thresholds, calls)
        refine = resolve_refinement(high_thresholds, merge_gap, thresholds, calls)
    msgr.part(f"Loading model: {model_dir.stem}")
    model, orcai_parameter, shape = load_orcai_model(model_dir)
    spec = None
    if device_labels and hasattr(model, "predict_spectrogram"):
        spec = label_spec(orcai_parameter, label_suffix, call_duration_limits, probabilities=save_probabilities, thresholds=thresholds, refine=refine,
                          scores=scores)
    if recording_path.suffix == ".wav" and channel == "all" and hasattr(model, "predict_batch"):
        return _predict_all_channels(recording_path, model, orcai_parameter, shape, output_path=output_path, overwrite=overwrite,
                                     save_probabilities=save_probabilities, call_duration_limits=call_duration_limits, label_suffix=label_suffix, msgr=msgr,
                                     device_labels=spec, thresholds=thresholds, refine=refine, scores=scores)
    if recording_path.suffix == ".wav":
        return _predict_and_save(recording_path=recording_path, channel=channel, model=model, orcai_parameter=orcai_parameter, shape=shape,
                                 output_path=output_path, overwrite=overwrite, save_probabilities=save_probabilities,
                                 call_duration_limits=call_duration_limits, label_suffix=label_suffix, msgr=msgr, progressbar=None, device_labels=spec,
                                 thresholds=thresholds, refine=refine, scores=scores)
    elif recording_path.suffix == ".csv":
        recording_table = pd.read_csv(recording_path)
    else:
        raise ValueError("Recording file must be a wav or csv file")
    if base_dir_recording is not None:
        recording_table["base_dir_recording"] = base_dir_recording
    if (output_path is not None) & (output_path != "default"):
        recording_table["output_path"] = [Path(output_path).joinpath(recording + "_" + model_dir.stem + "_predicted.txt") for recording in recording_table["recording"]]
    else:
        recording_table["output_path"] = output_path
    # one process per GPU (torchrun): each rank takes its own recordings; there is no data-path collective
    from orcai_amd import parallel

    rank, size, _ = parallel.init()
    if size > 1:
        mine = parallel.shard_indices(len(recording_table), rank, size)
        recording_table = recording_table.iloc[mine]
    msgr.part(f"Predicting annotations for {len(recording_table)} wav files" + (f" (rank {rank} of {size})" if size > 1 else ""))
    progressbar = tqdm(recording_table.index, desc="Starting ...", unit="file", disable=verbosity < 1)
    from orcai_amd import wavio

    # read the next recordings into page-locked memory on background threads while the GPU works on the current one (the samples are decoded on the
    # device: load_wav)
    wavio.set_prefetcher(wavio.WavPrefetcher([Path(recording_table.loc[i, "base_dir_recording"]).joinpath(recording_table.loc[i, "rel_recording_path"])
                                              for i in recording_table.index], raw=True))
    quiet = Messenger(verbosity=0)
    if batch_frames > 0 and hasattr(model, "predict_batch"):
        _predict_table_batched(recording_table, model, orcai_parameter, shape, batch_frames, overwrite=overwrite, save_probabilities=save_probabilities,
                               call_duration_limits=call_duration_limits, label_suffix=label_suffix, msgr=msgr, progressbar=progressbar, device_labels=spec,
                               thresholds=thresholds, refine=refine, scores=scores)
        wavio.set_prefetcher(None)
        msgr.success("Predictions finished.")
        return
    # one recording deep: the GPU half of recording i is queued before the host half of recording i - 1 (threshold, label table, files) runs
    in_flight = None  # (table index, state)

    def finish(entry):
        j, state = entry
        try:
            _finish_recording(state, save_probabilities=save_probabilities, call_duration_limits=call_duration_limits, label_suffix=label_suffix, msgr=quiet,
                              thresholds=thresholds, refine=refine, scores=scores)
        except Exception as e:  # predict.py:752-755: log and continue with the next recording
            msgr.error(f"Error predicting {recording_table.loc[j, 'recording']}: {e.args[0] if e.args else e}")

    for i in progressbar:
        launched = None
        try:
            launched = (i, _launch_recording(recording_path=Path(recording_table.loc[i, "base_dir_recording"]).joinpath(recording_table.loc[i, "rel_recording_path"]),
                                             channel=recording_table.loc[i, "channel"], model=model, orcai_parameter=orcai_parameter, shape=shape,
                                             output_path=recording_table.loc[i, "output_path"], overwrite=overwrite, msgr=quiet, progressbar=progressbar,
                                             device_labels=spec, scores=scores))
        except Exception as e:  # predict.py:752-755
            msgr.error(f"Error predicting {recording_table.loc[i, 'recording']}: {e.args[0] if e.args else e}")
        if in_flight is not None:
            finish(in_flight)
        in_flight = launched
    if in_flight is not None:
        finish(in_flight)
    wavio.set_prefetcher(None)
    msgr.success("Predictions finished.")
