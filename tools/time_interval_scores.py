"""Times the per-interval scores on cuda:0.  Cases and method are tools/time_label_refine.py's.

  kernel    orcai_interval_scores alone, and the extraction call followed by it (HIP events, median of 9 after 2 untimed calls), on synthetic averaged
            probabilities of an hour (42187 rows); the host twin (scores.interval_scores, wall clock, median of 9) on the same inputs:
              sparse7             7 labels, sparse calls of 8 rows, behind orcai_extract_labels_per_label;
              hour_run64          64 columns above the threshold for the whole hour: 64 runs of 165 tiles each;
              alternating64       64 columns alternating every row: 1.35 million runs of one row;
              alternating64_gap1  the same behind orcai_extract_labels_refined with a gap of one row: 64 runs of the whole hour.
  clips60   predict(table, batch_frames=675000) on 256 mono PCM16 clips of 60 s at 48 kHz (8 synthetic recordings, hard-linked to 256 names; orcai-V1
            shape, seeded untrained weights), on the host route and with device_labels, with scores off and on: four routes alternating for --reps
            rounds after --warmup untimed ones.  With the option off predict() makes the calls it made before it existed.

Every case runs in a child process of its own under a time limit; a case that fails ends the run.

    python tools/time_interval_scores.py [--reps 5] [--warmup 1] [--clips 256] [--out profiles/interval_scores_mi355x.json]
"""

from __future__ import annotations

import argparse
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from tools.time_label_refine import spread  # noqa: E402
from tools.time_predict_batch import HOUR_FRAMES, alternate, make_model_dir, summary  # noqa: E402

CASES = ("kernel", "clips60")


def run_kernel(a) -> dict:
    import numpy as np
    import torch

    from orcai_amd import _native as N
    from orcai_amd import scores as Z

    lib, st = N.lib(), N.stream_ptr()
    S = HOUR_FRAMES // 16
    rng = np.random.default_rng(0)
    sparse = np.repeat(np.where(rng.random((S // 8 + 1, 7)) < 0.02, 0.6, 0.1), 8, axis=0)[:S]
    alternating = np.where(np.arange(S)[:, None] % 2 == 0, 0.9, 0.0) + np.zeros((S, 64))
    shapes = {"sparse7": (sparse, None), "hour_run64": (np.full((S, 64), 0.6), None), "alternating64": (alternating, None), "alternating64_gap1": (alternating, 1)}
    doc = dict(rows=S, threshold=1.0, max_count=2.0)
    for name, (host, gap) in shapes.items():
        L = host.shape[1]
        agg, cnt = torch.from_numpy(np.ascontiguousarray(host)).cuda(), torch.full((S,), 2.0, dtype=torch.float64, device="cuda")
        table = torch.tensor([[0, 0, S, 0]], dtype=torch.int64, device="cuda")
        rank = torch.arange(L, dtype=torch.int32, device="cuda")
        low = torch.full((L,), 1.0, dtype=torch.float64, device="cuda")
        gaps = torch.full((L,), gap or 0, dtype=torch.int32, device="cuda")
        capacity = L * ((S + 1) // 2) + 1
        runs = torch.empty((capacity, 4), dtype=torch.int32, device="cuda")
        offsets = torch.empty(2, dtype=torch.int64, device="cuda")
        scores = torch.empty((capacity, 3), dtype=torch.int64, device="cuda")
        eager = torch.empty((4096, 3), dtype=torch.int64, device="cuda")
        refined = gap is not None
        ws_bytes = (lib.orcai_extract_labels_refined_workspace_bytes if refined else lib.orcai_extract_labels_workspace_bytes)(L, 1, S)
        score_bytes = lib.orcai_interval_scores_workspace_bytes(L, 1, S)
        ws, score_ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda"), torch.empty(score_bytes, dtype=torch.uint8, device="cuda")
        tail = (N.ptr(rank), None, 256 / 48000, 16, N.ptr(runs), capacity, N.ptr(offsets), N.ptr(ws), ws_bytes, st)

        def extract():
            if refined:
                N.check(lib.orcai_extract_labels_refined(N.ptr(agg), N.ptr(cnt), L, N.ptr(table), 1, S, N.ptr(low), N.ptr(low), N.ptr(gaps), *tail), "refined")
            else:
                N.check(lib.orcai_extract_labels_per_label(N.ptr(agg), N.ptr(cnt), L, N.ptr(table), 1, S, N.ptr(low), *tail), "per_label")

        def score():
            N.check(lib.orcai_interval_scores(N.ptr(agg), L, N.ptr(table), 1, S, N.ptr(runs), N.ptr(offsets), capacity, N.ptr(scores), N.ptr(eager), 4096,
                                              N.ptr(score_ws), score_bytes, st), "scores")

        def both():
            extract()
            score()

        extract()
        ms = {"extract": [], "scores": [], "extract_then_scores": []}
        for i in range(2 + 9):
            for route, call in (("extract", extract), ("scores", score), ("extract_then_scores", both)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                call()
                e1.record()
                e1.synchronize()
                if i >= 2:
                    ms[route].append(e0.elapsed_time(e1))
        found = int(offsets[1])
        host_runs = runs[:found].cpu().numpy()
        twin = []
        for i in range(2 + 9):
            t0 = time.perf_counter()
            peak, sums, rows = Z.interval_scores(host, host_runs[:, 0], host_runs[:, 1], host_runs[:, 2])
            if i >= 2:
                twin.append((time.perf_counter() - t0) * 1e3)
        words = scores[:found].cpu().numpy()
        same = words[:, 0].tobytes() == peak.tobytes() and words[:, 1].tobytes() == sums.tobytes() and words[:, 2].tobytes() == rows.tobytes()
        doc[name] = dict(labels=L, gap_rows=gap, runs=found, call="orcai_extract_labels_refined" if refined else "orcai_extract_labels_per_label",
                         extract=spread(ms["extract"]), scores=spread(ms["scores"]), extract_then_scores=spread(ms["extract_then_scores"]),
                         host_twin=spread(twin), same_bytes_as_host_twin=bool(same), workspace_bytes=int(score_bytes),
                         bytes_read_first_launch=int(S * L * 8), bytes_written=int(24 * found))
    return doc


def run_clips(seconds: float, a) -> dict:
    import numpy as np
    import pandas as pd

    from orcai_amd import predict as P
    from orcai_amd import wavio
    from orcai_amd.synthetic import synth_recording

    tmp = Path(tempfile.mkdtemp(prefix="orcai_scores_"))
    try:
        model_dir, (model, param, shape) = make_model_dir(tmp)
        clips = tmp / "clips"
        clips.mkdir()
        distinct = []
        for i in range(8):
            p = clips / f"src{i}.wav"
            wavio.write_wav_pcm16(p, synth_recording(seconds, 48000, seed=100 + i), 48000)
            distinct.append(p)
        names = [f"clip{i:03d}" for i in range(a.clips)]
        for i, n in enumerate(names):
            try:
                os.link(distinct[i % 8], clips / f"{n}.wav")
            except OSError:
                shutil.copyfile(distinct[i % 8], clips / f"{n}.wav")
            (clips / f"{n}.wav").read_bytes()
        pd.DataFrame({"recording": names, "base_dir_recording": [str(clips)] * len(names), "rel_recording_path": [f"{n}.wav" for n in names],
                      "channel": [1] * len(names)}).to_csv(tmp / "table.csv", index=False)
        _, agg, _ = P.predict_wav(distinct[0], 1, model, param, shape)
        low = {c: float(2 * np.quantile(agg[:, i], 0.5)) for i, c in enumerate(param["calls"])}
        routes = {}
        for device in (False, True):
            for on in (False, True):
                name = ("device" if device else "host") + ("_scores" if on else "_plain")
                (tmp / name).mkdir()
                routes[name] = lambda name=name, device=device, on=on: P.predict(
                    tmp / "table.csv", model_dir=model_dir, output_path=tmp / name, overwrite=True, verbosity=0, batch_frames=HOUR_FRAMES, device_labels=device,
                    thresholds=low, scores=on)
        audio = seconds * a.clips
        times = alternate(routes, a.reps, a.warmup)
        doc = dict(clips=a.clips, seconds_each=seconds, audio_seconds=audio, batch_frames=HOUR_FRAMES, thresholds=low)
        for name in routes:
            doc[name] = summary(times[name], audio)
            doc[name]["intervals"] = sum(len(f.read_text().strip().split("\n")) - 1 for f in (tmp / name).iterdir() if f.suffix == ".txt")
        labels = lambda folder: {f.name: f.read_bytes() for f in (tmp / folder).iterdir() if f.suffix == ".txt"}  # noqa: E731
        score_files = lambda folder: {f.name: f.read_bytes() for f in (tmp / folder).iterdir() if f.name.endswith("_scores.csv")}  # noqa: E731
        doc["same_label_files"] = labels("host_plain") == labels("host_scores") == labels("device_plain") == labels("device_scores") and len(labels("host_plain")) == a.clips
        doc["same_score_files"] = score_files("host_scores") == score_files("device_scores") and len(score_files("host_scores")) == a.clips
        return doc
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--clips", type=int, default=256)
    ap.add_argument("--timeout", type=int, default=420, help="seconds a case may take")
    ap.add_argument("--case", choices=CASES, default=None, help="run one case in this process and print its JSON line (what the parent starts)")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "interval_scores_mi355x.json"))
    a = ap.parse_args()
    if a.case is not None:
        import torch

        torch.cuda.set_device(0)
        doc = run_kernel(a) if a.case == "kernel" else run_clips(60.0, a)
        doc["device"] = torch.cuda.get_device_name(0)
        print("RESULT " + json.dumps(doc), flush=True)
        return
    doc = dict(model="orcai-V1 shape, f32, untrained seeded weights", reps=a.reps, warmup=a.warmup, cases={})
    for case in CASES:  # each GPU step in a child of its own, under its own time limit; the first failure ends the run
        cmd = [sys.executable, str(Path(__file__).resolve()), "--case", case, "--reps", str(a.reps), "--warmup", str(a.warmup), "--clips", str(a.clips)]
        done = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=a.timeout)  # the child's progress lines (stderr) pass through
        lines = [ln for ln in done.stdout.splitlines() if ln.startswith("RESULT ")]
        if done.returncode != 0 or not lines:
            sys.stderr.write(done.stdout[-2000:])
            raise SystemExit(f"case {case} failed with exit status {done.returncode}")
        doc["cases"][case] = json.loads(lines[-1][len("RESULT "):])
        print(case, json.dumps(doc["cases"][case]), flush=True)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    main()
