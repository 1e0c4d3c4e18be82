"""Times label extraction with hysteresis thresholds and gap merging on cuda:0.

  kernel    orcai_extract_labels_refined alone (HIP events, median of 9 after 2 untimed calls) on synthetic averaged probabilities of an hour
            (42187 rows), against orcai_extract_labels_per_label on the same probabilities in the same process, the two alternating:
              sparse7        7 labels, sparse calls of 8 rows, a fifth of them reaching the high threshold, gap 2 rows;
              alternating64  64 columns alternating every row, gap 1: 21094 candidates per column become one run each;
              hour_run64     64 columns above the low threshold for the whole hour, the only high row the last one.
  clips60   predict(table, batch_frames=675000) on 256 mono PCM16 clips of 60 s at 48 kHz (8 synthetic recordings, hard-linked to 256 names; orcai-V1
            shape, seeded untrained weights), on the host route and with device_labels, with --high-thresholds / --merge-gap on and off: four routes
            alternating for --reps rounds after --warmup untimed ones.  The thresholds are quantiles of the first clip's own probabilities (the
            median and the 80 % quantile), the gap 0.2 s.  With the options off predict() makes the calls it made before they existed.

Every case runs in a child process of its own under a time limit; a case that fails ends the run.

    python tools/time_label_refine.py [--reps 5] [--warmup 1] [--clips 256] [--out profiles/label_refine_mi355x.json]
"""

from __future__ import annotations

import argparse
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from tools.time_predict_batch import HOUR_FRAMES, alternate, make_model_dir, summary  # noqa: E402

CASES = ("kernel", "clips60")


def spread(ms: list) -> dict:
    return dict(median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms), ms=[round(x, 4) for x in ms])


def run_kernel(a) -> dict:
    import numpy as np
    import torch

    from orcai_amd import _native as N

    lib, st = N.lib(), N.stream_ptr()
    S = HOUR_FRAMES // 16
    rng = np.random.default_rng(0)
    sparse = np.repeat(np.where(rng.random((S // 8 + 1, 7)) < 0.02, 0.6, 0.1), 8, axis=0)[:S]
    sparse[::8] = np.where((sparse[::8] > 0.5) & (rng.random(sparse[::8].shape) < 0.2), 0.9, sparse[::8])
    hour_run = np.full((S, 64), 0.6)
    hour_run[-1] = 0.9
    shapes = {"sparse7": (sparse, 2), "alternating64": (np.where(np.arange(S)[:, None] % 2 == 0, 0.9, 0.0) + np.zeros((S, 64)), 1), "hour_run64": (hour_run, 0)}
    doc = dict(rows=S, low_threshold=1.0, high_threshold=1.6, max_count=2.0)
    for name, (host, gap) in shapes.items():
        L = host.shape[1]
        agg, cnt = torch.from_numpy(np.ascontiguousarray(host)).cuda(), torch.full((S,), 2.0, dtype=torch.float64, device="cuda")
        table = torch.tensor([[0, 0, S, 0]], dtype=torch.int64, device="cuda")
        rank = torch.arange(L, dtype=torch.int32, device="cuda")
        limits = torch.tensor([[0.2, 2.0]] * L, dtype=torch.float64, device="cuda")
        low, high = torch.full((L,), 1.0, dtype=torch.float64, device="cuda"), torch.full((L,), 1.6, dtype=torch.float64, device="cuda")
        gaps = torch.full((L,), gap, dtype=torch.int32, device="cuda")
        capacity = L * ((S + 1) // 2) + 1
        runs = torch.empty((capacity, 4), dtype=torch.int32, device="cuda")
        offsets = torch.empty(2, dtype=torch.int64, device="cuda")
        sizes = {"per_label": lib.orcai_extract_labels_workspace_bytes(L, 1, S), "refined": lib.orcai_extract_labels_refined_workspace_bytes(L, 1, S)}
        ws = torch.empty(max(sizes.values()), dtype=torch.uint8, device="cuda")
        tail = (N.ptr(rank), N.ptr(limits), 256 / 48000, 16, N.ptr(runs), capacity, N.ptr(offsets), N.ptr(ws))

        def per_label():
            N.check(lib.orcai_extract_labels_per_label(N.ptr(agg), N.ptr(cnt), L, N.ptr(table), 1, S, N.ptr(low), *tail, sizes["per_label"], st), "per_label")

        def refined():
            N.check(lib.orcai_extract_labels_refined(N.ptr(agg), N.ptr(cnt), L, N.ptr(table), 1, S, N.ptr(low), N.ptr(high), N.ptr(gaps), *tail, sizes["refined"], st),
                    "refined")

        ms, found = {"per_label": [], "refined": []}, {}
        for i in range(2 + 9):
            for route, call in (("per_label", per_label), ("refined", refined)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                call()
                e1.record()
                e1.synchronize()
                found[route] = int(offsets[1])
                if i >= 2:
                    ms[route].append(e0.elapsed_time(e1))
        doc[name] = dict(labels=L, gap_rows=gap, per_label=spread(ms["per_label"]), refined=spread(ms["refined"]), runs_per_label=found["per_label"],
                         runs_refined=found["refined"], workspace_bytes_per_label=int(sizes["per_label"]), workspace_bytes_refined=int(sizes["refined"]),
                         bytes_read=int(S * (L + 1) * 8))
    return doc


def run_clips(seconds: float, a) -> dict:
    import numpy as np
    import pandas as pd

    from orcai_amd import predict as P
    from orcai_amd import wavio
    from orcai_amd.synthetic import synth_recording

    tmp = Path(tempfile.mkdtemp(prefix="orcai_refine_"))
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
        options = {"high_thresholds": {c: float(2 * np.quantile(agg[:, i], 0.8)) for i, c in enumerate(param["calls"])}, "merge_gap": 0.2}
        routes = {}
        for device in (False, True):
            for on in (False, True):
                name = ("device" if device else "host") + ("_refined" if on else "_plain")
                (tmp / name).mkdir()
                routes[name] = lambda name=name, device=device, on=on: P.predict(
                    tmp / "table.csv", model_dir=model_dir, output_path=tmp / name, overwrite=True, verbosity=0, batch_frames=HOUR_FRAMES, device_labels=device,
                    thresholds=low, **(options if on else {}))
        audio = seconds * a.clips
        times = alternate(routes, a.reps, a.warmup)
        doc = dict(clips=a.clips, seconds_each=seconds, audio_seconds=audio, batch_frames=HOUR_FRAMES, thresholds=low, **options)
        for name in routes:
            doc[name] = summary(times[name], audio)
            doc[name]["intervals"] = sum(len(f.read_text().strip().split("\n")) - 1 for f in (tmp / name).iterdir())
        for kind in ("plain", "refined"):
            doc[f"same_files_{kind}"] = all((tmp / f"host_{kind}" / f.name).read_bytes() == f.read_bytes() for f in (tmp / f"device_{kind}").iterdir()) and \
                len(list((tmp / f"device_{kind}").iterdir())) == len(list((tmp / f"host_{kind}").iterdir())) == a.clips
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
    ap.add_argument("--out", default=str(ROOT / "profiles" / "label_refine_mi355x.json"))
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
