"""Times `orcai predict` with and without the label extraction on the GPU, on cuda:0, orcai-V1 shape (736 x 171, filters 30/40/50/60,
k 3, 128 units, f32, seeded untrained weights written to a temporary model directory).  device_labels=False is the route of the commit before the
flag existed, through the same call.

  clips60   256 mono PCM16 clips of 60 s at 48 kHz (8 synthetic recordings, hard-linked to 256 names): predict(table, batch_frames=675000) with
            device_labels on and off.
  clips10   the same for 256 clips of 10 s.
  hour      one one-hour recording (the 60 s synthetic recording tiled), predict(wav) without and with call_duration_limits, flag on and off.
  kernel    orcai_extract_labels alone (HIP events) on synthetic averaged probabilities of an hour (42187 x 7 and 42187 x 64): sparse calls, one run
            as long as the hour in every column, and every column alternating every row (the capacity bound).

Files are written to a temporary directory and read once, so they are in the page cache.  After --warmup untimed rounds the routes alternate for
--reps rounds; per route the median, minimum and maximum wall time.  One more instrumented pass per route over the clips, one by one, with a
synchronise after the launch half, splits the time per clip into the GPU half and the host half, and the host half into its parts: waiting for and
unpacking the copy + the label table (predict_wav_finish), the duration filter + `to_csv` (_save_recording); the file read is timed on its own.
Every case runs in a child process of its own under a time limit; a case that fails ends the run.

    python tools/time_device_labels.py [--reps 5] [--warmup 1] [--clips 256] [--out profiles/device_labels_mi355x.json]
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
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from tools.time_predict_batch import HOUR_FRAMES, alternate, make_model_dir, summary, wall_ms  # noqa: E402

CASES = ("clips60", "clips10", "hour", "kernel")
LIMITS = {"default": [0.2, 2.0]}


def run_clips(seconds: float, a) -> dict:
    import pandas as pd
    import torch

    from orcai_amd import predict as P
    from orcai_amd import wavio
    from orcai_amd.auxiliary import Messenger
    from orcai_amd.synthetic import synth_recording

    quiet = Messenger(verbosity=0)
    tmp = Path(tempfile.mkdtemp(prefix="orcai_labels_"))
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
        outs = {}
        for name in ("host", "device"):
            outs[name] = tmp / name
            outs[name].mkdir()

        def table(name):
            P.predict(tmp / "table.csv", model_dir=model_dir, output_path=outs[name], overwrite=True, verbosity=0, batch_frames=HOUR_FRAMES,
                      device_labels=name == "device")

        audio = seconds * a.clips
        times = alternate({"host": lambda: table("host"), "device": lambda: table("device")}, a.reps, a.warmup)
        doc = dict(clips=a.clips, seconds_each=seconds, audio_seconds=audio, batch_frames=HOUR_FRAMES, host_labels=summary(times["host"], audio),
                   device_labels=summary(times["device"], audio))
        doc["same_files"] = all((outs["host"] / f.name).read_bytes() == f.read_bytes() for f in outs["device"].iterdir()) and \
            len(list(outs["device"].iterdir())) == len(list(outs["host"].iterdir())) == a.clips
        doc["intervals"] = sum(len(f.read_text().strip().split("\n")) - 1 for f in outs["host"].iterdir())
        # instrumented, clip by clip: where the host half goes
        t0 = time.perf_counter()
        for n in names:
            (clips / f"{n}.wav").read_bytes()
        doc["file_read_ms_per_clip"] = (time.perf_counter() - t0) * 1e3 / a.clips
        for name in ("host", "device"):
            spec = P.label_spec(param, "*", None, probabilities=False) if name == "device" else None
            gpu = labels = save = 0.0
            for n in names:
                t0 = time.perf_counter()
                state = P.predict_wav_launch(clips / f"{n}.wav", 1, model, param, shape, msgr=quiet, device_labels=spec)
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                result = P.predict_wav_finish(state, msgr=quiet)
                t2 = time.perf_counter()
                P._save_recording(result, outs[name] / f"{n}_instrumented.txt", param, msgr=quiet)
                gpu, labels, save = gpu + t1 - t0, labels + t2 - t1, save + time.perf_counter() - t2
            doc[f"{name}_labels"]["per_clip_instrumented_ms"] = dict(gpu_half_with_file_read=gpu * 1e3 / a.clips, label_table=labels * 1e3 / a.clips,
                                                                     to_csv=save * 1e3 / a.clips)
        return doc
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def run_hour(a) -> dict:
    import numpy as np

    from orcai_amd import predict as P
    from orcai_amd import wavio
    from orcai_amd.synthetic import synth_recording

    tmp = Path(tempfile.mkdtemp(prefix="orcai_labels_"))
    try:
        model_dir, _ = make_model_dir(tmp)
        folders = {}
        wav = tmp / "hour.wav"
        wavio.write_wav_pcm16(wav, np.tile(synth_recording(60.0, 48000, seed=100), 60), 48000)
        wav.read_bytes()
        doc = dict(audio_seconds=3600.0)
        for limits_name, limits in (("no_limits", None), ("with_limits", LIMITS)):
            for name in ("host", "device"):
                folders[name] = tmp / f"{limits_name}_{name}"
                folders[name].mkdir()
                os.link(wav, folders[name] / "hour.wav")

            def one(name, limits=limits):
                P.predict(folders[name] / "hour.wav", model_dir=model_dir, overwrite=True, verbosity=0, call_duration_limits=limits, device_labels=name == "device")

            times = alternate({"host": lambda: one("host"), "device": lambda: one("device")}, a.reps, a.warmup)
            out = "hour_c1_orcai-v1_predicted.txt"
            doc[limits_name] = dict(host_labels=summary(times["host"], 3600.0), device_labels=summary(times["device"], 3600.0),
                                    same_files=(folders["host"] / out).read_bytes() == (folders["device"] / out).read_bytes(),
                                    intervals=len((folders["host"] / out).read_text().strip().split("\n")) - 1)
        return doc
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def run_kernel(a) -> dict:
    import numpy as np
    import torch

    from orcai_amd import _native as N
    from orcai_amd import predict as P

    lib, st = N.lib(), N.stream_ptr()
    S = HOUR_FRAMES // 16
    doc = dict(rows=S)
    rng = np.random.default_rng(0)
    for L in (7, 64):
        patterns = {"sparse": np.repeat(np.where(rng.random((S // 8 + 1, L)) < 0.02, 0.9, 0.1), 8, axis=0)[:S], "one_run_per_column": np.full((S, L), 0.9),
                    "alternating": np.where(np.arange(S)[:, None] % 2 == 0, 0.9, 0.0) + np.zeros((S, L))}
        for name, host in patterns.items():
            agg, cnt = torch.from_numpy(np.ascontiguousarray(host)).cuda(), torch.full((S,), 2.0, dtype=torch.float64, device="cuda")
            table = torch.tensor([[0, 0, S, 0]], dtype=torch.int64, device="cuda")
            rank = torch.arange(L, dtype=torch.int32, device="cuda")
            limits = torch.tensor([[0.2, 2.0]] * L, dtype=torch.float64, device="cuda")
            capacity = L * ((S + 1) // 2) + 1
            runs = torch.empty((capacity, 4), dtype=torch.int32, device="cuda")
            offsets = torch.empty(2, dtype=torch.int64, device="cuda")
            nbytes = lib.orcai_extract_labels_workspace_bytes(L, 1, S)
            ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
            ms = []
            for _ in range(2 + 9):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                N.check(lib.orcai_extract_labels(N.ptr(agg), N.ptr(cnt), L, N.ptr(table), 1, S, 0.5, N.ptr(rank), N.ptr(limits), 256 / 48000, 16, N.ptr(runs), capacity,
                                                 N.ptr(offsets), N.ptr(ws), nbytes, st), "orcai_extract_labels")
                e1.record()
                e1.synchronize()
                ms.append(e0.elapsed_time(e1))
            t0 = time.perf_counter()
            with np.errstate(all="ignore"):
                s, e, n = P.compute_binary_predictions(host, np.full(S, 2.0), [f"c{i:02d}" for i in range(L)])
                P.compute_labels(s, e, n, 16, "*")
            doc[f"L{L}_{name}"] = dict(kernel_ms=statistics.median(ms[2:]), runs=int(offsets[1]), bytes_read=int(S * (L + 1) * 8), bytes_of_runs=int(offsets[1]) * 16,
                                       workspace_bytes=int(nbytes), host_route_ms_without_filter=(time.perf_counter() - t0) * 1e3)
    return doc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--clips", type=int, default=256)
    ap.add_argument("--timeout", type=int, default=420, help="seconds a case may take")
    ap.add_argument("--case", choices=CASES, default=None, help="run one case in this process and print its JSON line (what the parent starts)")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "device_labels_mi355x.json"))
    a = ap.parse_args()
    if a.case is not None:
        import torch

        torch.cuda.set_device(0)
        doc = run_kernel(a) if a.case == "kernel" else run_hour(a) if a.case == "hour" else run_clips(60.0 if a.case == "clips60" else 10.0, a)
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
