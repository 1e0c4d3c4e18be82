"""Times `orcai test` on one dataset with the threshold sweep and without, on cuda:0, at the shape of tools/time_test_tables.py: orcai-V1
(736 x 171, filters 30/40/50/60, k 3, 128 units, 7 labels, f32, seeded untrained weights), --snippets 4096 in device batches of --batch 64.

  dataset   _test_model_on_dataset on the seeded in-memory dataset of time_test_tables.py: device_tables=True without the sweep (the route of the
            commit before the flag existed), device_tables=True with it, and the host route with it.  Wall time around the call, which ends in a copy
            to the host; after --warmup untimed rounds the three alternate for --reps rounds; per route the median, minimum and maximum.  Beside it,
            once each: the host statement of the histogram on the gathered arrays (what the host route adds) and the report from the histogram (what
            both routes add behind the pass).
  kernel    orcai_threshold_counts alone (HIP events around one call, median of 9 after 3 untimed) on 2944 rows x 7 labels at T = 200 and on
            2944 rows x 64 labels at T = 1024: uniform probabilities, and the probabilities of sparse calls (almost every element in one bin).

Every case runs in a child process of its own under a time limit; a case that fails ends the run.

    python tools/time_threshold_sweep.py [--reps 5] [--warmup 1] [--snippets 4096] [--batch 64] [--out profiles/threshold_sweep_mi355x.json]
"""

from __future__ import annotations

import argparse
import json
import shutil
import statistics
import subprocess
import sys
import tempfile
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from tools.time_predict_batch import alternate, make_model_dir  # noqa: E402
from tools.time_test_tables import spread  # noqa: E402

CASES = ("dataset", "kernel")
README_BASELINE_MS = 116.6  # device_tables=True at this shape in the README, measured at the commit before the sweep


def run_dataset(a) -> dict:
    import numpy as np
    import torch

    from orcai_amd import test as T
    from orcai_amd import threshold_sweep as W
    from orcai_amd.auxiliary import Messenger

    quiet = Messenger(verbosity=0)
    tmp = Path(tempfile.mkdtemp(prefix="orcai_sweep_"))
    try:
        _, (model, param, _) = make_model_dir(tmp)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    names = list(param["calls"])
    H, W_ = model.input_hw
    S, L, B = model.out_steps, model.num_labels, a.batch
    gen = torch.Generator(device="cuda").manual_seed(7)
    rng = np.random.default_rng(7)
    data = []
    for _ in range(a.snippets // B):
        x = torch.randn((B, H, W_), generator=gen, device="cuda", dtype=torch.float32)
        y = np.zeros((B, S, L), dtype=np.float32)
        calls = rng.random((B, S)) < 0.1  # a tenth of the time steps carry one call
        y[calls, rng.integers(0, L, int(calls.sum()))] = 1
        y[rng.random(y.shape) < 0.05] = -1
        data.append((x, torch.from_numpy(y).cuda()))
    results = {}

    def route(key, **flags):
        results[key] = T._test_model_on_dataset(model, data, names, "timed", quiet, **flags)

    times = alternate({"device_tables": lambda: route("dev", device_tables=True),
                       "device_tables_sweep": lambda: route("dev_sweep", device_tables=True, threshold_sweep=True, num_thresholds=a.num_thresholds),
                       "host_sweep": lambda: route("host_sweep", threshold_sweep=True, num_thresholds=a.num_thresholds)}, a.reps, a.warmup)
    dev, host = results["dev_sweep"]["threshold_sweep"], results["host_sweep"]["threshold_sweep"]
    doc = dict(snippets=len(data) * B, batch=B, rows=len(data) * B * S, labels=L, num_thresholds=a.num_thresholds, **{k: spread(v) for k, v in times.items()},
               same_sweep=bool(dev["sweep"].equals(host["sweep"])), same_auc=bool(dev["auc"] == host["auc"]), same_thresholds=bool(dev["thresholds"] == host["thresholds"]),
               same_tables=bool(results["dev"]["confusion_table"].equals(results["dev_sweep"]["confusion_table"])), MAUC=dev["auc"]["MAUC"])
    doc["sweep_adds_ms"] = doc["device_tables_sweep"]["median_ms"] - doc["device_tables"]["median_ms"]
    doc["spread_of_the_rounds_ms"] = doc["device_tables"]["max_ms"] - doc["device_tables"]["min_ms"]
    doc["readme_baseline_device_tables_ms"] = README_BASELINE_MS

    # the parts, once each
    probs = []
    for x, _ in data:
        out = torch.empty((B, S, L), dtype=torch.float32, device="cuda")
        model.forward_device(x.view(-1), H * W_, B, out, chunk=B)
        probs.append(out)
    y_host = np.concatenate([y.cpu().numpy() for _, y in data])
    p_host = np.concatenate([p.cpu().numpy() for p in probs])
    table = W.keras_thresholds(a.num_thresholds)
    t0 = time.perf_counter()
    hist = W.hist_from_arrays(y_host, p_host, table, -1.0)
    doc["host_hist_from_arrays_ms"] = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    W.report_from_hist(hist, table, names)
    doc["report_from_hist_ms"] = (time.perf_counter() - t0) * 1e3
    doc["bytes_to_host_per_dataset_sweep"] = 8 * L * 2 * (a.num_thresholds + 1)
    return doc


def run_kernel(a) -> dict:
    import numpy as np
    import torch

    from orcai_amd import _native as N
    from orcai_amd import threshold_sweep as W

    lib, st = N.lib(), N.stream_ptr()
    rng = np.random.default_rng(0)
    doc = {}
    M = 64 * 46
    for L, T in ((7, 200), (64, 1024)):
        table = W.keras_thresholds(T)
        td = torch.from_numpy(table).cuda()
        sparse_y = np.zeros((M, L), dtype=np.float32)
        calls = rng.random(M) < 0.1
        sparse_y[calls, rng.integers(0, L, int(calls.sum()))] = 1
        patterns = {"uniform": ((rng.random((M, L)) < 0.3).astype(np.float32), rng.random((M, L)).astype(np.float32)),
                    "sparse_calls": (sparse_y, np.where(sparse_y == 1, 0.9, 0.1).astype(np.float32))}
        for name, (y, p) in patterns.items():
            yd, pd_ = torch.from_numpy(y).cuda(), torch.from_numpy(p).cuda()
            buf = torch.zeros(L * 2 * (T + 1), dtype=torch.int64, device="cuda")
            ms = []
            for _ in range(3 + 9):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                N.check(lib.orcai_threshold_counts(N.ptr(pd_), N.ptr(yd), M, L, -1.0, N.ptr(td), T, N.ptr(buf), st), "orcai_threshold_counts")
                e1.record()
                e1.synchronize()
                ms.append(e0.elapsed_time(e1))
            exact = np.array_equal(buf.cpu().numpy().reshape(L, 2, T + 1), 12 * W.hist_from_arrays(y, p, table, -1.0))
            doc[f"{M}x{L}_T{T}_{name}"] = dict(rows=M, labels=L, thresholds=T, kernel_ms=statistics.median(ms[3:]), min_ms=min(ms[3:]), max_ms=max(ms[3:]),
                                               bytes_read=2 * M * L * 4, counts_exact_after_12_calls=bool(exact))
    return doc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--snippets", type=int, default=4096)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--num-thresholds", dest="num_thresholds", type=int, default=200)
    ap.add_argument("--timeout", type=int, default=420, help="seconds a case may take")
    ap.add_argument("--case", choices=CASES, default=None, help="run one case in this process and print its JSON line (what the parent starts)")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "threshold_sweep_mi355x.json"))
    a = ap.parse_args()
    if a.case is not None:
        import torch

        torch.cuda.set_device(0)
        doc = run_kernel(a) if a.case == "kernel" else run_dataset(a)
        doc["device"] = torch.cuda.get_device_name(0)
        print("RESULT " + json.dumps(doc), flush=True)
        return
    doc = dict(model="orcai-V1 shape, f32, untrained seeded weights", reps=a.reps, warmup=a.warmup, cases={})
    for case in CASES:  # each GPU step in a child of its own, under its own time limit; the first failure ends the run
        cmd = [sys.executable, str(Path(__file__).resolve()), "--case", case, "--reps", str(a.reps), "--warmup", str(a.warmup), "--snippets", str(a.snippets),
               "--batch", str(a.batch), "--num-thresholds", str(a.num_thresholds)]
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
