"""Times `orcai test` on one dataset with the tables' counts taken on the GPU and without, on cuda:0, orcai-V1 shape (736 x 171,
filters 30/40/50/60, k 3, 128 units, 7 labels, f32, seeded untrained weights).  device_tables=False is the route of the commit before the flag
existed, through the same call.

  dataset   _test_model_on_dataset on a seeded in-memory dataset (a list of device batches: --snippets 4096 in batches of --batch 64; noise
            spectrograms, sparse single labels with some masked elements), flag off / on: wall time around the call, which ends in a copy to the host.
            After --warmup untimed rounds the routes alternate for --reps rounds; per route the median, minimum and maximum.  Beside it, once each and
            synchronised: one forward pass over the dataset alone, the host route's table arithmetic on the concatenated arrays, the tables from counts.
  kernel    orcai_test_counts alone (HIP events around one call, median of 20 after 3 untimed) on one batch of 64 x 46 rows and on 64 such batches
            in one call, L = 7 and L = 64: all rows NOLABEL -> NOLABEL, sparse calls that the prediction follows, and every row with random predictions
            (no row in the NOLABEL -> NOLABEL bin).

Every case runs in a child process of its own under a time limit; a case that fails ends the run.

    python tools/time_test_tables.py [--reps 5] [--warmup 1] [--snippets 4096] [--batch 64] [--out profiles/test_tables_mi355x.json]
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

from tools.time_predict_batch import alternate, make_model_dir, wall_ms  # noqa: E402

CASES = ("dataset", "kernel")


def spread(ms: list) -> dict:
    return dict(median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms), ms=[round(x, 3) for x in ms])


def run_dataset(a) -> dict:
    import numpy as np
    import torch

    from orcai_amd import test as T
    from orcai_amd.auxiliary import Messenger
    from orcai_amd.device_tables import confusion_table_from_counts, counts_from_arrays, misclassification_tables_from_counts

    quiet = Messenger(verbosity=0)
    tmp = Path(tempfile.mkdtemp(prefix="orcai_tables_"))
    try:
        _, (model, param, _) = make_model_dir(tmp)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    names = list(param["calls"])
    H, W = model.input_hw
    S, L, B = model.out_steps, model.num_labels, a.batch
    gen = torch.Generator(device="cuda").manual_seed(7)
    rng = np.random.default_rng(7)
    data = []
    for _ in range(a.snippets // B):
        x = torch.randn((B, H, W), generator=gen, device="cuda", dtype=torch.float32)
        y = np.zeros((B, S, L), dtype=np.float32)
        calls = rng.random((B, S)) < 0.1  # a tenth of the time steps carry one call
        y[calls, rng.integers(0, L, int(calls.sum()))] = 1
        y[rng.random(y.shape) < 0.05] = -1
        data.append((x, torch.from_numpy(y).cuda()))
    results = {}

    def route(flag):
        results[flag] = T._test_model_on_dataset(model, data, names, "timed", quiet, device_tables=flag)

    times = alternate({"host_tables": lambda: route(False), "device_tables": lambda: route(True)}, a.reps, a.warmup)
    host, dev = results[False], results[True]
    same = host["confusion_table"].equals(dev["confusion_table"]) and all(t.equals(dev["misclassification_tables"][k]) for k, t in host["misclassification_tables"].items())
    doc = dict(snippets=len(data) * B, batch=B, rows=len(data) * B * S, labels=L, host_tables=spread(times["host_tables"]), device_tables=spread(times["device_tables"]),
               same_tables=bool(same), same_MBA=bool(host["data_metrics"]["MBA"] == dev["data_metrics"]["MBA"]),
               loss_relative_difference=float(abs(host["data_metrics"]["loss"] - dev["data_metrics"]["loss"]) / abs(host["data_metrics"]["loss"])))
    doc["device_over_host"] = doc["device_tables"]["median_ms"] / doc["host_tables"]["median_ms"]

    # the parts, once each
    probs = []

    def forward_only():
        for x, _ in data:
            out = torch.empty((B, S, L), dtype=torch.float32, device="cuda")
            model.forward_device(x.view(-1), H * W, B, out, chunk=B)
            probs.append(out)

    forward_only()
    probs.clear()
    doc["forward_pass_alone_ms"] = float(wall_ms(forward_only))
    y_host = np.concatenate([y.cpu().numpy() for _, y in data])
    p_host = np.concatenate([p.cpu().numpy() for p in probs])
    t0 = time.perf_counter()
    T.compute_confusion_table(y_host, p_host, names)
    T.compute_misclassification_tables(T._stack_batch(y_host), T._stack_batch((p_host >= 0.5).astype(int)), "true", "pred", names)
    doc["host_table_arithmetic_ms"] = (time.perf_counter() - t0) * 1e3
    conf, mis = counts_from_arrays(y_host, p_host)
    t0 = time.perf_counter()
    confusion_table_from_counts(conf, names)
    misclassification_tables_from_counts(mis, "true", "pred", names)
    doc["tables_from_counts_ms"] = (time.perf_counter() - t0) * 1e3
    pred = p_host.reshape(-1, L) >= 0.5
    doc["rows_in_nolabel_nolabel_bin"] = int((~pred.any(axis=1) & ~(y_host.reshape(-1, L) == 1).any(axis=1)).sum())
    doc["bytes_to_host_per_batch_host_tables"] = 2 * B * S * L * 4
    doc["bytes_to_host_per_dataset_device_tables"] = 8 * (4 * L + 2 * (L + 1) * (L + 1) * L) + 32
    return doc


def run_kernel(a) -> dict:
    import numpy as np
    import torch

    from orcai_amd import _native as N
    from orcai_amd.device_tables import counts_from_arrays

    lib, st = N.lib(), N.stream_ptr()
    rng = np.random.default_rng(0)
    doc = {}
    for L in (7, 64):
        for batches in (1, 64):
            M = batches * 64 * 46
            sparse_y = np.zeros((M, L), dtype=np.float32)
            calls = rng.random(M) < 0.1
            sparse_y[calls, rng.integers(0, L, int(calls.sum()))] = 1
            patterns = {"all_nolabel": (np.zeros((M, L), dtype=np.float32), np.zeros((M, L), dtype=np.float32)),
                        "sparse_calls": (sparse_y, np.where(sparse_y == 1, 0.9, 0.1).astype(np.float32)),
                        "every_row_predicted": (sparse_y, np.maximum(rng.random((M, L)), np.eye(L)[rng.integers(0, L, M)]).astype(np.float32))}
            for name, (y, p) in patterns.items():
                yd, pd_ = torch.from_numpy(y).cuda(), torch.from_numpy(p).cuda()
                buf = torch.zeros(4 * L + 2 * (L + 1) * (L + 1) * L, dtype=torch.int64, device="cuda")
                ms = []
                for _ in range(3 + 20):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    N.check(lib.orcai_test_counts(N.ptr(pd_), N.ptr(yd), M, L, -1.0, N.ptr(buf), buf.data_ptr() + 32 * L, st), "orcai_test_counts")
                    e1.record()
                    e1.synchronize()
                    ms.append(e0.elapsed_time(e1))
                conf, mis = counts_from_arrays(y, p)
                got = buf.cpu().numpy()
                exact = np.array_equal(got[: 4 * L].reshape(L, 4), 23 * conf) and np.array_equal(got[4 * L :].reshape(mis.shape), 23 * mis)
                doc[f"L{L}_{batches}x2944_{name}"] = dict(rows=M, kernel_ms=statistics.median(ms[3:]), min_ms=min(ms[3:]), max_ms=max(ms[3:]), bytes_read=2 * M * L * 4,
                                                          counts_exact_after_23_calls=bool(exact))
    return doc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--snippets", type=int, default=4096)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--timeout", type=int, default=420, help="seconds a case may take")
    ap.add_argument("--case", choices=CASES, default=None, help="run one case in this process and print its JSON line (what the parent starts)")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "test_tables_mi355x.json"))
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
               "--batch", str(a.batch)]
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
