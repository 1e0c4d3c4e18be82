"""Times the training augmentation on cuda:0.

  kernel  orcai_augment_apply alone at 64 x 736 x 171 (labels 46 x 7), HIP events, median [min - max] of 9 after 2 untimed rounds, for each option alone
          and all together (and with everything off: the plain copy).  Two figures per option: `rotating` goes round 8 input / output buffer pairs
          (512 MB, past the 256 MB Infinity Cache) inside one pair of events and divides by 8; `resident` repeats the call on one pair (64 MB: served
          from the cache).  The bytes a call moves are counted from the plan it ran (a mixed snippet reads two blocks), and the time those bytes take
          at the 4.0 - 4.3 TB/s that tools/microbench/stream_bw.hip shows for this library's access patterns is recorded beside the measurement.
          orcai_augment_plan is timed the same way.
  fit     FitLoop.fit on synthetic orcai-V1 data (64 x 736 x 171, default orcai-V1 model, the replayed graph), 24 steps an epoch from 8 batches resident
          on the device, with the augmentation off and on (all options), alternating for --reps rounds after --warmup untimed ones; wall clock around
          an epoch that ends in a device synchronise, per step.

Every case runs in a child process of its own under a time limit; a case that fails ends the run.

    python tools/time_augment.py [--reps 5] [--warmup 1] [--out profiles/augment_mi355x.json]
"""

from __future__ import annotations

import argparse
import json
import statistics
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

CASES = ("kernel", "fit")
SHAPE = (64, 736, 171, 46, 7)
OPTIONS = {
    "off": {},
    "time_masks": {"time_masks": 2, "time_mask_rows": 80},
    "freq_masks": {"freq_masks": 2, "freq_mask_bins": 24},
    "level_shift": {"level_shift": 0.1},
    "mix": {"mix_probability": 0.5},
    "mask_labels": {"time_masks": 2, "time_mask_rows": 80, "mask_labels": True},
    "all": {"time_masks": 2, "time_mask_rows": 80, "freq_masks": 2, "freq_mask_bins": 24, "level_shift": 0.1, "mix_probability": 0.5, "mask_labels": True},
}
STREAM_TBS = (4.0, 4.3)  # profiles/r03_stream_bw_microbench.log


def spread(v: list, unit: str = "us") -> dict:
    return {f"median_{unit}": statistics.median(v), f"min_{unit}": min(v), f"max_{unit}": max(v), unit: [round(x, 3) for x in v]}


def run_kernel(a) -> dict:
    import numpy as np
    import torch

    from orcai_amd import _native as N
    from orcai_amd import augment as A

    lib, st = N.lib(), N.stream_ptr()
    B, H, W, S, L = SHAPE
    rng = np.random.default_rng(0)
    sets = 8
    xs = [torch.from_numpy(rng.random((B, H, W), dtype=np.float32)).cuda() for _ in range(sets)]
    y = torch.from_numpy((rng.random((B, S, L)) < 0.3).astype(np.float32)).cuda()
    outs = [torch.empty_like(x) for x in xs]
    y_out = torch.empty_like(y)
    key = A.batch_key([12, 0], 0, 0, 0)
    doc = dict(shape=dict(B=B, H=H, W=W, S=S, L=L), rounds=9, untimed_rounds=2, buffer_pairs=sets, stream_tb_per_s=list(STREAM_TBS), options={})

    def timed(call, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(n):
            call(i)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / n  # microseconds per call

    for name, spec in OPTIONS.items():
        s = A.validate(spec, H, W)
        plan = torch.empty((B, A.PLAN_WORDS), dtype=torch.int32, device="cuda")
        flags = (A.FLAG_LEVEL_SHIFT if s["level_shift"] > 0 else 0) | (A.FLAG_MASK_LABELS if s["mask_labels"] else 0)

        def draw(i):
            N.check(lib.orcai_augment_plan(key, B, H, W, s["time_masks"], s["time_mask_rows"], s["freq_masks"], s["freq_mask_bins"], s["level_shift"],
                                           s["mix_probability"], plan.data_ptr(), st), "plan")

        def apply(i):
            N.check(lib.orcai_augment_apply(xs[i % sets].data_ptr(), y.data_ptr(), plan.data_ptr(), outs[i % sets].data_ptr(), y_out.data_ptr(), B, H, W, S, L,
                                            s["mask_value"], flags, st), "apply")

        draw(0)
        host_plan = plan.cpu().numpy()
        assert np.array_equal(host_plan, A.plan_ref(key, B, H, W, spec))
        mixed = int((host_plan[:, A.PLAN_PARTNER] >= 0).sum())
        moved = (2 * B + mixed) * H * W * 4 + (2 * B + mixed) * S * L * 4 + B * A.PLAN_WORDS * 4
        rot, res, pl = [], [], []
        for r in range(2 + 9):
            t = (timed(apply, sets), timed(lambda i: apply(0), sets), timed(draw, sets))
            if r >= 2:
                rot.append(t[0]), res.append(t[1]), pl.append(t[2])
        doc["options"][name] = dict(spec=spec, mixed_snippets=mixed, bytes_moved=moved, predicted_us_at_stream_rate=[round(moved / (tb * 1e6), 2) for tb in STREAM_TBS[::-1]],
                                    rotating=spread(rot), resident=spread(res), plan_call=spread(pl),
                                    rotating_tb_per_s=round(moved / (statistics.median(rot) * 1e6), 3))
    return doc


def run_fit(a) -> dict:
    import numpy as np
    import torch

    from orcai_amd import augment as A
    from orcai_amd.architectures import build_model
    from orcai_amd.io import read_json

    B, H, W, S, L = SHAPE
    param = read_json(ROOT / "orcai_amd" / "defaults" / "default_orcai_parameter.json")
    param["seed"] = 1
    model = build_model((H, W, 1), param)
    model.compile(learning_rate=param["model"]["learning_rate"], seed=1)
    rng = np.random.default_rng(0)
    batches = []
    for _ in range(8):
        x = torch.from_numpy(rng.random((B, H, W), dtype=np.float32)).cuda()
        batches.append((x, torch.from_numpy((rng.random((B, S, L)) < 0.3).astype(np.float32)).cuda()))

    class Resident(list):
        pass

    plain = Resident(batches * 3)
    routes = {"off": plain, "on": A.augmented(Resident(batches * 3), OPTIONS["all"], seed=[12, 1], rank=0)}
    ms = {k: [] for k in routes}
    for r in range(a.warmup + a.reps):
        for name, ds in routes.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            hist = model.fit(ds, epochs=1)
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) * 1e3 / len(ds)
            assert np.isfinite(hist.history["loss"][0])
            if r >= a.warmup:
                ms[name].append(dt)
    doc = dict(model="default orcai-V1 (ResNetLSTM, f32), replayed graph", batch=B, steps_per_epoch=len(plain), spec=OPTIONS["all"],
               graph_replayed=model._loop.trainer._graph is not None)
    for name in routes:
        doc[name] = spread(ms[name], "ms_per_step")
    doc["on_minus_off_ms_per_step"] = doc["on"]["median_ms_per_step"] - doc["off"]["median_ms_per_step"]
    return doc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--timeout", type=int, default=300, help="seconds a case may take")
    ap.add_argument("--case", choices=CASES, default=None, help="run one case in this process and print its JSON line (what the parent starts)")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "augment_mi355x.json"))
    a = ap.parse_args()
    if a.case is not None:
        import torch

        torch.cuda.set_device(0)
        doc = run_kernel(a) if a.case == "kernel" else run_fit(a)
        doc["device"] = torch.cuda.get_device_name(0)
        print("RESULT " + json.dumps(doc), flush=True)
        return
    doc = dict(reps=a.reps, warmup=a.warmup, cases={})
    for case in CASES:  # each GPU step in a child of its own, under its own time limit; the first failure ends the run
        cmd = [sys.executable, str(Path(__file__).resolve()), "--case", case, "--reps", str(a.reps), "--warmup", str(a.warmup)]
        done = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=a.timeout)
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
