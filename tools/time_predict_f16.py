"""Times predict_spectrogram on the f16 path over a whole recording, on cuda:0: BASELINE configs[2]'s model (736 x 171, filters 30/40/50/60, k 3,
128 LSTM units) at "precision": "f16" on a 1 h synthetic spectrogram (675 001 rows, 1 833 half-overlapping snippets), next to its f32 twin in the
same run.  Three variants, alternated inside every round so that they see the same machine state:

  f16          the model as built (share_overlap as the model sets it: the shared trunk of DESIGN 4.1 where HalfEngine has it)
  f16_unshared share_overlap = False: the per-snippet trunk
  f32          the f32 model as built

Each call is bracketed by device events after `--warmup` untimed rounds; the document holds per variant the median, the minimum and the
spread (max - min and the inter-quartile range) in ms, audio-seconds per second from the median, and one instrumented pass of per-label
kernel times (the model's kernel_events hook).  `f16_bits_equal` says whether f16 and f16_unshared gave the same bits.

    python tools/time_predict_f16.py [--seconds 3600] [--reps 9] [--warmup 2] [--out FILE]
"""

from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from orcai_amd.architectures import ResNetLSTM  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=3600.0)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--chunk", type=int, default=128)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    H, W = 736, 171
    T = 1 + int(a.seconds * 48000) // 256
    spec = torch.rand((T, W), device="cuda", generator=torch.Generator(device="cuda").manual_seed(3))

    def make(precision, share):
        m = ResNetLSTM((H, W, 1), 7, [30, 40, 50, 60], 3, 0.0, 128, seed=1)
        m.precision = precision
        if share is not None:
            m.share_overlap = share
        return m

    models = {"f16": make("f16", None), "f16_unshared": make("f16", False), "f32": make("f32", None)}
    times = {name: [] for name in models}
    outs = {}
    for r in range(a.warmup + a.reps):
        for name, m in models.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            outs[name] = m.predict_spectrogram(spec, chunk=a.chunk)
            e1.record()
            e1.synchronize()
            if r >= a.warmup:
                times[name].append(e0.elapsed_time(e1))
    doc = dict(device=torch.cuda.get_device_name(0), seconds=a.seconds, rows=T, snippets=int(outs["f16"].shape[0]), reps=a.reps, warmup=a.warmup, chunk=a.chunk,
               f16_shares=hasattr(models["f16"].half_engine(), "shared_geometry") and models["f16"].share_overlap,
               f16_bits_equal=bool(torch.equal(outs["f16"], outs["f16_unshared"])),
               f16_f32_max_abs_diff=float((outs["f16"] - outs["f32"]).abs().max()), variants={})
    for name, m in models.items():
        t = sorted(times[name])
        q = statistics.quantiles(t, n=4) if len(t) >= 2 else [t[0]] * 3
        m.kernel_events = {}
        m.predict_spectrogram(spec, chunk=a.chunk)
        torch.cuda.synchronize()
        labels = {label: round(sum(s.elapsed_time(e) for s, e in pairs), 4) for label, pairs in m.kernel_events.items()}
        m.kernel_events = None
        med = statistics.median(t)
        doc["variants"][name] = dict(median_ms=med, min_ms=t[0], max_ms=t[-1], spread_ms=t[-1] - t[0], iqr_ms=q[2] - q[0], audio_seconds_per_s=a.seconds / med * 1e3,
                                     label_ms_instrumented=labels)
    text = json.dumps(doc, indent=1)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text + "\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
