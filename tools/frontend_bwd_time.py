"""Times the spectrogram front end's forward (FrontEnd.make_spectrogram) and its backward w.r.t. the audio (FrontEnd.spectrogram_backward,
orcai_spectrogram_bwd) on the benchmark's recording -- bench.py's front-end workload: 1024 snippets of 736 frames at 48 kHz, 512 / 256, 171
bins -- in one process, with device events, and writes one JSON object (default profiles/frontend_backward.json).  Run it under `timeout`.

    timeout -k 10 300 python tools/frontend_bwd_time.py --steps 10 --warmup 3

Algorithmic bytes of the backward: pcm read + g read + dpcm written (the halo scheme has no workspace traffic)."""

from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "frontend_backward.json")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print("frontend_bwd_time: needs a ROCm GPU (nothing is measured without one)", file=sys.stderr)
        return 2
    import bench
    from orcai_amd.frontend import FrontEnd

    dev = torch.device("cuda", 0)
    fe = FrontEnd(dev)
    n = 1024 * bench.SNIPPET_FRAMES * 256
    sp = {"sampling_rate": 48000, "nfft": 512, "n_overlap": 256, "freq_range": [0, 16000], "quantiles": [0.01, 0.999]}
    pcm = bench.synth_pcm_device(n, 2, dev)
    spec, stats = fe.make_spectrogram(pcm, sp, return_stats=True)
    g = torch.randn(spec.shape, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    fwd, bwd = [], []
    for i in range(a.warmup + a.steps):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        e[0].record()
        spec, stats = fe.make_spectrogram(pcm, sp, return_stats=True)
        e[1].record()
        dpcm = fe.spectrogram_backward(pcm, g, stats, sp)
        e[2].record()
        torch.cuda.synchronize()
        if i >= a.warmup:
            fwd.append(e[0].elapsed_time(e[1]))
            bwd.append(e[1].elapsed_time(e[2]))
    assert bool(torch.isfinite(dpcm).all())
    alg = 4 * (n + g.numel() + n)
    res = {
        "workload": "frontend_1024_snippets_48kHz", "n_samples": n, "n_frames": int(spec.shape[0]), "bins": int(spec.shape[1]), "nfft": 512, "hop": 256,
        "steps": a.steps, "warmup": a.warmup,
        "forward_ms_median": round(float(np.median(fwd)), 4), "forward_ms_min": round(min(fwd), 4), "forward_ms_max": round(max(fwd), 4),
        "backward_ms_median": round(float(np.median(bwd)), 4), "backward_ms_min": round(min(bwd), 4), "backward_ms_max": round(max(bwd), 4),
        "backward_over_forward": round(float(np.median(bwd) / np.median(fwd)), 2),
        "backward_algorithmic_bytes": alg, "backward_algorithmic_bytes_parts": {"pcm_read": 4 * n, "g_read": 4 * g.numel(), "dpcm_written": 4 * n, "workspace": 0},
        "backward_achieved_GBs": round(alg / (float(np.median(bwd)) * 1e-3) / 1e9, 1), "hbm_peak_GBs": bench.HBM_PEAK_GBS,
        "device": torch.cuda.get_device_name(0),
    }
    a.out.parent.mkdir(parents=True, exist_ok=True)
    a.out.write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
