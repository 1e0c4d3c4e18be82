"""Times the mel front end's backward w.r.t. the audio (orcai_mel_spectrogram_bwd) beside the linear one (orcai_spectrogram_bwd, the yardstick) on a
one-hour synthetic recording at 48 kHz, 512 / 256, in one process with device events, and writes one JSON object (default
profiles/mel_grad_mi355x.json).  Each round runs, in this order: the linear backward at K = 171, the mel backward at n_mels = 64 (0 - 24 kHz), the mel
backward at n_mels = 128 (6 - 24 kHz), and the linear backward AGAIN -- the pair of linear timings brackets the mel ones, so a drift of the device
within a round shows as a difference between them.  Median [min - max] over the rounds after the warm-up rounds.  Run it under `timeout`.

    timeout -k 10 300 python tools/time_mel_grad.py --rounds 5 --warmup 2

There is no pass / fail ratio.  Per frame the mel step adds about 514 multiply-adds and a gather beside two 512-point transforms, so a mel backward
far above the linear one points at the band sums, not the transforms."""

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
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seconds", type=float, default=3600.0)
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "mel_grad_mi355x.json")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print("time_mel_grad: needs a ROCm GPU (nothing is measured without one)", file=sys.stderr)
        return 2
    import bench
    from orcai_amd import _native as N
    from orcai_amd.frontend import FrontEnd

    dev = torch.device("cuda", 0)
    fe = FrontEnd(dev)
    n = int(a.seconds * 48000)
    base = {"sampling_rate": 48000, "nfft": 512, "n_overlap": 256, "quantiles": [0.01, 0.999]}
    routes = {
        "linear_k171_first": dict(base, freq_range=[0, 16000]),
        "mel_64_0_24k": dict(base, freq_range=[0, 24000], mel={"n_mels": 64, "fmin": 0.0, "fmax": 24000.0}),
        "mel_128_6k_24k": dict(base, freq_range=[0, 24000], mel={"n_mels": 128, "fmin": 6000.0, "fmax": 24000.0}),
    }
    routes["linear_k171_last"] = routes["linear_k171_first"]
    pcm = bench.synth_pcm_device(n, 2, dev)
    state = {}
    for name, sp in routes.items():  # the forward once per route: its statistics and a gradient of its shape
        spec, stats = fe.make_spectrogram(pcm, sp, return_stats=True)
        g = torch.randn(spec.shape, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
        state[name] = (sp, g, stats)
        del spec
    ms = {name: [] for name in routes}
    for i in range(a.warmup + a.rounds):
        for name, (sp, g, stats) in state.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            dpcm = fe.backward(pcm, g, stats, sp)
            e1.record()
            torch.cuda.synchronize()
            assert bool(torch.isfinite(dpcm[:: 4099]).all())
            del dpcm
            if i >= a.warmup:
                ms[name].append(e0.elapsed_time(e1))
    lin = float(np.median(ms["linear_k171_first"] + ms["linear_k171_last"]))
    res = {
        "workload": "one_hour_48kHz_512_256", "n_samples": n, "n_frames": 1 + n // 256, "rounds": a.rounds, "warmup": a.warmup,
        "order_in_a_round": list(routes),
        "ms": {name: {"median": round(float(np.median(v)), 3), "min": round(min(v), 3), "max": round(max(v), 3)} for name, v in ms.items()},
        "linear_ms_median_of_both": round(lin, 3),
        "mel_over_linear": {name: round(float(np.median(ms[name])) / lin, 3) for name in ("mel_64_0_24k", "mel_128_6k_24k")},
        "occupancy_workgroups_per_cu": {"mel 512 / 64": N.lib().orcai_mel_spectrogram_bwd_occupancy(512, 64), "mel 512 / 128": N.lib().orcai_mel_spectrogram_bwd_occupancy(512, 128),
                                        "mel 4096 / 64": N.lib().orcai_mel_spectrogram_bwd_occupancy(4096, 64)},
        "device": torch.cuda.get_device_name(0),
    }
    a.out.parent.mkdir(parents=True, exist_ok=True)
    a.out.write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
