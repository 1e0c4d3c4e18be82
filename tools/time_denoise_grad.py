"""Times the denoised front end's backward w.r.t. the audio (orcai_denoised_spectrogram_bwd) beside the plain backward of the same route
(orcai_spectrogram_bwd / orcai_mel_spectrogram_bwd, the yardstick re-measured in this very run) on a one-hour synthetic recording at 48 kHz, 512 / 256,
linear K = 171 and 64 mel bands, in one process with device events, and writes one JSON object (default profiles/denoise_grad_mi355x.json).  Each round
runs, in this order: the plain linear backward, the denoised linear one, the plain mel backward, the denoised mel one -- the two kernels of a route
alternate, so a drift of the device falls on both.  Median [min - max] over the rounds after the warm-up rounds.  Run it under `timeout`.

    timeout -k 10 300 python tools/time_denoise_grad.py --rounds 5 --warmup 2

There is no pass / fail ratio.  The denoised kernels are the plain ones plus one cached load of floor[k] and one subtraction per gated element (and
ref_db formed once per workgroup), with the same launch plan: a difference beyond the plain kernel's own min - max spread needs an explanation from the
generated code."""

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
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "denoise_grad_mi355x.json")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print("time_denoise_grad: needs a ROCm GPU (nothing is measured without one)", file=sys.stderr)
        return 2
    import bench
    from orcai_amd import _native as N
    from orcai_amd.frontend import FrontEnd

    dev = torch.device("cuda", 0)
    fe = FrontEnd(dev)
    n = int(a.seconds * 48000)
    base = {"sampling_rate": 48000, "nfft": 512, "n_overlap": 256, "quantiles": [0.01, 0.999]}
    plain = {"linear_k171": dict(base, freq_range=[0, 16000]), "mel_64": dict(base, freq_range=[0, 24000], mel={"n_mels": 64, "fmin": 0.0, "fmax": 24000.0})}
    pcm = bench.synth_pcm_device(n, 2, dev)
    runs = {}  # name -> a call that returns dpcm; the forward once per entry: its statistics (and profile) and a gradient of its shape
    for route, sp in plain.items():
        spec, stats = fe.make_spectrogram(pcm, sp, return_stats=True)
        g = torch.randn(spec.shape, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
        del spec
        runs[route + "_plain"] = lambda sp=sp, g=g, stats=stats: fe.backward(pcm, g, stats, sp)
        dsp = dict(sp, denoise={"quantile": 0.5})
        spec, dstats, profile = fe.make_spectrogram(pcm, dsp, return_stats=True, return_profile=True)
        del spec
        runs[route + "_denoised"] = lambda dsp=dsp, g=g, dstats=dstats, profile=profile: fe.denoised_spectrogram_backward(pcm, g, dstats, profile, dsp)
    ms = {name: [] for name in runs}
    for i in range(a.warmup + a.rounds):
        for name, run in runs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            dpcm = run()
            e1.record()
            torch.cuda.synchronize()
            assert bool(torch.isfinite(dpcm[:: 4099]).all())
            del dpcm
            if i >= a.warmup:
                ms[name].append(e0.elapsed_time(e1))
    lib = N.lib()
    res = {
        "workload": "one_hour_48kHz_512_256", "n_samples": n, "n_frames": 1 + n // 256, "rounds": a.rounds, "warmup": a.warmup,
        "order_in_a_round": list(runs),
        "ms": {name: {"median": round(float(np.median(v)), 3), "min": round(min(v), 3), "max": round(max(v), 3)} for name, v in ms.items()},
        "denoised_over_plain": {route: round(float(np.median(ms[route + "_denoised"])) / float(np.median(ms[route + "_plain"])), 3) for route in plain},
        "occupancy_workgroups_per_cu": {"denoised linear 512": lib.orcai_denoised_spectrogram_bwd_occupancy(512, 0),
                                        "denoised mel 512 / 64": lib.orcai_denoised_spectrogram_bwd_occupancy(512, 64),
                                        "plain mel 512 / 64": lib.orcai_mel_spectrogram_bwd_occupancy(512, 64)},
        "device": torch.cuda.get_device_name(0),
    }
    a.out.parent.mkdir(parents=True, exist_ok=True)
    a.out.write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
