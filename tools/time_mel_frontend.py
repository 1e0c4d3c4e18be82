"""Times the front end on the 1 h 48 kHz synthetic recording at nfft 512 / hop 256 on cuda:0: the linear route (K = 171) beside the mel route at
n_mels = 64 and 128, in one process.

  whole   FrontEnd.make_spectrogram: reset, STFT launch(es), selection, finalize, clip / normalise
  stft    the STFT launch alone: orcai_stft_db (K = 171) beside orcai_stft_mel_db, after a reset

HIP events around each call; after --warmup untimed rounds the routes ALTERNATE for --reps rounds, and every figure is the median with its minimum
and maximum.  The yardstick of the mel route is the linear route of the same run; the occupancy the runtime reports for both kernels is recorded.

    python tools/time_mel_frontend.py [--reps 5] [--warmup 2] [--seconds 3600] [--out profiles/mel_frontend_mi355x.json]
"""

from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

SP = {"sampling_rate": 48000, "nfft": 512, "n_overlap": 256, "freq_range": [0, 16000], "quantiles": [0.01, 0.999]}
# 128 bands need fmin high enough that no band falls between two FFT bins (93.75 Hz apart): mel.mel_config refuses the others
ROUTES = {"linear171": None, "mel64": {"n_mels": 64, "fmax": 24000.0}, "mel128": {"n_mels": 128, "fmin": 6000.0, "fmax": 24000.0}}


def event_ms(fn) -> float:
    import torch

    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def summary(ms: list, audio_seconds: float, out_bytes: int, pcm_bytes: int) -> dict:
    med = statistics.median(ms)
    return {"median_ms": round(med, 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "ms": [round(x, 4) for x in ms],
            "audio_seconds_per_s": round(audio_seconds / med * 1e3, 1), "algorithmic_bytes": pcm_bytes + out_bytes,
            "algorithmic_gb_per_s": round((pcm_bytes + out_bytes) / med / 1e6, 1)}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seconds", type=float, default=3600.0)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "mel_frontend_mi355x.json"))
    args = ap.parse_args()

    import torch

    from orcai_amd import _native as N
    from orcai_amd import mel
    from orcai_amd.frontend import get_frontend
    from orcai_amd.synthetic import pcm16_to_float, synth_recording

    torch.cuda.set_device(0)
    fe = get_frontend()
    lib = fe.lib
    pcm = torch.from_numpy(pcm16_to_float(synth_recording(args.seconds, 48000, seed=1))).cuda()
    n = pcm.numel()
    T = 1 + n // 256
    ws, s = N.ptr(fe.workspace), N.stream_ptr()
    whole, stft, width = {}, {}, {}
    for name, m in ROUTES.items():
        sp = dict(SP, mel=m)
        K = fe.spectrogram_shape(n, sp)[1]
        width[name] = K
        out = torch.empty((T, K), dtype=torch.float32, device="cuda")
        whole[name] = lambda sp=sp, out=out: fe.make_spectrogram(pcm, sp, out=out)
        if m is None:
            def launch(out=out, K=K):
                N.check(lib.orcai_frontend_reset(ws, s), "reset")
                N.check(lib.orcai_stft_db(N.ptr(pcm), n, 512, 256, T, K, N.ptr(out), ws, s), "orcai_stft_db")
        else:
            t, w = fe._mel_table(sp, mel.mel_config(sp))

            def launch(out=out, K=K, t=t, w=w):
                N.check(lib.orcai_frontend_reset(ws, s), "reset")
                N.check(lib.orcai_stft_mel_db(N.ptr(pcm), n, 512, 256, T, K, t["lo"].ctypes.data, t["hi"].ctypes.data, t["off"].ctypes.data, N.ptr(w), w.numel(),
                                              N.ptr(out), ws, s), "orcai_stft_mel_db")
        stft[name] = launch
    result = {"device": torch.cuda.get_device_name(0), "audio_seconds": args.seconds, "n_samples": n, "n_frames": T, "nfft": 512, "hop": 256,
              "reps": args.reps, "warmup": args.warmup, "method": "HIP events; routes alternate within every round; median [min, max]",
              "occupancy_workgroups_per_cu": {"stft_db_kernel<true, true, 171>": lib.orcai_stft_occupancy(), "stft_mel_kernel<true, true>": lib.orcai_stft_mel_occupancy()},
              "routes": {k: {"width": width[k], "mel": ROUTES[k]} for k in ROUTES}}
    for what, fns in (("whole", whole), ("stft", stft)):
        times = {name: [] for name in fns}
        for r in range(args.warmup + args.reps):
            for name, fn in fns.items():
                ms = event_ms(fn)
                print(f"{what} round {r} {name}: {ms:.3f} ms", file=sys.stderr, flush=True)
                if r >= args.warmup:
                    times[name].append(ms)
        for name in fns:
            result["routes"][name][what] = summary(times[name], args.seconds, T * width[name] * 4 * (2 if what == "whole" else 1), n * 4)
    for name in ("mel64", "mel128"):
        for what in ("whole", "stft"):
            result["routes"][name][what]["ratio_to_linear_median"] = round(result["routes"][name][what]["median_ms"] / result["routes"]["linear171"][what]["median_ms"], 4)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(result, indent=1) + "\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
