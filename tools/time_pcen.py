"""Times the PCEN front end on the 1 h 48 kHz synthetic recording at nfft 512 / hop 256 on cuda:0, in one process:

  whole   FrontEnd.make_spectrogram for linear dB (K = 171, the yardstick), linear PCEN, mel-64 dB and mel-64 PCEN
  stages  orcai_pcen's three launches on their own (orcai_pcen_stage_ms: partials, carries, apply) on [T, 171] and [T, 64]
  steps   the calls orcai_make_pcen_spectrogram is made of, one by one, on the linear route

HIP events around each call; after --warmup untimed rounds the routes ALTERNATE for --reps rounds, and every figure is the median with its minimum
and maximum.

    python tools/time_pcen.py [--reps 5] [--warmup 2] [--seconds 3600] [--out profiles/pcen_mi355x.json]
"""

from __future__ import annotations

import argparse
import ctypes as C
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

SP = {"sampling_rate": 48000, "nfft": 512, "n_overlap": 256, "freq_range": [0, 16000], "quantiles": [0.01, 0.999]}
MEL64 = {"n_mels": 64, "fmax": 24000.0}
ROUTES = {"linear_db": {}, "linear_pcen": {"pcen": {}}, "mel64_db": {"mel": MEL64}, "mel64_pcen": {"mel": MEL64, "pcen": {}}}


def event_ms(fn) -> float:
    import torch

    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def summary(ms: list) -> dict:
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "ms": [round(x, 4) for x in ms]}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seconds", type=float, default=3600.0)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "pcen_mi355x.json"))
    args = ap.parse_args()

    import torch

    from orcai_amd import _native as N
    from orcai_amd import pcen
    from orcai_amd.frontend import get_frontend
    from orcai_amd.synthetic import pcm16_to_float, synth_recording

    torch.cuda.set_device(0)
    fe = get_frontend()
    lib = fe.lib
    pcm = torch.from_numpy(pcm16_to_float(synth_recording(args.seconds, 48000, seed=1))).cuda()
    n = pcm.numel()
    T = 1 + n // 256
    whole, width = {}, {}
    for name, extra in ROUTES.items():
        sp = dict(SP, **extra)
        K = fe.spectrogram_shape(n, sp)[1]
        width[name] = K
        out = torch.empty((T, K), dtype=torch.float32, device="cuda")
        whole[name] = lambda sp=sp, out=out: fe.make_spectrogram(pcm, sp, out=out)
    result = {"device": torch.cuda.get_device_name(0), "audio_seconds": args.seconds, "n_samples": n, "n_frames": T, "nfft": 512, "hop": 256,
              "chunk": pcen.CHUNK, "reps": args.reps, "warmup": args.warmup, "method": "HIP events; routes alternate within every round; median [min, max]",
              "routes": {k: {"width": width[k], "parameter": ROUTES[k]} for k in ROUTES}}
    times = {name: [] for name in whole}
    for r in range(args.warmup + args.reps):
        for name, fn in whole.items():
            ms = event_ms(fn)
            print(f"whole round {r} {name}: {ms:.3f} ms", file=sys.stderr, flush=True)
            if r >= args.warmup:
                times[name].append(ms)
    for name in whole:
        result["routes"][name]["whole"] = summary(times[name])
    for name, base in (("linear_pcen", "linear_db"), ("mel64_pcen", "mel64_db")):
        result["routes"][name]["whole"]["added_ms_over_db_median"] = round(result["routes"][name]["whole"]["median_ms"] - result["routes"][base]["whole"]["median_ms"], 4)

    # the three launches of orcai_pcen alone, on energies of the same shapes (the values do not change what the kernels do)
    cfg = pcen.pcen_config(dict(SP, pcen={}))
    a, b = pcen.smoother(cfg["time_constant"], 48000, 256)
    result["stages"] = {}
    for K in (171, 64):
        scratch = torch.empty(lib.orcai_pcen_scratch_bytes(T, K) // 4, dtype=torch.float32, device="cuda")
        src = torch.rand((T, K), device="cuda") * 1e-3
        x = torch.empty_like(src)
        stage = (C.c_float * 3)()
        rows = []
        for r in range(args.warmup + args.reps):
            x.copy_(src)
            N.check(lib.orcai_pcen_stage_ms(N.ptr(x), T, K, a, b, cfg["scale"], cfg["gain"], cfg["bias"], cfg["power"], cfg["eps"], N.ptr(scratch), N.stream_ptr(), stage),
                    "orcai_pcen_stage_ms")
            print(f"stages round {r} K={K}: partials {stage[0]:.3f} carries {stage[1]:.3f} apply {stage[2]:.3f} ms", file=sys.stderr, flush=True)
            if r >= args.warmup:
                rows.append(list(stage))
        nbytes = T * K * 4
        result["stages"][f"K{K}"] = {"array_bytes": nbytes, "chains": ((T + pcen.CHUNK - 1) // pcen.CHUNK) * K,
                                     "partials": summary([r[0] for r in rows]), "carries": summary([r[1] for r in rows]), "apply": summary([r[2] for r in rows])}
        s = result["stages"][f"K{K}"]
        s["partials"]["gb_per_s"] = round(nbytes / s["partials"]["median_ms"] / 1e6, 1)
        s["apply"]["gb_per_s"] = round(2 * nbytes / s["apply"]["median_ms"] / 1e6, 1)
    # the steps of orcai_make_pcen_spectrogram one by one on the linear route: which of them the added time goes to
    from orcai_amd.frontend import nearest_rank_index

    K = 171
    out = torch.empty((T, K), dtype=torch.float32, device="cuda")
    scratch = torch.empty(lib.orcai_pcen_scratch_bytes(T, K) // 4, dtype=torch.float32, device="cuda")
    ws, s = N.ptr(fe.workspace), N.stream_ptr()
    r_lo, r_hi = nearest_rank_index(T * K, SP["quantiles"][0]), nearest_rank_index(T * K, SP["quantiles"][1])
    steps = [("reset", lambda: lib.orcai_frontend_reset(ws, s)),
             ("energy", lambda: lib.orcai_stft_energy(N.ptr(pcm), n, 512, 256, T, K, N.ptr(out), s)),
             ("pcen", lambda: lib.orcai_pcen(N.ptr(out), T, K, a, b, cfg["scale"], cfg["gain"], cfg["bias"], cfg["power"], cfg["eps"], N.ptr(scratch), s)),
             ("hist_level1", lambda: lib.orcai_hist_level1(N.ptr(out), T * K, ws, s)),
             ("quantile_select", lambda: lib.orcai_quantile_select(N.ptr(out), T * K, r_lo, r_hi, ws, s)),
             ("finalize", lambda: lib.orcai_frontend_finalize(0, 0.0, ws, s)),
             ("clip_normalize", lambda: lib.orcai_clip_normalize(N.ptr(out), T * K, ws, s))]
    step_ms = {name: [] for name, _ in steps}
    below = None
    for r in range(args.warmup + args.reps):
        for name, fn in steps:
            step_ms[name].append(event_ms(lambda: N.check(fn(), name)))
            if name == "pcen" and below is None:
                below = float((out.flatten()[::97].abs() < 0.125).float().mean())
    result["composition_steps_linear"] = {name: summary(v[args.warmup:]) for name, v in step_ms.items()}
    result["composition_steps_linear"]["fraction_of_pcen_values_below_0.125"] = round(below, 4)
    result["composition_steps_linear"]["bounds"] = fe.stats()
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(result, indent=1) + "\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
