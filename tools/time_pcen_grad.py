"""Times the gradient of the PCEN front end on the 1 h 48 kHz synthetic recording at nfft 512 / hop 256 on cuda:0, in one process:

  whole   FrontEnd.backward with pcen set on the linear route (K = 171) and on mel-64, beside the two dB routes
  stages  orcai_pcen_bwd's six launches on their own (orcai_pcen_bwd_stage_ms) on [T, 171] and [T, 64]
  steps   the three calls orcai_pcen_spectrogram_bwd is made of, one by one, on both routes
  parent  with --parent-lib (a liborcai_hip.so built from the parent commit, loaded beside this tree's): orcai_spectrogram_bwd and
          orcai_mel_spectrogram_bwd of both libraries on the same inputs -- identical bits?  times within the spread?

HIP events around each call; after --warmup untimed rounds the candidates ALTERNATE for --reps rounds, and every figure is the median with its minimum
and maximum.

    python tools/time_pcen_grad.py [--reps 5] [--warmup 2] [--seconds 3600] [--parent-lib PATH] [--out profiles/pcen_grad_mi355x.json]
"""

from __future__ import annotations

import argparse
import ctypes as C
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))

from time_pcen import MEL64, SP, event_ms, summary  # noqa: E402

ROUTES = {"linear_db": {}, "linear_pcen": {"pcen": {}}, "mel64_db": {"mel": MEL64}, "mel64_pcen": {"mel": MEL64, "pcen": {}}}
STAGES = ("partials", "carries", "local", "reverse_partials", "reverse_carries", "apply")
PASSES = {"partials": 1, "local": 4, "reverse_partials": 1, "apply": 3}  # arrays of T K floats moved by each streaming launch


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seconds", type=float, default=3600.0)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "pcen_grad_mi355x.json"))
    args = ap.parse_args()

    import torch

    from orcai_amd import _native as N
    from orcai_amd import mel, pcen
    from orcai_amd.frontend import TOP_DB, get_frontend
    from orcai_amd.synthetic import pcm16_to_float, synth_recording

    torch.cuda.set_device(0)
    fe = get_frontend()
    lib = fe.lib
    pcm = torch.from_numpy(pcm16_to_float(synth_recording(args.seconds, 48000, seed=1))).cuda()
    n = pcm.numel()
    T = 1 + n // 256
    rounds = range(args.warmup + args.reps)
    result = {"device": torch.cuda.get_device_name(0), "audio_seconds": args.seconds, "n_samples": n, "n_frames": T, "nfft": 512, "hop": 256,
              "chunk": pcen.CHUNK, "reps": args.reps, "warmup": args.warmup, "method": "HIP events; candidates alternate within every round; median [min, max]",
              "routes": {}}

    # whole backwards, each from the statistics of its own forward
    whole, keep = {}, {}
    for name, extra in ROUTES.items():
        sp = dict(SP, **extra)
        spec, stats = fe.make_spectrogram(pcm, sp, return_stats=True)
        g = torch.randn(spec.shape, device="cuda", generator=torch.Generator("cuda").manual_seed(1))
        del spec
        keep[name] = (sp, g, stats)
        whole[name] = lambda sp=sp, g=g, stats=stats: fe.backward(pcm, g, stats, sp)
        result["routes"][name] = {"width": g.shape[1], "parameter": extra}
    times = {name: [] for name in whole}
    for r in rounds:
        for name, fn in whole.items():
            ms = event_ms(fn)
            print(f"whole round {r} {name}: {ms:.3f} ms", file=sys.stderr, flush=True)
            if r >= args.warmup:
                times[name].append(ms)
    for name in whole:
        result["routes"][name]["backward"] = summary(times[name])

    # the six launches of orcai_pcen_bwd alone
    cfg = pcen.pcen_config(dict(SP, pcen={}))
    a, b = pcen.smoother(cfg["time_constant"], 48000, 256)
    scalars = (a, b, cfg["scale"], cfg["gain"], cfg["bias"], cfg["power"], cfg["eps"])
    result["stages"] = {}
    for K in (171, 64):
        scratch = torch.empty(lib.orcai_pcen_bwd_scratch_bytes(T, K) // 4, dtype=torch.float32, device="cuda")
        E = torch.rand((T, K), device="cuda") * 1e-3
        g = torch.randn((T, K), device="cuda")
        dE = torch.empty_like(E)
        stats = torch.tensor([0.0, 0.0, 0.05, 3.0, 0.05, 3.0], device="cuda")
        stage = (C.c_float * 6)()
        rows = []
        for r in rounds:
            N.check(lib.orcai_pcen_bwd_stage_ms(N.ptr(E), N.ptr(g), N.ptr(stats), T, K, *scalars, N.ptr(dE), N.ptr(scratch), N.stream_ptr(), stage), "orcai_pcen_bwd_stage_ms")
            print(f"stages round {r} K={K}: " + " ".join(f"{s} {stage[i]:.3f}" for i, s in enumerate(STAGES)) + " ms", file=sys.stderr, flush=True)
            if r >= args.warmup:
                rows.append(list(stage))
        nbytes = T * K * 4
        s = {"array_bytes": nbytes, "chains": ((T + pcen.CHUNK - 1) // pcen.CHUNK) * K}
        for i, st in enumerate(STAGES):
            s[st] = summary([row[i] for row in rows])
            if st in PASSES:
                s[st]["passes"] = PASSES[st]
                s[st]["gb_per_s"] = round(PASSES[st] * nbytes / s[st]["median_ms"] / 1e6, 1)
        s["total"] = summary([sum(row) for row in rows])
        s["total"]["passes"] = sum(PASSES.values())
        s["total"]["ms_at_4300_gb_per_s"] = round(sum(PASSES.values()) * nbytes / 4.3e6 / 1e3, 4)
        result["stages"][f"K{K}"] = s
        del scratch, E, g, dE

    # the three steps of the one call
    result["steps"] = {}
    s = N.stream_ptr()
    for name in ("linear_pcen", "mel64_pcen"):
        sp, g, stats = keep[name]
        K = g.shape[1]
        E, dE, dpcm = torch.empty_like(g), torch.empty_like(g), torch.empty_like(pcm)
        scratch = torch.empty(lib.orcai_pcen_bwd_scratch_bytes(T, K) // 4, dtype=torch.float32, device="cuda")
        if "mel" in sp:
            t, w = fe._mel_table(sp, mel.mel_config(sp))
            tab = (t["lo"].ctypes.data, t["hi"].ctypes.data, t["off"].ctypes.data, N.ptr(w), w.numel())
            steps = [("energy", lambda: lib.orcai_stft_mel_energy(N.ptr(pcm), n, 512, 256, T, K, *tab, N.ptr(E), s)),
                     ("pcen_bwd", lambda: lib.orcai_pcen_bwd(N.ptr(E), N.ptr(g), N.ptr(stats), T, K, *scalars, N.ptr(dE), N.ptr(scratch), s)),
                     ("energy_bwd", lambda: lib.orcai_stft_mel_energy_bwd(N.ptr(pcm), n, 512, 256, T, K, *tab, N.ptr(dE), N.ptr(dpcm), s))]
        else:
            steps = [("energy", lambda: lib.orcai_stft_energy(N.ptr(pcm), n, 512, 256, T, K, N.ptr(E), s)),
                     ("pcen_bwd", lambda: lib.orcai_pcen_bwd(N.ptr(E), N.ptr(g), N.ptr(stats), T, K, *scalars, N.ptr(dE), N.ptr(scratch), s)),
                     ("energy_bwd", lambda: lib.orcai_stft_energy_bwd(N.ptr(pcm), n, 512, 256, T, K, N.ptr(dE), N.ptr(dpcm), s))]
        step_ms = {k: [] for k, _ in steps}
        for r in rounds:
            for k, fn in steps:
                step_ms[k].append(event_ms(lambda: N.check(fn(), k)))
        result["steps"][name] = {k: summary(v[args.warmup:]) for k, v in step_ms.items()}
        del E, dE, dpcm, scratch

    # this tree's dB backwards against the parent commit's, loaded side by side
    if args.parent_lib:
        parent = C.CDLL(str(Path(args.parent_lib).resolve()))
        for fn in ("orcai_spectrogram_bwd", "orcai_mel_spectrogram_bwd"):
            getattr(parent, fn).restype, getattr(parent, fn).argtypes = getattr(lib, fn).restype, getattr(lib, fn).argtypes
        result["parent"] = {}
        sp, g, stats = keep["linear_db"]
        spm, gm, statsm = keep["mel64_db"]
        t, w = fe._mel_table(spm, mel.mel_config(spm))
        tab = (t["lo"].ctypes.data, t["hi"].ctypes.data, t["off"].ctypes.data, N.ptr(w), w.numel())
        calls = {"orcai_spectrogram_bwd": lambda L, d: L.orcai_spectrogram_bwd(N.ptr(pcm), n, 512, 256, T, g.shape[1], N.ptr(g), N.ptr(stats), TOP_DB, N.ptr(d), s),
                 "orcai_mel_spectrogram_bwd": lambda L, d: L.orcai_mel_spectrogram_bwd(N.ptr(pcm), n, 512, 256, T, gm.shape[1], *tab, N.ptr(gm), N.ptr(statsm), TOP_DB,
                                                                                        N.ptr(d), s)}
        for fn, call in calls.items():
            outs = {"this": torch.empty_like(pcm), "parent": torch.empty_like(pcm)}
            ms = {"this": [], "parent": []}
            for r in rounds:
                for who, L in (("this", lib), ("parent", parent)):
                    ms[who].append(event_ms(lambda: N.check(call(L, outs[who]), fn)))
            same = bool(torch.equal(outs["this"].view(torch.int32), outs["parent"].view(torch.int32)))
            result["parent"][fn] = {"identical_bits": same, "this": summary(ms["this"][args.warmup:]), "parent": summary(ms["parent"][args.warmup:])}
            print(f"{fn}: identical bits {same}", file=sys.stderr, flush=True)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(result, indent=1) + "\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
