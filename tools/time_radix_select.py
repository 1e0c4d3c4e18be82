"""Times the two exact selects on the 1 h 48 kHz synthetic recording's arrays (T = 675 001 frames at nfft 512 / hop 256) on cuda:0, in one
process and one library:

  select  orcai_hist_level1 + orcai_quantile_select against orcai_quantile_select_radix on [T, 171] and [T, 64] arrays of five kinds: the recording's
          PCEN values, its dB values, a constant, two values, uniform random bit patterns
  whole   FrontEnd.make_spectrogram with "pcen" set (the radix select inside) against the composition it replaced, staged through the C ABI with the
          level-1 select, on the linear and the mel-64 route

HIP events around each call; after --warmup untimed rounds the contenders ALTERNATE for --reps rounds, and every figure is the median with its minimum
and maximum.  Every pair is also checked to select the same two keys.

    python tools/time_radix_select.py [--reps 5] [--warmup 2] [--seconds 3600] [--out profiles/radix_select_mi355x.json]
"""

from __future__ import annotations

import argparse
import json
import math
import statistics
import struct
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

SP = {"sampling_rate": 48000, "nfft": 512, "n_overlap": 256, "freq_range": [0, 16000], "quantiles": [0.01, 0.999]}
MEL64 = {"n_mels": 64, "fmax": 24000.0}
STREAM_TB_S = 4.3  # what this library's streaming kernels reach on the MI355X (orcai_pcen's apply pass)


def event_ms(fn) -> float:
    import torch

    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def bits_to_float(u: int) -> float:
    return struct.unpack("<f", struct.pack("<I", u))[0]


def summary(ms: list) -> dict:
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "ms": [round(x, 4) for x in ms]}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seconds", type=float, default=3600.0)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "radix_select_mi355x.json"))
    args = ap.parse_args()

    import torch

    from orcai_amd import _native as N
    from orcai_amd import pcen
    from orcai_amd.frontend import get_frontend, nearest_rank_index, resolve_route
    from orcai_amd.synthetic import pcm16_to_float, synth_recording

    torch.cuda.set_device(0)
    fe = get_frontend()
    lib = fe.lib
    pcm = torch.from_numpy(pcm16_to_float(synth_recording(args.seconds, 48000, seed=1))).cuda()
    n = pcm.numel()
    T = 1 + n // 256
    ws, s = N.ptr(fe.workspace), N.stream_ptr()
    cfg = pcen.pcen_config(dict(SP, pcen={}))
    a, b = pcen.smoother(cfg["time_constant"], 48000, 256)
    result = {"device": torch.cuda.get_device_name(0), "audio_seconds": args.seconds, "n_samples": n, "n_frames": T, "nfft": 512, "hop": 256, "reps": args.reps,
              "warmup": args.warmup, "method": "HIP events; contenders alternate within every round; median [min, max]",
              "stream_tb_per_s_assumed": STREAM_TB_S, "select": {}, "whole": {}}

    def pcen_values(K: int, sp: dict, out):
        """The PCEN values of the recording on the route of sp, un-normalised, into out [T, K]."""
        mel_cfg = resolve_route(sp).mel
        if mel_cfg is None:
            N.check(lib.orcai_stft_energy(N.ptr(pcm), n, 512, 256, T, K, N.ptr(out), s), "orcai_stft_energy")
        else:
            N.check(lib.orcai_stft_mel_energy(N.ptr(pcm), n, 512, 256, T, K, *fe._bands(sp, mel_cfg), N.ptr(out), s), "orcai_stft_mel_energy")
        scratch = fe._grown("pcen", lib.orcai_pcen_scratch_bytes(T, K) // 4)
        N.check(lib.orcai_pcen(N.ptr(out), T, K, a, b, cfg["scale"], cfg["gain"], cfg["bias"], cfg["power"], cfg["eps"], N.ptr(scratch), s), "orcai_pcen")

    def db_values(K: int, sp: dict, out):
        """The un-referenced dB values of the recording (what the dB routes select on)."""
        mel_cfg = resolve_route(sp).mel
        N.check(lib.orcai_frontend_reset(ws, s), "orcai_frontend_reset")
        if mel_cfg is None:
            N.check(lib.orcai_stft_db(N.ptr(pcm), n, 512, 256, T, K, N.ptr(out), ws, s), "orcai_stft_db")
        else:
            N.check(lib.orcai_stft_mel_db(N.ptr(pcm), n, 512, 256, T, K, *fe._bands(sp, mel_cfg), N.ptr(out), ws, s), "orcai_stft_mel_db")

    def keys():
        """The two selected values' f32 bit patterns."""
        N.check(lib.orcai_frontend_finalize(0, 0.0, ws, s), "orcai_frontend_finalize")
        return [int(v) & 0xFFFFFFFF for v in fe._stats_dev()[4:6].view(torch.int32).tolist()]

    # -- the selects alone
    for K, extra in ((171, {}), (64, {"mel": MEL64})):
        sp = dict(SP, **extra)
        total = T * K
        r_lo, r_hi = nearest_rank_index(total, SP["quantiles"][0]), nearest_rank_index(total, SP["quantiles"][1])
        x = torch.empty((T, K), dtype=torch.float32, device="cuda")
        floor_ms = 3 * total * 4 / (STREAM_TB_S * 1e12) * 1e3
        rows = {}
        for kind in ("pcen", "db", "constant", "two_values", "random_bits"):
            if kind == "pcen":
                pcen_values(K, sp, x)
            elif kind == "db":
                db_values(K, sp, x)
            elif kind == "constant":
                x.fill_(-80.0)
            elif kind == "two_values":
                x.copy_(torch.where(torch.rand((T, K), device="cuda") < 0.3, -3.5, 0.0625))
            else:
                x.view(torch.int32).random_(-(2**31), 2**31 - 1)

            def level1():
                N.check(lib.orcai_hist_level1(N.ptr(x), total, ws, s), "orcai_hist_level1")
                N.check(lib.orcai_quantile_select(N.ptr(x), total, r_lo, r_hi, ws, s), "orcai_quantile_select")

            def radix():
                N.check(lib.orcai_quantile_select_radix(N.ptr(x), total, r_lo, r_hi, ws, s), "orcai_quantile_select_radix")

            ms = {"level1": [], "radix": []}
            found = {}
            for r in range(args.warmup + args.reps):
                for name, fn in (("level1", level1), ("radix", radix)):
                    N.check(lib.orcai_frontend_reset(ws, s), "orcai_frontend_reset")  # the level-1 histogram accumulates; untimed
                    t = event_ms(fn)
                    print(f"select K={K} {kind} round {r} {name}: {t:.3f} ms", file=sys.stderr, flush=True)
                    if r >= args.warmup:
                        ms[name].append(t)
                    found[name] = keys()
            rows[kind] = {"level1": summary(ms["level1"]), "radix": summary(ms["radix"]), "selected_f32_bits": [f"0x{u:08x}" for u in found["radix"]],
                          "selected": [v if math.isfinite(v) else None for v in map(bits_to_float, found["radix"])],  # random bits may select a NaN pattern
                          "same_keys": found["level1"] == found["radix"]}
            rows[kind]["radix"]["times_three_reads"] = round(rows[kind]["radix"]["median_ms"] / floor_ms, 2)
        med = [rows[k]["radix"]["median_ms"] for k in rows]
        result["select"][f"K{K}"] = {"values": total, "array_bytes": 4 * total, "three_reads_ms_at_stream_rate": round(floor_ms, 4), "kinds": rows,
                                     "radix_slowest_over_fastest_kind": round(max(med) / min(med), 2)}

    # -- make_spectrogram with "pcen": the call as it is against the composition it replaced (the parent's), in the same run
    for name, extra in (("linear_pcen", {}), ("mel64_pcen", {"mel": MEL64})):
        sp = dict(SP, pcen={}, **extra)
        K = fe.spectrogram_shape(n, sp)[1]
        total = T * K
        r_lo, r_hi = nearest_rank_index(total, SP["quantiles"][0]), nearest_rank_index(total, SP["quantiles"][1])
        out_new = torch.empty((T, K), dtype=torch.float32, device="cuda")
        out_old = torch.empty((T, K), dtype=torch.float32, device="cuda")

        def staged():
            N.check(lib.orcai_frontend_reset(ws, s), "orcai_frontend_reset")
            pcen_values(K, sp, out_old)
            N.check(lib.orcai_hist_level1(N.ptr(out_old), total, ws, s), "orcai_hist_level1")
            N.check(lib.orcai_quantile_select(N.ptr(out_old), total, r_lo, r_hi, ws, s), "orcai_quantile_select")
            N.check(lib.orcai_frontend_finalize(0, 0.0, ws, s), "orcai_frontend_finalize")
            N.check(lib.orcai_clip_normalize(N.ptr(out_old), total, ws, s), "orcai_clip_normalize")

        ms = {"level1_composition": [], "make_spectrogram": []}
        for r in range(args.warmup + args.reps):
            for who, fn in (("level1_composition", staged), ("make_spectrogram", lambda: fe.make_spectrogram(pcm, sp, out=out_new))):
                t = event_ms(fn)
                print(f"whole {name} round {r} {who}: {t:.3f} ms", file=sys.stderr, flush=True)
                if r >= args.warmup:
                    ms[who].append(t)
        result["whole"][name] = {"width": K, "level1_composition": summary(ms["level1_composition"]), "make_spectrogram": summary(ms["make_spectrogram"]),
                                 "same_bytes": bool(torch.equal(out_new.view(torch.int32), out_old.view(torch.int32)))}
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(result, indent=1, allow_nan=False) + "\n")
    print(json.dumps(result, allow_nan=False))


if __name__ == "__main__":
    main()
