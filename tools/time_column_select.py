"""Times the segmented select on the 1 h 48 kHz synthetic recording's arrays (T = 675 001 frames at nfft 512 / hop 256) on cuda:0, in one
process and one library:

  select  orcai_column_select (the per-column median) on [T, 171] and [T, 64] arrays of three kinds -- the recording's referenced dB values, a constant,
          uniform random bit patterns -- and beside each the flat orcai_quantile_select_radix on the same array: three reads of it by code that was
          there before, the yardstick of what one read costs here.  orcai_subtract_columns on the same arrays as well.
  whole   FrontEnd.make_spectrogram with and without "denoise", on the linear and the mel-64 route

HIP events around each call; after --warmup untimed rounds the contenders ALTERNATE for --reps rounds, and every figure is the median with its minimum
and maximum.  Each column-select time is also given as a multiple of FOUR reads of the array at the streaming rate tools/microbench/stream_bw.hip
showed for this library's access patterns (profiles/r03_stream_bw_microbench.log: 4.0 - 4.3 TB/s; the upper figure is used, so the multiples are
not flattered).  The [T, 64] array (173 MB) fits the 256 MB Infinity Cache and the [T, 171] one (462 MB) does not: read the two rows apart.

    python tools/time_column_select.py [--reps 5] [--warmup 2] [--seconds 3600] [--out profiles/column_select_mi355x.json]
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
MEL64 = {"n_mels": 64, "fmax": 24000.0}
STREAM_TB_S = 4.3


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
    ap.add_argument("--out", default=str(ROOT / "profiles" / "column_select_mi355x.json"))
    args = ap.parse_args()

    import torch

    from orcai_amd import _native as N
    from orcai_amd.frontend import TOP_DB, get_frontend, nearest_rank_index, resolve_route
    from orcai_amd.synthetic import pcm16_to_float, synth_recording

    torch.cuda.set_device(0)
    fe = get_frontend()
    lib = fe.lib
    pcm = torch.from_numpy(pcm16_to_float(synth_recording(args.seconds, 48000, seed=1))).cuda()
    n = pcm.numel()
    T = 1 + n // 256
    ws, s = N.ptr(fe.workspace), N.stream_ptr()
    result = {"device": torch.cuda.get_device_name(0), "audio_seconds": args.seconds, "n_samples": n, "n_frames": T, "nfft": 512, "hop": 256, "reps": args.reps,
              "warmup": args.warmup, "method": "HIP events; contenders alternate within every round; median [min, max]",
              "stream_tb_per_s_assumed": STREAM_TB_S, "select": {}, "whole": {}}

    def referenced_db(K: int, sp: dict, out):
        """V = max(dB - ref_db, -top_db) of the recording: what the denoised front end selects on."""
        mel_cfg = resolve_route(sp).mel
        N.check(lib.orcai_frontend_reset(ws, s), "orcai_frontend_reset")
        if mel_cfg is None:
            N.check(lib.orcai_stft_db(N.ptr(pcm), n, 512, 256, T, K, N.ptr(out), ws, s), "orcai_stft_db")
        else:
            N.check(lib.orcai_stft_mel_db(N.ptr(pcm), n, 512, 256, T, K, *fe._bands(sp, mel_cfg), N.ptr(out), ws, s), "orcai_stft_mel_db")
        N.check(lib.orcai_frontend_finalize(1, TOP_DB, ws, s), "orcai_frontend_finalize")
        N.check(lib.orcai_db_reference(N.ptr(out), T * K, ws, s), "orcai_db_reference")

    # -- the selects alone
    rank = nearest_rank_index(T, 0.5)
    for K, extra in ((171, {}), (64, {"mel": MEL64})):
        sp = dict(SP, **extra)
        total = T * K
        r_lo, r_hi = nearest_rank_index(total, SP["quantiles"][0]), nearest_rank_index(total, SP["quantiles"][1])
        x = torch.empty((T, K), dtype=torch.float32, device="cuda")
        m = torch.empty(K, dtype=torch.float32, device="cuda")
        scratch = fe._grown("column_select", lib.orcai_column_select_scratch_bytes(K) // 4)
        read_ms = total * 4 / (STREAM_TB_S * 1e12) * 1e3
        rows = {}
        for kind in ("db", "constant", "random_bits"):
            if kind == "db":
                referenced_db(K, sp, x)
            elif kind == "constant":
                x.fill_(-80.0)
            else:
                x.view(torch.int32).random_(-(2**31), 2**31 - 1)
                x.nan_to_num_(nan=1.0)  # the selects' contract: no NaN

            def column():
                N.check(lib.orcai_column_select(N.ptr(x), T, K, rank, N.ptr(m), N.ptr(scratch), s), "orcai_column_select")

            def flat():
                N.check(lib.orcai_quantile_select_radix(N.ptr(x), total, r_lo, r_hi, ws, s), "orcai_quantile_select_radix")

            def subtract():  # in place: the values drift by m per round, the traffic does not
                N.check(lib.orcai_subtract_columns(N.ptr(x), T, K, N.ptr(m), s), "orcai_subtract_columns")

            ms = {"column_select": [], "flat_radix": [], "subtract_columns": []}
            for r in range(args.warmup + args.reps):
                for name, fn in (("column_select", column), ("flat_radix", flat)):
                    t = event_ms(fn)
                    print(f"select K={K} {kind} round {r} {name}: {t:.3f} ms", file=sys.stderr, flush=True)
                    if r >= args.warmup:
                        ms[name].append(t)
            sub = torch.sort(x[:, : min(K, 4)], dim=0).values[rank]  # the first columns against torch's sort, outside the timing
            same = bool(torch.equal(sub, m[: min(K, 4)]))
            m.fill_(0.0)  # subtracting 0 keeps x what it is
            for r in range(args.warmup + args.reps):
                t = event_ms(subtract)
                if r >= args.warmup:
                    ms["subtract_columns"].append(t)
            rows[kind] = {k: summary(v) for k, v in ms.items()}
            rows[kind]["first_columns_equal_sort"] = same
            rows[kind]["column_select"]["times_four_reads"] = round(rows[kind]["column_select"]["median_ms"] / (4 * read_ms), 2)
            rows[kind]["flat_radix"]["times_three_reads"] = round(rows[kind]["flat_radix"]["median_ms"] / (3 * read_ms), 2)
            rows[kind]["subtract_columns"]["times_read_plus_write"] = round(rows[kind]["subtract_columns"]["median_ms"] / (2 * read_ms), 2)
            rows[kind]["column_per_read_over_flat_per_read"] = round((rows[kind]["column_select"]["median_ms"] / 4) / (rows[kind]["flat_radix"]["median_ms"] / 3), 2)
        result["select"][f"K{K}"] = {"values": total, "array_bytes": 4 * total, "one_read_ms_at_stream_rate": round(read_ms, 4), "rank": rank, "kinds": rows}

    # -- make_spectrogram with and without "denoise", in the same run
    for name, extra in (("linear", {}), ("mel64", {"mel": MEL64})):
        sp = dict(SP, **extra)
        K = fe.spectrogram_shape(n, sp)[1]
        out_plain = torch.empty((T, K), dtype=torch.float32, device="cuda")
        out_den = torch.empty((T, K), dtype=torch.float32, device="cuda")
        ms = {"plain": [], "denoise": []}
        for r in range(args.warmup + args.reps):
            for who, fn in (("plain", lambda: fe.make_spectrogram(pcm, sp, out=out_plain)), ("denoise", lambda: fe.make_spectrogram(pcm, dict(sp, denoise={}), out=out_den))):
                t = event_ms(fn)
                print(f"whole {name} round {r} {who}: {t:.3f} ms", file=sys.stderr, flush=True)
                if r >= args.warmup:
                    ms[who].append(t)
        result["whole"][name] = {"width": K, "plain": summary(ms["plain"]), "denoise": summary(ms["denoise"]),
                                 "added_ms": round(statistics.median(ms["denoise"]) - statistics.median(ms["plain"]), 4)}
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(result, indent=1, allow_nan=False) + "\n")
    print(json.dumps(result, allow_nan=False))


if __name__ == "__main__":
    main()
