"""Times the time-varying noise floor on the 1 h 48 kHz synthetic recording's arrays (T = 675 001 frames at nfft 512 / hop 256) on cuda:0, in
one process and one library, for segments of 1 s, 10 s, 60 s and 600 s on the [T, 171] and [T, 64] referenced dB arrays:

  fused     orcai_segment_column_select_fused: one launch, a workgroup per (segment, 32 columns), four passes over its own slab
  loop      one orcai_column_select per segment's row range on the same array -- what a caller had before this entry existed, the yardstick
  entry     orcai_segment_column_select, which follows the route rule (orcai_segment_column_select_route is recorded beside it)
  global    orcai_column_select over all the rows of the same array
  subtract  orcai_subtract_segment_floor beside orcai_subtract_columns
  whole     FrontEnd.make_spectrogram with "denoise" and with "denoise" + "segment", on the linear and the mel-64 route

HIP events around each call; after --warmup untimed rounds the contenders ALTERNATE for --reps rounds, and every figure is the median with its minimum
and maximum.  Each select time is also given as a multiple of FOUR reads of the array at 4.3 TB/s (the streaming rate tools/microbench/stream_bw.hip
showed for this library's access patterns).  The [T, 64] array (173 MB) fits the 256 MB Infinity Cache and the [T, 171] one (462 MB) does not.

    python tools/time_segment_denoise.py [--reps 5] [--warmup 2] [--seconds 3600] [--out profiles/segment_denoise_mi355x.json]
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
SEGMENTS_S = (1.0, 10.0, 60.0, 600.0)


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


def alternate(contenders: dict, warmup: int, reps: int, tag: str) -> dict:
    ms = {name: [] for name in contenders}
    for r in range(warmup + reps):
        for name, fn in contenders.items():
            t = event_ms(fn)
            print(f"{tag} round {r} {name}: {t:.3f} ms", file=sys.stderr, flush=True)
            if r >= warmup:
                ms[name].append(t)
    return {name: summary(v) for name, v in ms.items()}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seconds", type=float, default=3600.0)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "segment_denoise_mi355x.json"))
    args = ap.parse_args()

    import torch

    from orcai_amd import _native as N
    from orcai_amd.denoise import segment_count, segment_rows
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
              "stream_tb_per_s_assumed": STREAM_TB_S, "select": {}, "subtract": {}, "whole": {}}

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

    for K, extra in ((171, {}), (64, {"mel": MEL64})):
        sp = dict(SP, **extra)
        x = torch.empty((T, K), dtype=torch.float32, device="cuda")
        referenced_db(K, sp, x)
        four_reads_ms = 4 * T * K * 4 / (STREAM_TB_S * 1e12) * 1e3
        rows, sub_rows = {}, {}
        m_global = torch.empty(K, dtype=torch.float32, device="cuda")
        for seconds in SEGMENTS_S:
            W = segment_rows(seconds, 48000, 256)
            S = segment_count(T, W)
            n_last = T - (S - 1) * W
            rank, rank_last = nearest_rank_index(W, 0.5), nearest_rank_index(n_last, 0.5)
            outs = {name: torch.empty((S, K), dtype=torch.float32, device="cuda") for name in ("fused", "loop", "entry")}
            scratch = fe._grown("column_select", lib.orcai_segment_column_select_scratch_bytes(T, K, W) // 4)

            def fused():
                N.check(lib.orcai_segment_column_select_fused(N.ptr(x), T, K, W, rank, rank_last, N.ptr(outs["fused"]), s), "orcai_segment_column_select_fused")

            def loop():
                for i in range(S):
                    last = i == S - 1
                    N.check(lib.orcai_column_select(x.data_ptr() + i * W * K * 4, n_last if last else W, K, rank_last if last else rank,
                                                    outs["loop"].data_ptr() + i * K * 4, N.ptr(scratch), s), "orcai_column_select")

            def entry():
                N.check(lib.orcai_segment_column_select(N.ptr(x), T, K, W, rank, rank_last, N.ptr(outs["entry"]), N.ptr(scratch), s), "orcai_segment_column_select")

            def whole_array():
                N.check(lib.orcai_column_select(N.ptr(x), T, K, nearest_rank_index(T, 0.5), N.ptr(m_global), N.ptr(scratch), s), "orcai_column_select")

            row = alternate({"fused": fused, "loop": loop, "entry": entry, "global": whole_array}, args.warmup, args.reps, f"select K={K} {seconds:g}s")
            row.update(seg_rows=W, segments=S, workgroups=S * -(-K // 32), slab_bytes=W * 128, route=lib.orcai_segment_column_select_route(T, K, W),
                       same_bytes=bool(torch.equal(outs["fused"].view(torch.int32), outs["loop"].view(torch.int32))
                                       and torch.equal(outs["entry"].view(torch.int32), outs["loop"].view(torch.int32))),
                       fused_times_four_reads=round(row["fused"]["median_ms"] / four_reads_ms, 2),
                       faster="fused" if row["fused"]["median_ms"] < row["loop"]["median_ms"] else "loop")
            rows[f"{seconds:g}s"] = row

            y = x.clone()
            zeros_seg, zeros_col = torch.zeros((S, K), dtype=torch.float32, device="cuda"), torch.zeros(K, dtype=torch.float32, device="cuda")  # x - 0: y stays x

            def segment_floor():
                N.check(lib.orcai_subtract_segment_floor(N.ptr(y), T, K, W, N.ptr(zeros_seg), s), "orcai_subtract_segment_floor")

            def columns():
                N.check(lib.orcai_subtract_columns(N.ptr(y), T, K, N.ptr(zeros_col), s), "orcai_subtract_columns")

            sub = alternate({"subtract_segment_floor": segment_floor, "subtract_columns": columns}, args.warmup, args.reps, f"subtract K={K} {seconds:g}s")
            sub["times_read_plus_write"] = round(sub["subtract_segment_floor"]["median_ms"] / (four_reads_ms / 2), 2)
            sub_rows[f"{seconds:g}s"] = sub
            del y
        result["select"][f"K{K}"] = {"array_bytes": 4 * T * K, "four_reads_ms_at_stream_rate": round(four_reads_ms, 4), "segments": rows}
        result["subtract"][f"K{K}"] = sub_rows
        del x

    for name, extra in (("linear", {}), ("mel64", {"mel": MEL64})):
        sp = dict(SP, **extra)
        K = fe.spectrogram_shape(n, sp)[1]
        out = torch.empty((T, K), dtype=torch.float32, device="cuda")
        contenders = {"denoise": lambda: fe.make_spectrogram(pcm, dict(sp, denoise={}), out=out)}
        for seconds in SEGMENTS_S:
            contenders[f"segment_{seconds:g}s"] = lambda seconds=seconds: fe.make_spectrogram(pcm, dict(sp, denoise={"segment": seconds}), out=out)
        result["whole"][name] = dict(alternate(contenders, args.warmup, args.reps, f"whole {name}"), width=K)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(result, indent=1, allow_nan=False) + "\n")
    print(json.dumps(result, allow_nan=False))


if __name__ == "__main__":
    main()
