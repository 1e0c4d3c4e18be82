#!/usr/bin/env python
"""Times orcai_resample_polyphase and its adjoint orcai_resample_polyphase_bwd on one hour of audio, 44.1 kHz -> 48 kHz and 22.05 kHz -> 48 kHz,
in one process: both launchers called through the C ABI on the same buffers, alternating, device events around windows of several launches.
Writes both times, their ratio and the spread to profiles/resample_grad_mi355x.json (DESIGN quotes it).  Needs the GPU: there is no fallback.

    python tools/time_resample_grad.py [--seconds 3600] [--warmup 3] [--windows 10] [--launches 5] [--out profiles/resample_grad_mi355x.json]
"""

from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--seconds", type=float, default=3600.0, help="length of the recording")
    ap.add_argument("--warmup", type=int, default=3, help="untimed launches of each kernel per rate pair")
    ap.add_argument("--windows", type=int, default=10, help="timed windows per kernel and rate pair")
    ap.add_argument("--launches", type=int, default=5, help="launches per timed window")
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "resample_grad_mi355x.json")
    args = ap.parse_args()

    import torch

    from orcai_amd import _native as N
    from orcai_amd.resample import device_table, output_length, ratio, resample_backward_device, resample_device

    if not torch.cuda.is_available():
        raise SystemExit("time_resample_grad: no GPU (a time taken anywhere else says nothing about the MI355X)")
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    lib, stream = N.lib(), N.stream_ptr()
    result = {"device": torch.cuda.get_device_name(0), "library": lib.orcai_version().decode(), "seconds_of_audio": args.seconds,
              "warmup": args.warmup, "windows": args.windows, "launches_per_window": args.launches, "clock": "device events around each window", "pairs": []}
    for sr_in, sr_out in ((44100, 48000), (22050, 48000)):
        L, M = ratio(sr_in, sr_out)
        table = device_table(L, M, dev)
        ntaps = int(table.shape[1])
        n_in = int(round(args.seconds * sr_in))
        n_out = output_length(n_in, sr_in, sr_out)
        gen = torch.Generator(dev).manual_seed(sr_in)
        x = torch.rand(n_in, device=dev, generator=gen) * 2 - 1
        g = torch.rand(n_out, device=dev, generator=gen) * 2 - 1
        y, dx = torch.empty(n_out, device=dev), torch.empty(n_in, device=dev)

        def fwd():
            N.check(lib.orcai_resample_polyphase(N.ptr(x), n_in, N.ptr(y), n_out, L, M, N.ptr(table), ntaps, stream), "orcai_resample_polyphase")

        def bwd():
            N.check(lib.orcai_resample_polyphase_bwd(N.ptr(g), n_out, N.ptr(dx), n_in, L, M, N.ptr(table), ntaps, stream), "orcai_resample_polyphase_bwd")

        for _ in range(args.warmup):
            fwd()
            bwd()
        torch.cuda.synchronize()
        # the results at the size that is timed: the launchers against the Python entry points, and the adjoint identity between the two
        assert torch.equal(y, resample_device(x, sr_in, sr_out)) and torch.equal(dx, resample_backward_device(g, n_in, sr_in, sr_out))
        lhs, rhs = float(torch.dot(y.double(), g.double())), float(torch.dot(x.double(), dx.double()))
        times = {"forward": [], "backward": []}
        for _ in range(args.windows):  # alternating, so that whatever else the machine does meets both alike
            for name, fn in (("forward", fwd), ("backward", bwd)):
                start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                start.record()
                for _ in range(args.launches):
                    fn()
                stop.record()
                stop.synchronize()
                times[name].append(start.elapsed_time(stop) / args.launches)
        pair = {"sr_in": sr_in, "sr_out": sr_out, "L": L, "M": M, "ntaps": ntaps, "table_bytes": 4 * L * ntaps, "n_in": n_in, "n_out": n_out,
                "fma": n_out * ntaps, "adjoint_identity": {"<y,g>": lhs, "<x,dx>": rhs, "relative_difference": abs(lhs - rhs) / max(abs(lhs), 1e-30)}}
        for name, t in times.items():
            med = statistics.median(t)
            pair[name] = {"ms_median": med, "ms_min": min(t), "ms_max": max(t), "gfma_per_s": n_out * ntaps / med / 1e6}
        pair["backward_over_forward"] = pair["backward"]["ms_median"] / pair["forward"]["ms_median"]
        result["pairs"].append(pair)
        print(f"{sr_in} -> {sr_out} Hz, {args.seconds:.0f} s: forward {pair['forward']['ms_median']:.3f} ms ({pair['forward']['ms_min']:.3f} .. "
              f"{pair['forward']['ms_max']:.3f}), backward {pair['backward']['ms_median']:.3f} ms ({pair['backward']['ms_min']:.3f} .. "
              f"{pair['backward']['ms_max']:.3f}), ratio {pair['backward_over_forward']:.2f}", flush=True)
        del x, g, y, dx
    args.out.parent.mkdir(parents=True, exist_ok=True)
    args.out.write_text(json.dumps(result, indent=1) + "\n")
    print(args.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
