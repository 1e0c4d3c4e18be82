"""What ResNet1DConv costs on the f16 path against f32, and what its f16 Dropout costs.

    python tools/conv1d_half_cost.py [--sets set1 set2 set3] [--reps 5] [--out profiles/conv1d_half.json]

(a) one training step (forward with the block and final Dropouts, loss, backward, Adam) of ResNet1DConv at 736 x 171, batch 64, k = 3,
    dropout rate 0.5, 7 labels, in f32 and in f16, for the three width sets of defaults/default_hps_parameter.json;
(b) the model forward (trunk + head, no front end) over a 1 h recording's 1 833 snippets in both precisions (width set3);
(c) the two f16 Dropout kernels alone on block 1's planes at batch 64 (set3: 30 channels -> 4 octets of 370 x 88 padded pixels): the mask draw
    (orcai_h_dropout_mask_dev, 2 bytes written per element) and the apply (orcai_h_mask_scale, 4 bytes read + 2 written), with the bandwidth
    that achieves; per width set, the step's own calls of the two kernels (per block: one draw, the forward apply, one backward apply) timed
    alone, and their share of the f16 step.  A `rocprofv3 --kernel-trace --stats` run of this tool gives the same kernels inside the steps.
Times are HIP-event brackets around `reps` calls after one warm-up.  Prints one JSON line and writes it to --out."""

from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

from orcai_amd import _native as N  # noqa: E402

H, W, L, K, RATE = 736, 171, 7, 3, 0.5
WIDTHS = json.loads((Path(__file__).resolve().parents[1] / "orcai_amd" / "defaults" / "default_hps_parameter.json").read_text())["filters"]


def _ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def train_step(filters, precision, reps, B=64):
    from orcai_amd.architectures import ResNet1DConv
    from orcai_amd.training import Trainer

    model = ResNet1DConv((H, W, 1), L, list(filters), K, RATE, seed=3, precision=precision)
    tr = Trainer(model, learning_rate=1e-4, seed=1)
    x = torch.rand((B * H * W,), device="cuda")
    y = (torch.rand((B, model.out_steps, L), device="cuda") > 0.5).float()
    ms = _ms(lambda: tr.train_step(x, H * W, B, y), reps)  # masks drawn inside the step from the device counter, as in training
    # elements of the block masks of one step (the octet / quad planes they multiply, pads included)
    masks = tr._masks(B, model.out_steps)
    n_block = sum(masks[f"block{i}"].numel() for i in range(1, len(filters) + 1))
    skipped = int(tr.skipped.item()) if tr.half else 0
    drop_ms = None
    if tr.half:  # the step's calls of the two f16 Dropout kernels, timed alone: per block one draw, the forward apply and one backward apply
        lib, st, counter, drop_ms = N.lib(), N.stream_ptr(), tr.counter, 0.0
        for i in range(1, len(filters) + 1):
            mk, x, y = masks[f"block{i}"], tr.trunk.buf[f"prev{i}"], tr.trunk.buf[f"prevd{i}"]
            drop_ms += _ms(lambda: N.check(lib.orcai_h_dropout_mask_dev(N.ptr(mk), mk.numel(), N.ptr(counter), 7, 1.0 - RATE, st), "h_dropout_mask_dev"), reps)
            drop_ms += 2 * _ms(lambda: N.check(lib.orcai_h_mask_scale(N.ptr(x), N.ptr(mk), 1.0 / (1.0 - RATE), x.numel(), N.ptr(y), st), "h_mask_scale"), reps)
    del tr, masks
    torch.cuda.empty_cache()
    return ms, n_block, skipped, drop_ms


def predict_forward(filters, precision, reps, n=1833):
    from orcai_amd.architectures import ResNet1DConv

    model = ResNet1DConv((H, W, 1), L, list(filters), K, 0.0, seed=3, precision=precision)
    x = torch.rand((n * H * W,), device="cuda")
    out = torch.empty((n, model.out_steps, L), device="cuda")
    ms = _ms(lambda: model.forward_device(x, H * W, n, out), reps)
    del model, x, out
    torch.cuda.empty_cache()
    return ms


def dropout_kernels(reps, B=64, C=30):
    """The two kernels on block 1's planes (set3): [B][ceil(C/8)][H/2 + 2][padded W/2][8] f16."""
    lib, st = N.lib(), N.stream_ptr()
    h, w = (H + 1) // 2, (W + 1) // 2
    shape = (B, (C + 7) // 8, h + 2, (w + 1 + 3) & ~3, 8)
    x = torch.randn(shape, device="cuda").half()
    m = torch.empty_like(x)
    y = torch.empty_like(x)
    n = x.numel()
    counter = torch.zeros(1, dtype=torch.int64, device="cuda")
    t_mask = _ms(lambda: N.check(lib.orcai_h_dropout_mask_dev(N.ptr(m), n, N.ptr(counter), 12345, 1.0 - RATE, st), "h_dropout_mask_dev"), reps)
    t_apply = _ms(lambda: N.check(lib.orcai_h_mask_scale(N.ptr(x), N.ptr(m), 1.0 / (1.0 - RATE), n, N.ptr(y), st), "h_mask_scale"), reps)
    return {"block1_elements": n, "mask_ms": round(t_mask, 4), "mask_GBps": round(2 * n / t_mask / 1e6, 1),
            "apply_ms": round(t_apply, 4), "apply_GBps": round(6 * n / t_apply / 1e6, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", nargs="+", default=["set1", "set2", "set3"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {"shape": [H, W], "batch": 64, "kernel_size": K, "dropout_rate": RATE, "labels": L, "train_step_ms": {}, "block_mask_elements": {}}
    for s in a.sets:
        row = {}
        for precision in ("f32", "f16"):
            ms, n_block, skipped, drop_ms = train_step(WIDTHS[s], precision, a.reps)
            row[precision] = round(ms, 3)
            if precision == "f16":
                res["block_mask_elements"][s] = n_block
                row["f16_skipped_steps"] = skipped
                row["f16_dropout_kernels_ms"] = round(drop_ms, 4)
                row["f16_dropout_share"] = round(drop_ms / ms, 4)
        row["f32_over_f16"] = round(row["f32"] / row["f16"], 3)
        res["train_step_ms"][s] = row
    res["predict_1h_model_forward_ms"] = {p: round(predict_forward(WIDTHS["set3"], p, max(1, a.reps // 2)), 2) for p in ("f32", "f16")}
    res["f16_dropout_kernels"] = dropout_kernels(a.reps)
    line = json.dumps({"conv1d_half_cost": res})
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
