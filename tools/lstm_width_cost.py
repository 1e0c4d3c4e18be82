"""What an LSTM width costs: the recurrence kernels and the whole training step at lstm_units = 128 and 256.

    python tools/lstm_width_cost.py [--units 128 256] [--reps 5] [--out profiles/lstm_widths.json]

(a) the inference recurrence of one BiLSTM layer over a 1 h predict's snippets (1 833 snippets x 46 steps, orcai_lstm_recurrent);
(b) the model forward (trunk + head, no front end) over those 1 833 snippets of 736 x 171, filters 30/40/50/60, 7 labels;
(c) the training recurrences at batch 64 (orcai_lstm_train_fwd, orcai_lstm_bwd) and one full f32 training step (forward, loss,
    backward) of a 736 x 171 model with filters 30/40/50/60 and 7 labels.
Times are HIP-event brackets around `reps` launches after one warm-up; run it under `rocprofv3 --kernel-trace --stats` for the
per-kernel statistics.  Prints one JSON line and writes it to --out."""

from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

from orcai_amd import _native as N  # noqa: E402


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


def recurrences(U, reps):
    lib, st = N.lib(), N.stream_ptr()
    rng = np.random.default_rng(U)
    Uw = torch.from_numpy((rng.standard_normal((2, U, 4 * U)) * (0.8 / np.sqrt(U))).astype(np.float32)).cuda()
    out = {}
    for name, B in (("predict_1h", 1833), ("train_b64", 64)):
        T = 46
        xz = torch.randn((B, T, 2, 4 * U), device="cuda")
        h = torch.empty((B, T, 2 * U), device="cuda")
        out[f"{name}/recurrent_ms"] = _ms(lambda: N.check(lib.orcai_lstm_recurrent(N.ptr(xz), N.ptr(Uw), B, T, U, N.ptr(h), st), "rec"), reps)
        if name == "train_b64":
            g = torch.empty((B, T, 2, 4 * U), device="cuda")
            c = torch.empty((B, T, 2, U), device="cuda")
            dH = torch.randn((B, T, 2 * U), device="cuda") * 1e-3
            dxz = torch.empty_like(g)
            out[f"{name}/train_fwd_ms"] = _ms(lambda: N.check(lib.orcai_lstm_train_fwd(N.ptr(xz), N.ptr(Uw), B, T, U, N.ptr(h), N.ptr(g), N.ptr(c), st), "fwd"), reps)
            out[f"{name}/bwd_ms"] = _ms(lambda: N.check(lib.orcai_lstm_bwd(N.ptr(dH), N.ptr(g), N.ptr(c), N.ptr(Uw), B, T, U, N.ptr(dxz), st), "bwd"), reps)
    return out


def train_step(U, reps):
    from orcai_amd.architectures import ResNetLSTM
    from orcai_amd.training import Trainer

    B, H, W, L = 64, 736, 171, 7
    model = ResNetLSTM((H, W, 1), L, [30, 40, 50, 60], 3, 0.0, U, seed=3)
    tr = Trainer(model, learning_rate=1e-3)
    x = torch.rand((B * H * W,), device="cuda")
    y = (torch.rand((B, H // 16, L), device="cuda") > 0.5).float()
    return {"train_b64/step_ms": _ms(lambda: tr.forward_backward(x, H * W, B, y, masks=None), reps)}


def predict_forward(U, reps):
    from orcai_amd.architectures import ResNetLSTM

    n, H, W, L = 1833, 736, 171, 7
    model = ResNetLSTM((H, W, 1), L, [30, 40, 50, 60], 3, 0.0, U, seed=3)
    x = torch.rand((n * H * W,), device="cuda")
    out = torch.empty((n, H // 16, L), device="cuda")
    return {"predict_1h/model_forward_ms": _ms(lambda: model.forward_device(x, H * W, n, out), reps)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--units", type=int, nargs="+", default=[128, 256])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {}
    for U in a.units:
        r = recurrences(U, a.reps)
        r.update(predict_forward(U, max(1, a.reps // 2)))
        r.update(train_step(U, a.reps))
        res[str(U)] = {k: round(v, 4) for k, v in r.items()}
    line = json.dumps({"lstm_width_cost": res})
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
