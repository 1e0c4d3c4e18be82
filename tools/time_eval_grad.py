"""Times the eval-mode input gradient at the orcai-V1 shape (736 x 171, filters 30/40/50/60, k 3, 128 units), B = 64, on cuda:0:

  (a) per layer, for each of orcai-V1's nine separable convs: the fused orcai_sepconv_dgrad against the composition of the launchers that existed
      before it (orcai_amd.eval_grad.compose_dgrad) on the same inputs, with the kernel's minimum HBM bytes against the HBM roof;
  (b) the whole gradient: EvalGrad.forward + backward against Trainer.forward_backward(..., dx=...), the only route to a dx before it, in the same
      process.

Medians of event-timed repetitions after warm-up; one JSON document to profiles/eval_grad_<tag>.json and stdout.

    python tools/time_eval_grad.py [--batch 64] [--reps 20] [--warmup 5] [--tag mi355x]
"""

from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from orcai_amd import _native as N  # noqa: E402
from orcai_amd.architectures import ENTRY_FILTERS, FINAL_FILTERS, ResNetLSTM  # noqa: E402
from orcai_amd.eval_grad import EvalGrad, compose_dgrad  # noqa: E402

HBM_ROOF_GBS = 8000.0  # MI355X peak; what a streaming kernel reaches is lower (tools/microbench/stream_bw.hip)


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return statistics.median(out), min(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--tag", default="mi355x")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    B, k = a.batch, 3
    model = ResNetLSTM((736, 171, 1), 7, [30, 40, 50, 60], k, 0.5, 128, seed=1)
    lib, st = N.lib(), N.stream_ptr()
    shapes = model.stage_shapes()
    layers, c = [], ENTRY_FILTERS
    for b, f in enumerate(model.filters, start=1):
        h, w, _ = shapes[b - 1]
        layers += [(f"b{b}/sep_a", c, f, h, w, True, True), (f"b{b}/sep_b", f, f, h, w, False, False)]
        c = f
    layers.append(("sep_f", c, FINAL_FILTERS, shapes[-1][0], shapes[-1][1], False, False))
    gen = torch.Generator(device="cuda").manual_seed(0)
    per_layer = []
    for name, cin, cout, h, w, ygate, xgate in layers:
        WP = model.padded_width(w)
        planes = lambda ch: torch.zeros((B, (ch + 3) // 4, h + 2, WP, 4), device="cuda")  # noqa: E731

        def fill(ch):
            t = planes(ch)
            t[:, :, 1 : 1 + h, :w, :] = torch.randn((B, (ch + 3) // 4, h, w, 4), device="cuda", generator=gen)
            return t

        g, y, x = fill(cout), fill(cout) if ygate else None, fill(cin) if xgate else None
        wts = torch.randn((cout, cin), device="cuda", generator=gen) / cout**0.5
        taps = torch.randn(((cin + 3) // 4, 9, 4), device="cuda", generator=gen) / 3
        dr, du, g2 = planes(cin), planes(cin), g.clone()

        def fused():
            N.check(lib.orcai_sepconv_dgrad(g.data_ptr(), None if y is None else y.data_ptr(), None if x is None else x.data_ptr(), B, cin, cout, h, w, k, wts.data_ptr(),
                                            taps.data_ptr(), dr.data_ptr(), st), "orcai_sepconv_dgrad")

        def composed():  # (gates g2 in place: after the first repetition the gate is idempotent, the traffic stays the same)
            compose_dgrad(lib, g2, y, x, B, cin, cout, h, w, k, wts, taps, dr, du, st)

        tf, tf_min = timed(fused, a.reps, a.warmup)
        tc, tc_min = timed(composed, a.reps, a.warmup)
        px = B * h * w
        nbytes = 16 * px * (((cout + 3) // 4) * (2 if ygate else 1) + ((cin + 3) // 4) * (2 if xgate else 1))
        per_layer.append(dict(layer=name, cin=cin, cout=cout, h=h, w=w, fused_ms=tf, fused_min_ms=tf_min, composed_ms=tc, composed_min_ms=tc_min, ratio=tc / tf,
                              min_hbm_bytes=nbytes, fused_gbs=nbytes / tf / 1e6, share_of_hbm_roof=nbytes / tf / 1e6 / HBM_ROOF_GBS,
                              lds_bytes_per_workgroup=8 * ((cin + 3) // 4) * 66 * 16, evalgrad_runs_fused=EvalGrad(model).fused(B, cin, h, w)))
        del g, y, x, dr, du, g2
    # (b) the whole gradient
    H, W = model.input_hw
    xs = torch.rand((B, H, W), device="cuda", generator=gen)
    eg = EvalGrad(model)
    probs, _ = eg.forward(xs)
    dprobs = torch.randn(probs.shape, device="cuda", generator=gen)

    def eval_grad():
        p, saved = eg.forward(xs)
        eg.backward(dprobs, saved)

    te, te_min = timed(eval_grad, a.reps, a.warmup)
    del eg
    torch.cuda.empty_cache()
    from orcai_amd.training import Trainer

    tr = Trainer(model, learning_rate=1e-4)
    labels = (torch.rand(probs.shape, device="cuda", generator=gen) > 0.5).float()
    dx = torch.empty((B, H, W), device="cuda")

    def train_grad():
        tr.forward_backward(xs.view(-1), H * W, B, labels, dx=dx)

    tt, tt_min = timed(train_grad, a.reps, a.warmup)
    doc = dict(device=torch.cuda.get_device_name(0), batch=B, reps=a.reps, warmup=a.warmup, per_layer=per_layer,
               whole=dict(eval_grad_ms=te, eval_grad_min_ms=te_min, trainer_forward_backward_dx_ms=tt, trainer_min_ms=tt_min, ratio=tt / te))
    out = ROOT / "profiles" / f"eval_grad_{a.tag}.json"
    out.write_text(json.dumps(doc, indent=1) + "\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
