"""Times the frozen-BatchNorm weight gradient at the orcai-V1 shape (736 x 171, filters 30/40/50/60, k 3, 128 units), B = 64, on cuda:0:

  (a) per layer, for each of orcai-V1's nine separable convs: the fused orcai_sepconv_wgrad_frozen + orcai_frozen_bn_finish against
      orcai_amd.eval_grad.compose_wgrad (the training step's reduction launchers and the same finish) on the same random planes -- the numbers that set
      EvalGrad.fused_wgrad's routing rule;
  (b) the whole gradient: EvalGrad.forward + backward(wgrad=True) against the same with wgrad=False (what the weight gradients add) and against
      Trainer.forward_backward, the only route to a weight gradient before it (training mode: batch statistics, Dropout), in the same process.

Medians of event-timed repetitions after warm-up; one JSON document to profiles/frozen_grad_<tag>.json (or --out) and stdout.

    python tools/time_frozen_grad.py [--batch 64] [--reps 20] [--warmup 5] [--tag mi355x] [--out FILE]
"""

from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))

from time_eval_grad import timed  # noqa: E402

from orcai_amd import _native as N  # noqa: E402
from orcai_amd.architectures import ENTRY_FILTERS, FINAL_FILTERS, ResNetLSTM  # noqa: E402
from orcai_amd.eval_grad import EvalGrad, compose_wgrad  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--tag", default="mi355x")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    B, k = a.batch, 3
    model = ResNetLSTM((736, 171, 1), 7, [30, 40, 50, 60], k, 0.5, 128, seed=1)
    lib, st = N.lib(), N.stream_ptr()
    shapes = model.stage_shapes()
    layers, c = [], ENTRY_FILTERS
    for b, f in enumerate(model.filters, start=1):
        h, w, _ = shapes[b - 1]
        layers += [(f"b{b}/sep_a", c, f, h, w, True, 1), (f"b{b}/sep_b", f, f, h, w, False, 0)]
        c = f
    layers.append(("sep_f", c, FINAL_FILTERS, shapes[-1][0], shapes[-1][1], False, 0))
    gen = torch.Generator(device="cuda").manual_seed(0)
    partials, scratch = torch.empty(512 * 64 * 64, device="cuda"), torch.zeros(64, dtype=torch.float64, device="cuda")
    fws = torch.empty(EvalGrad.WGRAD_WORKSPACE_FLOATS, device="cuda")
    per_layer = []
    for name, cin, cout, h, w, ygate, relu_in in layers:
        WP = model.padded_width(w)
        planes = lambda ch: torch.zeros((B, (ch + 3) // 4, h + 2, WP, 4), device="cuda")  # noqa: E731

        def fill(ch):
            t = planes(ch)
            t[:, :, 1 : 1 + h, :w, :] = torch.randn((B, (ch + 3) // 4, h, w, 4), device="cuda", generator=gen)
            return t

        g, y, x = fill(cout), fill(cout) if ygate else None, fill(cin)
        rnd = lambda *s: torch.randn(s, device="cuda", generator=gen)  # noqa: E731
        wts, pw, taps = rnd(cout, cin) / cout**0.5, rnd(cin, cout) / cin**0.5, rnd((cin + 3) // 4, 9, 4) / 3
        bias, gamma, mean, var = rnd(cout), rnd(cout), rnd(cout), torch.rand(cout, device="cuda", generator=gen) + 0.5
        u, du = planes(cin), planes(cin)
        G, sums, dWdw = torch.zeros(cout * cin, device="cuda"), torch.zeros(cout, device="cuda"), torch.zeros(9 * cin, device="cuda")
        dWpw, dbias, dgamma, dbeta = torch.zeros(cin * cout, device="cuda"), torch.zeros(cout, device="cuda"), torch.zeros(cout, device="cuda"), torch.zeros(cout, device="cuda")

        def composed():  # (gates g in place: idempotent after the first repetition; G and dWdw keep accumulating, which costs the same)
            compose_wgrad(lib, g, y, x, relu_in, B, cin, cout, h, w, k, taps, wts, pw, bias, gamma, mean, var, u, du, G, sums, scratch, partials, dWdw, dWpw, dbias, dgamma, dbeta, st)

        def fused():
            N.check(lib.orcai_sepconv_wgrad_frozen(x.data_ptr(), g.data_ptr(), None if y is None else y.data_ptr(), relu_in, B, cin, cout, h, w, k, taps.data_ptr(), wts.data_ptr(),
                                                   G.data_ptr(), sums.data_ptr(), dWdw.data_ptr(), fws.data_ptr(), fws.numel(), st), "orcai_sepconv_wgrad_frozen")
            N.check(lib.orcai_frozen_bn_finish(G.data_ptr(), sums.data_ptr(), pw.data_ptr(), bias.data_ptr(), gamma.data_ptr(), mean.data_ptr(), var.data_ptr(), 1e-3, cin, cout,
                                               dWpw.data_ptr(), dbias.data_ptr(), dgamma.data_ptr(), dbeta.data_ptr(), st), "orcai_frozen_bn_finish")

        tf, tf_min = timed(fused, a.reps, a.warmup)
        tc, tc_min = timed(composed, a.reps, a.warmup)
        px = B * h * w
        nbytes = 16 * px * (((cout + 3) // 4) * (2 if ygate else 1) + (cin + 3) // 4)  # one pass over g (and y_gate) and x: what the fused kernel must read
        per_layer.append(dict(layer=name, cin=cin, cout=cout, h=h, w=w, fused_ms=tf, fused_min_ms=tf_min, composed_ms=tc, composed_min_ms=tc_min, ratio=tc / tf,
                              min_hbm_bytes=nbytes, fused_gbs=nbytes / tf / 1e6, evalgrad_runs_fused=EvalGrad(model).fused_wgrad(B, cin, h, w)))
        del g, y, x, u, du
    H, W = model.input_hw
    xs = torch.rand((B, H, W), device="cuda", generator=gen)
    eg = EvalGrad(model)
    probs, _ = eg.forward(xs)
    dprobs = torch.randn(probs.shape, device="cuda", generator=gen)

    def frozen_grad():
        p, saved = eg.forward(xs)
        eg.backward(dprobs, saved, wgrad=True)

    def input_grad():
        p, saved = eg.forward(xs)
        eg.backward(dprobs, saved)

    tw, tw_min = timed(frozen_grad, a.reps, a.warmup)
    ti, ti_min = timed(input_grad, a.reps, a.warmup)
    del eg
    torch.cuda.empty_cache()
    from orcai_amd.training import Trainer

    tr = Trainer(model, learning_rate=1e-4)
    labels = (torch.rand(probs.shape, device="cuda", generator=gen) > 0.5).float()

    def train_grad():
        tr.forward_backward(xs.view(-1), H * W, B, labels)

    tt, tt_min = timed(train_grad, a.reps, a.warmup)
    doc = dict(device=torch.cuda.get_device_name(0), batch=B, reps=a.reps, warmup=a.warmup, per_layer=per_layer,
               whole=dict(frozen_grad_ms=tw, frozen_grad_min_ms=tw_min, eval_input_grad_only_ms=ti, eval_input_grad_only_min_ms=ti_min, trainer_forward_backward_ms=tt,
                          trainer_min_ms=tt_min, frozen_over_trainer=tw / tt))
    out = Path(a.out) if a.out else ROOT / "profiles" / f"frozen_grad_{a.tag}.json"
    out.write_text(json.dumps(doc, indent=1) + "\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
