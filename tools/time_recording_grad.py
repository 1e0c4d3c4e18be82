"""Times the whole-recording gradient at the orcai-V1 shape (736 x 171, filters 30/40/50/60, k 3, 128 units) on cuda:0, on synthetic spectrograms:

  (a) RecordingGrad.forward + backward (chunks of --chunk snippets: the stored activations do not grow with the recording) on a 10-minute recording
      (112500 frames at 48 kHz / hop 256) and on a short one of exactly --chunk snippets;
  (b) the only route before it: every snippet of the recording in ONE EvalGrad batch (as_strided + contiguous), the overlap average and its adjoint in
      torch, torch index_add_ into the spectrogram gradient.  It is run where the batch fits: while the flat `saved` tensor of the batch stays below 2^31
      floats (the batch sizes EvalGrad has been run at); beyond that only its activation bytes are stated, computed from the shapes, not measured.

Medians of event-timed repetitions after warm-up, and torch.cuda.max_memory_allocated beyond what is alive before the call (the spectrogram and the
bound weights are alive before it).  One JSON document to <out-dir>/recording_grad_<tag>.json and stdout.

    python tools/time_recording_grad.py [--chunk 64] [--minutes 10] [--reps 10] [--warmup 2] [--tag mi355x] [--out-dir profiles]
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

from orcai_amd.architectures import ResNetLSTM  # noqa: E402
from orcai_amd.eval_grad import EvalGrad, RecordingGrad  # noqa: E402

FRAMES_PER_SECOND = 48000 / 256


def peak_beyond_start(fn) -> int:
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def whole_batch_route(eg: EvalGrad, spec: torch.Tensor, davg: torch.Tensor, g: dict):
    """(avg, dspec) with all n snippets in one EvalGrad batch; the average and its adjoint by torch indexing."""
    T, W = spec.shape
    n, H, shift, P, step, S = g["n"], g["H"], g["shift"], g["P"], g["step"], g["S"]
    x = torch.as_strided(spec, (n, H, W), (shift * W, W, 1)).contiguous()
    probs, saved = eg.forward(x)
    L = probs.shape[2]
    rows = (torch.arange(n, device=spec.device)[:, None] * step + torch.arange(P, device=spec.device)[None, :]).reshape(-1)
    cnt = torch.zeros(S, device=spec.device).index_add_(0, rows, torch.ones(n * P, device=spec.device))
    avg = torch.zeros((S, L), device=spec.device).index_add_(0, rows, probs.reshape(n * P, L)) / cnt.clamp(min=1.0)[:, None]
    dpred = (davg / cnt.clamp(min=1.0)[:, None])[rows].reshape(n, P, L)
    dx = eg.backward(dpred, saved)
    frames = (torch.arange(n, device=spec.device)[:, None] * shift + torch.arange(H, device=spec.device)[None, :]).reshape(-1)
    dspec = torch.zeros((T, W), device=spec.device).index_add_(0, frames, dx.reshape(n * H, W))
    return avg, dspec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunk", type=int, default=64)
    ap.add_argument("--minutes", type=float, default=10.0)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--tag", default="mi355x")
    ap.add_argument("--out-dir", default=str(ROOT / "profiles"))
    a = ap.parse_args()
    torch.cuda.set_device(0)
    model = ResNetLSTM((736, 171, 1), 7, [30, 40, 50, 60], 3, 0.5, 128, seed=1)
    H, W = model.input_hw
    rg = RecordingGrad(model, chunk=a.chunk)
    per_snippet = rg.eg.per_snippet
    gen = torch.Generator(device="cuda").manual_seed(0)
    runs = []
    for label, T in (("short", H + (H // 2) * (a.chunk - 1)), ("long", int(a.minutes * 60 * FRAMES_PER_SECOND))):
        g = rg.geometry(T)
        spec = torch.rand((T, W), device="cuda", generator=gen)
        davg = torch.randn((g["S"], model.num_labels), device="cuda", generator=gen)
        out = {}

        def recording_grad():
            out["avg"] = rg.forward(spec)
            out["dspec"] = rg.backward(spec, davg)

        recording_grad()  # binds the weights, builds the workspaces
        peak = peak_beyond_start(recording_grad)
        ms, ms_min = timed(recording_grad, a.reps, a.warmup)
        run = dict(recording=label, frames=T, seconds=T / FRAMES_PER_SECOND, snippets=g["n"], chunk=a.chunk,
                   recording_grad=dict(forward_backward_ms=ms, min_ms=ms_min, peak_bytes_beyond_start=peak, stored_activation_bytes=4 * min(a.chunk, g["n"]) * per_snippet),
                   whole_batch_stored_activation_bytes=4 * g["n"] * per_snippet)
        if g["n"] * per_snippet < 2**31:
            eg = EvalGrad(model)
            res = {}

            def whole():
                res["avg"], res["dspec"] = whole_batch_route(eg, spec, davg, g)

            whole()
            peak_w = peak_beyond_start(whole)
            ms_w, ms_w_min = timed(whole, a.reps, a.warmup)
            scale = float(res["dspec"].abs().max())
            run["whole_batch"] = dict(forward_backward_ms=ms_w, min_ms=ms_w_min, peak_bytes_beyond_start=peak_w, ratio_to_recording_grad=ms_w / ms,
                                      max_abs_dspec_difference_over_max=float((res["dspec"] - out["dspec"]).abs().max()) / scale,
                                      max_abs_avg_difference=float((res["avg"] - out["avg"]).abs().max()))
            del eg, res
        else:
            run["whole_batch"] = "not run: the batch's stored activations pass 2^31 floats; its bytes above are computed from the shapes, not measured"
        runs.append(run)
        del spec, davg, out
        torch.cuda.empty_cache()
    doc = dict(device=torch.cuda.get_device_name(0), model="orcai-V1 shape, f32", per_snippet_floats=per_snippet, reps=a.reps, warmup=a.warmup, runs=runs)
    path = Path(a.out_dir) / f"recording_grad_{a.tag}.json"
    path.parent.mkdir(parents=True, exist_ok=True)
    path.write_text(json.dumps(doc, indent=1) + "\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
