"""Writes down every C-ABI launcher call of predict_spectrogram, for both precisions, on a handful of small layouts that between them take
every route of the shared-trunk driver: two levels, two levels with several tail chunks and launch groups, one level, nothing
shared (f32's two-phase loop, f16's chunk loop) and the benchmarked plane.

A record is the ordered list of [launcher, [every argument whose ctypes type in _native._SIGNATURES is not c_void_p]]: pointers differ from run
to run, integers and floats do not.  Recorded after one warm-up call (weights prepared, workspaces allocated).  The host-side planning has no
other output, so two commits with equal records launch the same kernels on the same shapes in the same order.

    python tools/record_predict_launches.py [--out tests/golden/predict_launch_record.json]

tests/test_predict_launch_record_gpu.py replays the scenarios against the committed file; run this tool on the commit whose launches are to be
pinned and commit its output unchanged.
"""

from __future__ import annotations

import argparse
import ctypes
import json
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]

from recording_lib import RecordingLib  # noqa: E402

from orcai_amd import _native as N  # noqa: E402
from orcai_amd.architectures import ResNetLSTM  # noqa: E402

GOLDEN = ROOT / "tests" / "golden" / "predict_launch_record.json"
SNIPPETS = 17
# name: (input plane, model attributes set after construction, predict_spectrogram keywords)
SCENARIOS = {
    "192x21_two_levels": ((192, 21), {}, {}),
    "192x21_three_tail_chunks": ((192, 21), {"tail_chunk": 8, "shared_strides": 3}, {"chunk": 1}),
    "200x21_one_level": ((200, 21), {}, {}),
    "196x21_unshared_chunk5": ((196, 21), {}, {"chunk": 5}),
    "736x171_benchmarked": ((736, 171), {}, {}),
}
PRECISIONS = ("f32", "f16")


def record(name: str, precision: str) -> list:
    """The launch record of one scenario at one precision, on the current device."""
    (H, W), attrs, kw = SCENARIOS[name]
    model = ResNetLSTM((H, W, 1), 7, [30, 40, 50, 60], 3, lstm_units=128, seed=1)
    model.precision = precision
    for key, value in attrs.items():
        setattr(model, key, value)
    extra = 101 if H // 2 > 101 else 37  # fewer extra rows than a snippet stride: exactly SNIPPETS snippets
    spec = torch.rand(((SNIPPETS + 1) * (H // 2) + extra, W), generator=torch.Generator(device="cuda").manual_seed(0), device="cuda")
    assert model.predict_spectrogram(spec, **kw).shape[0] == SNIPPETS  # warm-up: the record below is the steady state
    rec, real = RecordingLib(N.lib()), N.lib
    N.lib = lambda: rec
    try:
        model.predict_spectrogram(spec, **kw)
        torch.cuda.synchronize()
    finally:
        N.lib = real
    return [[fn, [a for a, t in zip(args, N._SIGNATURES[fn][1], strict=True) if t is not ctypes.c_void_p]] for fn, _, args in rec.calls]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(GOLDEN))
    a = ap.parse_args()
    torch.cuda.set_device(0)
    lines = []
    for name in SCENARIOS:
        for precision in PRECISIONS:
            calls = ",\n".join("   " + json.dumps(c) for c in record(name, precision))
            lines.append(f'  {json.dumps(name + "/" + precision)}: [\n{calls}\n  ]')
    head = dict(snippets=SNIPPETS, model="ResNetLSTM k=3 filters (30, 40, 50, 60), 7 labels, 128 LSTM units, seed 1",
                scenarios={k: dict(input_hw=hw, attributes=at, predict_kwargs=kw) for k, (hw, at, kw) in SCENARIOS.items()})
    text = '{\n "about": ' + json.dumps(head) + ',\n "records": {\n' + ",\n".join(lines) + "\n }\n}\n"
    json.loads(text)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(text)
    print(f"{a.out}: {len(lines)} records, {len(text)} bytes")


if __name__ == "__main__":
    main()
