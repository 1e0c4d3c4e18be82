"""Times the short-clip and the multi-channel shapes of `orcai predict` with and without the batched detector pass, on cuda:0, orcai-V1
shape (736 x 171, filters 30/40/50/60, k 3, 128 units, f32, seeded untrained weights written to a temporary model directory).

  clips60   256 mono PCM16 clips of 60 s at 48 kHz (8 synthetic recordings, hard-linked to 256 names), table mode: predict(table, batch_frames=675000)
            against predict(table, batch_frames=0), the one-pass-per-recording path, in the same process.  Both load the model once per call.
  clips10   the same for 256 clips of 10 s.
  fourch    10 min of four-channel PCM24 at 22.05 kHz: the all-channels route (one read, one upload, orcai_pcm_decode_planar, the channels as one batch)
            against four single-channel routes (four reads, uploads and passes), on a loaded model, files written in both; and the decode kernels alone
            (HIP events): bytes read + written per second of orcai_pcm_decode_planar beside orcai_pcm_decode of one channel.

Files are written to a temporary directory and read once, so they are in the page cache.  After --warmup untimed rounds the two routes alternate for
--reps rounds; per route the median, minimum and maximum wall time (the call ends in the host half of the last batch, which waits for its copy) and the
audio seconds per second.  One more instrumented pass per route, with a synchronise after every launch half, splits the time into the GPU half (read,
upload, decode, front end, detector, average, copy) and the host half (threshold, label table; no files) and gives the share of straddling snippets.
Every case runs in a child process of its own under a time limit; a case that fails ends the run.

    python tools/time_predict_batch.py [--reps 5] [--warmup 1] [--clips 256] [--out profiles/predict_batch_mi355x.json]
"""

from __future__ import annotations

import argparse
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

CASES = ("clips60", "clips10", "fourch")
HOUR_FRAMES = 675_000


def summary(ms: list, audio_seconds: float) -> dict:
    med = statistics.median(ms)
    return dict(median_ms=med, min_ms=min(ms), max_ms=max(ms), ms=[round(x, 3) for x in ms], audio_seconds_per_s=audio_seconds / med * 1e3)


def wall_ms(fn) -> float:
    import torch

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def alternate(routes: dict, reps: int, warmup: int) -> dict:
    times = {name: [] for name in routes}
    for r in range(warmup + reps):
        for name, fn in routes.items():
            ms = wall_ms(fn)
            print(f"round {r} {name}: {ms:.1f} ms", file=sys.stderr, flush=True)
            if r >= warmup:
                times[name].append(ms)
    return times


def make_model_dir(tmp: Path):
    from orcai_amd.architectures import build_model
    from orcai_amd.auxiliary import Messenger
    from orcai_amd.io import WEIGHTS_SUFFIX, load_orcai_model, read_json

    src = ROOT / "orcai_amd" / "models" / "orcai-V1"
    d = tmp / "model"
    d.mkdir()
    for n in ("orcai_parameter.json", "model_shape.json"):
        shutil.copyfile(src / n, d / n)
    param = read_json(d / "orcai_parameter.json")
    shape = read_json(d / "model_shape.json")
    model = build_model(tuple(shape["input_shape"]), {**param, "model": {**param["model"], "seed": 1}}, msgr=Messenger(verbosity=0))
    model.save_weights(d / (param["name"] + WEIGHTS_SUFFIX))
    return d, load_orcai_model(d)


def run_clips(seconds: float, a) -> dict:
    import pandas as pd
    import torch

    from orcai_amd import predict as P
    from orcai_amd import wavio
    from orcai_amd.auxiliary import Messenger
    from orcai_amd.synthetic import synth_recording

    quiet = Messenger(verbosity=0)
    tmp = Path(tempfile.mkdtemp(prefix="orcai_batch_"))
    try:
        model_dir, (model, param, shape) = make_model_dir(tmp)
        clips = tmp / "clips"
        clips.mkdir()
        distinct = []
        for i in range(8):
            p = clips / f"src{i}.wav"
            wavio.write_wav_pcm16(p, synth_recording(seconds, 48000, seed=100 + i), 48000)
            distinct.append(p)
        names = [f"clip{i:03d}" for i in range(a.clips)]
        for i, n in enumerate(names):
            try:
                os.link(distinct[i % 8], clips / f"{n}.wav")
            except OSError:
                shutil.copyfile(distinct[i % 8], clips / f"{n}.wav")
            (clips / f"{n}.wav").read_bytes()
        pd.DataFrame({"recording": names, "base_dir_recording": [str(clips)] * len(names), "rel_recording_path": [f"{n}.wav" for n in names],
                      "channel": [1] * len(names)}).to_csv(tmp / "table.csv", index=False)
        outs = {}
        for name in ("one_by_one", "batched"):
            outs[name] = tmp / name
            outs[name].mkdir()

        def table(name, batch_frames):
            P.predict(tmp / "table.csv", model_dir=model_dir, output_path=outs[name], overwrite=True, verbosity=0, batch_frames=batch_frames)

        audio = seconds * a.clips
        times = alternate({"one_by_one": lambda: table("one_by_one", 0), "batched": lambda: table("batched", HOUR_FRAMES)}, a.reps, a.warmup)
        doc = dict(clips=a.clips, seconds_each=seconds, audio_seconds=audio, batch_frames=HOUR_FRAMES, model_load_ms=wall_ms(lambda: make_model_dir_load(model_dir)),
                   one_by_one=summary(times["one_by_one"], audio), batched=summary(times["batched"], audio))
        doc["same_files"] = all((outs["one_by_one"] / f.name).read_bytes() == f.read_bytes() for f in outs["batched"].iterdir()) and \
            len(list(outs["batched"].iterdir())) == len(list(outs["one_by_one"].iterdir())) == a.clips
        # instrumented: a synchronise after every launch half
        items = [(clips / f"{n}.wav", 1) for n in names]
        gpu = host = 0.0
        for path, channel in items:
            t0 = time.perf_counter()
            state = P.predict_wav_launch(path, channel, model, param, shape, msgr=quiet)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            P.predict_wav_finish(state, msgr=quiet)
            gpu, host = gpu + t1 - t0, host + time.perf_counter() - t1
        doc["one_by_one"]["halves_instrumented"] = dict(gpu_half_ms=gpu * 1e3, host_half_ms=host * 1e3)
        gpu = host = 0.0
        junk = total = batches = 0
        states = P.predict_wavs_launch(items, model, param, shape, max_frames=HOUR_FRAMES, msgr=quiet)
        while True:
            t0 = time.perf_counter()
            state = next(states, None)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            if state is None:
                break
            P.predict_wavs_finish(state, msgr=quiet)
            gpu, host = gpu + t1 - t0, host + time.perf_counter() - t1
            junk, total, batches = junk + state.get("junk_snippets", 0), total + state.get("snippets", 0), batches + 1
        doc["batched"]["halves_instrumented"] = dict(gpu_half_ms=gpu * 1e3, host_half_ms=host * 1e3, batches=batches, snippets=total, junk_snippets=junk,
                                                     junk_share=junk / max(total, 1))
        return doc
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def make_model_dir_load(model_dir):
    from orcai_amd.io import load_orcai_model

    load_orcai_model(model_dir)


def run_fourch(a) -> dict:
    import numpy as np
    import torch

    from orcai_amd import _native as N
    from orcai_amd import predict as P
    from orcai_amd import wavio
    from orcai_amd.auxiliary import Messenger
    from orcai_amd.synthetic import synth_recording
    from tools.time_predict_from_wav import write_pcm24

    quiet = Messenger(verbosity=0)
    tmp = Path(tempfile.mkdtemp(prefix="orcai_batch_"))
    try:
        model_dir, (model, param, shape) = make_model_dir(tmp)
        seconds, rate, channels = a.fourch_seconds, 22050, 4
        folders = {}
        for name in ("four_calls", "all_channels"):
            folders[name] = tmp / name
            folders[name].mkdir()
        wav = folders["four_calls"] / "array.wav"
        write_pcm24(wav, np.stack([synth_recording(seconds, rate, seed=10 + c) for c in range(channels)]), rate)
        os.link(wav, folders["all_channels"] / "array.wav")
        wav.read_bytes()

        def four_calls():
            for c in range(1, channels + 1):
                P._predict_and_save(folders["four_calls"] / "array.wav", c, model, param, shape, overwrite=True, msgr=quiet)

        def all_channels():
            P._predict_all_channels(folders["all_channels"] / "array.wav", model, param, shape, overwrite=True, msgr=quiet)

        audio = seconds * channels
        times = alternate({"four_calls": four_calls, "all_channels": all_channels}, a.reps, a.warmup)
        doc = dict(audio_seconds_per_channel=seconds, channels=channels, bytes=wav.stat().st_size, four_calls=summary(times["four_calls"], audio),
                   all_channels=summary(times["all_channels"], audio))
        names = [f"array_c{c}_{param['name']}_predicted.txt" for c in range(1, channels + 1)]
        doc["same_files"] = all((folders["four_calls"] / n).read_bytes() == (folders["all_channels"] / n).read_bytes() for n in names)
        # the GPU half / host half of the all-channels route, and its junk share
        from orcai_amd.spectrogram import load_wav_all

        t0 = time.perf_counter()
        pcms = load_wav_all(wav, param["spectrogram"]["sampling_rate"], quiet)
        states = list(P._launch_batches(((c, lambda pcm=pcm: pcm) for c, pcm in enumerate(pcms, start=1)), model, param, shape, max_frames=10**9, msgr=quiet))
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        for state in states:
            P._finish_batch(state, msgr=quiet)
        doc["all_channels"]["halves_instrumented"] = dict(gpu_half_ms=(t1 - t0) * 1e3, host_half_ms=(time.perf_counter() - t1) * 1e3, batches=len(states),
                                                          snippets=sum(s["snippets"] for s in states), junk_snippets=sum(s["junk_snippets"] for s in states))
        doc["all_channels"]["halves_instrumented"]["junk_share"] = doc["all_channels"]["halves_instrumented"]["junk_snippets"] / doc["all_channels"]["halves_instrumented"]["snippets"]
        # the decode kernels alone
        raw = wavio.read_wav_raw(wav)
        nbytes = raw.payload.size
        dev = torch.zeros(-(-nbytes // 16) * 16, dtype=torch.uint8, device="cuda")
        dev[:nbytes] = torch.from_numpy(raw.payload).cuda()
        stride = -(-raw.n_frames // 4) * 4
        planes = torch.empty((channels, stride), dtype=torch.float32, device="cuda")
        one = torch.empty(raw.n_frames, dtype=torch.float32, device="cuda")
        lib, st = N.lib(), N.stream_ptr()

        def kernel_ms(fn):
            ms = []
            for _ in range(2 + 9):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                N.check(fn(), "decode")
                e1.record()
                e1.synchronize()
                ms.append(e0.elapsed_time(e1))
            return statistics.median(ms[2:])

        planar = kernel_ms(lambda: lib.orcai_pcm_decode_planar(N.ptr(dev), raw.n_frames, channels, raw.format, N.ptr(planes), stride, st))
        single = kernel_ms(lambda: lib.orcai_pcm_decode(N.ptr(dev), raw.n_frames, channels, 1, raw.format, N.ptr(one), st))
        doc["decode_kernels"] = dict(
            planar=dict(ms=planar, bytes_read=int(nbytes), bytes_written=4 * raw.n_frames * channels, gb_per_s=(nbytes + 4 * raw.n_frames * channels) / planar / 1e6),
            one_channel=dict(ms=single, bytes_read=int(nbytes), bytes_written=4 * raw.n_frames, gb_per_s=(nbytes + 4 * raw.n_frames) / single / 1e6,
                             note="reads only the words that hold the channel's samples; bytes_read counts the whole chunk, as profiles/predict_from_wav_mi355x.json does"))
        return doc
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--clips", type=int, default=256)
    ap.add_argument("--fourch-seconds", type=float, default=600.0)
    ap.add_argument("--timeout", type=int, default=420, help="seconds a case may take")
    ap.add_argument("--case", choices=CASES, default=None, help="run one case in this process and print its JSON line (what the parent starts)")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "predict_batch_mi355x.json"))
    a = ap.parse_args()
    if a.case is not None:
        import torch

        torch.cuda.set_device(0)
        doc = run_fourch(a) if a.case == "fourch" else run_clips(60.0 if a.case == "clips60" else 10.0, a)
        doc["device"] = torch.cuda.get_device_name(0)
        print("RESULT " + json.dumps(doc), flush=True)
        return
    doc = dict(model="orcai-V1 shape, f32, untrained seeded weights", reps=a.reps, warmup=a.warmup, cases={})
    for case in CASES:  # each GPU step in a child of its own, under its own time limit; the first failure ends the run
        cmd = [sys.executable, str(Path(__file__).resolve()), "--case", case, "--reps", str(a.reps), "--warmup", str(a.warmup), "--clips", str(a.clips),
               "--fourch-seconds", str(a.fourch_seconds)]
        done = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=a.timeout)  # the child's progress lines (stderr) pass through
        lines = [ln for ln in done.stdout.splitlines() if ln.startswith("RESULT ")]
        if done.returncode != 0 or not lines:
            sys.stderr.write(done.stdout[-2000:])
            raise SystemExit(f"case {case} failed with exit status {done.returncode}")
        doc["cases"][case] = json.loads(lines[-1][len("RESULT "):])
        print(case, json.dumps(doc["cases"][case]), flush=True)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    main()
