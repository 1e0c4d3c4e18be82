"""Times `orcai predict` from the FILE: wall time from a .wav path to the overlap-averaged probabilities on the host (the call ends in a device
synchronise), on cuda:0, orcai-V1 shape (736 x 171, filters 30/40/50/60, k 3, 128 units, f32), for the two routes a recording's samples can take:

  (a) host decode   wavio.read_wav (every channel to f32 on the host) -> channel pick -> .cuda() from pageable memory -> resample_device where the rates
                    differ -> make_spectrogram -> predict_spectrogram + overlap average.  The route before the device decode, composed here.
  (b) device decode spectrogram.make_spectrogram_device (wavio.read_wav_raw into a page-locked buffer -> non-blocking upload of the file's bytes ->
                    orcai_pcm_decode -> resample_device -> make_spectrogram) -> the same detector.

Files (written to a temporary directory, then read once, so they are in the page cache): 1 h mono PCM16 at 48 kHz (synthetic.synth_recording) and 10 min
of four-channel PCM24 at 22.05 kHz (channel 2 is used).  In one process, after --warmup untimed rounds, the routes alternate for --reps rounds; per route
the median, minimum and maximum.  One more instrumented pass per route, with a synchronise after every stage, splits the time into file read, decode,
H2D, front end and detector (these add up to more than the un-instrumented time wherever stages overlap).  Table mode: both routes over 6 links to the
1 h file, each with its WavPrefetcher (raw=False / raw=True), recording after recording.  Also states whether both routes gave the same probabilities.

    python tools/time_predict_from_wav.py [--reps 5] [--warmup 2] [--hour-seconds 3600] [--out profiles/predict_from_wav_mi355x.json]
"""

from __future__ import annotations

import argparse
import json
import os
import shutil
import statistics
import struct
import sys
import tempfile
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from orcai_amd import frontend as fe  # noqa: E402
from orcai_amd import wavio  # noqa: E402
from orcai_amd.architectures import ResNetLSTM  # noqa: E402
from orcai_amd.auxiliary import Messenger  # noqa: E402
from orcai_amd.io import read_json  # noqa: E402
from orcai_amd.predict import compute_aggregated_predictions  # noqa: E402
from orcai_amd.resample import resample_device  # noqa: E402
from orcai_amd.spectrogram import DEFAULT_ORCAI_PARAMETER, make_spectrogram_device  # noqa: E402
from orcai_amd.synthetic import synth_recording  # noqa: E402

QUIET = Messenger(verbosity=0)


def write_pcm24(path: Path, samples: np.ndarray, rate: int) -> None:
    """samples int16 [channels, frames] -> 24-bit PCM (the 16-bit value in the upper bytes, a counter in the lowest so that no byte is constant)."""
    channels, n = samples.shape
    v = (samples.T.astype(np.int32) << 8) | (np.arange(n * channels, dtype=np.int32).reshape(n, channels) & 0xFF)
    payload = np.ascontiguousarray(v).view(np.uint8).reshape(-1, 4)[:, :3].tobytes()
    header = b"RIFF" + struct.pack("<I", 36 + len(payload)) + b"WAVE"
    header += b"fmt " + struct.pack("<IHHIIHH", 16, wavio.WAVE_FORMAT_PCM, channels, rate, rate * channels * 3, channels * 3, 24)
    path.write_bytes(header + b"data" + struct.pack("<I", len(payload)) + payload)


class Routes:
    def __init__(self):
        self.param = read_json(DEFAULT_ORCAI_PARAMETER)
        self.sp = self.param["spectrogram"]
        self.model = ResNetLSTM((736, 171, 1), 7, list(self.param["model"]["filters"]), 3, 0.0, 128, seed=1)
        self.shape = {"input_shape": [736, 171, 1], "num_labels": 7}

    def detect(self, path, spec):
        return compute_aggregated_predictions(Path(path), spec, self.model, self.param, self.shape, msgr=QUIET)[0]  # ends in .cpu(): synchronises

    def host_pcm(self, path, channel, reader=wavio.read_wav):
        wav, rate = reader(path)
        mono = wav[channel - 1] if wav.shape[0] > 1 else wav[0]
        pcm = torch.from_numpy(np.ascontiguousarray(mono)).cuda()
        return resample_device(pcm, rate, self.sp["sampling_rate"]) if rate != self.sp["sampling_rate"] else pcm

    def host_decode(self, path, channel, reader=wavio.read_wav):
        return self.detect(path, fe.get_frontend().make_spectrogram(self.host_pcm(path, channel, reader), self.sp))

    def device_decode(self, path, channel):
        return self.detect(path, make_spectrogram_device(path, channel, self.param, QUIET)[0])

    # ---- one pass with a synchronise after every stage
    def host_decode_stages(self, path, channel) -> dict:
        t = [time.perf_counter()]

        def lap():
            torch.cuda.synchronize()
            t.append(time.perf_counter())

        Path(path).read_bytes()
        lap()  # the read alone; read_wav below reads again (page cache) and decodes
        wav, rate = wavio.read_wav(path)
        mono = np.ascontiguousarray(wav[channel - 1] if wav.shape[0] > 1 else wav[0])
        lap()
        pcm = torch.from_numpy(mono).cuda()
        lap()
        if rate != self.sp["sampling_rate"]:
            pcm = resample_device(pcm, rate, self.sp["sampling_rate"])
        spec = fe.get_frontend().make_spectrogram(pcm, self.sp)
        lap()
        self.detect(path, spec)
        lap()
        d = np.diff(t) * 1e3
        return dict(file_read_ms=d[0], decode_ms=d[1] - d[0], h2d_ms=d[2], front_end_ms=d[3], detector_ms=d[4], h2d_bytes=int(mono.nbytes),
                    note="decode_ms = read_wav + channel pick minus the plain read; the sum counts the read once")

    def device_decode_stages(self, path, channel) -> dict:
        t = [time.perf_counter()]

        def lap():
            torch.cuda.synchronize()
            t.append(time.perf_counter())

        raw = wavio.read_wav_raw(path, pin=True)
        lap()
        nbytes = raw.n_frames * raw.channels * wavio.BYTES_PER_SAMPLE[raw.format]
        frames = torch.empty(-(-nbytes // 16) * 16, dtype=torch.uint8, device="cuda")
        frames[:nbytes].copy_(raw.payload, non_blocking=True)
        lap()
        raw.release()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        pcm = wavio.decode_device(frames, raw.n_frames, raw.channels, range(raw.channels)[channel - 1] if raw.channels > 1 else 0, raw.format)
        e1.record()
        lap()
        if raw.rate != self.sp["sampling_rate"]:
            pcm = resample_device(pcm, raw.rate, self.sp["sampling_rate"])
        spec = fe.get_frontend().make_spectrogram(pcm, self.sp)
        lap()
        self.detect(path, spec)
        lap()
        d = np.diff(t) * 1e3
        kernel_ms = e0.elapsed_time(e1)
        return dict(file_read_ms=d[0], h2d_ms=d[1], decode_ms=d[2], front_end_ms=d[3], detector_ms=d[4], h2d_bytes=int(nbytes), decode_kernel_ms=kernel_ms,
                    decode_bytes_read=int(nbytes), decode_bytes_written=4 * raw.n_frames,
                    decode_gb_per_s=(nbytes + 4 * raw.n_frames) / kernel_ms / 1e6)


def wall_ms(fn) -> float:
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def summary(ms: list) -> dict:
    return dict(median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms), range_ms=max(ms) - min(ms), ms=[round(x, 3) for x in ms])


def verdict(a: dict, b: dict) -> str:
    if b["median_ms"] <= a["median_ms"] + a["range_ms"]:
        return "device decode is not slower than host decode beyond host decode's own range"
    return "DEVICE DECODE IS SLOWER than host decode beyond host decode's own range"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--hour-seconds", type=float, default=3600.0)
    ap.add_argument("--copies", type=int, default=6)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "predict_from_wav_mi355x.json"))
    a = ap.parse_args()
    torch.cuda.set_device(0)
    R = Routes()
    tmp = Path(tempfile.mkdtemp(prefix="orcai_from_wav_"))
    doc = dict(device=torch.cuda.get_device_name(0), model="orcai-V1 shape, f32", reps=a.reps, warmup=a.warmup, files={})
    try:
        hour = tmp / "hour_mono_pcm16_48k.wav"
        wavio.write_wav_pcm16(hour, synth_recording(a.hour_seconds, 48000, seed=1), 48000)
        four = tmp / "10min_4ch_pcm24_22k.wav"
        write_pcm24(four, np.stack([synth_recording(600.0, 22050, seed=10 + c) for c in range(4)]), 22050)
        for name, path, channel, seconds in (("1h_mono_pcm16_48k", hour, 1, a.hour_seconds), ("10min_4ch_pcm24_22k", four, 2, 600.0)):
            path.read_bytes()
            times = {"host_decode": [], "device_decode": []}
            out = {}
            for r in range(a.warmup + a.reps):
                for route, fn in (("host_decode", R.host_decode), ("device_decode", R.device_decode)):
                    ms = wall_ms(lambda: out.__setitem__(route, fn(path, channel)))
                    if r >= a.warmup:
                        times[route].append(ms)
            sa, sb = summary(times["host_decode"]), summary(times["device_decode"])
            for s in (sa, sb):
                s["audio_seconds_per_s"] = seconds / s["median_ms"] * 1e3
            sa["stages_instrumented"] = R.host_decode_stages(path, channel)
            sb["stages_instrumented"] = R.device_decode_stages(path, channel)
            doc["files"][name] = dict(bytes=path.stat().st_size, audio_seconds=seconds, channel=channel, host_decode=sa, device_decode=sb,
                                      same_probabilities=bool(np.array_equal(out["host_decode"], out["device_decode"])), verdict=verdict(sa, sb))
            print(name, json.dumps(doc["files"][name]), flush=True)
        # table mode: recording after recording, the reads of the next ones running ahead on the prefetcher's threads
        copies = []
        for i in range(a.copies):
            p = tmp / f"copy{i}.wav"
            try:
                os.link(hour, p)
            except OSError:
                shutil.copyfile(hour, p)
            copies.append(p)

        def table(raw: bool):
            wavio.set_prefetcher(wavio.WavPrefetcher(copies, raw=raw))
            try:
                for p in copies:
                    if raw:
                        R.device_decode(p, 1)
                    else:
                        R.host_decode(p, 1, reader=wavio.read_wav_prefetched)
            finally:
                wavio.set_prefetcher(None)

        times = {"host_decode": [], "device_decode": []}
        for r in range(1 + a.reps):
            for route, raw in (("host_decode", False), ("device_decode", True)):
                ms = wall_ms(lambda: table(raw))
                if r >= 1:
                    times[route].append(ms)
        sa, sb = summary(times["host_decode"]), summary(times["device_decode"])
        for s in (sa, sb):
            s["audio_seconds_per_s"] = a.copies * a.hour_seconds / s["median_ms"] * 1e3
        doc["table_mode"] = dict(recordings=a.copies, audio_seconds_each=a.hour_seconds, host_decode=sa, device_decode=sb, verdict=verdict(sa, sb))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(doc, indent=1) + "\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
