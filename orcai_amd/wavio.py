"""WAV reading for the front end (replaces the soundfile half of ``librosa.load``,
reference ``src/orcAI/spectrogram.py:23-27``).

Scaling follows libsndfile's float read: PCM16 / 2**15, PCM24 / 2**23, PCM32 / 2**31,
unsigned 8-bit (x - 128) / 2**7, IEEE float passed through.

Two routes.  ``read_wav`` decodes every channel on the host (numpy only).  ``read_wav_raw`` parses the container the same way but leaves the data
chunk as the bytes of the file, read straight into a (page-locked) buffer; ``decode_device`` turns those bytes, uploaded, into one channel's f32
samples with ``orcai_pcm_decode`` (csrc/wav_decode.hip), ``decode_device_planar`` into every channel's with ``orcai_pcm_decode_planar``, bit for bit what
``read_wav`` gives.  The predict path takes the second route.
"""

from __future__ import annotations

import struct
import threading
from dataclasses import dataclass, field
from pathlib import Path

import numpy as np

WAVE_FORMAT_PCM = 1
WAVE_FORMAT_IEEE_FLOAT = 3
WAVE_FORMAT_EXTENSIBLE = 0xFFFE


def read_wav(path: str | Path) -> tuple[np.ndarray, int]:
    """Returns (float32 array [channels, frames], sampling rate)."""
    data = Path(path).read_bytes()
    if len(data) < 12 or data[0:4] != b"RIFF" or data[8:12] != b"WAVE":
        raise ValueError(f"{path}: not a RIFF/WAVE file")
    pos = 12
    fmt = None
    payload = None
    while pos + 8 <= len(data):
        cid = data[pos : pos + 4]
        size = struct.unpack_from("<I", data, pos + 4)[0]
        body = data[pos + 8 : pos + 8 + size]
        if cid == b"fmt ":
            tag, channels, rate, _, block_align, bits = struct.unpack_from("<HHIIHH", body, 0)
            if tag == WAVE_FORMAT_EXTENSIBLE and len(body) >= 26:
                tag = struct.unpack_from("<H", body, 24)[0]
            fmt = (tag, channels, rate, block_align, bits)
        elif cid == b"data":
            payload = body
        pos += 8 + size + (size & 1)
    if fmt is None or payload is None:
        raise ValueError(f"{path}: missing fmt or data chunk")
    tag, channels, rate, block_align, bits = fmt
    frame_bytes = channels * (bits // 8)
    n = len(payload) // frame_bytes
    payload = payload[: n * frame_bytes]
    if tag == WAVE_FORMAT_PCM:
        if bits == 16:
            x = np.frombuffer(payload, dtype="<i2").astype(np.float32) / np.float32(32768.0)
        elif bits == 8:
            x = (np.frombuffer(payload, dtype=np.uint8).astype(np.float32) - np.float32(128.0)) / np.float32(128.0)
        elif bits == 24:
            b = np.frombuffer(payload, dtype=np.uint8).reshape(-1, 3).astype(np.int32)
            v = b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)
            v = np.where(v & 0x800000, v - 0x1000000, v)
            x = (v.astype(np.float64) / 8388608.0).astype(np.float32)
        elif bits == 32:
            x = (np.frombuffer(payload, dtype="<i4").astype(np.float64) / 2147483648.0).astype(np.float32)
        else:
            raise ValueError(f"{path}: unsupported PCM width {bits}")
    elif tag == WAVE_FORMAT_IEEE_FLOAT:
        if bits == 32:
            x = np.frombuffer(payload, dtype="<f4").astype(np.float32)
        elif bits == 64:
            x = np.frombuffer(payload, dtype="<f8").astype(np.float32)
        else:
            raise ValueError(f"{path}: unsupported float width {bits}")
    else:
        raise ValueError(f"{path}: unsupported WAVE format tag {tag}")
    return np.ascontiguousarray(x.reshape(n, channels).T), int(rate)


FORMAT_U8, FORMAT_S16, FORMAT_S24, FORMAT_S32, FORMAT_F32, FORMAT_F64 = range(6)  # `format` of orcai_pcm_decode (include/orcai_hip.h)
BYTES_PER_SAMPLE = (1, 2, 3, 4, 4, 8)
MAX_DEVICE_CHANNELS = 64  # orcai_pcm_decode's limit; a wider file is decoded by read_wav


def _sample_format(path, tag: int, bits: int) -> int:
    """The orcai_pcm_decode format of a (format tag, bits per sample) pair; read_wav's ValueErrors for what it refuses."""
    if tag == WAVE_FORMAT_PCM:
        if bits not in (8, 16, 24, 32):
            raise ValueError(f"{path}: unsupported PCM width {bits}")
        return {8: FORMAT_U8, 16: FORMAT_S16, 24: FORMAT_S24, 32: FORMAT_S32}[bits]
    if tag == WAVE_FORMAT_IEEE_FLOAT:
        if bits not in (32, 64):
            raise ValueError(f"{path}: unsupported float width {bits}")
        return FORMAT_F32 if bits == 32 else FORMAT_F64
    raise ValueError(f"{path}: unsupported WAVE format tag {tag}")


class _PinnedPool:
    """Page-locked staging buffers for the data chunks on their way to the device.  Page-locking hundreds of MB per recording would cost more than the
    pinned copy saves, so buffers are kept: one grows to the largest payload it has met and serves recording after recording.  A buffer that is handed
    back comes with the event recorded after its host-to-device copy; it is handed out again only once that event has completed, and only the host
    thread that wants the buffer waits for it."""

    GRANULE = 1 << 20

    def __init__(self):
        self.lock = threading.Lock()
        self.free: list = []  # [tensor, event or None], oldest first

    def take(self, nbytes: int):
        import torch

        with self.lock:
            ready = [e for e in self.free if e[1] is None or e[1].query()]
            fitting = [e for e in ready if e[0].numel() >= nbytes]
            entry = min(fitting, key=lambda e: e[0].numel()) if fitting else (ready[0] if ready else (self.free[0] if self.free else None))
            if entry is not None:
                self.free = [e for e in self.free if e is not entry]  # by identity: == on an entry would compare tensors
        if entry is not None:
            buf, event = entry
            if event is not None:
                event.synchronize()  # returns at once when the copy is done; otherwise this thread alone waits for it
            if buf.numel() >= nbytes:
                return buf
            del buf, entry  # too small: let it go and lock a larger one in its place
        size = max(self.GRANULE, -(-nbytes // self.GRANULE) * self.GRANULE)
        return torch.empty(size, dtype=torch.uint8, pin_memory=True)

    def give(self, buf, event) -> None:
        with self.lock:
            self.free.append([buf, event])


_pinned_pool = _PinnedPool()


@dataclass
class RawWav:
    """A WAV file with its data chunk left as it lies in the file.  payload: uint8[n_frames * channels * bytes per sample], whole frames only, a
    numpy array or (pin=True) a page-locked torch tensor on loan from the pool: call release(event) with the event recorded after its upload."""

    payload: object
    format: int
    channels: int
    rate: int
    n_frames: int
    bits: int
    _pinned: object = field(default=None, repr=False, compare=False)

    def release(self, event=None) -> None:
        """Hands a pinned buffer back to the pool; it is reused once `event` (the end of its host-to-device copy) has completed.  payload is dead after."""
        buf, self._pinned = self._pinned, None
        if buf is not None:
            self.payload = None
            _pinned_pool.give(buf, event)

    def __del__(self):  # a recording the caller dropped unread (skipped, cancelled): the buffer goes back
        try:
            self.release()
        except Exception:
            pass


def _readinto_all(f, view) -> int:
    got = 0
    while got < len(view):
        n = f.readinto(view[got:])
        if not n:
            break
        got += n
    return got


def read_wav_raw(path: str | Path, pin: bool = False) -> RawWav:
    """read_wav's container rules (chunk walk with odd-size padding, EXTENSIBLE sub-format, the last data chunk wins, fmt may follow data, a chunk size
    beyond the end of the file is clipped, whole frames only, the same ValueErrors) without its copies: seeks from chunk header to chunk header and reads
    the data chunk straight into the destination, a page-locked torch tensor from the pool with pin=True (where there is a GPU), else a numpy buffer."""
    with open(path, "rb") as f:
        head = f.read(12)
        if len(head) < 12 or head[0:4] != b"RIFF" or head[8:12] != b"WAVE":
            raise ValueError(f"{path}: not a RIFF/WAVE file")
        file_size = f.seek(0, 2)
        pos = 12
        fmt = None
        data = None  # (offset, size) of the body of the last data chunk
        while pos + 8 <= file_size:
            f.seek(pos)
            cid, size = struct.unpack("<4sI", f.read(8))
            if cid == b"fmt ":
                body = f.read(min(size, 26))
                tag, channels, rate, _, block_align, bits = struct.unpack_from("<HHIIHH", body, 0)
                if tag == WAVE_FORMAT_EXTENSIBLE and len(body) >= 26:
                    tag = struct.unpack_from("<H", body, 24)[0]
                fmt = (tag, channels, rate, block_align, bits)
            elif cid == b"data":
                data = (pos + 8, min(size, file_size - (pos + 8)))
            pos += 8 + size + (size & 1)
        if fmt is None or data is None:
            raise ValueError(f"{path}: missing fmt or data chunk")
        tag, channels, rate, block_align, bits = fmt
        frame_bytes = channels * (bits // 8)
        n = data[1] // frame_bytes
        sample_format = _sample_format(path, tag, bits)
        nbytes = n * frame_bytes
        pinned = None
        if pin:
            import torch

            if torch.cuda.is_available():
                pinned = _pinned_pool.take(nbytes)
        if pinned is not None:
            payload = pinned[:nbytes]
            view = memoryview(pinned.numpy())[:nbytes]
        else:
            payload = np.empty(nbytes, dtype=np.uint8)
            view = memoryview(payload)
        raw = RawWav(payload, sample_format, int(channels), int(rate), int(n), int(bits), pinned)
        f.seek(data[0])
        if _readinto_all(f, view) != nbytes:
            raise OSError(f"{path}: short read of the data chunk")
        return raw


def decode_device(frames, n_frames: int, channels: int, channel: int, sample_format: int):
    """orcai_pcm_decode: uint8 cuda `frames` (the data chunk, padded to a multiple of 16 bytes) -> f32 cuda [n_frames], the samples of 0-based `channel`."""
    import torch

    from orcai_amd import _native as N

    if not (frames.is_cuda and frames.dtype == torch.uint8 and frames.dim() == 1 and frames.is_contiguous()):
        raise TypeError("frames must be a contiguous 1-D uint8 CUDA tensor")
    if not 0 <= sample_format < len(BYTES_PER_SAMPLE):
        raise ValueError(f"unknown sample format {sample_format}")
    need = -(-n_frames * channels * BYTES_PER_SAMPLE[sample_format] // 16) * 16
    if frames.numel() < need:
        raise ValueError(f"frames holds {frames.numel()} bytes; {n_frames} frames need {need} (rounded up to 16)")
    out = torch.empty(n_frames, dtype=torch.float32, device=frames.device)
    with torch.cuda.device(frames.device):
        N.check(N.lib().orcai_pcm_decode(N.ptr(frames), n_frames, channels, channel, sample_format, N.ptr(out), N.stream_ptr()), "orcai_pcm_decode")
    return out


def _upload(raw: RawWav):
    """The payload bytes of a RawWav on the current device, padded to a multiple of 16: a non-blocking copy when the payload is page-locked.  A pinned
    payload goes back to the pool, gated by the event recorded after its copy."""
    import torch

    nbytes = raw.n_frames * raw.channels * BYTES_PER_SAMPLE[raw.format]
    frames = torch.empty(-(-nbytes // 16) * 16, dtype=torch.uint8, device="cuda")
    if raw._pinned is not None:
        frames[:nbytes].copy_(raw.payload, non_blocking=True)
        event = torch.cuda.Event()
        event.record()
        raw.release(event)
    else:
        frames[:nbytes].copy_(torch.from_numpy(raw.payload))
    return frames


def upload_and_decode(raw: RawWav, channel: int):
    """The samples of 0-based `channel` of a RawWav as f32 on the current device: non-blocking upload of the payload bytes, then orcai_pcm_decode."""
    import torch

    if raw.n_frames == 0:
        raw.release()
        return torch.empty(0, dtype=torch.float32, device="cuda")
    return decode_device(_upload(raw), raw.n_frames, raw.channels, channel, raw.format)


def decode_device_planar(frames, n_frames: int, channels: int, sample_format: int):
    """orcai_pcm_decode_planar: uint8 cuda `frames` (the data chunk, padded to a multiple of 16 bytes) -> f32 cuda [channels][n_frames], a view of
    planes roundup(n_frames, 4) floats apart (each starts 16-byte aligned and is contiguous); plane c equals decode_device(..., channel=c, ...)."""
    import torch

    from orcai_amd import _native as N

    if not (frames.is_cuda and frames.dtype == torch.uint8 and frames.dim() == 1 and frames.is_contiguous()):
        raise TypeError("frames must be a contiguous 1-D uint8 CUDA tensor")
    if not 0 <= sample_format < len(BYTES_PER_SAMPLE):
        raise ValueError(f"unknown sample format {sample_format}")
    need = -(-n_frames * channels * BYTES_PER_SAMPLE[sample_format] // 16) * 16
    if frames.numel() < need:
        raise ValueError(f"frames holds {frames.numel()} bytes; {n_frames} frames need {need} (rounded up to 16)")
    stride = -(-n_frames // 4) * 4
    out = torch.empty((channels, stride), dtype=torch.float32, device=frames.device)
    with torch.cuda.device(frames.device):
        N.check(N.lib().orcai_pcm_decode_planar(N.ptr(frames), n_frames, channels, sample_format, N.ptr(out), stride, N.stream_ptr()), "orcai_pcm_decode_planar")
    return out[:, :n_frames]


def upload_and_decode_all(raw: RawWav):
    """Every channel of a RawWav as f32 [channels][n_frames] on the current device from ONE upload of the payload bytes and one orcai_pcm_decode_planar."""
    import torch

    if raw.n_frames == 0:
        raw.release()
        return torch.empty((raw.channels, 0), dtype=torch.float32, device="cuda")
    return decode_device_planar(_upload(raw), raw.n_frames, raw.channels, raw.format)


def write_wav_pcm16(path: str | Path, samples: np.ndarray, rate: int) -> None:
    """samples: int16 [frames] or [channels, frames]."""
    s = np.asarray(samples)
    if s.dtype != np.int16:
        raise TypeError("write_wav_pcm16 wants int16 samples")
    if s.ndim == 1:
        s = s[None, :]
    channels, n = s.shape
    payload = np.ascontiguousarray(s.T).astype("<i2").tobytes()
    header = b"RIFF" + struct.pack("<I", 36 + len(payload)) + b"WAVE"
    header += b"fmt " + struct.pack("<IHHIIHH", 16, WAVE_FORMAT_PCM, channels, rate, rate * channels * 2, channels * 2, 16)
    header += b"data" + struct.pack("<I", len(payload))
    Path(path).write_bytes(header + payload)


class WavPrefetcher:
    """Decodes the next recordings of a table on background threads while the GPU works on the current one.  The reference's table
    mode is strictly serial (predict.py:729-755); on MI355X one hour of audio is ~60 ms of GPU work but several hundred ms of file
    read + PCM16 -> float32 conversion, so without this the host side bounds table-mode throughput.  Order of results and error
    behaviour are unchanged: a decode error surfaces when THAT recording is requested (and is logged per recording by the caller).
    raw=True (what `orcai predict` builds): the workers only read -- read_wav_raw(pin=True), the data chunk into a page-locked buffer of the pool -- and
    get returns RawWavs; the conversion to float32 then runs on the device (upload_and_decode)."""

    def __init__(self, paths, depth: int = 2, workers: int = 2, raw: bool = False):
        from concurrent.futures import ThreadPoolExecutor

        self.raw = bool(raw)  # True: the workers read the data chunk into page-locked buffers (read_wav_raw) and the decode runs on the device
        self.device = None  # raw: the caller's device, so that a worker thread page-locks in that device's context and not in device 0's
        if self.raw:
            import torch

            if torch.cuda.is_available():
                self.device = torch.cuda.current_device()

        self.paths = [str(p) for p in paths]
        self.depth = max(1, int(depth))
        self.pool = ThreadPoolExecutor(max_workers=max(1, int(workers)), thread_name_prefix="orcai-wav")
        self.futures: dict[int, object] = {}
        self.next_to_schedule = 0
        self.index = {}
        for i, p in enumerate(self.paths):
            self.index.setdefault(p, []).append(i)

    def _schedule_up_to(self, i: int) -> None:
        while self.next_to_schedule < len(self.paths) and self.next_to_schedule <= i:
            k = self.next_to_schedule
            self.futures[k] = self.pool.submit(self._read, self.paths[k])
            self.next_to_schedule += 1

    def _read(self, path):
        if not self.raw:
            return read_wav(path)
        if self.device is None:
            return read_wav_raw(path, pin=True)
        import torch

        with torch.cuda.device(self.device):
            return read_wav_raw(path, pin=True)

    def get(self, path):
        """The recording (as read_wav; raw=True: as read_wav_raw) -- from the prefetch queue when it is one of the scheduled paths."""
        slots = self.index.get(str(path))
        if not slots:
            return self._read(path)
        i = slots.pop(0)
        # recordings before i that were scheduled but never asked for (the caller skipped them: output exists, bad row, ...):
        # cancel what has not started and drop the decoded audio of the rest -- an hour of 48 kHz mono is 0.7 GB of float32
        for k in [k for k in self.futures if k < i]:
            self.futures.pop(k).cancel()
        self.next_to_schedule = max(self.next_to_schedule, i)  # never decode a recording the caller has already passed
        self._schedule_up_to(i + self.depth)
        fut = self.futures.pop(i)
        return fut.result()

    def skip(self, path) -> None:
        """The caller will not read this recording: release its slot (and its decoded audio, if any) now."""
        slots = self.index.get(str(path))
        if slots:
            fut = self.futures.pop(slots.pop(0), None)
            if fut is not None:
                fut.cancel()

    def close(self) -> None:
        self.pool.shutdown(wait=False, cancel_futures=True)
        self.futures.clear()


_prefetcher: WavPrefetcher | None = None


def set_prefetcher(p: WavPrefetcher | None) -> None:
    global _prefetcher
    if _prefetcher is not None and p is not _prefetcher:
        _prefetcher.close()
    _prefetcher = p


def read_wav_prefetched(path: str | Path) -> tuple[np.ndarray, int]:
    """read_wav through the active WavPrefetcher, if any."""
    return _prefetcher.get(path) if _prefetcher is not None and not _prefetcher.raw else read_wav(path)


def read_wav_raw_prefetched(path: str | Path) -> RawWav:
    """read_wav_raw(pin=True) through the active raw WavPrefetcher, if any."""
    return _prefetcher.get(path) if _prefetcher is not None and _prefetcher.raw else read_wav_raw(path, pin=True)
