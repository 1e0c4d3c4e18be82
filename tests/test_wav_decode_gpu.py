"""orcai_pcm_decode and the device route of load_wav on the GPU, bit for bit against the host decode (wavio.read_wav): every sample format x channel count
x channel x run length (one lane owns 16 frames: below, at and above one run, above one block), byte offsets beyond 2^32, the launcher's refusals,
load_wav against read_wav -> channel pick -> .cuda() -> resample_device, reuse of the page-locked pool, opcheck of orcai::decode_pcm."""

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from test_wav_decode import FORMATS, riff, sample_bytes  # noqa: E402

from orcai_amd import _native as N  # noqa: E402
from orcai_amd import wavio  # noqa: E402


def bits(t):
    return t.contiguous().view(torch.int32)


def upload(payload: bytes):
    """The payload on the device, padded to a multiple of 16 bytes with a byte pattern that is not silence in any format."""
    n = len(payload)
    dev = torch.full((-(-n // 16) * 16,), 0xA5, dtype=torch.uint8, device="cuda")
    dev[:n] = torch.frombuffer(bytearray(payload), dtype=torch.uint8).cuda()
    return dev


@pytest.mark.parametrize("fmt", FORMATS)
def test_kernel_matches_read_wav_bit_for_bit(tmp_path, fmt):
    sample_format = FORMATS.index(fmt)
    path = tmp_path / "a.wav"
    for channels in (1, 2, 3, 5):
        for frames in (1, 15, 16, 17, 1023, 4096 + 5):
            payload = sample_bytes(fmt, channels * frames, seed=1000 * channels + frames)
            path.write_bytes(riff(fmt, channels, 8000, payload))
            with np.errstate(over="ignore", under="ignore", invalid="ignore"):
                ref = torch.from_numpy(wavio.read_wav(path)[0]).cuda()
            dev = upload(payload)
            for channel in range(channels):
                out = wavio.decode_device(dev, frames, channels, channel, sample_format)
                assert out.shape == (frames,) and torch.equal(bits(out), bits(ref[channel])), (fmt, channels, frames, channel)


def test_writes_exactly_n_frames():
    """The guarded tail: the floats after the last frame keep what they held."""
    frames, channels = 4096 + 5, 2
    dev = upload(sample_bytes("S24", channels * frames, seed=3))
    out = torch.full((frames + 32,), -7.0, device="cuda")
    N.check(N.lib().orcai_pcm_decode(N.ptr(dev), frames, channels, 1, wavio.FORMAT_S24, N.ptr(out), N.stream_ptr()), "orcai_pcm_decode")
    assert torch.equal(out[:frames], wavio.decode_device(dev, frames, channels, 1, wavio.FORMAT_S24))
    assert bool((out[frames:] == -7.0).all())


def test_offsets_beyond_32_bits():
    """S16, 4 channels, 2^29 + 1024 frames: a 4 GiB + 8 KiB payload, a 2 GiB output; the first frames, the frames around byte offset 2^32 and the last
    frames against the same arithmetic in torch."""
    channels, channel, frames, window = 4, 2, (1 << 29) + 1024, 4096
    if torch.cuda.mem_get_info()[0] < 8 << 30:
        pytest.skip("needs 8 GiB of free device memory")
    nbytes = frames * channels * 2
    payload = torch.randint(-(1 << 31), 1 << 31, (nbytes // 4,), dtype=torch.int32, device="cuda").view(torch.uint8)
    assert payload.numel() == nbytes and nbytes % 16 == 0
    out = wavio.decode_device(payload, frames, channels, channel, wavio.FORMAT_S16)
    samples = payload.view(torch.int16)
    for start in (0, (1 << 32) // (2 * channels) - window + 512, frames - window):  # the second: 512 of its frames lie beyond byte 2^32 (1024 frames do in all)
        ref = samples[start * channels : (start + window) * channels].view(window, channels)[:, channel].to(torch.float32) * 2.0 ** -15
        assert torch.equal(bits(out[start : start + window]), bits(ref)), start
    del out, payload, samples
    torch.cuda.empty_cache()


def test_launcher_refusals():
    dev = upload(sample_bytes("S16", 64, seed=0))
    out = torch.full((64,), -7.0, device="cuda")
    f, o, s = N.ptr(dev), N.ptr(out), N.stream_ptr()
    cases = {
        "null frames": (None, 16, 2, 0, 1, o), "null out": (f, 16, 2, 0, 1, None), "misaligned frames": (f + 4, 16, 2, 0, 1, o),
        "misaligned out": (f, 16, 2, 0, 1, o + 4), "no frames": (f, 0, 2, 0, 1, o), "negative frames": (f, -1, 2, 0, 1, o),
        "no channels": (f, 16, 0, 0, 1, o), "65 channels": (f, 1, 65, 0, 0, o), "channel -1": (f, 16, 2, -1, 1, o), "channel == channels": (f, 16, 2, 2, 1, o),
        "format -1": (f, 16, 2, 0, -1, o), "format 6": (f, 16, 2, 0, 6, o),
    }
    for name, args in cases.items():
        assert N.lib().orcai_pcm_decode(*args, s) == N.E_BADARG, name
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())  # nothing was launched
    with pytest.raises(ValueError):
        wavio.decode_device(dev, 64, 2, 0, wavio.FORMAT_S16)  # 256 bytes needed, 128 given: refused before the launch


class Recorder:
    def __init__(self):
        self.warnings = []

    def warning(self, message, **kwargs):
        self.warnings.append(message)


def old_route(path, sampling_rate: int, channel: int):
    from orcai_amd.resample import resample_device

    wav, rate = wavio.read_wav(path)
    mono = wav[channel - 1] if wav.shape[0] > 1 else wav[0]
    pcm = torch.from_numpy(np.ascontiguousarray(mono)).cuda()
    return resample_device(pcm, rate, sampling_rate) if rate != sampling_rate else pcm


@pytest.mark.parametrize("fmt,channels,rate", [("S16", 1, 48000), ("S24", 2, 22050), ("F32", 3, 44100)])
def test_load_wav_matches_the_host_route(tmp_path, fmt, channels, rate):
    from orcai_amd.spectrogram import load_wav

    frames = 6000 + 7
    rng = np.random.default_rng(channels)
    x = (0.3 * rng.standard_normal(frames * channels)).astype(np.float32)
    payload = {"S16": lambda: (x * 32767).astype("<i2").tobytes(), "F32": lambda: x.tobytes(),
               "S24": lambda: (x * 8388607).astype("<i4").view(np.uint8).reshape(-1, 4)[:, :3].tobytes()}[fmt]()
    path = tmp_path / "a.wav"
    path.write_bytes(riff(fmt, channels, rate, payload))
    for channel in range(0, channels + 1):  # 0 picks the last channel (Python's indexing of channel - 1)
        msgr = Recorder()
        got = load_wav(path, 48000, channel, msgr)
        ref = old_route(path, 48000, channel)
        assert got.is_cuda and got.dtype == torch.float32 and got.shape == ref.shape and torch.equal(bits(got), bits(ref)), (fmt, channel)
        assert msgr.warnings == ([f"Multiple channels found, using channel {channel}"] if channels > 1 else [])
    if channels > 1:
        assert torch.equal(bits(load_wav(path, 48000, 0, Recorder())), bits(old_route(path, 48000, channels)))
        msgr = Recorder()
        with pytest.raises(IndexError):
            load_wav(path, 48000, channels + 1, msgr)
        assert msgr.warnings == [f"Multiple channels found, using channel {channels + 1}"]


def test_pool_reuse_gives_each_file_its_own_samples(tmp_path):
    """Six files of decreasing length and different formats through the raw prefetcher: a stale tail of a longer predecessor in a reused page-locked buffer,
    or a buffer refilled before its upload finished, would show as another file's samples."""
    from orcai_amd.spectrogram import load_wav

    paths = []
    for i, fmt in enumerate(["F64", "S32", "F32", "S24", "S16", "U8"]):
        channels, frames = 1 + i % 3, 300000 - 50000 * i + i
        p = tmp_path / f"r{i}.wav"
        p.write_bytes(riff(fmt, channels, 8000 + i, sample_bytes(fmt, channels * frames, seed=50 + i)))
        paths.append((p, channels))
    wavio.set_prefetcher(wavio.WavPrefetcher([p for p, _ in paths], depth=2, workers=2, raw=True))
    try:
        got = [load_wav(p, 8000 + i, channels, Recorder()) for i, (p, channels) in enumerate(paths)]  # queued back to back: no synchronise in between
    finally:
        wavio.set_prefetcher(None)
    for i, (p, channels) in enumerate(paths):
        with np.errstate(over="ignore", under="ignore", invalid="ignore"):
            ref = torch.from_numpy(wavio.read_wav(p)[0][channels - 1]).cuda()
        assert torch.equal(bits(got[i]), bits(ref)), i


def test_decode_pcm_op():
    from torch.library import opcheck

    import orcai_amd.torch_ops  # noqa: F401

    frames, channels = 1000 + 3, 3
    payload = sample_bytes("S24", channels * frames, seed=9)
    dev = torch.frombuffer(bytearray(payload), dtype=torch.uint8).cuda()  # 9027 bytes: not a multiple of 16, the op pads
    out = torch.ops.orcai.decode_pcm(dev, channels, 1, wavio.FORMAT_S24)
    assert torch.equal(bits(out), bits(wavio.decode_device(upload(payload), frames, channels, 1, wavio.FORMAT_S24)))
    opcheck(torch.ops.orcai.decode_pcm.default, (dev, channels, 1, wavio.FORMAT_S24))
    opcheck(torch.ops.orcai.decode_pcm.default, (upload(sample_bytes("F64", 64, seed=1)), 2, 0, wavio.FORMAT_F64))
    with pytest.raises(ValueError):
        torch.ops.orcai.decode_pcm(dev, channels, 3, wavio.FORMAT_S24)
