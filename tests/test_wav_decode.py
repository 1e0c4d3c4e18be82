"""wavio.read_wav_raw against wavio.read_wav, without a GPU: the container rules (every variation crossed with every sample format), the errors, the
raw prefetcher, and the fake implementation of orcai::decode_pcm.  The RIFF bytes are built here with struct and numpy; the numpy decode of the payload
is the format table of include/orcai_hip.h (orcai_pcm_decode), written out once more."""

import struct

import numpy as np
import pytest

from orcai_amd import wavio

FORMATS = ["U8", "S16", "S24", "S32", "F32", "F64"]
TAG_BITS = {"U8": (1, 8), "S16": (1, 16), "S24": (1, 24), "S32": (1, 32), "F32": (3, 32), "F64": (3, 64)}
VARIATIONS = ["plain", "extensible", "odd_list", "fmt_after_data", "two_data", "size_beyond_eof", "partial_frame"]


def sample_bytes(fmt: str, n: int, seed: int) -> bytes:
    """n samples of format fmt as they lie in a file: random values and the extremes of the format."""
    rng = np.random.default_rng(seed)
    if fmt == "U8":
        v = np.concatenate([[0, 127, 128, 129, 255], rng.integers(0, 256, n)])[:n].astype(np.uint8)
        return v.tobytes()
    if fmt == "S16":
        v = np.concatenate([[-32768, -1, 0, 1, 32767], rng.integers(-32768, 32768, n)])[:n].astype("<i2")
        return v.tobytes()
    if fmt == "S24":
        v = np.concatenate([[-(1 << 23), -1, 0, 1, (1 << 23) - 1], rng.integers(-(1 << 23), 1 << 23, n)])[:n].astype("<i4")
        return v.view(np.uint8).reshape(-1, 4)[:, :3].tobytes()
    if fmt == "S32":  # 0x7fffff80 and 0x01000001 round up / down to even on a tie; 0x7fffffff rounds to 1.0
        v = np.concatenate([[-(1 << 31), -1, 0, 1, (1 << 31) - 1, 0x7FFFFF80, 0x7FFFFF40, 0x01000001, 0x01000003, -0x01000001], rng.integers(-(1 << 31), 1 << 31, n)])[:n]
        return v.astype("<i4").tobytes()
    if fmt == "F32":
        bits = np.concatenate([[0x00000000, 0x80000000, 0x7FC00001, 0xFFC12345, 0x7F800001, 0x7F800000, 0x00000001, 0x3F800000],
                               rng.integers(0, 1 << 32, n)])[:n].astype("<u4")
        return bits.tobytes()
    f32_max = float(np.finfo(np.float32).max)
    v = np.concatenate([[0.0, -0.0, f32_max, f32_max * (1 + 2.0 ** -25), f32_max * (1 + 2.0 ** -24), -1e39, 1e300, 2.0 ** -149, 2.0 ** -150, 1.5 * 2.0 ** -150,
                         -3.3 * 2.0 ** -140, 2.0 ** -126 * (1 - 2.0 ** -25), 1e-320, 1 + 2.0 ** -24, 1 + 3 * 2.0 ** -24, np.inf, -np.inf],
                        rng.standard_normal(n) * np.exp2(rng.uniform(-160, 10, n))])[:n].astype("<f8")
    return v.tobytes()


def riff(fmt: str, channels: int, rate: int, payload: bytes, variation: str = "plain", tag_bits=None) -> bytes:
    tag, bits = tag_bits or TAG_BITS[fmt]
    block = channels * (bits // 8)
    if variation == "extensible":
        sub = struct.pack("<H", tag) + b"\x00\x00\x00\x00\x10\x00\x80\x00\x00\xaa\x00\x38\x9b\x71"
        fmt_body = struct.pack("<HHIIHH", 0xFFFE, channels, rate, rate * block, block, bits) + struct.pack("<HHI", 22, bits, 0) + sub
    else:
        fmt_body = struct.pack("<HHIIHH", tag, channels, rate, rate * block, block, bits)

    def chunk(cid, body, size=None):
        return cid + struct.pack("<I", len(body) if size is None else size) + body + (b"\x00" if len(body) & 1 else b"")

    f, d = chunk(b"fmt ", fmt_body), chunk(b"data", payload)
    if variation == "odd_list":
        chunks = f + chunk(b"LIST", b"INFOabc") + d  # 7 bytes: one pad byte follows
    elif variation == "fmt_after_data":
        chunks = d + f
    elif variation == "two_data":
        chunks = chunk(b"data", payload[::-1][: len(payload) // 2 * 2 + 1]) + f + d  # an odd-sized decoy first: the last data chunk wins
    elif variation == "size_beyond_eof":
        chunks = f + chunk(b"data", payload, size=len(payload) + 1000)[: 8 + len(payload)]
    elif variation == "partial_frame":
        chunks = f + chunk(b"data", payload + payload[: block - 1])
    else:
        chunks = f + d
    return b"RIFF" + struct.pack("<I", 4 + len(chunks)) + b"WAVE" + chunks


def decode_numpy(payload: np.ndarray, sample_format: int, channels: int) -> np.ndarray:
    """The format table of orcai_pcm_decode on the payload bytes: f32 [channels, frames]."""
    if sample_format == wavio.FORMAT_U8:
        x = (payload.astype(np.int32) - 128).astype(np.float32) * np.float32(2.0 ** -7)
    elif sample_format == wavio.FORMAT_S16:
        x = payload.view("<i2").astype(np.float32) * np.float32(2.0 ** -15)
    elif sample_format == wavio.FORMAT_S24:
        b = payload.reshape(-1, 3).astype(np.uint32)
        v = ((b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)) << 8).astype(np.uint32).view(np.int32) >> 8  # sign-extend the 24-bit value
        x = v.astype(np.float32) * np.float32(2.0 ** -23)
    elif sample_format == wavio.FORMAT_S32:
        x = payload.view("<i4").astype(np.float32) * np.float32(2.0 ** -31)  # int32 -> f32 rounds once (nearest even); the scale is exact
    elif sample_format == wavio.FORMAT_F32:
        x = payload.view("<f4")
    else:
        with np.errstate(over="ignore", under="ignore"):
            x = payload.view("<f8").astype(np.float32)
    return np.ascontiguousarray(x.reshape(-1, channels).T)


def same_bits(a: np.ndarray, b: np.ndarray) -> bool:
    return a.dtype == b.dtype == np.float32 and a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("variation", VARIATIONS)
@pytest.mark.parametrize("fmt", FORMATS)
def test_raw_read_matches_read_wav(tmp_path, fmt, variation):
    channels, frames, rate = 3, 37, 22050 + FORMATS.index(fmt)
    path = tmp_path / "a.wav"
    path.write_bytes(riff(fmt, channels, rate, sample_bytes(fmt, channels * frames, seed=FORMATS.index(fmt)), variation))
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        ref, ref_rate = wavio.read_wav(path)
    raw = wavio.read_wav_raw(path)
    assert isinstance(raw.payload, np.ndarray) and raw.payload.dtype == np.uint8
    assert (raw.channels, raw.rate, raw.n_frames) == (ref.shape[0], ref_rate, ref.shape[1]) == (channels, rate, frames)
    assert raw.format == FORMATS.index(fmt) and raw.bits == TAG_BITS[fmt][1]
    assert raw.payload.size == frames * channels * wavio.BYTES_PER_SAMPLE[raw.format]
    assert same_bits(decode_numpy(raw.payload, raw.format, raw.channels), ref)


def test_raw_read_refuses_what_read_wav_refuses(tmp_path):
    cases = {
        "not_riff": (b"RIFX" + riff("S16", 1, 8000, b"\x00" * 8)[4:], "not a RIFF/WAVE file"),
        "short": (b"RIFF", "not a RIFF/WAVE file"),
        "no_fmt": (b"RIFF" + struct.pack("<I", 20) + b"WAVE" + b"data" + struct.pack("<I", 8) + b"\x00" * 8, "missing fmt or data chunk"),
        "pcm12": (riff("S16", 1, 8000, b"\x00" * 8, tag_bits=(1, 12)), "unsupported PCM width 12"),
        "float16": (riff("S16", 1, 8000, b"\x00" * 8, tag_bits=(3, 16)), "unsupported float width 16"),
        "tag": (riff("S16", 1, 8000, b"\x00" * 8, tag_bits=(85, 16)), "unsupported WAVE format tag 85"),
    }
    for name, (data, text) in cases.items():
        path = tmp_path / f"{name}.wav"
        path.write_bytes(data)
        with pytest.raises(ValueError) as a:
            wavio.read_wav(path)
        with pytest.raises(ValueError) as b:
            wavio.read_wav_raw(path)
        assert text in str(a.value) and str(a.value) == str(b.value), name


def test_raw_prefetcher_order_duplicates_and_unknown_paths(tmp_path):
    rng = np.random.default_rng(0)
    paths = []
    for i in range(4):
        p = tmp_path / f"r{i}.wav"
        wavio.write_wav_pcm16(p, (rng.standard_normal((1 + i % 2, 1000 - 100 * i)) * 3000).astype(np.int16), 22050 + i)
        paths.append(p)
    missing = tmp_path / "missing.wav"
    order = [paths[0], paths[1], missing, paths[2], paths[1], paths[3]]
    wavio.set_prefetcher(wavio.WavPrefetcher(order, depth=2, workers=2, raw=True))
    try:
        for p in order:
            if p == missing:
                with pytest.raises(FileNotFoundError):
                    wavio.read_wav_raw_prefetched(p)
                continue
            raw = wavio.read_wav_raw_prefetched(p)
            assert isinstance(raw, wavio.RawWav)
            ref, rate = wavio.read_wav(p)
            payload = raw.payload if isinstance(raw.payload, np.ndarray) else raw.payload.numpy()
            assert raw.rate == rate and same_bits(decode_numpy(payload, raw.format, raw.channels), ref)
            raw.release()
            assert same_bits(wavio.read_wav_prefetched(p)[0], ref)  # the host route does not draw from a raw queue
        other = tmp_path / "other.wav"
        wavio.write_wav_pcm16(other, np.zeros(10, dtype=np.int16), 8000)
        assert wavio.read_wav_raw_prefetched(other).rate == 8000  # not in the schedule: read directly
        wavio.set_prefetcher(wavio.WavPrefetcher(order, depth=2, workers=2))  # raw=False: arrays, as before
        a, rate = wavio.read_wav_prefetched(paths[0])
        assert isinstance(a, np.ndarray) and rate == 22050
        assert isinstance(wavio.read_wav_raw_prefetched(paths[1]), wavio.RawWav)  # and the raw route does not draw from a host queue
    finally:
        wavio.set_prefetcher(None)
    assert wavio.read_wav_raw_prefetched(paths[0]).rate == 22050  # no prefetcher: plain read


def test_decode_pcm_fake_shape():
    torch = pytest.importorskip("torch")
    import orcai_amd.torch_ops  # noqa: F401  (registers the ops)

    for sample_format, channels, nbytes in ((0, 1, 17), (1, 2, 4000), (2, 3, 100), (3, 5, 64), (4, 4, 160), (5, 2, 1000)):
        out = torch.ops.orcai.decode_pcm(torch.empty(nbytes, dtype=torch.uint8, device="meta"), channels, 0, sample_format)
        assert out.dtype == torch.float32 and out.device.type == "meta"
        assert tuple(out.shape) == (nbytes // (channels * wavio.BYTES_PER_SAMPLE[sample_format]),)
    with pytest.raises((RuntimeError, ValueError), match="cuda"):
        torch.ops.orcai.decode_pcm(torch.zeros(32, dtype=torch.uint8), 1, 0, 1)  # no CPU implementation of the decode
