"""The denoised front end on the GPU (spectrogram parameter "denoise"; orcai_make_denoised_spectrogram): every channel of the referenced dB spectrogram
minus its own order statistic over the recording, then the global percentile clip.

The signal: 3 s of seeded noise at 48 kHz, a steady tone at 3750 Hz -- bin 40 of the 512-point transform, bin 20 of the 256-point one -- and one short
chirp.  Three cases: orcai-V1's spectrogram parameters, the same with mel {n_mels: 64}, both with denoise {}; and linear with nfft 256 and quantile 0.25.
Everything is exact: the one call against the staged C calls byte for byte, the staged profile and denoised values against the numpy specification
bit for bit, and the final array against numpy's clip and normalise by value -- the tolerance tests/test_frontend_gpu.py applies to orcai_clip_normalize
against numpy's (the reference's) clip and normalise, which is none: `assert np.array_equal(out, g["out"])`, tests/test_frontend_gpu.py:69."""

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

RATE, TONE_HZ = 48000, 3750.0
V1 = {"sampling_rate": RATE, "nfft": 512, "n_overlap": 256, "freq_range": [0, 16000], "quantiles": [0.01, 0.999]}  # orcai-V1's spectrogram section
CASES = {
    "linear": dict(V1, denoise={}),
    "mel64": dict(V1, mel={"n_mels": 64}, denoise={}),
    "linear-256-q25": dict(V1, nfft=256, n_overlap=128, denoise={"quantile": 0.25}),
}


def signal() -> np.ndarray:
    rng = np.random.default_rng(20260101)
    n = 3 * RATE + 17
    t = np.arange(n) / RATE
    x = 0.01 * rng.standard_normal(n) + 0.5 * np.sin(2 * np.pi * TONE_HZ * t)
    on = (t >= 1.0) & (t < 1.2)  # the chirp: 5 -> 9 kHz in 0.2 s
    x[on] += 0.3 * np.sin(2 * np.pi * (5000.0 * (t[on] - 1.0) + 0.5 * 20000.0 * (t[on] - 1.0) ** 2))
    return x.astype(np.float32)


@pytest.fixture(scope="module")
def fe():
    from orcai_amd.frontend import get_frontend

    return get_frontend()


@pytest.fixture(scope="module")
def pcm():
    return torch.from_numpy(signal()).cuda()


@pytest.fixture(scope="module")
def runs(fe, pcm):
    """Per case, computed once: the one call's (out, stats, profile) and the staged composition's V, m, Y, out on the host."""
    from orcai_amd import _native as N
    from orcai_amd.denoise import denoise_config
    from orcai_amd.frontend import TOP_DB, nearest_rank_index, resolve_route

    res = {}
    lib, s = fe.lib, N.stream_ptr()
    for name, sp in CASES.items():
        got, stats, profile = fe.make_spectrogram(pcm, sp, return_stats=True, return_profile=True)
        n_fft, hop, K, cfg, pc = resolve_route(sp)
        q = denoise_config(sp)["quantile"]
        n = pcm.numel()
        T = 1 + n // hop
        assert tuple(got.shape) == (T, K) and tuple(profile.shape) == (K,) and pc is None
        ws = torch.full_like(fe.workspace, 0xA5)  # orcai_frontend_reset opens the sequence
        out = torch.empty((T, K), dtype=torch.float32, device="cuda")
        m = torch.empty(K, dtype=torch.float32, device="cuda")
        scratch = torch.full((lib.orcai_column_select_scratch_bytes(K),), 0x5A, dtype=torch.uint8, device="cuda")
        r_col = nearest_rank_index(T, q)
        r_lo, r_hi = (nearest_rank_index(T * K, v) for v in sp["quantiles"])
        assert lib.orcai_frontend_reset(N.ptr(ws), s) == 0
        if cfg is None:
            assert lib.orcai_stft_db(N.ptr(pcm), n, n_fft, hop, T, K, N.ptr(out), N.ptr(ws), s) == 0
        else:
            assert lib.orcai_stft_mel_db(N.ptr(pcm), n, n_fft, hop, T, K, *fe._bands(sp, cfg), N.ptr(out), N.ptr(ws), s) == 0
        assert lib.orcai_frontend_finalize(1, TOP_DB, N.ptr(ws), s) == 0
        assert lib.orcai_db_reference(N.ptr(out), T * K, N.ptr(ws), s) == 0
        V = out.cpu().numpy()
        assert lib.orcai_column_select(N.ptr(out), T, K, r_col, N.ptr(m), N.ptr(scratch), s) == 0
        assert lib.orcai_subtract_columns(N.ptr(out), T, K, N.ptr(m), s) == 0
        Y = out.cpu().numpy()
        assert lib.orcai_quantile_select_radix(N.ptr(out), T * K, r_lo, r_hi, N.ptr(ws), s) == 0
        assert lib.orcai_frontend_finalize(0, 0.0, N.ptr(ws), s) == 0
        assert lib.orcai_clip_normalize(N.ptr(out), T * K, N.ptr(ws), s) == 0
        staged_stats = torch.empty(6, dtype=torch.float32, device="cuda")
        assert lib.orcai_frontend_stats_dev(N.ptr(ws), N.ptr(staged_stats), s) == 0
        res[name] = dict(sp=sp, T=T, K=K, q=q, r_col=r_col, got=got.cpu().numpy(), stats=stats.cpu().numpy(), profile=profile.cpu().numpy(), V=V, m=m.cpu().numpy(),
                         Y=Y, out=out.cpu().numpy(), staged_stats=staged_stats.cpu().numpy(), Y_dev=torch.from_numpy(Y).cuda())
    return res


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------ 5. one call = the composition
@pytest.mark.parametrize("name", list(CASES))
def test_one_call_is_the_staged_composition(runs, name):
    r = runs[name]
    assert np.array_equal(bits(r["got"]), bits(r["out"]))
    assert np.array_equal(bits(r["profile"]), bits(r["m"]))
    assert np.array_equal(bits(r["stats"]), bits(r["staged_stats"]))
    assert r["got"].min() == 0.0 and r["got"].max() == 1.0
    assert r["stats"][0] > 0.0  # pmax of the STFT


def test_out_and_no_profile(fe, pcm, runs):
    """out= (the batch path of predict_wavs) and the call without a profile give the same bytes."""
    r = runs["linear"]
    buf = torch.zeros((r["T"] + 8, r["K"]), dtype=torch.float32, device="cuda")
    ret = fe.make_spectrogram(pcm, r["sp"], out=buf[4 : 4 + r["T"]])  # rows of a batch buffer start 16-byte aligned (batch.layout), as every route's out must
    assert ret.data_ptr() == buf[4].data_ptr()
    host = buf.cpu().numpy()
    assert np.array_equal(bits(host[4:-4]), bits(r["got"])) and not host[:4].any() and not host[-4:].any()
    spec, stats = fe.make_spectrogram(pcm, r["sp"], return_stats=True)
    assert np.array_equal(bits(spec.cpu().numpy()), bits(r["got"])) and np.array_equal(bits(stats.cpu().numpy()), bits(r["stats"]))
    with pytest.raises(ValueError, match="return_profile"):
        fe.make_spectrogram(pcm, V1, return_profile=True)


# ------------------------------------------------------------------------------------------------ 6. against numpy
@pytest.mark.parametrize("name", list(CASES))
def test_staged_values_are_the_numpy_specification(runs, name):
    from orcai_amd.denoise import denoise_ref

    r = runs[name]
    V, sp = r["V"], r["sp"]
    assert V.min() >= -80.0 and (V.max() == 0.0 or sp.get("mel") is not None)  # referenced dB: the loudest bin (the tone's, a kept one) is the reference
    Y_ref, m_ref = denoise_ref(V, r["q"])
    assert np.array_equal(bits(r["m"]), bits(m_ref))
    assert np.array_equal(bits(r["Y"]), bits(Y_ref))
    p_lo, p_hi = (np.percentile(r["Y"], 100 * v, method="nearest") for v in sp["quantiles"])
    assert p_lo.dtype == np.float32 and p_lo < p_hi
    assert (bits(r["stats"][2:4]) == bits(np.array([p_lo, p_hi]))).all()  # p_lo / p_hi as values of Y
    clipped = np.clip(r["Y"], p_lo, p_hi)
    want = (clipped - clipped.min()) / (clipped.max() - clipped.min())
    assert want.dtype == np.float32
    assert np.array_equal(r["out"], want)  # no tolerance: what tests/test_frontend_gpu.py:69 applies to orcai_clip_normalize against numpy


# ------------------------------------------------------------------------------------------------ 7. the property the feature exists for
@pytest.mark.parametrize("name", list(CASES))
def test_the_floor_of_the_denoised_channels_is_zero_and_the_profile_finds_the_tone(fe, runs, name):
    from orcai_amd import _native as N
    from orcai_amd import mel

    r = runs[name]
    K = r["K"]
    floor = torch.full((K,), -1.0, dtype=torch.float32, device="cuda")
    scratch = torch.empty(fe.lib.orcai_column_select_scratch_bytes(K), dtype=torch.uint8, device="cuda")
    assert fe.lib.orcai_column_select(N.ptr(r["Y_dev"]), r["T"], K, r["r_col"], N.ptr(floor), N.ptr(scratch), N.stream_ptr()) == 0
    assert (bits(floor.cpu().numpy()) == 0).all()  # exactly +0.0 in every channel
    sp = r["sp"]
    tone_bin = int(round(TONE_HZ * sp["nfft"] / RATE))
    assert tone_bin * RATE / sp["nfft"] == TONE_HZ
    if sp.get("mel") is None:
        assert int(np.argmax(r["profile"])) == tone_bin
    else:  # the band that weighs the tone's bin and its two Hann side lobes (a quarter of the power each) most
        W = mel.dense_from_table(mel.table_for(sp, mel.mel_config(sp)), sp["nfft"]).astype(np.float64)
        assert int(np.argmax(r["profile"])) == int(np.argmax(W[:, tone_bin - 1 : tone_bin + 2] @ np.array([0.25, 1.0, 0.25])))


# ------------------------------------------------------------------------------------------------ 8. nothing changes when off
@pytest.mark.parametrize("route", ["linear", "mel64", "pcen", "pcen-mel64"])
def test_nothing_changes_when_off(fe, pcm, route):
    sp = dict(V1)
    if "mel64" in route:
        sp["mel"] = {"n_mels": 64}
    if "pcen" in route:
        sp["pcen"] = {}
    want, want_stats = fe.make_spectrogram(pcm, sp, return_stats=True)
    got, got_stats = fe.make_spectrogram(pcm, dict(sp, denoise=None), return_stats=True)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32)) and torch.equal(got_stats.view(torch.int32), want_stats.view(torch.int32))
    again = fe.make_spectrogram(pcm, sp)  # after denoised runs of the same front end
    assert torch.equal(again.view(torch.int32), want.view(torch.int32))
    if "pcen" not in route:
        changed = fe.make_spectrogram(pcm, dict(sp, denoise={}))
        assert not torch.equal(changed, want)


# ------------------------------------------------------------------------------------------------ 9. hosted entry
def test_hosted_entry_on_a_wav_file(fe, tmp_path):
    from orcai_amd import wavio
    from orcai_amd.spectrogram import make_spectrogram

    x16 = np.round(signal()[:40000] * 20000.0).astype(np.int16)
    path = tmp_path / "tone.wav"
    wavio.write_wav_pcm16(path, x16, RATE)
    sp = CASES["linear"]
    spec, frequencies, times = make_spectrogram(path, 1, {"spectrogram": sp}, verbosity=0)
    want = fe.make_spectrogram(torch.from_numpy(x16.astype(np.float32) / np.float32(32768.0)).cuda(), sp).cpu().numpy()
    assert spec.dtype == np.float32 and spec.shape == want.shape == (1 + 40000 // 256, 171) == (len(times), 171)
    assert np.array_equal(bits(spec), bits(want))
    assert len(frequencies) == 257
