"""The front end with a time-varying noise floor on the GPU (spectrogram parameter ``denoise`` with ``segment``; orcai_make_segment_denoised_spectrogram):
every (segment, channel) of the referenced dB spectrogram gets its own order statistic, and each frame loses the floor interpolated between the segment
centres before the global percentile clip.

The signal: 4 s of seeded noise at 48 kHz with a steady tone at 3750 Hz -- bin 40 of the 512-point transform, bin 20 of the 256-point one -- that
switches on at 2 s, over a faint steady line at 7500 Hz.  Three cases with half-second segments: orcai-V1's parameters, the same with mel {n_mels: 64}, and linear with nfft 256 and quantile
0.25.  Everything is exact: the one call against the staged C calls byte for byte, the staged profile and denoised values against the numpy
specification (denoise.segment_denoise_ref on the device's V) bit for bit, the final array against numpy's clip and normalise with no tolerance (what
tests/test_denoise_gpu.py applies to the global floor)."""

import json
from pathlib import Path

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
RATE, TONE_HZ, HUM_HZ, SECONDS, TONE_ON = 48000, 3750.0, 7500.0, 4, 2.0
V1 = {"sampling_rate": RATE, "nfft": 512, "n_overlap": 256, "freq_range": [0, 16000], "quantiles": [0.01, 0.999]}  # orcai-V1's spectrogram section
CASES = {
    "linear": dict(V1, denoise={"segment": 0.5}),
    "mel64": dict(V1, mel={"n_mels": 64}, denoise={"quantile": 0.5, "segment": 0.5}),
    "linear-256-q25": dict(V1, nfft=256, n_overlap=128, denoise={"quantile": 0.25, "segment": 0.5}),
}


def signal() -> np.ndarray:
    rng = np.random.default_rng(20261021)
    n = SECONDS * RATE + 17
    t = np.arange(n) / RATE
    x = 0.01 * rng.standard_normal(n) + 0.02 * np.sin(2 * np.pi * HUM_HZ * t)  # a faint steady line: the loudest channel while the tone is off
    x[t >= TONE_ON] += 0.5 * np.sin(2 * np.pi * TONE_HZ * t[t >= TONE_ON])
    return x.astype(np.float32)


@pytest.fixture(scope="module")
def fe():
    from orcai_amd.frontend import get_frontend

    return get_frontend()


@pytest.fixture(scope="module")
def pcm():
    return torch.from_numpy(signal()).cuda()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def runs(fe, pcm):
    """Per case, computed once: the one call's (out, stats, profile) and the staged composition's V, m, Y, out on the host."""
    from orcai_amd import _native as N
    from orcai_amd.denoise import denoise_config, segment_count, segment_rows
    from orcai_amd.frontend import TOP_DB, nearest_rank_index, resolve_route

    res = {}
    lib, s = fe.lib, N.stream_ptr()
    for name, sp in CASES.items():
        got, stats, profile = fe.make_spectrogram(pcm, sp, return_stats=True, return_profile=True)
        n_fft, hop, K, cfg, pc = resolve_route(sp)
        dn = denoise_config(sp)
        n = pcm.numel()
        T = 1 + n // hop
        W = segment_rows(dn["segment"], RATE, hop)
        S = segment_count(T, W)
        assert W == {256: 94, 128: 188}[hop] and S == T // W and S >= 7
        assert tuple(got.shape) == (T, K) and tuple(profile.shape) == (S, K) and pc is None
        ws = torch.full_like(fe.workspace, 0xA5)  # orcai_frontend_reset opens the sequence
        out = torch.empty((T, K), dtype=torch.float32, device="cuda")
        m = torch.empty((S, K), dtype=torch.float32, device="cuda")
        scratch = torch.full((lib.orcai_segment_column_select_scratch_bytes(T, K, W),), 0x5A, dtype=torch.uint8, device="cuda")
        r_seg, r_last = nearest_rank_index(W, dn["quantile"]), nearest_rank_index(T - (S - 1) * W, dn["quantile"])
        r_lo, r_hi = (nearest_rank_index(T * K, v) for v in sp["quantiles"])
        assert lib.orcai_frontend_reset(N.ptr(ws), s) == 0
        if cfg is None:
            assert lib.orcai_stft_db(N.ptr(pcm), n, n_fft, hop, T, K, N.ptr(out), N.ptr(ws), s) == 0
        else:
            assert lib.orcai_stft_mel_db(N.ptr(pcm), n, n_fft, hop, T, K, *fe._bands(sp, cfg), N.ptr(out), N.ptr(ws), s) == 0
        assert lib.orcai_frontend_finalize(1, TOP_DB, N.ptr(ws), s) == 0
        assert lib.orcai_db_reference(N.ptr(out), T * K, N.ptr(ws), s) == 0
        V = out.cpu().numpy()
        assert lib.orcai_segment_column_select(N.ptr(out), T, K, W, r_seg, r_last, N.ptr(m), N.ptr(scratch), s) == 0
        assert lib.orcai_subtract_segment_floor(N.ptr(out), T, K, W, N.ptr(m), s) == 0
        Y = out.cpu().numpy()
        assert lib.orcai_quantile_select_radix(N.ptr(out), T * K, r_lo, r_hi, N.ptr(ws), s) == 0
        assert lib.orcai_frontend_finalize(0, 0.0, N.ptr(ws), s) == 0
        assert lib.orcai_clip_normalize(N.ptr(out), T * K, N.ptr(ws), s) == 0
        staged_stats = torch.empty(6, dtype=torch.float32, device="cuda")
        assert lib.orcai_frontend_stats_dev(N.ptr(ws), N.ptr(staged_stats), s) == 0
        res[name] = dict(sp=sp, T=T, K=K, W=W, S=S, q=dn["quantile"], got=got.cpu().numpy(), stats=stats.cpu().numpy(), profile=profile.cpu().numpy(), V=V,
                         m=m.cpu().numpy(), Y=Y, out=out.cpu().numpy(), staged_stats=staged_stats.cpu().numpy())
    return res


# ------------------------------------------------------------------------------------------------ one call = the composition
@pytest.mark.parametrize("name", list(CASES))
def test_one_call_is_the_staged_composition(runs, name):
    r = runs[name]
    assert np.array_equal(bits(r["got"]), bits(r["out"]))
    assert np.array_equal(bits(r["profile"]), bits(r["m"]))
    assert np.array_equal(bits(r["stats"]), bits(r["staged_stats"]))
    assert r["got"].min() == 0.0 and r["got"].max() == 1.0
    assert r["stats"][0] > 0.0  # pmax of the STFT


def test_out_and_no_profile(fe, pcm, runs):
    r = runs["linear"]
    buf = torch.zeros((r["T"] + 8, r["K"]), dtype=torch.float32, device="cuda")
    ret = fe.make_spectrogram(pcm, r["sp"], out=buf[4 : 4 + r["T"]])
    assert ret.data_ptr() == buf[4].data_ptr()
    host = buf.cpu().numpy()
    assert np.array_equal(bits(host[4:-4]), bits(r["got"])) and not host[:4].any() and not host[-4:].any()
    spec, stats = fe.make_spectrogram(pcm, r["sp"], return_stats=True)
    assert np.array_equal(bits(spec.cpu().numpy()), bits(r["got"])) and np.array_equal(bits(stats.cpu().numpy()), bits(r["stats"]))
    op = torch.ops.orcai.segment_denoised_spectrogram(pcm, RATE, 512, 256, 16000.0, 0, 0.0, 0.0, False, True, 0.5, 0.5, 0.01, 0.999)
    assert np.array_equal(bits(op.cpu().numpy()), bits(r["got"]))


# ------------------------------------------------------------------------------------------------ against numpy
@pytest.mark.parametrize("name", list(CASES))
def test_staged_values_are_the_numpy_specification(runs, name):
    from orcai_amd.denoise import segment_denoise_ref

    r = runs[name]
    V, sp = r["V"], r["sp"]
    assert V.min() >= -80.0 and not (bits(V) == 0x80000000).any()  # referenced dB without -0.0: np.sort's by-value order is the kernels' key order
    Y_ref, m_ref = segment_denoise_ref(V, r["q"], r["W"])
    assert m_ref.shape == (r["S"], r["K"])
    assert np.array_equal(bits(r["m"]), bits(m_ref))
    assert np.array_equal(bits(r["Y"]), bits(Y_ref))
    p_lo, p_hi = (np.percentile(r["Y"], 100 * v, method="nearest") for v in sp["quantiles"])
    assert p_lo.dtype == np.float32 and p_lo < p_hi
    assert (bits(r["stats"][2:4]) == bits(np.array([p_lo, p_hi]))).all()  # p_lo / p_hi as values of Y
    clipped = np.clip(r["Y"], p_lo, p_hi)
    want = (clipped - clipped.min()) / (clipped.max() - clipped.min())
    assert want.dtype == np.float32
    assert np.array_equal(r["out"], want)  # no tolerance


# ------------------------------------------------------------------------------------------------ the property the feature exists for
@pytest.mark.parametrize("name", list(CASES))
def test_the_profile_follows_the_tone_in_time_and_the_global_floor_cannot(fe, pcm, runs, name):
    from orcai_amd import mel

    r = runs[name]
    sp, S, W = r["sp"], r["S"], r["W"]
    hop = sp["n_overlap"]
    tone_bin = int(round(TONE_HZ * sp["nfft"] / RATE))
    if sp.get("mel") is not None:
        Wm = mel.dense_from_table(mel.table_for(sp, mel.mel_config(sp)), sp["nfft"]).astype(np.float64)
        tone_bin = int(np.argmax(Wm[:, tone_bin - 1 : tone_bin + 2] @ np.array([0.25, 1.0, 0.25])))
    on_frame = TONE_ON * RATE / hop
    later = [s for s in range(S) if s * W >= on_frame + 1]  # frame t is centred on sample t * hop and nfft = 2 hop long: wholly behind the onset
    earlier = [s for s in range(S) if (s + 1) * W <= on_frame - 1]
    assert len(later) >= 3 and len(earlier) >= 3
    peak = np.argmax(r["profile"], axis=1)
    assert all(peak[s] == tone_bin for s in later) and all(peak[s] != tone_bin for s in earlier)
    assert min(r["profile"][s, tone_bin] for s in later) > max(r["profile"][s, tone_bin] for s in earlier) + 30.0  # dB
    glob = dict(sp, denoise={"quantile": r["q"]})
    _, one = fe.make_spectrogram(pcm, glob, return_profile=True)
    assert tuple(one.shape) == (r["K"],)  # one floor per channel for the whole recording: no time axis to show the switch on


# ------------------------------------------------------------------------------------------------ the edges of the parameter
@pytest.mark.parametrize("name", list(CASES))
def test_a_segment_longer_than_the_recording_is_the_global_floor(fe, pcm, runs, name):
    r = runs[name]
    sp = r["sp"]
    glob = dict(sp, denoise={"quantile": r["q"]})
    want, want_stats, want_profile = fe.make_spectrogram(pcm, glob, return_stats=True, return_profile=True)
    for seconds in (60.0, 2.5):  # W > T, and T // W == 1 with a remainder
        got, stats, profile = fe.make_spectrogram(pcm, dict(sp, denoise={"quantile": r["q"], "segment": seconds}), return_stats=True, return_profile=True)
        assert tuple(profile.shape) == (1, r["K"])
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)) and torch.equal(stats.view(torch.int32), want_stats.view(torch.int32))
        assert torch.equal(profile[0].view(torch.int32), want_profile.view(torch.int32))
    assert not np.array_equal(want.cpu().numpy(), r["got"])


def test_segment_null_is_absent(fe, pcm):
    for sp in (dict(V1, denoise={}), dict(V1, mel={"n_mels": 64}, denoise={"quantile": 0.25})):
        want, want_stats, want_profile = fe.make_spectrogram(pcm, sp, return_stats=True, return_profile=True)
        got, stats, profile = fe.make_spectrogram(pcm, dict(sp, denoise=dict(sp["denoise"], segment=None)), return_stats=True, return_profile=True)
        assert tuple(profile.shape) == tuple(want_profile.shape) == (want.shape[1],)
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)) and torch.equal(stats.view(torch.int32), want_stats.view(torch.int32))
        assert torch.equal(profile.view(torch.int32), want_profile.view(torch.int32))


def test_gradient_entries_refuse_with_real_tensors(fe, pcm, runs):
    r = runs["linear"]
    spec, stats, profile = fe.make_spectrogram(pcm, r["sp"], return_stats=True, return_profile=True)
    with pytest.raises(NotImplementedError, match=r"denoise\.segment"):
        fe.denoised_spectrogram_backward(pcm, torch.ones_like(spec), stats, profile[0].contiguous(), r["sp"])


# ------------------------------------------------------------------------------------------------ hosted entry and predict
def test_hosted_entry_on_a_wav_file(fe, tmp_path):
    from orcai_amd import wavio
    from orcai_amd.spectrogram import make_spectrogram

    x16 = np.round(signal()[RATE : RATE + 120000] * 20000.0).astype(np.int16)  # 2.5 s around the onset
    path = tmp_path / "tone.wav"
    wavio.write_wav_pcm16(path, x16, RATE)
    sp = CASES["linear"]
    spec, frequencies, times = make_spectrogram(path, 1, {"spectrogram": sp}, verbosity=0)
    want = fe.make_spectrogram(torch.from_numpy(x16.astype(np.float32) / np.float32(32768.0)).cuda(), sp).cpu().numpy()
    assert spec.dtype == np.float32 and spec.shape == want.shape == (1 + 120000 // 256, 171) == (len(times), 171)
    assert np.array_equal(bits(spec), bits(want))
    plain, _, _ = make_spectrogram(path, 1, {"spectrogram": dict(sp, denoise={})}, verbosity=0)
    assert not np.array_equal(spec, plain)


def test_predict_runs_with_the_key_set(tmp_path):
    """`orcai init-weights` on a copy of orcai-V1's model directory whose spectrogram section carries denoise {segment}, then `predict` on a short wav."""
    import pandas as pd
    from click.testing import CliRunner

    from orcai_amd.cli import cli
    from orcai_amd.predict import predict
    from orcai_amd.synthetic import synth_recording
    from orcai_amd.wavio import write_wav_pcm16

    v1 = ROOT / "orcai_amd" / "models" / "orcai-V1"
    param, shape = json.loads((v1 / "orcai_parameter.json").read_text()), json.loads((v1 / "model_shape.json").read_text())
    param["spectrogram"]["denoise"] = {"quantile": 0.5, "segment": 2.0}
    mdir = tmp_path / "model"
    mdir.mkdir()
    (mdir / "orcai_parameter.json").write_text(json.dumps(param))
    (mdir / "model_shape.json").write_text(json.dumps(shape))
    res = CliRunner().invoke(cli, ["init-weights", str(mdir), "--seed", "3"], catch_exceptions=False)
    assert res.exit_code == 0, res.output
    wav = tmp_path / "rec.wav"
    write_wav_pcm16(wav, synth_recording(9.0, 48000, seed=5), 48000)
    out = tmp_path / "rec_predicted.txt"
    predict(wav, model_dir=mdir, output_path=out, save_probabilities=True, verbosity=0)
    probs = pd.read_csv(tmp_path / "rec_predicted_probabilities.csv.gz", index_col="time")
    assert list(probs.columns) == param["calls"] and len(probs) > 0 and np.isfinite(probs.to_numpy()).all()
    assert list(pd.read_csv(out, sep="\t").columns) == ["start", "stop", "label"]
