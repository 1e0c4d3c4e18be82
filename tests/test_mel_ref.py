"""The host half of the mel front end (orcai_amd/mel.py), the float64 reference and bound of tests/mel_ref.py, and the host routing of FrontEnd on the
``mel`` key.  No GPU."""

import numpy as np
import pytest

import mel_ref as MR
import stft_ref as R
from orcai_amd import mel

SP = {"sampling_rate": 48000, "nfft": 512, "n_overlap": 256, "freq_range": [0, 16000], "quantiles": [0.01, 0.999]}


# ------------------------------------------------------------------------------------------------ scales
def test_slaney_scale_identities():
    assert mel.hz_to_mel(1000.0) == 15.0
    f = np.array([0.0, 100.0, 200.0 / 3.0, 999.0])
    np.testing.assert_allclose(mel.hz_to_mel(f), f * 3.0 / 200.0, rtol=1e-15)  # linear below 1 kHz
    np.testing.assert_allclose(mel.hz_to_mel(6400.0), 15.0 + 27.0, rtol=1e-14)  # 27 logarithmic steps from 1 kHz to 6.4 kHz
    f = np.array([0.0, 50.0, 999.9, 1000.0, 1000.1, 4000.0, 24000.0])
    np.testing.assert_allclose(mel.mel_to_hz(mel.hz_to_mel(f)), f, rtol=1e-13, atol=1e-12)


def test_htk_scale():
    f = np.array([0.0, 700.0, 1000.0, 24000.0])
    np.testing.assert_allclose(mel.hz_to_mel(f, htk=True), 2595.0 * np.log10(1.0 + f / 700.0), rtol=1e-15)
    assert abs(mel.hz_to_mel(700.0, htk=True) - 2595.0 * np.log10(2.0)) < 1e-12
    np.testing.assert_allclose(mel.mel_to_hz(mel.hz_to_mel(f, htk=True), htk=True), f, rtol=1e-13, atol=1e-10)


def test_mel_frequencies_are_equally_spaced_in_mel():
    for htk in (False, True):
        f = mel.mel_frequencies(42, 300.0, 20000.0, htk)
        assert f[0] == pytest.approx(300.0) and f[-1] == pytest.approx(20000.0)
        d = np.diff(mel.hz_to_mel(f, htk))
        np.testing.assert_allclose(d, d[0], rtol=1e-10)


# ------------------------------------------------------------------------------------------------ filterbank
@pytest.mark.parametrize("htk", [False, True])
@pytest.mark.parametrize("nfft,n_mels,fmin,fmax", [(512, 40, 0.0, 16000.0), (1024, 64, 300.0, 20000.0), (4096, 256, 0.0, 24000.0)])
def test_unnormalised_triangles_partition_unity(nfft, n_mels, fmin, fmax, htk):
    W = mel.mel_filterbank(48000, nfft, n_mels, fmin, fmax, htk, None)
    assert W.shape == (n_mels, 1 + nfft // 2) and W.dtype == np.float64 and W.min() >= 0.0 and W.max() <= 1.0
    pts = mel.mel_frequencies(n_mels + 2, fmin, fmax, htk)
    f = np.fft.rfftfreq(nfft, 1.0 / 48000)
    inside = (f >= pts[1]) & (f <= pts[-2])  # between the first and the last centre
    assert inside.sum() > n_mels
    np.testing.assert_allclose(W[:, inside].sum(axis=0), 1.0, rtol=0, atol=1e-12)
    outside = (f <= pts[0]) | (f >= pts[-1])
    assert not W[:, outside].any()


@pytest.mark.parametrize("htk", [False, True])
def test_slaney_norm_is_two_over_the_band_width(htk):
    Wn = mel.mel_filterbank(48000, 512, 40, 0.0, 16000.0, htk, "slaney")
    Wu = mel.mel_filterbank(48000, 512, 40, 0.0, 16000.0, htk, None)
    pts = mel.mel_frequencies(42, 0.0, 16000.0, htk)
    np.testing.assert_allclose(Wn, Wu * (2.0 / (pts[2:] - pts[:-2]))[:, None], rtol=1e-15)


@pytest.mark.parametrize("case", sorted({c[:1] + c[3:] for c in MR.cases()}))
def test_band_table_reconstructs_the_dense_matrix(case):
    nfft, n_mels, fmin, fmax, htk, norm = case
    t = mel.band_table(MR.SR, nfft, n_mels, fmin, fmax, htk, norm)
    W32 = mel.mel_filterbank(MR.SR, nfft, n_mels, fmin, fmax, htk, norm).astype(np.float32)
    assert np.array_equal(mel.dense_from_table(t, nfft), W32)
    assert t["weights"].dtype == np.float32 and all(t[k].dtype == np.int32 for k in ("lo", "hi", "off"))
    assert t["weights"].size == int((t["hi"] - t["lo"]).sum()) <= 2 * (1 + nfft // 2)
    assert (t["weights"] != 0).all(), "a band's range holds only bins with a non-zero weight"
    assert np.array_equal(t["centres"], mel.mel_frequencies(n_mels + 2, fmin, fmax, htk)[1:-1])
    # what the GPU test relies on: no band is empty
    assert ((t["hi"] - t["lo"]) >= 1).all(), (case, np.flatnonzero(t["hi"] == t["lo"]))
    sp = dict(SP, nfft=nfft, mel={"n_mels": n_mels, "fmin": fmin, "fmax": fmax, "htk": htk, "norm": norm})
    assert mel.mel_config(sp) == {"n_mels": n_mels, "fmin": fmin, "fmax": fmax, "htk": htk, "norm": norm}


def test_gpu_cases_cover_what_the_issue_lists():
    cs = MR.cases()
    assert {c[3] for c in cs} >= {8, 40, 128, 256} and any(c[0] == 4096 and c[3] == 256 for c in cs)
    assert {c[0] for c in cs} == {128, 512, 1024, 4096}
    assert {c[6] for c in cs} == {False, True} and {c[7] for c in cs} == {"slaney", None}
    routes = {(hop, n): R.stft_route(n, 512, hop, 171)["labels"] for N, hop, n, _ in MR.SHAPES if N == 512}
    assert {"fast171", "mixed_head", "mixed_tail"} <= routes[(256, 10000)] and R.num_frames(10000, 512, 256) == 40
    assert "mixed_only" in routes[(256, 4100)] and "odd_hop" in routes[(255, 3000)]


# ------------------------------------------------------------------------------------------------ validation
def _sp(**m):
    return dict(SP, mel=m)


@pytest.mark.parametrize("bad,key", [
    ({"fmin": 0}, "n_mels"), ({"n_mels": 7}, "n_mels"), ({"n_mels": 257}, "n_mels"), ({"n_mels": 40.0}, "n_mels"), ({"n_mels": True}, "n_mels"),
    ({"n_mels": "40"}, "n_mels"), ({"n_mels": 40, "fmin": -1.0}, "fmin"), ({"n_mels": 40, "fmin": "0"}, "fmin"), ({"n_mels": 40, "fmax": 24000.5}, "fmax"),
    ({"n_mels": 40, "fmax": None}, "fmax"), ({"n_mels": 40, "fmin": 8000.0, "fmax": 8000.0}, "fmin"), ({"n_mels": 40, "fmin": float("nan")}, "fmin"),
    ({"n_mels": 40, "htk": 1}, "htk"), ({"n_mels": 40, "norm": "l1"}, "norm"), ({"n_mels": 40, "norm": 1}, "norm"), ({"n_mels": 40, "nmels": 3}, "nmels"),
    ({"n_mels": 40, "top_db": 80}, "top_db"),
])
def test_validation_names_the_key(bad, key):
    with pytest.raises(ValueError, match=key):
        mel.mel_config(_sp(**bad))


def test_validation_of_the_whole_value_and_the_empty_band():
    with pytest.raises(ValueError, match="mel"):
        mel.mel_config(dict(SP, mel=64))
    with pytest.raises(ValueError, match="mel"):
        mel.mel_config(dict(SP, mel=[64]))
    with pytest.raises(ValueError) as e:
        mel.mel_config(_sp(n_mels=128))  # 128 bands from 0 Hz over 171 bins of 93.75 Hz: the low bands fall between bins
    assert "n_mels" in str(e.value) and "nfft" in str(e.value)
    for nfft in (500, 64, 8192, 384):
        with pytest.raises(NotImplementedError) as e:
            mel.mel_config(dict(SP, nfft=nfft, mel={"n_mels": 8}))
        assert "nfft" in str(e.value) and "mel" in str(e.value)
    assert mel.mel_config(SP) is None and mel.mel_config(dict(SP, mel=None)) is None
    assert mel.mel_config(_sp(n_mels=40)) == {"n_mels": 40, "fmin": 0.0, "fmax": 16000.0, "htk": False, "norm": "slaney"}  # defaults: freq_range, Slaney


# ------------------------------------------------------------------------------------------------ the bound against an f32 emulation
def emulate_f32(x, n_fft, hop, table):
    """The kernels' arithmetic on the CPU in f32: f32 window product, complex64 FFT (pocketfft keeps single precision), |X|^2 by two f32 roundings, the
    band sum one f32 multiply-add at a time in ascending bins, 10 log10 in f32."""
    n, half = x.size, n_fft // 2
    T = R.num_frames(n, n_fft, hop)
    seg = np.zeros((T - 1) * hop + n_fft, dtype=np.float32)
    seg[half : half + n] = x[: seg.size - half]
    w = R.hann(n_fft).astype(np.float32)
    fr = np.lib.stride_tricks.sliding_window_view(seg, n_fft)[::hop] * w[None, :]
    X = np.fft.rfft(fr.astype(np.float32), axis=1).astype(np.complex64)
    P = (X.real * X.real + X.imag * X.imag).astype(np.float32)
    M = np.zeros((T, table["lo"].size), dtype=np.float32)
    for m in range(table["lo"].size):
        acc = np.zeros(T, dtype=np.float32)
        for j, k in enumerate(range(table["lo"][m], table["hi"][m])):
            acc = (acc + table["weights"][table["off"][m] + j] * P[:, k]).astype(np.float32)
        M[:, m] = acc
    return (np.float32(10.0) * np.log10(np.maximum(M, np.float32(1e-10)))).astype(np.float32), M


@pytest.mark.parametrize("family", MR.FAMILIES)
@pytest.mark.parametrize("case", [c for c in MR.cases() if c[0] in (128, 512) or c[3] == 40])
def test_f32_emulation_stays_under_the_bound(case, family):
    nfft, hop, n, n_mels, fmin, fmax, htk, norm = case
    x = MR.make_input(family, n, nfft, hop, MR.SR, MR.edge_frequency(n_mels, fmin, fmax, htk))
    P, S1 = MR.power_ref(x, nfft, hop)
    a_ref, _, S1_ref = R.stft_ref(x, nfft, hop)
    np.testing.assert_allclose(np.sqrt(np.maximum(P, R.AMIN_POW)), a_ref, rtol=1e-12)  # the same framing as tests/stft_ref.py
    np.testing.assert_allclose(S1, S1_ref, rtol=1e-12)
    W = MR.weights_f64(MR.SR, nfft, n_mels, fmin, fmax, htk, norm)
    A_ref, M_ref, dM = MR.mel_bound(P, S1, W, nfft)
    L, M = emulate_f32(x, nfft, hop, mel.band_table(MR.SR, nfft, n_mels, fmin, fmax, htk, norm))
    assert (np.abs(M.astype(np.float64) - M_ref) <= dM).all()
    ratio = MR.ratio_from_db(L, A_ref, dM)
    assert ratio.max() <= 1.0, (case, family, float(ratio.max()))
    if family == "silence":
        assert (M == 0).all() and (np.abs(L + 100.0) <= R.CLAMP_DB_TOL).all() and (A_ref == 1e-5).all()
    if family == "band_edge_tone":  # the tone's energy sits in the two bands that share the edge
        t = A_ref.shape[0] // 2
        assert set(np.argsort(M_ref[t])[-2:]) <= {n_mels // 2 - 1, n_mels // 2, n_mels // 2 + 1}


def test_bound_is_tight_enough_to_catch_a_wrong_weight_or_a_dropped_bin():
    nfft, hop, n, (n_mels, fmin, fmax, htk, norm) = 512, 256, 4100, MR.MELS[512][1]
    x = MR.make_input("noise", n, nfft, hop)
    P, S1 = MR.power_ref(x, nfft, hop)
    A_ref, _, dM = MR.mel_bound(P, S1, MR.weights_f64(MR.SR, nfft, n_mels, fmin, fmax, htk, norm), nfft)
    t = mel.band_table(MR.SR, nfft, n_mels, fmin, fmax, htk, norm)
    broken = {k: v.copy() for k, v in t.items()}
    broken["hi"][n_mels // 2] -= 1  # the band's last bin dropped
    assert MR.ratio_from_db(emulate_f32(x, nfft, hop, broken)[0], A_ref, dM).max() > 1.0
    broken = {k: v.copy() for k, v in t.items()}
    broken["weights"][t["off"][3]] *= np.float32(1.01)
    assert MR.ratio_from_db(emulate_f32(x, nfft, hop, broken)[0], A_ref, dM).max() > 1.0


def test_clip_normalize_ref_is_the_reference_pipeline():
    rng = np.random.default_rng(5)
    L = (rng.standard_normal((37, 40)) * 20 - 40).astype(np.float32)
    out, (ref, p_lo, p_hi) = MR.clip_normalize_ref(L, 0.01, 0.999)
    v = np.maximum(L - L.max(), np.float32(-80.0))
    lo, hi = np.percentile(v, 1.0, method="nearest"), np.percentile(v, 99.9, method="nearest")
    assert lo == p_lo and hi == p_hi and ref == L.max()
    assert np.array_equal(out, ((np.clip(v, lo, hi) - lo) / (hi - lo)).astype(np.float32)) and out.min() == 0.0 and out.max() == 1.0


# ------------------------------------------------------------------------------------------------ host routing
def _frontend_without_gpu():
    from orcai_amd.frontend import FrontEnd

    fe = FrontEnd.__new__(FrontEnd)  # the shape arithmetic needs neither the library nor a device
    fe._mel_tables = {}
    return fe


def test_spectrogram_shape_routes_on_the_mel_key():
    fe = _frontend_without_gpu()
    assert fe.spectrogram_shape(10000, SP) == (40, 171)
    assert fe.spectrogram_shape(10000, dict(SP, mel=None)) == (40, 171)
    assert fe.spectrogram_shape(10000, _sp(n_mels=64)) == (40, 64)
    assert fe.spectrogram_shape(3000, dict(SP, n_overlap=255, mel={"n_mels": 8, "fmax": 24000.0})) == (12, 8)
    with pytest.raises(ValueError, match="n_mels"):
        fe.spectrogram_shape(10000, _sp(n_mels=300))
    with pytest.raises(NotImplementedError, match="mel"):
        fe.spectrogram_shape(10000, dict(SP, nfft=500, mel={"n_mels": 8}))
    assert fe.spectrogram_shape(10000, dict(SP, nfft=500)) == (40, 167)  # the linear route keeps running other sizes


def test_linear_only_surfaces_refuse_the_mel_key():
    from orcai_amd import spectrogram as S

    sp = _sp(n_mels=40)
    with pytest.raises(NotImplementedError, match="mel"):
        S.calculate_spectrogram("unused.wav", 1, sp)
    with pytest.raises(NotImplementedError, match="mel"):
        S.preprocess_spectrogram(np.zeros((257, 4), dtype=np.float32), np.zeros(257), sp)
    with pytest.raises(NotImplementedError, match="mel"):
        _frontend_without_gpu().spectrogram_backward(None, None, None, sp)
    torch_ops = pytest.importorskip("orcai_amd.torch_ops")
    with pytest.raises(NotImplementedError, match="mel"):
        torch_ops.WaveformFrontEnd(sp, 96000)
    assert torch_ops.WaveformFrontEnd(dict(SP, mel=None), 96000).nfft == 512


def test_mel_op_schema_and_fake_shape():
    torch = pytest.importorskip("torch")
    import orcai_amd.torch_ops  # noqa: F401
    from torch._subclasses.fake_tensor import FakeTensorMode

    assert str(torch.ops.orcai.mel_spectrogram.default._schema) == (
        "orcai::mel_spectrogram(Tensor pcm, SymInt sampling_rate, SymInt nfft, SymInt hop, SymInt n_mels, float fmin, float fmax, bool htk, "
        "bool slaney_norm, float q_lo, float q_hi) -> Tensor")
    with FakeTensorMode():
        y = torch.ops.orcai.mel_spectrogram(torch.empty(10000), 48000, 512, 256, 64, 0.0, 16000.0, False, True, 0.01, 0.999)
    assert tuple(y.shape) == (40, 64) and y.dtype == torch.float32
    assert "mel_spectrogram" in orcai_amd.torch_ops.__doc__ and "NO autograd" in orcai_amd.torch_ops.__doc__
