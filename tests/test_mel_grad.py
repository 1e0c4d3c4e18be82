"""CPU half of the mel front end's gradient w.r.t. the audio: the float64 reference of tests/mel_grad_ref.py is pinned to tests/mel_ref.py's contract and
to the written definition of include/orcai_hip.h (orcai_mel_spectrogram_bwd), the test cases satisfy their conditions (valid parameters, tie share), the
parity rule the launcher relies on holds over a grid of band tables, and the Python surface (ctypes table, op schemas and fake shapes, the factory)
exists.  No GPU."""

import itertools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import mel_grad_ref as R  # noqa: E402
import mel_ref  # noqa: E402
from orcai_amd import mel  # noqa: E402

SHORT = (512, 256, 64, 0.0, 24000.0, False, "slaney")
OP_ARGS = (48000, 512, 256, 64, 0.0, 24000.0, False, True, 0.01, 0.999)


def test_every_case_is_a_valid_mel_parameter_with_no_empty_band():
    assert len(R.CASES) == 6
    for c in R.CASES:
        cfg = mel.mel_config(R.parameter(c, "a"))  # raises on an empty band or a refused size
        assert cfg["n_mels"] == c[2]
        t = R.table_of(c)
        assert (t["hi"] > t["lo"]).all() and R.parity_rule_holds(t)


def test_restated_forward_agrees_with_the_float64_contract():
    """M of the restatement against mel_ref.power_ref / weights_f64 (numpy, another framing), and the dB / clip / normalise chain against numpy."""
    nfft, hop, n_mels, fmin, fmax, htk, norm = SHORT
    y = R.G.recording("b")[40000:56001].copy()
    out, aux = R.forward(torch.from_numpy(y).double(), SHORT, (0.10, 0.999))
    P, _ = mel_ref.power_ref(y, nfft, hop)
    M = P @ mel_ref.weights_f64(R.SR, nfft, n_mels, fmin, fmax, htk, norm).T
    assert aux["M"].shape == M.shape
    np.testing.assert_allclose(aux["M"].numpy(), M, rtol=1e-10, atol=1e-16)
    L = 10.0 * np.log10(np.maximum(M, 1e-10))
    v = np.maximum(L - L.max(), -80.0)
    srt = np.sort(v, axis=None)
    from oracle.frontend_ref import nearest_rank_index

    lo, hi = srt[nearest_rank_index(v.size, 0.10)], srt[nearest_rank_index(v.size, 0.999)]
    np.testing.assert_allclose(out.numpy(), (np.clip(v, lo, hi) - lo) / (hi - lo), rtol=0, atol=1e-9)


@pytest.mark.parametrize("index", [2, 1])  # 128 / 32 / 8 bands, unnormalised; 512 / 255 / 128 bands above 6 kHz
def test_autograd_gradient_equals_the_written_formula(index):
    mc = R.CASES[index]
    n = 6000 if index == 2 else 9000
    pcm = torch.from_numpy(R.G.recording("b")[47000 : 47000 + n].copy())  # runs into the digital silence: floored bands and M <= 1e-10
    c = R.build_case(pcm, mc, (0.10, 0.999), seed=5 + index)
    assert c["floored_share"] > 0.1 and float(c["dpcm64"].abs().max()) > 0
    want = R.dpcm_by_formula(c, mc)
    err = float((want - c["dpcm64"]).abs().max() / c["dpcm64"].abs().max())
    assert err <= 1e-12, err


def test_tie_share_of_every_case():
    for which in ("a", "b"):
        for i in range(len(R.CASES)):
            share = R.case(which, i)["tie_share"]
            assert share <= R.TIE_SHARE_MAX, (which, i, share)
    floored = [R.case("b", i)["floored_share"] for i in range(len(R.CASES))]
    assert min(floored) > 0.03, floored  # recording (b) exercises the floor and the M <= 1e-10 gate in every case


def test_parity_rule_and_the_per_bin_gather_over_a_grid_of_band_tables():
    """band_hi[m] <= band_lo[m + 2]: two bands of equal parity never share a bin, so one even and one odd entry per bin hold the whole filterbank."""
    seen = 0
    for sr, nfft, n_mels, htk, norm, (f0, f1) in itertools.product((16000, 48000, 96000), (128, 512, 1024, 4096), (8, 40, 64, 128, 256), (False, True),
                                                                   ("slaney", None), ((0.0, 0.5), (0.125, 0.5), (0.0, 1.0 / 3.0))):
        t = mel.band_table(sr, nfft, n_mels, f0 * sr, f1 * sr, htk, norm)
        if (t["hi"] == t["lo"]).any():
            continue  # mel_config refuses a table with an empty band
        seen += 1
        assert R.parity_rule_holds(t), (sr, nfft, n_mels, htk, norm, f0, f1)
        eb, ew, ob, ow = R.bin_table(t, nfft)
        W = np.zeros((n_mels, 1 + nfft // 2), dtype=np.float32)
        k = np.arange(1 + nfft // 2)
        W[eb, k] = ew
        W[ob, k] += ow  # (band 1 with weight 0 where no odd band covers the bin)
        assert np.array_equal(W, mel.dense_from_table(t, nfft)), (sr, nfft, n_mels)
    assert seen >= 200, seen


def test_native_table_declares_the_launcher():
    from orcai_amd import _native as N

    ret, args = N._SIGNATURES["orcai_mel_spectrogram_bwd"]
    assert len(args) == 16
    assert "orcai_mel_spectrogram_bwd" in N.exported_symbols()


def test_schema_and_fake_shapes_of_the_new_ops():
    import orcai_amd.torch_ops  # noqa: F401
    from torch._subclasses.fake_tensor import FakeTensorMode

    s = str(torch.ops.orcai.mel_spectrogram_wrt_pcm.default._schema)
    assert "Tensor pcm" in s and "n_mels" in s and "slaney_norm" in s and s.endswith("-> Tensor")
    assert "Tensor grad, Tensor pcm, Tensor stats" in str(torch.ops.orcai.mel_spectrogram_backward.default._schema)
    with FakeTensorMode():
        pcm = torch.empty(10000, dtype=torch.float32, device="cuda")
        out = torch.ops.orcai.mel_spectrogram_wrt_pcm(pcm, *OP_ARGS)
        assert out.shape == (1 + 10000 // 256, 64) and out.dtype == torch.float32
        spec, stats = torch.ops.orcai.mel_spectrogram_with_stats(pcm, *OP_ARGS)
        assert spec.shape == out.shape and stats.shape == (6,)
        d = torch.ops.orcai.mel_spectrogram_backward(spec, pcm, stats, *OP_ARGS[:8])
        assert d.shape == (10000,) and d.dtype == torch.float32


def test_factory_returns_the_class_the_parameter_asks_for():
    from orcai_amd import torch_ops as TO

    lin = {"sampling_rate": 48000, "nfft": 512, "n_overlap": 256, "freq_range": [0, 16000], "quantiles": [0.01, 0.999]}
    m = TO.waveform_front_end(R.parameter(R.CASES[0], "a"), 96000)
    assert type(m) is TO.MelWaveformFrontEnd and (m.n_mels, m.fmax, m.slaney_norm, m.native_rate) == (64, 24000.0, True, 96000)
    assert type(TO.waveform_front_end(lin, 96000)) is TO.WaveformFrontEnd
    assert type(TO.waveform_front_end(dict(lin, mel=None), 96000)) is TO.WaveformFrontEnd
    with pytest.raises(NotImplementedError, match="waveform_front_end"):
        TO.WaveformFrontEnd(R.parameter(R.CASES[0], "a"), 96000)
    with pytest.raises(ValueError, match="mel"):
        TO.MelWaveformFrontEnd(lin, 96000)
    with pytest.raises(NotImplementedError, match="nfft"):
        TO.waveform_front_end(dict(R.parameter(R.CASES[0], "a"), nfft=500), 96000)
