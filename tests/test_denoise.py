"""The per-channel noise floor without a GPU: denoise.denoise_config and its refusals, the numpy specification denoise_ref on hand-made arrays, the
backward entries and differentiable modules that refuse a parameter with ``denoise`` set (reached as tests/test_frontend_route.py reaches its table of
refusals: a FrontEnd without library or device, no tensors), the new symbols, their host-side ORCAI_E_BADARG refusals, and orcai::column_percentile's
fake implementation, CPU refusal and schema.  What the kernels compute is tests/test_column_select_gpu.py's and tests/test_denoise_gpu.py's part."""

import re
from pathlib import Path

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import orcai_amd.torch_ops  # noqa: E402, F401  (registers the ops)
from orcai_amd import denoise, frontend  # noqa: E402

LIN = {"sampling_rate": 48000, "nfft": 512, "n_overlap": 256, "freq_range": [0, 16000], "quantiles": [0.01, 0.999]}
MEL = dict(LIN, mel={"n_mels": 64})
NEW_SYMBOLS = ("orcai_column_select_scratch_bytes", "orcai_column_select", "orcai_subtract_columns", "orcai_make_denoised_spectrogram")


def _fe():
    fe = frontend.FrontEnd.__new__(frontend.FrontEnd)  # host arithmetic only: neither the library nor a device
    fe._mel_tables = {}
    return fe


# ---------------------------------------------------------------------------------------------------------------- 10. configuration
def test_config_defaults_and_off():
    assert denoise.denoise_config(LIN) is None
    assert denoise.denoise_config(dict(LIN, denoise=None)) is None
    assert denoise.denoise_config(dict(LIN, denoise={})) == {"quantile": 0.5}
    assert denoise.denoise_config(dict(MEL, denoise={"quantile": 0.25})) == {"quantile": 0.25}
    for q in (0, 1, np.float32(0.5), np.int64(1)):
        cfg = denoise.denoise_config(dict(LIN, denoise={"quantile": q}))
        assert cfg == {"quantile": float(q)} and type(cfg["quantile"]) is float
    assert denoise.denoise_config(dict(LIN, denoise={}, pcen=None)) == {"quantile": 0.5}


@pytest.mark.parametrize("value,names", [
    ({"quantil": 0.5}, ["denoise", "quantil"]),
    ({"quantile": 0.5, "window": 3}, ["denoise", "window"]),
    ({"quantile": "0.5"}, ["denoise.quantile"]),
    ({"quantile": None}, ["denoise.quantile"]),
    ({"quantile": True}, ["denoise.quantile"]),
    ({"quantile": float("nan")}, ["denoise.quantile"]),
    ({"quantile": -0.01}, ["denoise.quantile", "[0, 1]"]),
    ({"quantile": 1.5}, ["denoise.quantile", "[0, 1]"]),
    (True, ["denoise"]),
    (0.5, ["denoise"]),
])
def test_config_refusals_name_the_key(value, names):
    with pytest.raises(ValueError) as e:
        denoise.denoise_config(dict(LIN, denoise=value))
    for name in names:
        assert name in str(e.value), (name, str(e.value))


def test_denoise_with_pcen_names_both_keys():
    for sp in (dict(LIN, denoise={}, pcen={}), dict(MEL, denoise={"quantile": 0.3}, pcen={"gain": 0.9})):
        with pytest.raises(ValueError) as e:
            denoise.denoise_config(sp)
        assert "denoise" in str(e.value) and "pcen" in str(e.value)
        with pytest.raises(ValueError, match="denoise.*pcen"):
            _fe().make_spectrogram(None, sp)


def test_route_keeps_its_five_fields():
    for sp, K in ((dict(LIN, denoise={}), 171), (dict(MEL, denoise={"quantile": 0.25}), 64)):
        route = frontend.resolve_route(sp)
        assert route._fields == ("nfft", "hop", "K", "mel", "pcen") and len(route) == 5
        n_fft, hop, k, cfg, pc = route
        assert (n_fft, hop, k, pc) == (512, 256, K, None)
        assert _fe().spectrogram_shape(10000, sp) == (40, K) == _fe().spectrogram_shape(10000, {k_: v for k_, v in sp.items() if k_ != "denoise"})
    with pytest.raises(ValueError, match="denoise"):  # validated by make_spectrogram before any tensor is looked at
        _fe().make_spectrogram(None, dict(LIN, denoise={"quantile": 2}))
    with pytest.raises(ValueError, match="return_profile"):
        _fe().make_spectrogram(None, LIN, return_profile=True)


def test_denoise_ref_on_hand_made_arrays():
    # column 0: a tie at the rank (rank 2 of 5 falls on one of three 1.0); column 1: constant; column 2: distinct values, -0.0 among them
    V = np.array([[1.0, -7.5, 3.0], [5.0, -7.5, -0.0], [1.0, -7.5, -2.0], [0.0, -7.5, 9.0], [1.0, -7.5, 4.0]], dtype=np.float32)
    Y, m = denoise.denoise_ref(V, 0.5)
    assert m.dtype == Y.dtype == np.float32
    assert m.tolist() == [1.0, -7.5, 3.0]
    assert Y.tolist() == (V - np.array([1.0, -7.5, 3.0], dtype=np.float32)).tolist()
    assert (Y[:, 1] == 0.0).all()
    assert np.sort(Y, axis=0)[2].tolist() == [0.0, 0.0, 0.0]  # the property the feature exists for: the selected rank of Y is exactly 0
    Y0, m0 = denoise.denoise_ref(V, 0.0)
    assert m0.tolist() == [0.0, -7.5, -2.0] and Y0.min(axis=0).tolist() == [0.0, 0.0, 0.0]
    Y1, m1 = denoise.denoise_ref(V, 1.0)
    assert m1.tolist() == [5.0, -7.5, 9.0] and Y1.max(axis=0).tolist() == [0.0, 0.0, 0.0]
    one = np.array([[3.5, -80.0, 0.0]], dtype=np.float32)  # one row: every quantile is the row itself
    for q in (0.0, 0.5, 1.0):
        Yq, mq = denoise.denoise_ref(one, q)
        assert mq.tolist() == one[0].tolist() and Yq.tolist() == [[0.0, 0.0, 0.0]]
    with pytest.raises(ValueError):
        denoise.denoise_ref(np.zeros(4, dtype=np.float32), 0.5)


# ---------------------------------------------------------------------------------------------------------------- 11. backward refusals
DEN_LIN, DEN_MEL = dict(LIN, denoise={}), dict(MEL, denoise={"quantile": 0.25})
BACKWARD_REFUSALS = [(method, sp) for method in ("backward", "spectrogram_backward", "mel_spectrogram_backward", "pcen_spectrogram_backward")
                     for sp in (DEN_LIN, DEN_MEL)]
MODULE_REFUSALS = [(name, sp) for name in ("waveform_front_end", "WaveformFrontEnd", "MelWaveformFrontEnd", "PcenWaveformFrontEnd") for sp in (DEN_LIN, DEN_MEL)]


@pytest.mark.parametrize("method,sp", BACKWARD_REFUSALS)
def test_backward_entries_refuse_denoise(method, sp):
    with pytest.raises(NotImplementedError) as e:
        getattr(_fe(), method)(None, None, None, sp)
    assert "denoise" in str(e.value) and "forward" in str(e.value) and "gradient" in str(e.value)


@pytest.mark.parametrize("name,sp", MODULE_REFUSALS)
def test_waveform_front_ends_refuse_denoise(name, sp):
    with pytest.raises(NotImplementedError) as e:
        getattr(orcai_amd.torch_ops, name)(sp, 96000)
    assert "denoise" in str(e.value) and "forward" in str(e.value) and "gradient" in str(e.value)


def test_backward_ops_reach_the_same_refusal():
    """orcai::<base>_backward is FrontEnd.backward on the parameter its arguments make: a parameter maker that sets denoise is refused there, before any
    tensor is looked at, so a *_wrt_pcm op can never differentiate a denoised forward."""
    fe = _fe()
    sp = orcai_amd.torch_ops._spectrogram_parameter(48000, 512, 256, 16000.0)
    sp["denoise"] = {}
    with pytest.raises(NotImplementedError, match="denoise"):
        fe.backward(None, None, None, sp, who="spectrogram_backward")


def test_two_step_api_refuses_denoise():
    from orcai_amd import spectrogram

    for call in (lambda: spectrogram.calculate_spectrogram("no-such-file.wav", 1, DEN_LIN),
                 lambda: spectrogram.preprocess_spectrogram(np.zeros((257, 4), dtype=np.float32), np.zeros(257), DEN_LIN)):
        with pytest.raises(NotImplementedError, match="denoise"):
            call()
    with pytest.raises(ValueError, match="denoise"):  # validated before the file is read
        spectrogram.make_spectrogram_device("no-such-file.wav", 1, {"spectrogram": dict(LIN, denoise={"quantile": 7})}, None)


# ---------------------------------------------------------------------------------------------------------------- 12. symbols and the op
def test_symbols_are_exported_and_declared():
    from orcai_amd import _native as N

    header = (Path(__file__).resolve().parents[1] / "include" / "orcai_hip.h").read_text()
    lib = N.lib()
    for name in NEW_SYMBOLS:
        assert name in N.exported_symbols() and name in N._SIGNATURES
        assert re.search(r"\b" + name + r"\(", header), name
        assert getattr(lib, name) is not None
    assert lib.orcai_column_select_scratch_bytes(171) >= 171 * (256 * 4 + 8)
    assert lib.orcai_column_select_scratch_bytes(0) == 0 and lib.orcai_column_select_scratch_bytes(4097) == 0
    assert lib.orcai_column_select_scratch_bytes(1) < lib.orcai_column_select_scratch_bytes(2) < lib.orcai_column_select_scratch_bytes(4096)


def test_badarg_needs_no_device():
    """Refused before anything is launched: the pointers are never dereferenced (16, 32, 48 stand for aligned device addresses)."""
    from orcai_amd import _native as N

    lib = N.lib()
    x, out, scr = 16, 32, 48
    bad_select = [(None, 10, 3, 0, out, scr), (x, 10, 3, 0, None, scr), (x, 10, 3, 0, out, None), (x, 0, 3, 0, out, scr), (x, -1, 3, 0, out, scr),
                  (x, 2**32, 3, 0, out, scr), (x, 2**40, 3, 0, out, scr), (x, 10, 0, 0, out, scr), (x, 10, -3, 0, out, scr), (x, 10, 4097, 0, out, scr),
                  (x, 10, 3, -1, out, scr), (x, 10, 3, 10, out, scr), (x, 10, 3, 2**33, out, scr), (x + 1, 10, 3, 0, out, scr), (x + 2, 10, 3, 0, out, scr)]
    for i, args in enumerate(bad_select):
        assert lib.orcai_column_select(*args, None) == N.E_BADARG, i
    bad_subtract = [(None, 10, 3, out), (x, 10, 3, None), (x, 0, 3, out), (x, 2**32, 3, out), (x, 10, 0, out), (x, 10, 4097, out), (x + 2, 10, 3, out)]
    for i, args in enumerate(bad_subtract):
        assert lib.orcai_subtract_columns(*args, None) == N.E_BADARG, i
    pcm, ws = 64, 256
    bands = (None, None, None, None, 0)

    def make(pcm=pcm, T=40, k=171, rank_col=20, r_lo=0, r_hi=100, out=out, profile=None, scratch=scr, workspace=ws):
        return lib.orcai_make_denoised_spectrogram(pcm, 10000, 512, 256, T, k, *bands, rank_col, r_lo, r_hi, 80.0, out, profile, scratch, workspace, None)

    for i, kw in enumerate([dict(out=None), dict(scratch=None), dict(workspace=None), dict(T=0), dict(k=0), dict(k=4097), dict(rank_col=-1), dict(rank_col=40),
                            dict(r_lo=-1), dict(r_hi=40 * 171), dict(out=out + 4)]):
        assert make(**kw) == N.E_BADARG, i


def test_column_percentile_op_shape_on_fake_tensors_and_cpu_refusal():
    import orcai_amd.torch_ops as O
    from torch._subclasses.fake_tensor import FakeTensorMode

    assert "orcai.column_percentile" in O.__doc__
    with FakeTensorMode():
        x = torch.empty((37, 4, 5))
        out = torch.ops.orcai.column_percentile(x, [0.0, 0.5, 1.0])
        assert tuple(out.shape) == (3, 4, 5) and out.dtype == torch.float32 and out.device == x.device
        out = torch.ops.orcai.column_percentile(torch.empty((3001, 171)).double(), [0.25])
        assert tuple(out.shape) == (1, 171) and out.dtype == torch.float32
    with pytest.raises(TypeError, match="CUDA"):
        torch.ops.orcai.column_percentile(torch.zeros(8, 2), [0.5])
    schema = str(torch.ops.orcai.column_percentile.default._schema)
    assert "Tensor x" in schema and "float[] q" in schema and schema.endswith("-> Tensor")
    assert O.column_percentile.__doc__ and "axis=0" in O.column_percentile.__doc__
