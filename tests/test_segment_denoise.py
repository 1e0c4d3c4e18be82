"""The time-varying noise floor (``denoise.segment``) without a GPU: the parameter and its refusals, the numpy specification segment_denoise_ref by hand
on a 7 x 2 array, S == 1 against denoise_ref, the gradient entries that refuse the key, the new symbols, their host-side ORCAI_E_BADARG refusals, the
route rule's query and the fake implementations of the two new ops.  What the kernels compute is tests/test_segment_select_gpu.py's and
tests/test_segment_denoise_gpu.py's part."""

import re
from pathlib import Path

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import orcai_amd.torch_ops  # noqa: E402, F401  (registers the ops)
from orcai_amd import denoise, frontend  # noqa: E402

LIN = {"sampling_rate": 48000, "nfft": 512, "n_overlap": 256, "freq_range": [0, 16000], "quantiles": [0.01, 0.999]}
MEL = dict(LIN, mel={"n_mels": 64})
NEW_SYMBOLS = ("orcai_segment_column_select_scratch_bytes", "orcai_segment_column_select_route", "orcai_segment_column_select",
               "orcai_segment_column_select_fused", "orcai_subtract_segment_floor", "orcai_make_segment_denoised_spectrogram")


def _fe():
    fe = frontend.FrontEnd.__new__(frontend.FrontEnd)  # host arithmetic only: neither the library nor a device
    fe._mel_tables = {}
    return fe


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).tolist()


# ---------------------------------------------------------------------------------------------------------------- configuration
def test_config_defaults_and_absent_segment():
    assert denoise.denoise_config(dict(LIN, denoise={})) == {"quantile": 0.5}  # what it is without the key: no "segment" entry
    assert denoise.denoise_config(dict(LIN, denoise={"segment": None})) == {"quantile": 0.5}
    assert denoise.denoise_config(dict(LIN, denoise={"quantile": 0.25, "segment": None})) == {"quantile": 0.25}
    assert denoise.denoise_config(dict(LIN, denoise={"quantile": 0.5, "segment": 10.0})) == {"quantile": 0.5, "segment": 10.0}
    for v in (1, 0.004, np.float32(2.5), np.int64(600)):
        cfg = denoise.denoise_config(dict(MEL, denoise={"segment": v}))
        assert cfg == {"quantile": 0.5, "segment": float(v)} and type(cfg["segment"]) is float
    assert "segment" in denoise.DENOISE_KEYS and "quantile" in denoise.DENOISE_KEYS
    assert denoise.denoise_config(LIN) is None and denoise.denoise_config(dict(LIN, denoise=None)) is None


@pytest.mark.parametrize("value", [0, -1.0, "10", True, float("nan"), float("inf"), [10.0], {}])
def test_segment_refusals_name_the_key(value):
    with pytest.raises(ValueError, match=r"denoise\.segment"):
        denoise.denoise_config(dict(LIN, denoise={"segment": value}))


def test_window_is_still_unknown_and_pcen_still_refused():
    with pytest.raises(ValueError) as e:
        denoise.denoise_config(dict(LIN, denoise={"segment": 10.0, "window": 3}))
    assert "window" in str(e.value) and "unknown" in str(e.value)
    with pytest.raises(ValueError, match="denoise.*pcen"):
        denoise.denoise_config(dict(LIN, denoise={"segment": 10.0}, pcen={}))


def test_segment_rows_and_count():
    assert denoise.segment_rows(10.0, 48000, 256) == 1875
    assert denoise.segment_rows(1.0, 48000, 256) == 188  # rint(187.5): half to even
    assert denoise.segment_rows(0.001, 48000, 256) == 1
    assert [denoise.segment_count(T, 2) for T in (1, 2, 3, 4, 7)] == [1, 1, 1, 2, 3]
    assert denoise.segment_count(675001, 1875) == 360


# ---------------------------------------------------------------------------------------------------------------- the specification
def test_segment_denoise_ref_by_hand():
    """7 x 2, W = 2: segments [0, 2), [2, 4), [4, 7) with centres 0.5, 2.5, 5 (doubled: 1, 5, 10).  Median ranks: nearest_rank_index(2, 0.5) = 0 (0.5
    rounds half to even) and nearest_rank_index(3, 0.5) = 1."""
    V = np.array([[4.0, -1.0], [2.0, -3.0], [10.0, 0.0], [8.0, -0.0], [1.0, 5.0], [3.0, 7.0], [2.0, 6.0]], dtype=np.float32)
    Y, m = denoise.segment_denoise_ref(V, 0.5, 2)
    assert m.dtype == Y.dtype == np.float32 and m.shape == (3, 2) and Y.shape == V.shape
    assert m.tolist() == [[2.0, -3.0], [8.0, 0.0], [2.0, 6.0]]  # by value, as denoise_ref: the sign of a zero floor is the kernels' (-0.0 first)
    f32 = np.float32
    a = {1: f32(np.float64(1) / np.float64(4)), 2: f32(np.float64(3) / np.float64(4)), 3: f32(np.float64(1) / np.float64(5)), 4: f32(np.float64(3) / np.float64(5))}
    F = np.empty((7, 2), dtype=np.float32)
    F[0] = m[0]                                        # u = 0 <= 1
    F[1] = m[0] + a[1] * (m[1] - m[0])                 # u = 2: 1/4 of the way from centre 0.5 to 2.5
    F[2] = m[0] + a[2] * (m[1] - m[0])                 # u = 4: 3/4
    F[3] = m[1] + a[3] * (m[2] - m[1])                 # u = 6: 1/5 of the way from 2.5 to 5
    F[4] = m[1] + a[4] * (m[2] - m[1])                 # u = 8: 3/5
    F[5] = m[2]                                        # u = 10: exactly on the last centre
    F[6] = m[2]
    assert F[1].tolist() == [3.5, -2.25] and F[2].tolist() == [6.5, -0.75]
    assert bits(Y) == bits(V - F)
    assert Y[5].tolist() == [1.0, 1.0] and Y[0].tolist() == [2.0, 2.0]
    # a frame exactly on an inner centre: W = 3, T = 9 -> centres 1, 4, 7
    V9 = np.arange(18, dtype=np.float32).reshape(9, 2) ** 2
    Y9, m9 = denoise.segment_denoise_ref(V9, 0.0, 3)
    assert m9.tolist() == V9[[0, 3, 6]].tolist()
    assert bits(Y9[4]) == bits(V9[4] - m9[1]) and bits(Y9[1]) == bits(V9[1] - m9[0]) and bits(Y9[8]) == bits(V9[8] - m9[2])
    with pytest.raises(ValueError):
        denoise.segment_denoise_ref(V, 0.5, 0)


@pytest.mark.parametrize("T,W", [(1, 1), (5, 3), (5, 5), (5, 9), (37, 19)])
def test_one_segment_is_denoise_ref(T, W):
    rng = np.random.default_rng(T * 31 + W)
    V = (-40 + 12 * rng.standard_normal((T, 6))).astype(np.float32)
    V[0, 0], V[T // 2, 1] = -0.0, 0.0
    for q in (0.0, 0.25, 0.5, 1.0):
        Y, m = denoise.segment_denoise_ref(V, q, W)
        Y1, m1 = denoise.denoise_ref(V, q)
        assert m.shape == (1, 6) and bits(m[0]) == bits(m1) and bits(Y) == bits(Y1)


def test_ref_segments_follow_the_rule_and_hold_outside_the_centres():
    rng = np.random.default_rng(3)
    T, W = 23, 4  # S = 5: four full segments and a last one of 7 rows
    V = rng.standard_normal((T, 3)).astype(np.float32)
    Y, m = denoise.segment_denoise_ref(V, 0.5, W)
    assert m.shape == (5, 3)
    for s in range(5):
        seg = V[s * W: (s + 1) * W if s < 4 else T]
        assert m[s].tolist() == np.sort(seg, axis=0)[frontend.nearest_rank_index(len(seg), 0.5)].tolist()
    assert bits(Y[:2]) == bits(V[:2] - m[0]) and bits(Y[19:]) == bits(V[19:] - m[4])  # centres 1.5 and 19


# ---------------------------------------------------------------------------------------------------------------- gradient refusals
SEG_LIN, SEG_MEL = dict(LIN, denoise={"segment": 10.0}), dict(MEL, denoise={"quantile": 0.25, "segment": 1.0})


@pytest.mark.parametrize("sp", [SEG_LIN, SEG_MEL], ids=["linear", "mel"])
def test_the_three_gradient_entries_refuse_segment(sp):
    import orcai_amd.torch_ops as O

    with pytest.raises(NotImplementedError, match=r"denoise\.segment"):
        _fe().denoised_spectrogram_backward(None, None, None, None, sp)
    with pytest.raises(NotImplementedError, match=r"denoise\.segment"):
        O.DenoisedWaveformFrontEnd(sp, 96000)
    with pytest.raises(NotImplementedError, match=r"denoise\.segment"):
        O._denoised_parameter(48000, 512, 256, 16000.0, 0, 0.0, 0.0, False, True, sp["denoise"]["quantile"] if "quantile" in sp["denoise"] else 0.5,
                              segment=sp["denoise"]["segment"])
    assert "segment" not in O._denoised_parameter(48000, 512, 256, 16000.0, 0, 0.0, 0.0, False, True, 0.5)["denoise"]
    for method in ("backward", "spectrogram_backward", "mel_spectrogram_backward", "pcen_spectrogram_backward"):  # the plain entries: as for any denoise
        with pytest.raises(NotImplementedError, match="denoise"):
            getattr(_fe(), method)(None, None, None, sp)
    with pytest.raises(NotImplementedError, match="denoise"):
        O.waveform_front_end(sp, 96000)
    O.DenoisedWaveformFrontEnd(dict(LIN, denoise={"segment": None}), 96000)  # null is absent


def test_segment_null_resolves_like_absent_and_profile_needs_denoise():
    assert _fe().spectrogram_shape(10000, SEG_LIN) == (40, 171) and _fe().spectrogram_shape(10000, SEG_MEL) == (40, 64)
    with pytest.raises(ValueError, match=r"denoise\.segment"):  # validated by make_spectrogram before any tensor is looked at
        _fe().make_spectrogram(None, dict(LIN, denoise={"segment": -2}))


# ---------------------------------------------------------------------------------------------------------------- symbols, host-side refusals, the rule
def test_symbols_are_exported_and_declared():
    from orcai_amd import _native as N

    header = (Path(__file__).resolve().parents[1] / "include" / "orcai_hip.h").read_text()
    lib = N.lib()
    for name in NEW_SYMBOLS:
        assert name in N.exported_symbols() and name in N._SIGNATURES
        assert re.search(r"\b" + name + r"\(", header), name
        assert getattr(lib, name) is not None
    base = lib.orcai_column_select_scratch_bytes(171)
    assert lib.orcai_segment_column_select_scratch_bytes(675001, 171, 1875) == base - 171 * 4 + 360 * 171 * 4
    assert lib.orcai_segment_column_select_scratch_bytes(100, 171, 1000) == base  # one segment: orcai_column_select's own
    for bad in ((0, 171, 10), (10, 0, 10), (10, 4097, 10), (10, 171, 0), (2**32, 171, 10)):
        assert lib.orcai_segment_column_select_scratch_bytes(*bad) == 0 and lib.orcai_segment_column_select_route(*bad) == N.E_BADARG


def test_route_rule_is_one_function_of_the_segments():
    """Fused exactly while 61 ns x the rows of the longest segment <= 45 us x S (measured): the hour at 48 kHz goes fused at 1 s, 10 s and
    60 s and to the loop at 600 s whatever K, and both sides of the boundary."""
    from orcai_amd import _native as N

    route = N.lib().orcai_segment_column_select_route
    hour = {188: 1, 1875: 1, 11250: 1, 112500: 0}
    for W, want in hour.items():
        assert route(675001, 171, W) == route(675001, 64, W) == want, W
    for rows, cols, W in ((675001, 171, 188), (675001, 64, 112500), (737, 5, 1000), (738, 5, 1000), (1475, 1, 737), (1477, 1, 738), (40, 4096, 8),
                          (70001, 7, 35000), (1300, 171, 601), (1, 1, 1), (10**6, 3, 10**6), (10**6, 3, 1000), (2**32 - 1, 4096, 1)):
        S = max(1, rows // W)
        longest = rows - (S - 1) * W
        assert route(rows, cols, W) == int(61 * longest <= 45000 * S), (rows, cols, W)
    assert route(737, 5, 1000) == 1 and route(738, 5, 1000) == 0


def test_badarg_needs_no_device():
    """Refused before anything is launched: the pointers are never dereferenced (16, 32, 48 stand for aligned device addresses)."""
    from orcai_amd import _native as N

    lib = N.lib()
    x, out, scr = 16, 32, 48
    # rows 7, W 2: S = 3, full segments of 2 rows, the last one 3
    bad = [(None, 7, 2, 2, 0, 0, out, scr), (x, 7, 2, 2, 0, 0, None, scr), (x, 7, 2, 2, 0, 0, out, None), (x + 2, 7, 2, 2, 0, 0, out, scr),
           (x, 7, 2, 2, 0, 0, out + 1, scr), (x, 7, 2, 2, 0, 0, out, scr + 2), (x, 0, 2, 2, 0, 0, out, scr), (x, -7, 2, 2, 0, 0, out, scr),
           (x, 2**32, 2, 2, 0, 0, out, scr), (x, 7, 0, 2, 0, 0, out, scr), (x, 7, 4097, 2, 0, 0, out, scr), (x, 7, 2, 0, 0, 0, out, scr),
           (x, 7, 2, -1, 0, 0, out, scr), (x, 7, 2, 2, 2, 0, out, scr), (x, 7, 2, 2, -1, 0, out, scr), (x, 7, 2, 2, 0, 3, out, scr),
           (x, 7, 2, 2, 0, -1, out, scr), (x, 3, 2, 5, 0, 3, out, scr)]
    for i, args in enumerate(bad):
        assert lib.orcai_segment_column_select(*args, None) == N.E_BADARG, i
        if args[7] is not None and args[7] == scr:  # the fused entry takes no scratch
            assert lib.orcai_segment_column_select_fused(*args[:7], None) == N.E_BADARG, i
    bad_subtract = [(None, 7, 2, 2, out), (x, 7, 2, 2, None), (x, 0, 2, 2, out), (x, 2**32, 2, 2, out), (x, 7, 0, 2, out), (x, 7, 4097, 2, out), (x, 7, 2, 0, out),
                    (x + 2, 7, 2, 2, out), (x, 7, 2, 2, out + 2)]
    for i, args in enumerate(bad_subtract):
        assert lib.orcai_subtract_segment_floor(*args, None) == N.E_BADARG, i
    pcm, ws = 64, 256
    bands = (None, None, None, None, 0)

    def make(T=40, k=171, W=8, rank=3, rank_last=3, r_lo=0, r_hi=100, out=out, profile=None, scratch=scr, workspace=ws):
        return lib.orcai_make_segment_denoised_spectrogram(pcm, 10000, 512, 256, T, k, *bands, W, rank, rank_last, r_lo, r_hi, 80.0, out, profile, scratch,
                                                           workspace, None)

    for i, kw in enumerate([dict(out=None), dict(scratch=None), dict(workspace=None), dict(T=0), dict(k=0), dict(k=4097), dict(W=0), dict(rank=-1), dict(rank=8),
                            dict(rank_last=8), dict(rank_last=-1), dict(r_lo=-1), dict(r_hi=40 * 171), dict(out=out + 4), dict(profile=34)]):
        assert make(**kw) == N.E_BADARG, i


# ---------------------------------------------------------------------------------------------------------------- the ops on fake tensors
def test_the_two_ops_on_fake_tensors_and_cpu_refusal():
    import orcai_amd.torch_ops as O
    from torch._subclasses.fake_tensor import FakeTensorMode

    assert "orcai.segment_column_percentile" in O.__doc__ and "orcai.segment_denoised_spectrogram" in O.__doc__
    with FakeTensorMode():
        x = torch.empty((37, 4, 5))
        for W, S in ((10, 3), (37, 1), (100, 1), (1, 37)):
            out = torch.ops.orcai.segment_column_percentile(x, [0.0, 0.5, 1.0], W)
            assert tuple(out.shape) == (3, S, 4, 5) and out.dtype == torch.float32 and out.device == x.device
        pcm = torch.empty(4113)
        lin = torch.ops.orcai.segment_denoised_spectrogram(pcm, 48000, 512, 256, 16000.0, 0, 0.0, 0.0, False, True, 0.5, 10.0, 0.01, 0.999)
        mel = torch.ops.orcai.segment_denoised_spectrogram(pcm, 48000, 512, 256, 0.0, 64, 0.0, 24000.0, False, True, 0.25, 1.0, 0.01, 0.999)
        assert tuple(lin.shape) == (17, 171) and tuple(mel.shape) == (17, 64) and lin.dtype == mel.dtype == torch.float32
        g = torch.empty(4113, requires_grad=True)
        spec = torch.ops.orcai.segment_denoised_spectrogram(g, 48000, 512, 256, 16000.0, 0, 0.0, 0.0, False, True, 0.5, 10.0, 0.01, 0.999)
        assert spec.requires_grad
        with pytest.raises(NotImplementedError, match="forward only"):
            torch.autograd.grad(spec.sum(), g)
    with pytest.raises(TypeError, match="CUDA"):
        torch.ops.orcai.segment_column_percentile(torch.zeros(8, 2), [0.5], 2)
    schema = str(torch.ops.orcai.segment_column_percentile.default._schema)
    assert "Tensor x" in schema and "float[] q" in schema and "SymInt segment_rows" in schema and schema.endswith("-> Tensor")
    schema = str(torch.ops.orcai.segment_denoised_spectrogram.default._schema)
    assert "float quantile, float segment, float q_lo, float q_hi" in schema
    assert not hasattr(torch.ops.orcai, "segment_denoised_spectrogram_wrt_pcm")
