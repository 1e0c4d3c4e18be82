"""The front end's route plan, the parts that need no GPU: frontend.resolve_route over every kind of spectrogram parameter, the refusals (type and full
message as recorded before the routes were merged into one plan and, for the denoised route, before it joined the one wiring:
tests/golden/frontend_route_refusals.json), frontend.n_frames against the two spellings it replaced, and the shapes the sixteen ops of the four
differentiable routes give on fake tensors, with their schemas."""

import json
from pathlib import Path

import pytest

torch = pytest.importorskip("torch")

import orcai_amd.torch_ops  # noqa: E402, F401  (registers the ops)
from orcai_amd import frontend  # noqa: E402

LIN = {"sampling_rate": 48000, "nfft": 512, "n_overlap": 256, "freq_range": [0, 16000], "quantiles": [0.01, 0.999]}
MEL = dict(LIN, mel={"n_mels": 64})
GOLDEN = json.loads((Path(__file__).parent / "golden" / "frontend_route_refusals.json").read_text())


def _fe():
    fe = frontend.FrontEnd.__new__(frontend.FrontEnd)  # host arithmetic only: neither the library nor a device
    fe._mel_tables = {}
    return fe


# name -> (parameter, n_samples, T, K, mel set, pcen set)
ROUTES = {
    "linear-512": (LIN, 10000, 40, 171, False, False),
    "linear-500": (dict(LIN, nfft=500, n_overlap=250), 4001, 17, 167, False, False),  # forward only
    "linear-odd": (dict(LIN, nfft=675, n_overlap=100), 1000, 10, 225, False, False),  # odd nfft: one frame fewer than 1 + n // hop; bin 225 is 16 kHz
    "mel64-512": (MEL, 10000, 40, 64, True, False),
    "pcen-linear": (dict(LIN, pcen={}), 10000, 40, 171, False, True),
    "pcen-mel": (dict(MEL, pcen={"time_constant": 0.1}), 10000, 40, 64, True, True),
    "linear-from-1kHz": (dict(LIN, freq_range=[1000, 16000]), 10000, 40, 171, False, False),  # crop_indices starts at the first bin <= 1 kHz, which is bin 0
}


@pytest.mark.parametrize("name", list(ROUTES))
def test_route_resolution(name):
    from orcai_amd import mel, pcen

    sp, n, T, K, has_mel, has_pcen = ROUTES[name]
    route = frontend.resolve_route(sp)
    assert isinstance(route, tuple) and route._fields == ("nfft", "hop", "K", "mel", "pcen")
    assert (route.nfft, route.hop, route.K) == (sp["nfft"], sp["n_overlap"], K)
    assert route.mel == mel.mel_config(sp) and (route.mel is not None) == has_mel
    assert route.pcen == pcen.pcen_config(sp) and (route.pcen is not None) == has_pcen
    with pytest.raises(AttributeError):
        route.K = 1
    fe = _fe()
    assert fe.spectrogram_shape(n, sp) == (T, K) == (frontend.n_frames(n, route.nfft, route.hop), fe._kept_bins(sp))


def test_each_config_runs_once_per_resolution(monkeypatch):
    from orcai_amd import mel, pcen

    calls = []
    real = {"mel": mel.mel_config, "pcen": pcen.pcen_config}
    monkeypatch.setattr(mel, "mel_config", lambda sp: (calls.append("mel"), real["mel"](sp))[1])
    monkeypatch.setattr(pcen, "pcen_config", lambda sp: (calls.append("pcen"), real["pcen"](sp))[1])
    for sp in (LIN, ROUTES["pcen-mel"][0]):
        del calls[:]
        _fe().spectrogram_shape(10000, sp)
        assert calls == ["pcen", "mel"]


# ---------------------------------------------------------------------------------------------------------------- refusals
# name -> (what raises, parameter).  "route": resolve_route, _kept_bins and spectrogram_shape; "backward": FrontEnd.backward and the route's named
# method, with no tensors (refused before any is looked at); a method's name: that method on a parameter of another route; a name of torch_ops: that
# module class, or waveform_front_end, constructed at a native rate of 96 kHz.  denoised_spectrogram_backward takes the profile as well: four Nones.
PCEN_LIN = dict(LIN, pcen={})
DN_LIN = dict(LIN, denoise={})
DN_MEL = dict(MEL, denoise={"quantile": 0.25})
REFUSALS = {
    "linear-nfft-1": ("route", dict(LIN, nfft=1)),
    "linear-nfft-8192": ("route", dict(LIN, nfft=8192)),
    "mel-nfft-500": ("route", dict(MEL, nfft=500)),
    "mel-nfft-64": ("route", dict(MEL, nfft=64)),
    "mel-nfft-8192": ("route", dict(MEL, nfft=8192)),
    "pcen-nfft-500": ("route", dict(PCEN_LIN, nfft=500)),
    "pcen-nfft-16": ("route", dict(PCEN_LIN, nfft=16)),
    "pcen-mel-nfft-64": ("route", dict(MEL, nfft=64, pcen={})),
    "pcen-unknown-key": ("route", dict(LIN, pcen={"alpha": 0.98})),
    "pcen-not-a-dict": ("route", dict(LIN, pcen=True)),
    "pcen-bad-value": ("route", dict(LIN, pcen={"gain": 1.5})),
    "mel-empty-band": ("route", dict(LIN, mel={"n_mels": 128})),
    "mel-unknown-key": ("route", dict(LIN, mel={"n_mels": 40, "nmels": 3})),
    "pcen-before-mel": ("route", dict(LIN, pcen={"alpha": 0.98}, mel={"n_mels": 7})),
    "mel-before-nfft": ("route", dict(LIN, nfft=8192, mel={"n_mels": 7})),
    "backward-linear-nfft-500": ("backward", dict(LIN, nfft=500, n_overlap=250)),
    "backward-linear-nfft-16": ("backward", dict(LIN, nfft=16, n_overlap=8)),
    "backward-linear-nfft-8192": ("backward", dict(LIN, nfft=8192)),
    "backward-mel-nfft-500": ("backward", dict(MEL, nfft=500)),
    "backward-pcen-nfft-500": ("backward", dict(PCEN_LIN, nfft=500)),
    "backward-linear-hop-0": ("backward", dict(LIN, n_overlap=0)),
    "backward-mel-hop-0": ("backward", dict(MEL, n_overlap=0)),
    "backward-pcen-hop-0": ("backward", dict(PCEN_LIN, n_overlap=0)),
    "linear-method-on-mel": ("spectrogram_backward", MEL),
    "linear-method-on-pcen": ("spectrogram_backward", PCEN_LIN),
    "mel-method-on-linear": ("mel_spectrogram_backward", LIN),
    "mel-method-on-pcen": ("mel_spectrogram_backward", dict(MEL, pcen={})),
    "pcen-method-on-linear": ("pcen_spectrogram_backward", LIN),
    "pcen-method-on-mel": ("pcen_spectrogram_backward", MEL),
    "module-linear-crop-start": ("WaveformFrontEnd", dict(LIN, freq_range=[1000, 16000])),
    "module-pcen-crop-start": ("PcenWaveformFrontEnd", dict(PCEN_LIN, freq_range=[1000, 16000])),
    "module-linear-on-mel": ("WaveformFrontEnd", MEL),
    "module-linear-on-pcen": ("WaveformFrontEnd", PCEN_LIN),
    "module-mel-on-linear": ("MelWaveformFrontEnd", LIN),
    "module-mel-on-pcen": ("MelWaveformFrontEnd", dict(MEL, pcen={})),
    "module-mel-nfft-500": ("MelWaveformFrontEnd", dict(MEL, nfft=500)),
    "module-pcen-on-linear": ("PcenWaveformFrontEnd", LIN),
    "module-pcen-unknown-key": ("PcenWaveformFrontEnd", dict(LIN, pcen={"alpha": 0.98})),
    "module-factory-on-pcen": ("waveform_front_end", PCEN_LIN),
    "module-factory-on-pcen-mel": ("waveform_front_end", dict(MEL, pcen={})),
    "denoised-method-on-linear": ("denoised_spectrogram_backward", LIN),
    "denoised-method-on-mel": ("denoised_spectrogram_backward", MEL),
    "denoised-method-on-pcen": ("denoised_spectrogram_backward", PCEN_LIN),
    "denoised-method-on-null": ("denoised_spectrogram_backward", dict(LIN, denoise=None)),
    "denoised-method-with-pcen": ("denoised_spectrogram_backward", dict(DN_LIN, pcen={})),  # denoise_config before resolve_route: not a PCEN route
    "denoised-method-with-bad-pcen": ("denoised_spectrogram_backward", dict(DN_LIN, pcen={"alpha": 0.98})),
    "denoised-method-bad-quantile": ("denoised_spectrogram_backward", dict(LIN, denoise={"quantile": 2})),
    "denoised-method-unknown-key": ("denoised_spectrogram_backward", dict(LIN, denoise={"q": 0.5})),
    "denoised-method-not-a-dict": ("denoised_spectrogram_backward", dict(LIN, denoise=True)),
    "denoised-method-linear-nfft-500": ("denoised_spectrogram_backward", dict(DN_LIN, nfft=500, n_overlap=250)),
    "denoised-method-linear-nfft-16": ("denoised_spectrogram_backward", dict(DN_LIN, nfft=16, n_overlap=8)),
    "denoised-method-linear-nfft-8192": ("denoised_spectrogram_backward", dict(DN_LIN, nfft=8192)),
    "denoised-method-mel-nfft-64": ("denoised_spectrogram_backward", dict(DN_MEL, nfft=64)),
    "denoised-method-mel-bad-quantile-nfft-64": ("denoised_spectrogram_backward", dict(MEL, denoise={"quantile": 2}, nfft=64)),
    "denoised-method-mel-nfft-64-hop-0": ("denoised_spectrogram_backward", dict(DN_MEL, nfft=64, n_overlap=0)),
    "denoised-method-linear-nfft-500-hop-0": ("denoised_spectrogram_backward", dict(DN_LIN, nfft=500, n_overlap=0)),
    "denoised-method-linear-hop-0": ("denoised_spectrogram_backward", dict(DN_LIN, n_overlap=0)),
    "denoised-method-mel-hop-0": ("denoised_spectrogram_backward", dict(DN_MEL, n_overlap=0)),
    "denoised-method-pcm": ("denoised_spectrogram_backward", DN_LIN),  # the parameter passes: the pcm (None) is refused next
    "linear-method-on-denoised": ("spectrogram_backward", DN_LIN),
    "mel-method-on-denoised": ("mel_spectrogram_backward", DN_MEL),
    "pcen-method-on-denoised": ("pcen_spectrogram_backward", DN_LIN),
    "module-denoised-on-linear": ("DenoisedWaveformFrontEnd", LIN),
    "module-denoised-on-mel": ("DenoisedWaveformFrontEnd", MEL),
    "module-denoised-on-pcen": ("DenoisedWaveformFrontEnd", PCEN_LIN),
    "module-denoised-with-pcen": ("DenoisedWaveformFrontEnd", dict(DN_LIN, pcen={})),
    "module-denoised-bad-quantile": ("DenoisedWaveformFrontEnd", dict(LIN, denoise={"quantile": 2})),
    "module-denoised-crop-start": ("DenoisedWaveformFrontEnd", dict(DN_LIN, freq_range=[1000, 16000])),
    "module-denoised-nfft-500": ("DenoisedWaveformFrontEnd", dict(DN_LIN, nfft=500)),
    "module-denoised-nfft-500-crop-start": ("DenoisedWaveformFrontEnd", dict(DN_LIN, nfft=500, freq_range=[1000, 16000])),
    "module-denoised-mel-nfft-500": ("DenoisedWaveformFrontEnd", dict(DN_MEL, nfft=500)),
    "module-denoised-mel-unknown-key": ("DenoisedWaveformFrontEnd", dict(DN_LIN, mel={"n_mels": 40, "nmels": 3})),
    "module-pcen-on-mel": ("PcenWaveformFrontEnd", MEL),
    "module-pcen-on-denoised": ("PcenWaveformFrontEnd", DN_LIN),
    "module-pcen-mel-nfft-500": ("PcenWaveformFrontEnd", dict(MEL, nfft=500, pcen={})),
    "module-pcen-bad-value-crop-start": ("PcenWaveformFrontEnd", dict(LIN, pcen={"gain": 1.5}, freq_range=[1000, 16000])),
    "module-linear-on-denoised": ("WaveformFrontEnd", DN_LIN),
    "module-mel-on-denoised": ("MelWaveformFrontEnd", DN_MEL),
    "module-factory-on-denoised": ("waveform_front_end", DN_LIN),
}


def named_method(sp: dict) -> str:
    return "pcen_spectrogram_backward" if sp.get("pcen") is not None else "mel_spectrogram_backward" if sp.get("mel") is not None else "spectrogram_backward"


def _raised(call):
    with pytest.raises(Exception) as e:
        call()
    return [type(e.value).__name__, str(e.value)]


@pytest.mark.parametrize("name", list(REFUSALS))
def test_refusals_are_what_they_were(name):
    what, sp = REFUSALS[name]
    fe = _fe()
    if what == "route":
        calls = [lambda: frontend.resolve_route(sp), lambda: fe._kept_bins(sp), lambda: fe.spectrogram_shape(10000, sp),
                 lambda: fe.make_spectrogram(None, sp)]
    elif what == "backward":
        calls = [lambda: fe.backward(None, None, None, sp), lambda: getattr(fe, named_method(sp))(None, None, None, sp)]
    elif hasattr(fe, what):
        calls = [lambda: getattr(fe, what)(*(None,) * (4 if what == "denoised_spectrogram_backward" else 3), sp)]
    else:
        calls = [lambda: getattr(orcai_amd.torch_ops, what)(sp, 96000)]
    for call in calls:
        assert _raised(call) == GOLDEN[name]


# name -> (method, parameter, which tensor is wrong).  The tensors are fake CUDA tensors, so the refusals that follow the pcm check are raised for real
# without a GPU: pcm has 4113 samples (17 frames at hop 256), grad [17, K], stats [6], and for the denoised method profile [K]; the wrong one is one short.
TENSOR_REFUSALS = {
    "backward-linear-grad": ("backward", LIN, "grad"),
    "backward-linear-stats": ("backward", LIN, "stats"),
    "backward-mel-grad": ("backward", MEL, "grad"),
    "backward-pcen-mel-stats": ("backward", dict(MEL, pcen={}), "stats"),
    "denoised-linear-grad": ("denoised_spectrogram_backward", DN_LIN, "grad"),
    "denoised-linear-stats": ("denoised_spectrogram_backward", DN_LIN, "stats"),
    "denoised-linear-profile": ("denoised_spectrogram_backward", DN_LIN, "profile"),
    "denoised-mel-grad": ("denoised_spectrogram_backward", DN_MEL, "grad"),
    "denoised-mel-stats": ("denoised_spectrogram_backward", DN_MEL, "stats"),
    "denoised-mel-profile": ("denoised_spectrogram_backward", DN_MEL, "profile"),
    "denoised-linear-grad-before-stats": ("denoised_spectrogram_backward", DN_LIN, "grad stats profile"),
    "denoised-linear-stats-before-profile": ("denoised_spectrogram_backward", DN_LIN, "stats profile"),
}


@pytest.mark.parametrize("name", list(TENSOR_REFUSALS))
def test_tensor_refusals_are_what_they_were(name):
    from torch._subclasses.fake_tensor import FakeTensorMode

    method, sp, wrong = TENSOR_REFUSALS[name]
    K = frontend.resolve_route(sp).K
    with FakeTensorMode():
        shapes = {"grad": (17, K), "stats": (6,), "profile": (K,)}
        t = {k: torch.empty(v[:-1] + (v[-1] - (k in wrong.split()),), device="cuda") for k, v in shapes.items()}
        pcm = torch.empty(4113, device="cuda")
        tensors = (t["grad"], t["stats"]) + ((t["profile"],) if method == "denoised_spectrogram_backward" else ())
        assert _raised(lambda: getattr(_fe(), method)(pcm, *tensors, sp)) == GOLDEN[name]


def test_the_static_size_checks_are_what_they_were():
    for nfft in (1, 8192):
        assert _raised(lambda: frontend.FrontEnd._check_nfft(nfft)) == GOLDEN[f"_check_nfft-{nfft}"]
    for nfft in (500, 16, 255, 8192):
        assert _raised(lambda: frontend.FrontEnd._check_nfft_backward(nfft)) == GOLDEN[f"_check_nfft_backward-{nfft}"]
    for nfft in (2, 500, 4096):
        frontend.FrontEnd._check_nfft(nfft)
    for nfft in (32, 512, 4096):
        frontend.FrontEnd._check_nfft_backward(nfft)


# ---------------------------------------------------------------------------------------------------------------- n_frames
@pytest.mark.parametrize("n,nfft,hop", [(0, 512, 256), (5, 512, 256), (255, 512, 256), (256, 512, 256), (48017, 512, 256), (1000, 1024, 300), (77, 2, 1),
                                        (0, 675, 100), (99, 675, 100), (100, 675, 100), (1000, 675, 100), (3001, 4095, 77)])
def test_n_frames_is_both_old_spellings(n, nfft, hop):
    assert frontend.n_frames(n, nfft, hop) == 1 + (n - (nfft & 1)) // hop
    if nfft % 2 == 0:
        assert frontend.n_frames(n, nfft, hop) == 1 + n // hop
    if n >= nfft & 1:  # librosa, center=True
        assert frontend.n_frames(n, nfft, hop) == 1 + (n + 2 * (nfft // 2) - nfft) // hop


# ---------------------------------------------------------------------------------------------------------------- the ops
LIN_ARGS = (48000, 512, 256, 16000.0, 0.01, 0.999)
MEL_ARGS = (48000, 512, 256, 64, 0.0, 24000.0, False, True, 0.01, 0.999)
PCEN_TAIL = (0.4, 0.98, 2.0, 0.5, 1e-6, 2.0**31, 0.01, 0.999)
OPS = {
    "spectrogram": (LIN_ARGS, 171),
    "mel_spectrogram": (MEL_ARGS, 64),
    "pcen_spectrogram": ((48000, 512, 256, 16000.0, 0, 0.0, 0.0, False, True) + PCEN_TAIL, 171),
    "pcen_spectrogram-mel": ((48000, 512, 256, 0.0, 64, 0.0, 24000.0, False, True) + PCEN_TAIL, 64),
    "denoised_spectrogram": ((48000, 512, 256, 16000.0, 0, 0.0, 0.0, False, True, 0.5, 0.01, 0.999), 171),
    "denoised_spectrogram-mel": ((48000, 512, 256, 0.0, 64, 0.0, 24000.0, False, True, 0.25, 0.01, 0.999), 64),
}
EXTRAS = {"denoised_spectrogram": 1}  # what a route saves for its backward beside the statistics: the denoised one its noise profile f32[K]


@pytest.mark.parametrize("n", [20000, 5, 0])
@pytest.mark.parametrize("name", list(OPS))
def test_fake_tensors_get_todays_shapes_and_dtypes(name, n):
    from torch._subclasses.fake_tensor import FakeTensorMode

    args, K = OPS[name]
    ops = torch.ops.orcai
    base = name.split("-")[0]
    with FakeTensorMode():
        pcm = torch.empty(n)
        spec = getattr(ops, base + "_wrt_pcm")(pcm, *args)
        plain = getattr(ops, base)(pcm, *args)
        spec2, stats, *extras = getattr(ops, base + "_with_stats")(pcm, *args)
        dpcm = getattr(ops, base + "_backward")(spec, pcm, stats, *extras, *args[:-2])
    T = 1 + n // 256
    assert tuple(spec.shape) == tuple(plain.shape) == tuple(spec2.shape) == (T, K) and tuple(stats.shape) == (6,) and tuple(dpcm.shape) == (n,)
    assert spec.dtype == plain.dtype == spec2.dtype == stats.dtype == dpcm.dtype == torch.float32
    assert [(tuple(e.shape), e.dtype) for e in extras] == [((K,), torch.float32)] * EXTRAS.get(base, 0)


def test_fake_gradient_through_the_generic_function():
    """The Autograd kernel on fake tensors: one node per route, whose backward gives pcm's shape and nothing for the other arguments."""
    from torch._subclasses.fake_tensor import FakeTensorMode

    for name, (args, K) in OPS.items():
        with FakeTensorMode():
            pcm = torch.empty(4113, requires_grad=True)
            spec = getattr(torch.ops.orcai, name.split("-")[0] + "_wrt_pcm")(pcm, *args)
            assert spec.requires_grad and type(spec.grad_fn).__name__ == "_WrtPcmFunctionBackward"
            (d,) = torch.autograd.grad(spec.sum(), pcm)
        assert tuple(spec.shape) == (17, K) and tuple(d.shape) == (4113,) and d.dtype == torch.float32


@pytest.mark.parametrize("base", ["pcen_spectrogram", "denoised_spectrogram"])
def test_a_forward_only_op_runs_and_its_backward_refuses(base):
    """The two plain ops with an autograd registration of their own: with a pcm that requires grad the forward gives today's shape, the backward raises
    the recorded text, which names the op's *_wrt_pcm twin."""
    from torch._subclasses.fake_tensor import FakeTensorMode

    args, K = OPS[base]
    with FakeTensorMode():
        pcm = torch.empty(4113, requires_grad=True)
        spec = getattr(torch.ops.orcai, base)(pcm, *args)
        assert tuple(spec.shape) == (17, K) and spec.requires_grad
        got = _raised(lambda: torch.autograd.grad(spec.sum(), pcm))
    assert got == GOLDEN["forward-only-" + base] and got[0] == "NotImplementedError" and f"orcai::{base}_wrt_pcm" in got[1]


def test_schemas_are_what_they_were():
    for name, schema in GOLDEN["schemas"].items():
        assert str(getattr(torch.ops.orcai, name).default._schema) == schema, name
    assert len(GOLDEN["schemas"]) == 16
