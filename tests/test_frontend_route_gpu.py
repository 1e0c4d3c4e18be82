"""The one backward behind the front end's four routes, on the GPU: FrontEnd.backward against the route's named method and against the gradient the
route's *_wrt_pcm op delivers, bit for bit (all three are the same C call), on the tuned size 512 and the general radix-2 size 1024, and the named
methods of the other routes still refusing.  On the denoised route FrontEnd.backward refuses as well: the named method, which also takes the profile,
is its only entry.  The parameters are the ones the gradient tests of each route use."""

import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import frontend_grad_ref as G  # noqa: E402
import mel_grad_ref as MG  # noqa: E402
import denoise_grad_ref as D  # noqa: E402
import pcen_grad_ref as R  # noqa: E402
import orcai_amd.torch_ops  # noqa: E402, F401  (registers the ops)
from orcai_amd import pcen  # noqa: E402

MEL_512, MEL_1024 = MG.CASES[0], MG.CASES[3]
# name -> (spectrogram parameter, its route's method): SP of test_frontend_grad_gpu.py and test_mel_grad_gpu.py, SP_LIN and SP_MEL of test_pcen_grad_gpu.py, and
# their 1024-point counterparts from the same case tables; the denoised rows are built by tests/denoise_grad_ref.py's parameter() at its table's two denoise
# quantiles -- the 512-point ones from its own LINEAR and MEL routes, the 1024-point ones, which that table lacks, from the routes the rows above use
CASES = {
    "linear-db-512": (G.parameter(512, 256, "a"), "spectrogram_backward"),
    "linear-db-1024": (G.parameter(1024, 512, "a"), "spectrogram_backward"),
    "mel-db-512": (MG.parameter(MEL_512, "a"), "mel_spectrogram_backward"),
    "mel-db-1024": (MG.parameter(MEL_1024, "a"), "mel_spectrogram_backward"),
    "linear-pcen-512": (R.parameter(R.CASES[0], "a"), "pcen_spectrogram_backward"),
    "linear-pcen-1024": (R.parameter(R.CASES[1], "a"), "pcen_spectrogram_backward"),
    "mel-pcen-512": (R.parameter(R.CASES[4], "a"), "pcen_spectrogram_backward"),
    "mel-pcen-1024": (R.parameter(("mel", MEL_1024), "a"), "pcen_spectrogram_backward"),
    "linear-denoised-512": (D.parameter(D.LINEAR[0], "a"), "denoised_spectrogram_backward"),
    "linear-denoised-1024": (D.parameter((1024, 512), "a", 0.25), "denoised_spectrogram_backward"),
    "mel-denoised-512": (D.parameter(D.MEL[0], "a", 0.25), "denoised_spectrogram_backward"),
    "mel-denoised-1024": (D.parameter(MEL_1024, "a"), "denoised_spectrogram_backward"),
}
REFUSING = {  # method -> what it raises on a parameter of another route, as before the routes shared one backward
    "spectrogram_backward": NotImplementedError,
    "mel_spectrogram_backward": lambda sp: NotImplementedError if sp.get("pcen") is not None else ValueError,
    "pcen_spectrogram_backward": ValueError,
    "denoised_spectrogram_backward": ValueError,
}


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(torch.int32), b.view(torch.int32))


def op_of(sp):
    """(the route's *_wrt_pcm op, its arguments after pcm) of a spectrogram parameter."""
    head = (sp["sampling_rate"], sp["nfft"], sp["n_overlap"])
    m = sp.get("mel")
    mel_args = (m["n_mels"], m["fmin"], m["fmax"], m["htk"], m["norm"] == "slaney") if m else None
    route = (0.0, *mel_args) if m else (float(sp["freq_range"][1]), 0, 0.0, 0.0, False, True)
    if sp.get("denoise") is not None:
        return torch.ops.orcai.denoised_spectrogram_wrt_pcm, (*head, *route, sp["denoise"]["quantile"], *sp["quantiles"])
    if sp.get("pcen") is not None:
        pc = pcen.pcen_config(sp)
        return torch.ops.orcai.pcen_spectrogram_wrt_pcm, (*head, *route, *(pc[k] for k in pcen.PCEN_KEYS), *sp["quantiles"])
    if m:
        return torch.ops.orcai.mel_spectrogram_wrt_pcm, (*head, *mel_args, *sp["quantiles"])
    return torch.ops.orcai.spectrogram_wrt_pcm, (*head, float(sp["freq_range"][1]), *sp["quantiles"])


@pytest.mark.parametrize("name", list(CASES))
def test_one_backward_serves_the_named_method_and_the_op(name):
    from orcai_amd.frontend import get_frontend

    sp, method = CASES[name]
    fe = get_frontend()
    hop = sp["n_overlap"]
    n = 16 * hop + 17  # 17 frames, the last one ragged
    pcm = torch.from_numpy(G.recording("a")[1000 : 1000 + n].copy()).cuda()
    denoised = sp.get("denoise") is not None
    spec, *saved = fe.make_spectrogram(pcm, sp, return_stats=True, return_profile=denoised)  # the statistics, and the profile of a denoised parameter
    assert spec.shape[0] == 17 and len(saved) == 1 + denoised
    grad = torch.randn(spec.shape, device="cuda", generator=torch.Generator("cuda").manual_seed(7))
    want = getattr(fe, method)(pcm, grad, *saved, sp)
    assert want.shape == (n,) and torch.isfinite(want).all() and float(want.abs().max()) > 0
    if denoised:
        with pytest.raises(NotImplementedError, match="denoised_spectrogram_backward"):
            fe.backward(pcm, grad, saved[0], sp)
    else:
        assert same_bits(fe.backward(pcm, grad, *saved, sp), want)
    op, args = op_of(sp)
    x = pcm.clone().requires_grad_()
    y = op(x, *args)
    assert same_bits(y.detach(), spec)
    (d,) = torch.autograd.grad(y, x, grad)
    assert same_bits(d, want)
    for other, error in REFUSING.items():
        if other != method:
            profile = (saved[0],) if other == "denoised_spectrogram_backward" else ()  # any tensor in the profile's place: the parameter is refused first
            with pytest.raises(NotImplementedError if denoised else error if isinstance(error, type) else error(sp)):
                getattr(fe, other)(pcm, grad, saved[0], *profile, sp)
