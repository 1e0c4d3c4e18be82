"""PyTorch custom ops in the ``orcai`` namespace: the front end, the model's forward (inference and training mode, with autograd w.r.t.
the weights and, through ``forward_wrt_input``, the input) and the whole-recording predict, so that the HIP path composes with a caller's
own loss, ``torch.optim`` and ``torch.compile``.  Every op calls the library through its C ABI only (orcai_amd/_native.py); each has a fake implementation, so shapes are
known without a GPU.

    torch.ops.orcai.spectrogram(pcm, sampling_rate, nfft, hop, freq_hi, q_lo, q_hi) -> f32[T, K]
    torch.ops.orcai.spectrogram_wrt_pcm(pcm, sampling_rate, nfft, hop, freq_hi, q_lo, q_hi) -> f32[T, K]
    torch.ops.orcai.mel_spectrogram(pcm, sampling_rate, nfft, hop, n_mels, fmin, fmax, htk, slaney_norm, q_lo, q_hi) -> f32[T, n_mels]
    torch.ops.orcai.mel_spectrogram_wrt_pcm(pcm, sampling_rate, nfft, hop, n_mels, fmin, fmax, htk, slaney_norm, q_lo, q_hi) -> f32[T, n_mels]
    torch.ops.orcai.pcen_spectrogram(pcm, sampling_rate, nfft, hop, freq_hi, n_mels, fmin, fmax, htk, slaney_norm, time_constant, gain, bias, power, eps,
                                     scale, q_lo, q_hi) -> f32[T, K]
    torch.ops.orcai.pcen_spectrogram_wrt_pcm(pcm, <the same arguments>) -> f32[T, K]
    torch.ops.orcai.denoised_spectrogram(pcm, sampling_rate, nfft, hop, freq_hi, n_mels, fmin, fmax, htk, slaney_norm, quantile, q_lo, q_hi) -> f32[T, K]
    torch.ops.orcai.denoised_spectrogram_wrt_pcm(pcm, <the same arguments>) -> f32[T, K]
    torch.ops.orcai.percentile(x f32[...], q) -> f32[len(q)]
    torch.ops.orcai.column_percentile(x f32[R, ...], q) -> f32[len(q), ...]   (per column of [R, C]: np.percentile(x, 100 q, axis=0, method="nearest"))
    torch.ops.orcai.segment_column_percentile(x f32[R, ...], q, segment_rows) -> f32[len(q), S, ...]   (the same inside every segment of segment_rows rows)
    torch.ops.orcai.segment_denoised_spectrogram(pcm, <denoised_spectrogram's arguments up to quantile>, segment, q_lo, q_hi) -> f32[T, K]   (forward only)
    torch.ops.orcai.resample(pcm, sr_in, sr_out) -> f32[ceil(n * sr_out / sr_in)]
    torch.ops.orcai.decode_pcm(frames uint8[nbytes], channels, channel, format) -> f32[n_frames]
    torch.ops.orcai.forward(x f32[B, H, W], weights, stats, config, training, dropout_seed) -> f32[B, steps, labels]
    torch.ops.orcai.forward_wrt_input(x f32[B, H, W], weights, stats, config, training, dropout_seed) -> f32[B, steps, labels]
    torch.ops.orcai.detect_wrt_input(x f32[B, H, W], weights, stats, config) -> f32[B, steps, labels]
    torch.ops.orcai.detect_wrt_params(x f32[B, H, W], weights, stats, config) -> f32[B, steps, labels]
    torch.ops.orcai.predict_spectrogram(spec f32[T, W], weights, stats, config) -> f32[n, steps, labels]
    torch.ops.orcai.detect_recording(spec f32[T, W], weights, stats, config, chunk) -> f32[T // tpo, labels]
    torch.ops.orcai.detect_recording_wrt_params(spec f32[T, W], weights, stats, config, chunk) -> f32[T // tpo, labels]

``weights`` / ``stats`` are the trainable variables and the BatchNorm moving statistics in ``variable_spec()`` order (Keras layouts);
``config`` is the JSON string ``model_config`` makes.  ``OrcaiModule`` wraps all of it as a ``torch.nn.Module``.

Training mode keeps the activations of its forward for the backward (``Trainer.forward_train`` / ``backward_from_probs``): per config and
device ONE step is open at a time, from the forward to its backward.  A second training forward while the autograd graph of the first is
still alive raises instead of overwriting what that graph's backward needs (``forward`` and ``forward_wrt_input`` share that step).

``forward`` differentiates w.r.t. the weights only and refuses an ``x`` that requires grad; ``forward_wrt_input`` is the same computation
whose training-mode backward also delivers dL/dx (``orcai_conv0_bn_bwd_dx``), for anything trainable or differentiable in front of the
detector.

The front end has four routes, one op each, all ``FrontEnd.make_spectrogram``: ``spectrogram`` (the bins 0 .. freq_hi in dB; ``orcai_make_spectrogram``),
``mel_spectrogram`` (the spectrogram parameter ``mel``: filterbank and dB fused into the STFT kernel, no frequency crop; ``orcai_make_mel_spectrogram``),
``pcen_spectrogram`` (the spectrogram parameter ``pcen``, orcai_amd/pcen.py; ``orcai_make_pcen_spectrogram``) and ``denoised_spectrogram`` (the spectrogram
parameter ``denoise``, orcai_amd/denoise.py; ``orcai_make_denoised_spectrogram``; its arguments are pcen_spectrogram's with ``quantile`` in place of the six PCEN
values).  The last two choose between the linear and the mel route themselves: n_mels = 0 is the bins 0 .. freq_hi and the mel arguments are ignored,
n_mels > 0 the mel bands and freq_hi is ignored.  These four are forward only: they have fake implementations and no gradient (``spectrogram`` and
``mel_spectrogram`` have NO autograd of their own; a backward through ``pcen_spectrogram`` or ``denoised_spectrogram`` raises NotImplementedError that names the
op's ``_wrt_pcm`` twin).  Each has a differentiable twin built by one wiring (``_register_wrt_pcm``): ``<op>_wrt_pcm`` is the same computation (same bits) whose
backward delivers dL/dpcm through the functional op ``orcai::<op>_backward(grad, pcm, stats, <the arguments but the quantiles>)`` -- ``FrontEnd.backward``, i.e.
``orcai_spectrogram_bwd``, ``orcai_mel_spectrogram_bwd`` or ``orcai_pcen_spectrogram_bwd`` -- from the six statistics ``orcai::<op>_with_stats`` returned beside
the forward.  The denoised route saves one tensor more: ``orcai::denoised_spectrogram_with_stats`` also returns the noise profile f32[K], and
``orcai::denoised_spectrogram_backward(grad, pcm, stats, profile, ...)`` is ``FrontEnd.denoised_spectrogram_backward`` (``orcai_denoised_spectrogram_bwd``).  The
normalisation statistics and the profile are held constant, the filterbank weights and the PCEN parameters get no gradient.  So the chain pcm -> spectrogram ->
snippets -> probabilities is differentiable down to the waveform.  ``WaveformFrontEnd``, ``MelWaveformFrontEnd``, ``PcenWaveformFrontEnd`` and
``DenoisedWaveformFrontEnd`` are resample + the route's ``_wrt_pcm`` op as a ``torch.nn.Module``; each refuses a parameter of another route, and
``waveform_front_end(spectrogram_parameter, native_rate)`` returns whichever of the first two the parameter asks for (a parameter whose ``pcen`` or ``denoise`` key
is set: NotImplementedError that names ``PcenWaveformFrontEnd`` or ``DenoisedWaveformFrontEnd``).
``resample`` is the polyphase resampler ``orcai predict`` runs on a recording that is not at the model's rate (``resample_device``,
same bits) with autograd w.r.t. the audio: it is linear, so its backward, the functional op ``orcai::resample_backward(grad, n_in, sr_in,
sr_out)``, is its adjoint with the same filter table (``orcai_resample_polyphase_bwd``; no float atomics, two runs give the same bits).
``decode_pcm`` is the stage in front of both: the data chunk of a WAV file, uploaded as the bytes of the file (``wavio.read_wav_raw``), -> the f32 samples
of one 0-based channel (``orcai_pcm_decode``; format 0 U8, 1 S16, 2 S24, 3 S32, 4 F32, 5 F64; the same bits as ``wavio.read_wav``).  Its input is integer
bytes, so it has no autograd.

``detect_wrt_input`` is the PREDICT-TIME network (BatchNorm with the moving statistics, no Dropout, nothing written to ``stats``) with
autograd w.r.t. ``x`` only: saliency, robustness probes, training something in front of the detector that will be deployed
(orcai_amd/eval_grad.py: one orcai_sepconv_dgrad per separable conv, no weight-gradient launcher).  Its forward keeps what the backward
reads in a tensor of its own, so any number of forwards may be alive at once.  ``forward`` / ``forward_wrt_input`` with training=False keep
refusing a backward: they run the fused inference path, which stores nothing.

``detect_wrt_params`` is the same predict-time network with autograd w.r.t. the weights as well (and ``x`` when it requires grad): fine-tuning with
BatchNorm FROZEN on its moving statistics and no Dropout -- the network ``orcai predict`` runs -- through ``OrcaiModule(model, frozen_bn=True)`` and any
``torch.optim``.  Its backward is the functional op ``orcai::detect_backward_params(grad, saved, weights, stats, config) -> (dx, dwflat)``
(``EvalGrad.backward(wgrad=True)``); ``stats`` get no gradient and are never written.  ``detect_wrt_input`` keeps returning no weight gradient.

``detect_recording`` is the function ``orcai predict`` reports -- every 50 %-overlapping snippet of ``spec`` through the predict-time network
(``predict_spectrogram``, the shared-trunk path) and the overlap average of their probabilities, rounded to f32 (tpo = 2 ** len(filters)) -- with autograd
w.r.t. ``spec``: its backward is the functional op ``orcai::detect_recording_bwd(grad, spec, weights, stats, config, chunk) -> dspec``
(``RecordingGrad.backward``: the detector recomputed in chunks of ``chunk`` snippets, so the stored activations do not grow with T).  Nothing but
``spec`` and the variables is saved.  ``detect_recording_wrt_params`` is the same function with autograd w.r.t. the weights as well (BatchNorm frozen on
``stats``); its backward is ``orcai::detect_recording_bwd_params(...) -> (dspec, dwflat)``.  Behind ``WaveformFrontEnd`` the gradient reaches the samples
at their native rate.

What does not exist: a weight gradient in eval mode on the f16 path, the CLI ``orcai train`` on the frozen network (its fused ``Trainer`` step is training mode),
a backward of ``orcai::predict_spectrogram`` itself (the shared-trunk kernels are not differentiated: ``detect_recording`` recomputes the snippets as a batch),
any input gradient on the f16 path (f32 models only); ``orcai::spectrogram`` and ``orcai::mel_spectrogram``
themselves have no backward, the mel filterbank weights and the three normalisation statistics get no gradient, and ``orcai::resample`` /
``orcai::resample_backward`` and the four front-end backwards have no second derivative.
"""

from __future__ import annotations

import functools
import json
import os
import weakref
from pathlib import Path

import torch

from orcai_amd.architectures import ResNet1DConv, ResNetLSTM

Tensor = torch.Tensor
CONFIG_KEYS = ("architecture", "input_shape", "filters", "kernel_size", "lstm_units", "num_labels", "dropout_rate")


# ---------------------------------------------------------------------------------------------------------------- configs
def model_config(model) -> str:
    """The ``config`` string of the ops for a ResNetLSTM / ResNet1DConv (canonical JSON of CONFIG_KEYS)."""
    precision = getattr(model, "precision", "f32")
    if precision != "f32":
        raise NotImplementedError(f"orcai torch ops: precision {precision!r} is not supported (f32 models only)")
    H, W = model.input_hw
    cfg = {"architecture": model.architecture, "input_shape": [H, W, 1], "filters": list(model.filters), "kernel_size": model.kernel_size,
           "lstm_units": model.lstm_units, "num_labels": model.num_labels, "dropout_rate": model.dropout_rate}
    return json.dumps(cfg, sort_keys=True)


@functools.lru_cache(maxsize=None)
def _parse(config: str) -> dict:
    cfg = json.loads(config)
    if cfg.get("precision", "f32") != "f32":
        raise NotImplementedError(f"orcai torch ops: precision {cfg['precision']!r} is not supported (f32 models only)")
    missing = [k for k in CONFIG_KEYS if k not in cfg and not (k == "lstm_units" and cfg.get("architecture") == "ResNet1DConv")]
    if missing:
        raise ValueError(f"orcai torch ops: config lacks {missing}")
    if cfg["architecture"] not in ("ResNetLSTM", "ResNet1DConv"):
        raise ValueError(f"orcai torch ops: unknown architecture {cfg['architecture']!r}")
    return cfg


def _build(config: str):
    cfg = _parse(config)
    args = (tuple(cfg["input_shape"]), cfg["num_labels"], list(cfg["filters"]), cfg["kernel_size"], cfg["dropout_rate"])
    if cfg["architecture"] == "ResNet1DConv":
        return ResNet1DConv(*args, seed=0)
    return ResNetLSTM(*args, lstm_units=cfg.get("lstm_units", 128), seed=0)


@functools.lru_cache(maxsize=None)
def _skeleton(config: str):
    """Host-only model of the config: shapes and variable_spec for the fake implementations (never touches a device)."""
    return _build(config)


def _out_steps(config: str) -> int:
    cfg = _parse(config)
    h = int(cfg["input_shape"][0])
    for _ in cfg["filters"]:
        h = -(-h // 2)
    return h


def _check_vars(config: str, weights, stats) -> None:
    lay = _skeleton(config).layout()
    ws, ss = [v[2] for v in lay.w.values()], [v[2] for v in lay.s.values()]
    got_w, got_s = [tuple(w.shape) for w in weights], [tuple(s.shape) for s in stats]
    if got_w != ws or got_s != ss:
        raise ValueError(f"orcai torch ops: weights / stats do not follow variable_spec() of the config ({len(ws)} weights, {len(ss)} statistics expected, "
                         f"got {len(got_w)} and {len(got_s)} with other shapes)")
    for t in list(weights) + list(stats):
        if t.dtype != torch.float32 or not t.is_cuda:
            raise ValueError("orcai torch ops: weights and stats must be f32 cuda tensors")


def _check_x(config: str, x: Tensor, who: str) -> None:
    H, W = (int(v) for v in _parse(config)["input_shape"][:2])
    if x.dim() != 3 or tuple(x.shape[1:]) != (H, W) or x.dtype != torch.float32:
        raise ValueError(f"{who}: x must be f32 [B, {H}, {W}], got {x.dtype} {tuple(x.shape)}")


def _check_pcm(pcm: Tensor, who: str) -> None:
    if pcm.dim() != 1 or pcm.dtype != torch.float32 or not pcm.is_cuda:
        raise ValueError(f"{who}: pcm must be a 1-d f32 cuda tensor")


def _probs_fake(x, weights, stats, config, training=None, dropout_seed=None):
    return x.new_empty((x.shape[0], _out_steps(config), _parse(config)["num_labels"]), dtype=torch.float32)


def _flat_grad_fake(grad, config):
    return grad.new_empty((_skeleton(config).layout().n_w,), dtype=torch.float32)


_LIB = torch.library.Library("orcai", "FRAGMENT")


def _register(name: str, schema: str, impl, fake, autograd) -> None:
    """An op on _LIB: torch.library.custom_op registers no autograd formula for an op that mutates an argument (orcai::forward's moving statistics) and
    none around an inner op, so these are defined with torch.library directly: the CUDA kernel (the CPU one refuses: its checks name the missing
    GPU), the fake implementation, and an Autograd kernel around a torch.autograd.Function that redispatches below autograd."""
    _LIB.define(name + schema)
    _LIB.impl(name, impl, "CUDA")
    _LIB.impl(name, impl, "CPU")
    torch.library.register_fake("orcai::" + name, fake, lib=_LIB)
    _LIB.impl(name, autograd, "Autograd")


# ---------------------------------------------------------------------------------------------------------------- per (config, device) state
class _Engine:
    """The model object of a config on one device: its inference workspaces, and the training engine (flat parameters, activations of the
    open training step)."""

    def __init__(self, config: str, device: torch.device):
        self.config, self.device = config, device
        self.model = _build(config)
        self._trainer = None
        self.token = None  # weakref to the autograd node's token of the open training step (None: no graph was built for it)

    def trainer(self):
        if self._trainer is None:
            from orcai_amd.training import Trainer

            class OpTrainer(Trainer):
                def broadcast_parameters(self, src: int = 0) -> None:  # the ops pass the weights in on every call: nothing to broadcast
                    return

            with torch.cuda.device(self.device):
                self._trainer = OpTrainer(self.model)
        return self._trainer

    def flat(self, weights, stats):
        lay = self.model.layout()
        return lay.flatten(dict(zip(lay.w_names + lay.s_names, [*weights, *stats])), self.device)

    def eval_forward(self, x: Tensor, weights, stats) -> Tensor:
        m = self.model
        H, W = m.input_hw
        B = int(x.shape[0])
        out = torch.empty((B, m.out_steps, m.num_labels), dtype=torch.float32, device=x.device)
        if B == 0:
            return out
        with m.bound(m.prepare_device(*self.flat(weights, stats))):
            m.forward_device(x.detach().contiguous().view(-1), H * W, B, out)
        return out

    def predict(self, spec: Tensor, weights, stats) -> Tensor:
        m = self.model
        with m.bound(m.prepare_device(*self.flat(weights, stats))):
            return m.predict_spectrogram(spec.detach().contiguous())

    def train_forward(self, x: Tensor, weights, stats, dropout_seed: int) -> Tensor:
        from orcai_amd.training import BN_MOMENTUM

        tr = self.trainer()
        if tr._pending is not None:
            if self.token is not None and self.token() is not None:
                raise RuntimeError("orcai::forward(training=True): the previous training forward of this model has not been backpropagated, and its autograd "
                                   "graph is still alive; its backward needs the activations this forward would overwrite.  Call backward on the "
                                   "previous result first.")
            tr.abandon_forward()  # its graph is gone (or was never built: no_grad): nobody will run its backward
        self.token = None
        m, P = self.model, tr.P
        H, W = m.input_hw
        torch.cat([w.detach().reshape(-1) for w in weights], out=P.w)
        torch.cat([s.detach().reshape(-1) for s in stats], out=P.stats_flat)
        tr.seed = int(dropout_seed)  # the masks Trainer(seed=dropout_seed) draws at its step 0 (the counter is never advanced here)
        probs = tr.forward_train(x.detach().contiguous().view(-1), H * W, int(x.shape[0]))
        P.ema_all(BN_MOMENTUM)  # batch statistics -> moving statistics, the kernel Trainer.apply runs
        for s, n in zip(stats, P.layout.s_names):
            s.copy_(P.stats[n].view(s.shape))
        return probs

    def backward(self, grad: Tensor, probs: Tensor, want_dx: bool = False):
        """The flat weight gradient of the open step; with want_dx also dL/dx f32[B, H, W] (one more launch: orcai_conv0_bn_bwd_dx)."""
        tr = self._trainer
        if tr is None or tr._pending is None:
            raise RuntimeError("orcai::forward backward: no training forward of this model is waiting for its backward (a backward runs once per forward)")
        self.token = None
        if not want_dx:
            tr.backward_from_probs(grad.contiguous(), probs)
            return tr.P.g.clone()
        H, W = self.model.input_hw
        dx = torch.empty((int(tr._pending.shape[0]), H, W), dtype=torch.float32, device=grad.device)
        if probs.data_ptr() != tr._pending.data_ptr() and probs.shape == tr._pending.shape and torch.equal(probs, tr._pending):
            probs = tr._pending  # a copy of the open step's probabilities (torch.library.opcheck clones the arguments) names the same step
        tr.backward_from_probs(grad.contiguous(), probs, dx=dx)
        return tr.P.g.clone(), dx


_ENGINES: dict = {}


def _key(config: str, device: torch.device):
    return config, device.index if device.index is not None else torch.cuda.current_device()


def _engine(config: str, device: torch.device) -> _Engine:
    if device.type != "cuda":
        raise RuntimeError(f"orcai torch ops run on a ROCm GPU only (got a tensor on {device}); there is no CPU fallback")
    key = _key(config, device)
    eng = _ENGINES.get(key)
    if eng is None:
        _parse(config)
        eng = _ENGINES[key] = _Engine(config, torch.device("cuda", key[1]))
    return eng


# ---------------------------------------------------------------------------------------------------------------- orcai::spectrogram
def _bins(sampling_rate: int, nfft: int, freq_hi: float) -> int:
    from orcai_amd.frontend import crop_indices, fft_frequencies

    return crop_indices(fft_frequencies(sampling_rate, nfft), [0, freq_hi])[1]


def _spec_fake(pcm, nfft, hop, K):
    from orcai_amd.frontend import n_frames

    return pcm.new_empty((n_frames(pcm.shape[0], nfft, hop), K), dtype=torch.float32)


def _front_end_impl(who: str, parameter, return_stats: bool = False, return_profile: bool = False):
    """The kernel of a front-end op (pcm, *args): FrontEnd.make_spectrogram with the spectrogram parameter that `parameter` makes of args."""

    def impl(pcm, *args):
        from orcai_amd.frontend import get_frontend

        _check_pcm(pcm, who)
        with torch.cuda.device(pcm.device):
            return get_frontend(pcm.device).make_spectrogram(pcm.detach(), parameter(*args), return_stats=return_stats, return_profile=return_profile)

    return impl


def _spectrogram_parameter(sampling_rate, nfft, hop, freq_hi, q_lo=0.0, q_hi=1.0) -> dict:
    return {"sampling_rate": sampling_rate, "nfft": nfft, "n_overlap": hop, "freq_range": [0, freq_hi], "quantiles": [q_lo, q_hi]}


@torch.library.custom_op("orcai::spectrogram", mutates_args=())
def spectrogram(pcm: Tensor, sampling_rate: int, nfft: int, hop: int, freq_hi: float, q_lo: float, q_hi: float) -> Tensor:
    """FrontEnd.make_spectrogram of f32 pcm[n] (already at sampling_rate): frequencies 0 .. freq_hi, quantile normalisation (q_lo, q_hi)."""
    from orcai_amd.frontend import get_frontend

    _check_pcm(pcm, "orcai::spectrogram")
    with torch.cuda.device(pcm.device):
        return get_frontend(pcm.device).make_spectrogram(pcm, _spectrogram_parameter(sampling_rate, nfft, hop, freq_hi, q_lo, q_hi))


@spectrogram.register_fake
def _spectrogram_fake(pcm, sampling_rate, nfft, hop, freq_hi, q_lo, q_hi):
    return _spec_fake(pcm, nfft, hop, _bins(sampling_rate, nfft, freq_hi))


# ---------------------------------------------------------------------------------------------------------------- orcai::mel_spectrogram
# The mel route of the front end (spectrogram parameter "mel"; orcai_make_mel_spectrogram): no frequency crop, K = n_mels.  This op has NO autograd
# formula and a pcm that requires grad gets PyTorch's own refusal; orcai::mel_spectrogram_wrt_pcm below is the differentiable one.
def _mel_parameter(sampling_rate, nfft, hop, n_mels, fmin, fmax, htk, slaney_norm, q_lo=0.0, q_hi=1.0) -> dict:
    return {"sampling_rate": sampling_rate, "nfft": nfft, "n_overlap": hop, "freq_range": [fmin, fmax], "quantiles": [q_lo, q_hi],
            "mel": {"n_mels": n_mels, "fmin": fmin, "fmax": fmax, "htk": htk, "norm": "slaney" if slaney_norm else None}}


@torch.library.custom_op("orcai::mel_spectrogram", mutates_args=())
def mel_spectrogram(pcm: Tensor, sampling_rate: int, nfft: int, hop: int, n_mels: int, fmin: float, fmax: float, htk: bool, slaney_norm: bool,
                    q_lo: float, q_hi: float) -> Tensor:
    """FrontEnd.make_spectrogram of f32 pcm[n] (already at sampling_rate) with the mel parameter {n_mels, fmin, fmax, htk, norm = "slaney" if
    slaney_norm else null}: f32[T, n_mels] in [0, 1].  nfft a power of two from 128 to 4096."""
    from orcai_amd.frontend import get_frontend

    _check_pcm(pcm, "orcai::mel_spectrogram")
    with torch.cuda.device(pcm.device):
        return get_frontend(pcm.device).make_spectrogram(pcm, _mel_parameter(sampling_rate, nfft, hop, n_mels, fmin, fmax, htk, slaney_norm, q_lo, q_hi))


@mel_spectrogram.register_fake
def _mel_spectrogram_fake(pcm, sampling_rate, nfft, hop, n_mels, fmin, fmax, htk, slaney_norm, q_lo, q_hi):
    return _spec_fake(pcm, nfft, hop, n_mels)


# ---------------------------------------------------------------------------------------------------------------- orcai::pcen_spectrogram, orcai::denoised_spectrogram
# The front end with the spectrogram parameter "pcen" (orcai_make_pcen_spectrogram) or "denoise" (orcai_make_denoised_spectrogram) set, beside the linear
# and the mel op.  Both choose their route by n_mels: 0 is the bins 0 .. freq_hi and the mel arguments are ignored, n_mels > 0 the mel bands and freq_hi
# is ignored.  Forward only: each op HAS an autograd registration (_register_forward_only), whose backward raises a NotImplementedError that names
# orcai::<op>_wrt_pcm (further down), the differentiable one.
def _linear_or_mel_parameter(sampling_rate, nfft, hop, freq_hi, n_mels, fmin, fmax, htk, slaney_norm, q_lo, q_hi) -> dict:
    if n_mels > 0:
        return _mel_parameter(sampling_rate, nfft, hop, n_mels, fmin, fmax, htk, slaney_norm, q_lo, q_hi)
    return _spectrogram_parameter(sampling_rate, nfft, hop, freq_hi, q_lo, q_hi)


def _pcen_parameter(sampling_rate, nfft, hop, freq_hi, n_mels, fmin, fmax, htk, slaney_norm, time_constant, gain, bias, power, eps, scale, q_lo=0.0, q_hi=1.0) -> dict:
    sp = _linear_or_mel_parameter(sampling_rate, nfft, hop, freq_hi, n_mels, fmin, fmax, htk, slaney_norm, q_lo, q_hi)
    sp["pcen"] = {"time_constant": time_constant, "gain": gain, "bias": bias, "power": power, "eps": eps, "scale": scale}
    return sp


def _denoised_parameter(sampling_rate, nfft, hop, freq_hi, n_mels, fmin, fmax, htk, slaney_norm, quantile, q_lo=0.0, q_hi=1.0, segment=None) -> dict:
    """The parameter of orcai::denoised_spectrogram and its *_wrt_pcm family, whose schemas have no segment: the global floor.  segment exists so that a
    caller who builds the differentiable ops' parameter from a parameter file cannot drop the key silently: set, it is refused here."""
    sp = _linear_or_mel_parameter(sampling_rate, nfft, hop, freq_hi, n_mels, fmin, fmax, htk, slaney_norm, q_lo, q_hi)
    sp["denoise"] = {"quantile": quantile}
    if segment is not None:
        from orcai_amd import denoise

        denoise.no_segment_gradient(dict(sp, denoise={"quantile": quantile, "segment": segment}), "orcai::denoised_spectrogram_wrt_pcm")
    return sp


def _segment_denoised_parameter(sampling_rate, nfft, hop, freq_hi, n_mels, fmin, fmax, htk, slaney_norm, quantile, segment, q_lo=0.0, q_hi=1.0) -> dict:
    sp = _linear_or_mel_parameter(sampling_rate, nfft, hop, freq_hi, n_mels, fmin, fmax, htk, slaney_norm, q_lo, q_hi)
    sp["denoise"] = {"quantile": quantile, "segment": segment}
    return sp


def _linear_or_mel_fake(pcm, sampling_rate, nfft, hop, freq_hi, n_mels, *rest):
    return _spec_fake(pcm, nfft, hop, n_mels if n_mels > 0 else _bins(sampling_rate, nfft, freq_hi))


class _ForwardOnlyFunction(torch.autograd.Function):
    """forward(pcm, base, *args) of orcai::<base>(pcm, *args), an op that runs under autograd and has no gradient."""

    @staticmethod
    def forward(ctx, pcm, base, *args):
        ctx.base = base
        with torch._C._AutoDispatchBelowAutograd():
            return getattr(torch.ops.orcai, base)(pcm, *args)

    @staticmethod
    def backward(ctx, grad):
        if ctx.base == "segment_denoised_spectrogram":
            raise NotImplementedError("orcai::segment_denoised_spectrogram has no gradient: the time-varying floor (denoise.segment) is forward only, and "
                                      "orcai::denoised_spectrogram_wrt_pcm differentiates the global floor, another forward")
        raise NotImplementedError(f"orcai::{ctx.base} has no gradient (as orcai::spectrogram and orcai::mel_spectrogram have none): "
                                  f"orcai::{ctx.base}_wrt_pcm is the same computation with the gradient w.r.t. pcm")


def _register_forward_only(base: str, schema: str, parameter) -> None:
    """orcai::<base>(pcm, <schema>), one of the two ops above."""

    def autograd(pcm, *args):
        if torch.is_grad_enabled() and pcm.requires_grad:
            return _ForwardOnlyFunction.apply(pcm, base, *args)
        with torch._C._AutoDispatchBelowAutograd():
            return getattr(torch.ops.orcai, base)(pcm, *args)

    _register(base, f"(Tensor pcm, {schema}) -> Tensor", _front_end_impl("orcai::" + base, parameter), _linear_or_mel_fake, autograd)


_ROUTE_ARGUMENTS = "SymInt sampling_rate, SymInt nfft, SymInt hop, float freq_hi, SymInt n_mels, float fmin, float fmax, bool htk, bool slaney_norm, "
_PCEN_ARGUMENTS = _ROUTE_ARGUMENTS + "float time_constant, float gain, float bias, float power, float eps, float scale, float q_lo, float q_hi"
_DENOISED_ARGUMENTS = _ROUTE_ARGUMENTS + "float quantile, float q_lo, float q_hi"
_register_forward_only("pcen_spectrogram", _PCEN_ARGUMENTS, _pcen_parameter)
_register_forward_only("denoised_spectrogram", _DENOISED_ARGUMENTS, _denoised_parameter)
# the time-varying floor (denoise.segment, seconds): forward only and, unlike the two above, with no *_wrt_pcm twin yet
_SEGMENT_DENOISED_ARGUMENTS = _ROUTE_ARGUMENTS + "float quantile, float segment, float q_lo, float q_hi"
_register_forward_only("segment_denoised_spectrogram", _SEGMENT_DENOISED_ARGUMENTS, _segment_denoised_parameter)


def pcen_spectrogram(pcm: Tensor, sampling_rate: int, nfft: int, hop: int, freq_hi: float, n_mels: int, fmin: float, fmax: float, htk: bool, slaney_norm: bool,
                     time_constant: float, gain: float, bias: float, power: float, eps: float, scale: float, q_lo: float, q_hi: float) -> Tensor:
    """FrontEnd.make_spectrogram of f32 pcm[n] (already at sampling_rate) with the pcen parameter {time_constant, gain, bias, power, eps, scale}: n_mels = 0
    on the bins 0 .. freq_hi, n_mels > 0 on the mel bands {n_mels, fmin, fmax, htk, norm}.  f32[T, K] in [0, 1]; nfft a power of two.  No gradient:
    pcen_spectrogram_wrt_pcm has it."""
    return torch.ops.orcai.pcen_spectrogram(pcm, sampling_rate, nfft, hop, freq_hi, n_mels, fmin, fmax, htk, slaney_norm, time_constant, gain, bias, power, eps, scale,
                                            q_lo, q_hi)


def denoised_spectrogram(pcm: Tensor, sampling_rate: int, nfft: int, hop: int, freq_hi: float, n_mels: int, fmin: float, fmax: float, htk: bool, slaney_norm: bool,
                         quantile: float, q_lo: float, q_hi: float) -> Tensor:
    """FrontEnd.make_spectrogram of f32 pcm[n] (already at sampling_rate) with the denoise parameter {quantile}: n_mels = 0 on the bins 0 .. freq_hi,
    n_mels > 0 on the mel bands {n_mels, fmin, fmax, htk, norm}.  f32[T, K] in [0, 1].  No gradient: denoised_spectrogram_wrt_pcm has it."""
    return torch.ops.orcai.denoised_spectrogram(pcm, sampling_rate, nfft, hop, freq_hi, n_mels, fmin, fmax, htk, slaney_norm, quantile, q_lo, q_hi)


def segment_denoised_spectrogram(pcm: Tensor, sampling_rate: int, nfft: int, hop: int, freq_hi: float, n_mels: int, fmin: float, fmax: float, htk: bool,
                                 slaney_norm: bool, quantile: float, segment: float, q_lo: float, q_hi: float) -> Tensor:
    """FrontEnd.make_spectrogram of f32 pcm[n] (already at sampling_rate) with the denoise parameter {quantile, segment}: the per-channel floor taken per
    segment of `segment` seconds and interpolated between the segment centres (orcai_make_segment_denoised_spectrogram).  f32[T, K] in [0, 1].  No gradient."""
    return torch.ops.orcai.segment_denoised_spectrogram(pcm, sampling_rate, nfft, hop, freq_hi, n_mels, fmin, fmax, htk, slaney_norm, quantile, segment, q_lo, q_hi)


# ---------------------------------------------------------------------------------------------------------------- orcai::percentile
# FrontEnd.percentiles: exact nearest-rank percentiles of any contiguous f32 tensor, taken flat, by the radix select (orcai_quantile_select_radix).
# Forward only, like the front-end ops: an order statistic is held constant everywhere else in this package, so its backward raises.
def _percentile_impl(x, q):
    from orcai_amd.frontend import get_frontend

    if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32):
        raise TypeError(f"orcai::percentile: x must be a float32 CUDA tensor, got {getattr(x, 'dtype', None)} on {getattr(x, 'device', None)}")
    with torch.cuda.device(x.device):
        return get_frontend(x.device).percentiles(x.detach(), q)


def _percentile_fake(x, q):
    return x.new_empty((len(q),), dtype=torch.float32)


class _PercentileFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, q):
        with torch._C._AutoDispatchBelowAutograd():
            return torch.ops.orcai.percentile(x, q)

    @staticmethod
    def backward(ctx, grad):
        raise NotImplementedError("orcai::percentile has no gradient: an order statistic is a constant of every backward in this package "
                                  "(the quantile bounds of the front ends are held constant too)")


def _percentile_autograd(x, q):
    if torch.is_grad_enabled() and x.requires_grad:
        return _PercentileFunction.apply(x, q)
    with torch._C._AutoDispatchBelowAutograd():
        return torch.ops.orcai.percentile(x, q)


_register("percentile", "(Tensor x, float[] q) -> Tensor", _percentile_impl, _percentile_fake, _percentile_autograd)


def percentile(x: Tensor, q: list[float]) -> Tensor:
    """f32[len(q)] on x's device: element i is what ``np.percentile(x, 100 * q[i], method="nearest")`` returns for the float32 values of x, exactly;
    x any contiguous f32 CUDA tensor, q fractions in [0, 1].  No host synchronisation, no gradient."""
    return torch.ops.orcai.percentile(x, [float(v) for v in q])


# ---------------------------------------------------------------------------------------------------------------- orcai::column_percentile
# FrontEnd.percentiles(dim=0): the same exact nearest-rank percentiles per column of x read as [R, C] (C the product of the dimensions after the first, at
# most 4096), by the segmented radix select (orcai_column_select), one call per q.  Forward only, for the reason orcai::percentile is.
def _column_percentile_impl(x, q):
    from orcai_amd.frontend import get_frontend

    if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32):
        raise TypeError(f"orcai::column_percentile: x must be a float32 CUDA tensor, got {getattr(x, 'dtype', None)} on {getattr(x, 'device', None)}")
    with torch.cuda.device(x.device):
        return get_frontend(x.device).percentiles(x.detach(), q, dim=0)


def _column_percentile_fake(x, q):
    return x.new_empty((len(q), *x.shape[1:]), dtype=torch.float32)


class _ColumnPercentileFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, q):
        with torch._C._AutoDispatchBelowAutograd():
            return torch.ops.orcai.column_percentile(x, q)

    @staticmethod
    def backward(ctx, grad):
        raise NotImplementedError("orcai::column_percentile has no gradient: an order statistic is a constant of every backward in this package "
                                  "(the quantile bounds of the front ends are held constant too)")


def _column_percentile_autograd(x, q):
    if torch.is_grad_enabled() and x.requires_grad:
        return _ColumnPercentileFunction.apply(x, q)
    with torch._C._AutoDispatchBelowAutograd():
        return torch.ops.orcai.column_percentile(x, q)


_register("column_percentile", "(Tensor x, float[] q) -> Tensor", _column_percentile_impl, _column_percentile_fake, _column_percentile_autograd)


def column_percentile(x: Tensor, q: list[float]) -> Tensor:
    """f32[len(q), *x.shape[1:]] on x's device: what ``np.percentile(x, 100 * q, axis=0, method="nearest")`` returns for the float32 values of x, exactly;
    x a contiguous f32 CUDA tensor of at least two dimensions with at most 4096 columns, q fractions in [0, 1].  No host synchronisation, no gradient."""
    return torch.ops.orcai.column_percentile(x, [float(v) for v in q])


# ---------------------------------------------------------------------------------------------------------------- orcai::segment_column_percentile
# FrontEnd.percentiles(dim=0, segment_rows=W): the column percentiles inside every segment of W rows (S = max(1, R // W) segments, the last one taking the
# remainder), by orcai_segment_column_select, one call per q.  Forward only, for the reason orcai::percentile is.
def _segment_column_percentile_impl(x, q, segment_rows):
    from orcai_amd.frontend import get_frontend

    if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32):
        raise TypeError(f"orcai::segment_column_percentile: x must be a float32 CUDA tensor, got {getattr(x, 'dtype', None)} on {getattr(x, 'device', None)}")
    with torch.cuda.device(x.device):
        return get_frontend(x.device).percentiles(x.detach(), list(q), dim=0, segment_rows=segment_rows)


def _segment_column_percentile_fake(x, q, segment_rows):
    S = x.shape[0] // segment_rows
    return x.new_empty((len(q), S if S > 1 else 1, *x.shape[1:]), dtype=torch.float32)


class _SegmentColumnPercentileFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, q, segment_rows):
        with torch._C._AutoDispatchBelowAutograd():
            return torch.ops.orcai.segment_column_percentile(x, q, segment_rows)

    @staticmethod
    def backward(ctx, grad):
        raise NotImplementedError("orcai::segment_column_percentile has no gradient: an order statistic is a constant of every backward in this package "
                                  "(the quantile bounds of the front ends are held constant too)")


def _segment_column_percentile_autograd(x, q, segment_rows):
    if torch.is_grad_enabled() and x.requires_grad:
        return _SegmentColumnPercentileFunction.apply(x, q, segment_rows)
    with torch._C._AutoDispatchBelowAutograd():
        return torch.ops.orcai.segment_column_percentile(x, q, segment_rows)


_register("segment_column_percentile", "(Tensor x, float[] q, SymInt segment_rows) -> Tensor", _segment_column_percentile_impl, _segment_column_percentile_fake,
          _segment_column_percentile_autograd)


def segment_column_percentile(x: Tensor, q: list[float], segment_rows: int) -> Tensor:
    """f32[len(q), S, *x.shape[1:]] on x's device: for every segment of segment_rows rows of x (S = max(1, R // segment_rows), the last one taking the
    remainder) what ``np.percentile(segment, 100 * q, axis=0, method="nearest")`` returns, exactly.  No host synchronisation, no gradient."""
    return torch.ops.orcai.segment_column_percentile(x, [float(v) for v in q], int(segment_rows))


# ---------------------------------------------------------------------------------------------------------------- orcai::forward, orcai::forward_wrt_input
# forward_wrt_input is orcai::forward with the gradient w.r.t. the snippets as well: for something trainable or differentiable IN FRONT of the
# detector (a learnable gain / equaliser / denoiser on the spectrogram, differentiable augmentation, adversarial or gradient-penalty training,
# saliency of a training loss).  Its own op, because orcai::forward's refusal of x.requires_grad is part of that op's contract; the CUDA / CPU /
# fake implementations are shared, and so are the per-(config, device) engine and its one open step.  The backwards are the functional ops
# orcai::forward_backward and orcai::forward_wrt_input_backward.  Training mode only: the eval-mode forward (moving statistics) has no backward.
_FORWARD_SCHEMA = "(Tensor x, Tensor[] weights, Tensor(a!)[] stats, str config, bool training, SymInt dropout_seed) -> Tensor"


def forward(x: Tensor, weights: list[Tensor], stats: list[Tensor], config: str, training: bool, dropout_seed: int) -> Tensor:
    """The model on snippets x[B][H][W].  training=False: the inference kernels on weights prepared on the device (BatchNorm with the moving
    statistics).  training=True: the training-mode forward (batch statistics, Dropout drawn from dropout_seed); the moving statistics in
    `stats` are updated in place (momentum 0.99) and the step stays open for the backward."""
    return torch.ops.orcai.forward(x, weights, stats, config, training, dropout_seed)


def forward_wrt_input(x: Tensor, weights: list[Tensor], stats: list[Tensor], config: str, training: bool, dropout_seed: int) -> Tensor:
    """orcai::forward whose training-mode backward also returns dL/dx (f32 [B, H, W]) when x requires grad."""
    return torch.ops.orcai.forward_wrt_input(x, weights, stats, config, training, dropout_seed)


def _forward_impl(x, weights, stats, config, training, dropout_seed):
    _check_x(config, x, "orcai::forward")
    _check_vars(config, weights, stats)
    eng = _engine(config, x.device)
    with torch.cuda.device(x.device):
        if training:
            if x.shape[0] == 0:
                raise ValueError("orcai::forward(training=True): empty batch")
            return eng.train_forward(x, weights, stats, dropout_seed)
        return eng.eval_forward(x, weights, stats)


@torch.library.custom_op("orcai::forward_backward", mutates_args=())
def forward_backward(grad: Tensor, probs: Tensor, config: str) -> Tensor:
    """The backward of the open training forward of `config` from dL/dprobs: the flat weight gradient (variable_spec order, no L2 term)."""
    with torch.cuda.device(grad.device):
        return _engine(config, grad.device).backward(grad, probs)


@forward_backward.register_fake
def _forward_backward_fake(grad, probs, config):
    return _flat_grad_fake(grad, config)


@torch.library.custom_op("orcai::forward_wrt_input_backward", mutates_args=())
def forward_wrt_input_backward(grad: Tensor, probs: Tensor, config: str) -> tuple[Tensor, Tensor]:
    """The backward of the open training forward of `config` from dL/dprobs: the flat weight gradient (as orcai::forward_backward) and the
    gradient w.r.t. the snippets, f32 [B, H, W] (orcai_conv0_bn_bwd_dx behind the entry conv's weight gradient)."""
    with torch.cuda.device(grad.device):
        return _engine(config, grad.device).backward(grad, probs, want_dx=True)


@forward_wrt_input_backward.register_fake
def _forward_wrt_input_backward_fake(grad, probs, config):
    H, W = (int(v) for v in _parse(config)["input_shape"][:2])
    return _flat_grad_fake(grad, config), grad.new_empty((probs.shape[0], H, W), dtype=torch.float32)


class _GraphToken:
    """Lives on the autograd node of a training forward: while it does, that forward's backward may still come."""


def _training_autograd(name: str, backward_name: str, returns_dx: bool, eval_refusal: str, x_refusal: str | None = None):
    """The Autograd kernel of orcai::<name>: a Function whose backward is orcai::<backward_name> (the flat weight gradient, with returns_dx also dL/dx).
    eval_refusal: what a backward through training=False raises; x_refusal: what an x that requires grad raises (None: it gets dx)."""

    class Function(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x, stats, config, training, dropout_seed, *weights):
            with torch._C._AutoDispatchBelowAutograd():
                out = getattr(torch.ops.orcai, name)(x, list(weights), stats, config, training, dropout_seed)
            ctx.training, ctx.config = bool(training), config
            ctx.save_for_backward(out)
            if training and not torch._subclasses.fake_tensor.is_fake(out):
                ctx.token = _GraphToken()
                eng = _ENGINES.get(_key(config, out.device))
                if eng is not None:
                    eng.token = weakref.ref(ctx.token)
            return out

        @staticmethod
        def backward(ctx, grad):
            if not ctx.training:
                raise RuntimeError(eval_refusal)
            (probs,) = ctx.saved_tensors
            res = getattr(torch.ops.orcai, backward_name)(grad, probs, ctx.config)
            flat, dx = res if returns_dx else (res, None)
            need = ctx.needs_input_grad
            wgrads = [g if n else None for g, n in zip(_skeleton(ctx.config).layout().split_w(flat), need[5:])]
            return (dx if need[0] else None, None, None, None, None, *wgrads)

    Function.__name__ = Function.__qualname__ = "_" + "".join(part.capitalize() for part in name.split("_")) + "Function"  # the node's name in traces

    def autograd(x, weights, stats, config, training, dropout_seed):
        if torch.is_grad_enabled():
            if x.requires_grad and x_refusal is not None:
                raise NotImplementedError(x_refusal)
            if x.requires_grad or any(w.requires_grad for w in weights):
                return Function.apply(x, stats, config, training, dropout_seed, *weights)
        with torch._C._AutoDispatchBelowAutograd():
            return getattr(torch.ops.orcai, name)(x, weights, stats, config, training, dropout_seed)

    return autograd


_register("forward", _FORWARD_SCHEMA, _forward_impl, _probs_fake, _training_autograd(
    "forward", "forward_backward", False,
    "orcai::forward(training=False) has no backward (BatchNorm with moving statistics); run the forward with training=True to train",
    "orcai::forward computes no gradient w.r.t. its input x (only w.r.t. the weights): pass x with requires_grad=False"))
_register("forward_wrt_input", _FORWARD_SCHEMA, _forward_impl, _probs_fake, _training_autograd(
    "forward_wrt_input", "forward_wrt_input_backward", True,
    "orcai::forward_wrt_input(training=False) has no backward (BatchNorm with moving statistics): the gradient w.r.t. the "
    "input, too, needs the forward with training=True"))


# ---------------------------------------------------------------------------------------------------------------- orcai::*_wrt_pcm
# The four front-end ops with the gradient w.r.t. the audio, for anything trainable or differentiable in the WAVEFORM domain in front of the detector
# (a learnable band-pass or denoiser on the hydrophone signal, adversarial or gradient-penalty robustness on audio, saliency of a detection in the
# recording).  Each is its own op, as forward_wrt_input is: the schema and behaviour of orcai::<base> stay what they are.  One wiring serves the four
# routes (_register_wrt_pcm): orcai::<base>_wrt_pcm runs the same launch sequence as orcai::<base> (same bits); with a pcm that requires grad its
# Autograd kernel runs orcai::<base>_with_stats instead, which also returns the run's six statistics (orcai_frontend_stats_dev) -- and, on the denoised
# route, the noise profile f32[K] -- and its backward is the functional op orcai::<base>_backward (FrontEnd.backward; FrontEnd.denoised_spectrogram_backward
# on the denoised route), which holds what the forward saved constant (include/orcai_hip.h).
class _WrtPcmFunction(torch.autograd.Function):
    """forward(pcm, base, check, *args) of orcai::<base>_wrt_pcm(pcm, *args); check(*args), when given, refuses before the forward what the backward
    could not differentiate.  What orcai::<base>_with_stats returns after the spectrogram is saved beside pcm and goes to the backward op in that order,
    followed by all of args but the two quantiles."""

    @staticmethod
    def forward(ctx, pcm, base, check, *args):
        if check is not None:
            check(*args)
        with torch._C._AutoDispatchBelowAutograd():
            spec, stats, *extras = getattr(torch.ops.orcai, base + "_with_stats")(pcm, *args)
        ctx.backward_op, ctx.args, ctx.n_inputs = getattr(torch.ops.orcai, base + "_backward"), args[:-2], 2 + len(args)
        ctx.save_for_backward(pcm, stats, *extras)
        return spec

    @staticmethod
    def backward(ctx, grad):
        pcm, stats, *extras = ctx.saved_tensors
        return (ctx.backward_op(grad, pcm, stats, *extras, *ctx.args),) + (None,) * ctx.n_inputs


_FRONT_END_OPS: dict = {}  # name -> CustomOpDef of the inner ops (torch refers to a definition weakly: dropping it would unregister the op)


def _register_wrt_pcm(base: str, schema: str, parameter, fake, check=None, profile: bool = False) -> None:
    """orcai::<base>_wrt_pcm, orcai::<base>_with_stats and orcai::<base>_backward.  schema: the arguments of orcai::<base> after pcm, the two
    quantiles last; parameter: the spectrogram parameter of those arguments (the quantiles optional); fake: orcai::<base>'s fake implementation.
    profile: the route's backward also reads the noise profile f32[K] -- orcai::<base>_with_stats returns it third, orcai::<base>_backward takes it
    after stats."""
    no_quantiles = schema.removesuffix(", float q_lo, float q_hi")
    assert no_quantiles != schema, schema

    def with_stats_fake(pcm, *args):
        spec = fake(pcm, *args)
        shapes = ((6,), (spec.shape[1],)) if profile else ((6,),)
        return (spec, *(pcm.new_empty(shape, dtype=torch.float32) for shape in shapes))

    def backward_impl(grad, pcm, stats, *rest):
        from orcai_amd.frontend import get_frontend

        _check_pcm(pcm, f"orcai::{base}_backward")
        with torch.cuda.device(pcm.device):
            fe = get_frontend(pcm.device)
            if profile:
                return fe.denoised_spectrogram_backward(pcm.detach(), grad.contiguous(), stats, rest[0], parameter(*rest[1:]))
            return fe.backward(pcm.detach(), grad.contiguous(), stats, parameter(*rest), who=base + "_backward")

    def autograd(pcm, *args):
        if torch.is_grad_enabled() and pcm.requires_grad:
            return _WrtPcmFunction.apply(pcm, base, check, *args)
        with torch._C._AutoDispatchBelowAutograd():
            return getattr(torch.ops.orcai, base + "_wrt_pcm")(pcm, *args)

    saved, returns = ("Tensor stats, Tensor profile", "(Tensor, Tensor, Tensor)") if profile else ("Tensor stats", "(Tensor, Tensor)")
    with_stats = torch.library.custom_op(f"orcai::{base}_with_stats", _front_end_impl(f"orcai::{base}_with_stats", parameter, return_stats=True, return_profile=profile),
                                         mutates_args=(), schema=f"(Tensor pcm, {schema}) -> {returns}")
    with_stats.register_fake(with_stats_fake)
    backward = torch.library.custom_op(f"orcai::{base}_backward", backward_impl, mutates_args=(), schema=f"(Tensor grad, Tensor pcm, {saved}, {no_quantiles}) -> Tensor")
    backward.register_fake(lambda grad, pcm, *rest: pcm.new_empty((pcm.shape[0],), dtype=torch.float32))
    _FRONT_END_OPS[base + "_with_stats"], _FRONT_END_OPS[base + "_backward"] = with_stats, backward
    _register(base + "_wrt_pcm", f"(Tensor pcm, {schema}) -> Tensor", _front_end_impl("orcai::" + base, parameter), fake, autograd)


def _linear_gradient_sizes(sampling_rate, nfft, *rest) -> None:
    """The linear route has a forward that takes sizes its backward does not."""
    from orcai_amd.frontend import FrontEnd

    FrontEnd._check_nfft_backward(nfft)


def _denoised_gradient_sizes(sampling_rate, nfft, hop, freq_hi, n_mels, *rest) -> None:
    """So has the denoised route on the linear bins (the mel route's refusals are mel.mel_config's, in the forward)."""
    if n_mels <= 0:
        _linear_gradient_sizes(sampling_rate, nfft)


_register_wrt_pcm("spectrogram", "SymInt sampling_rate, SymInt nfft, SymInt hop, float freq_hi, float q_lo, float q_hi", _spectrogram_parameter, _spectrogram_fake,
                  check=_linear_gradient_sizes)
_register_wrt_pcm("mel_spectrogram", "SymInt sampling_rate, SymInt nfft, SymInt hop, SymInt n_mels, float fmin, float fmax, bool htk, bool slaney_norm, "
                  "float q_lo, float q_hi", _mel_parameter, _mel_spectrogram_fake)
_register_wrt_pcm("pcen_spectrogram", _PCEN_ARGUMENTS, _pcen_parameter, _linear_or_mel_fake)
_register_wrt_pcm("denoised_spectrogram", _DENOISED_ARGUMENTS, _denoised_parameter, _linear_or_mel_fake, check=_denoised_gradient_sizes, profile=True)


def spectrogram_wrt_pcm(pcm: Tensor, sampling_rate: int, nfft: int, hop: int, freq_hi: float, q_lo: float, q_hi: float) -> Tensor:
    """orcai::spectrogram (same bits) whose backward returns dL/dpcm when pcm requires grad; nfft a power of two from 32 to 4096."""
    return torch.ops.orcai.spectrogram_wrt_pcm(pcm, sampling_rate, nfft, hop, freq_hi, q_lo, q_hi)


def mel_spectrogram_wrt_pcm(pcm: Tensor, sampling_rate: int, nfft: int, hop: int, n_mels: int, fmin: float, fmax: float, htk: bool, slaney_norm: bool,
                            q_lo: float, q_hi: float) -> Tensor:
    """orcai::mel_spectrogram (same bits) whose backward returns dL/dpcm when pcm requires grad; nfft a power of two from 128 to 4096."""
    return torch.ops.orcai.mel_spectrogram_wrt_pcm(pcm, sampling_rate, nfft, hop, n_mels, fmin, fmax, htk, slaney_norm, q_lo, q_hi)


def pcen_spectrogram_wrt_pcm(pcm: Tensor, sampling_rate: int, nfft: int, hop: int, freq_hi: float, n_mels: int, fmin: float, fmax: float, htk: bool, slaney_norm: bool,
                             time_constant: float, gain: float, bias: float, power: float, eps: float, scale: float, q_lo: float, q_hi: float) -> Tensor:
    """orcai::pcen_spectrogram (same bits) whose backward returns dL/dpcm when pcm requires grad; nfft a power of two from 32 (n_mels > 0: 128) to 4096."""
    return torch.ops.orcai.pcen_spectrogram_wrt_pcm(pcm, sampling_rate, nfft, hop, freq_hi, n_mels, fmin, fmax, htk, slaney_norm, time_constant, gain, bias, power, eps,
                                                    scale, q_lo, q_hi)


def denoised_spectrogram_wrt_pcm(pcm: Tensor, sampling_rate: int, nfft: int, hop: int, freq_hi: float, n_mels: int, fmin: float, fmax: float, htk: bool,
                                 slaney_norm: bool, quantile: float, q_lo: float, q_hi: float) -> Tensor:
    """orcai::denoised_spectrogram (same bits) whose backward returns dL/dpcm when pcm requires grad, the per-channel floor held constant like the other
    statistics; nfft a power of two from 32 (n_mels > 0: 128) to 4096.  No second derivative."""
    return torch.ops.orcai.denoised_spectrogram_wrt_pcm(pcm, sampling_rate, nfft, hop, freq_hi, n_mels, fmin, fmax, htk, slaney_norm, quantile, q_lo, q_hi)


# ---------------------------------------------------------------------------------------------------------------- orcai::resample
# The project's polyphase resampler (orcai_amd/resample.py, what `orcai predict` runs on a recording that is not at the model's rate) as an op with
# autograd w.r.t. the audio.  It is linear, so its backward is its adjoint with the same table: the functional op orcai::resample_backward
# (orcai_resample_polyphase_bwd).  Nothing is saved for the backward but the input's length.  Equal rates: both ops copy (an op may not alias its input).
def _no_pcen(spectrogram_parameter: dict, who: str) -> None:
    if spectrogram_parameter.get("pcen") is not None:
        raise NotImplementedError(f"{who}: spectrogram parameter pcen is set and this is a dB front end; "
                                  "torch_ops.PcenWaveformFrontEnd(spectrogram_parameter, native_rate) is the differentiable PCEN front end")


def _no_denoise(spectrogram_parameter: dict, who: str) -> None:
    """The plain differentiable modules run *_wrt_pcm ops that have no denoise argument: a parameter that asks for it is refused, not silently run without
    (DenoisedWaveformFrontEnd is the module for it)."""
    from orcai_amd import denoise

    denoise.no_gradient(spectrogram_parameter, who)


def _check_rates(sr_in, sr_out, who: str) -> None:
    if sr_in <= 0 or sr_out <= 0:
        raise ValueError(f"{who}: sr_in and sr_out must be positive, got {sr_in} and {sr_out}")


def _resampled_length(n, sr_in: int, sr_out: int):
    """ceil(n * sr_out / sr_in) in integers (n may be symbolic); resample.output_length for every length a recording has."""
    return (n * sr_out + sr_in - 1) // sr_in


def resample(pcm: Tensor, sr_in: int, sr_out: int) -> Tensor:
    """resample_device (same bits) of f32 pcm[n] at sr_in -> f32[ceil(n * sr_out / sr_in)] at sr_out; its backward returns dL/dpcm when pcm requires grad."""
    return torch.ops.orcai.resample(pcm, sr_in, sr_out)


def _resample_impl(pcm, sr_in, sr_out):
    from orcai_amd.resample import resample_device

    _check_pcm(pcm, "orcai::resample")
    _check_rates(sr_in, sr_out, "orcai::resample")
    if sr_in == sr_out:
        return pcm.detach().clone()
    return resample_device(pcm.detach(), sr_in, sr_out)


def _resample_fake(pcm, sr_in, sr_out):
    return pcm.new_empty((pcm.shape[0] if sr_in == sr_out else _resampled_length(pcm.shape[0], sr_in, sr_out),), dtype=torch.float32)


@torch.library.custom_op("orcai::resample_backward", mutates_args=())
def resample_backward(grad: Tensor, n_in: int, sr_in: int, sr_out: int) -> Tensor:
    """dL/dpcm f32[n_in] from grad = dL/d(resampled) f32[ceil(n_in * sr_out / sr_in)]: the adjoint of orcai::resample."""
    from orcai_amd.resample import resample_backward_device

    if grad.dim() != 1 or grad.dtype != torch.float32 or not grad.is_cuda:
        raise ValueError("orcai::resample_backward: grad must be a 1-d f32 cuda tensor")
    _check_rates(sr_in, sr_out, "orcai::resample_backward")
    if sr_in == sr_out:
        if grad.shape[0] != n_in:
            raise ValueError(f"orcai::resample_backward: grad has {grad.shape[0]} samples, n_in is {n_in}")
        return grad.detach().clone()
    return resample_backward_device(grad.detach(), n_in, sr_in, sr_out)


@resample_backward.register_fake
def _resample_backward_fake(grad, n_in, sr_in, sr_out):
    return grad.new_empty((n_in,), dtype=torch.float32)


class _ResampleFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pcm, sr_in, sr_out):
        with torch._C._AutoDispatchBelowAutograd():
            out = torch.ops.orcai.resample(pcm, sr_in, sr_out)
        ctx.args = (pcm.shape[0], sr_in, sr_out)
        return out

    @staticmethod
    def backward(ctx, grad):
        return torch.ops.orcai.resample_backward(grad, *ctx.args), None, None


def _resample_autograd(pcm, sr_in, sr_out):
    if torch.is_grad_enabled() and pcm.requires_grad:
        return _ResampleFunction.apply(pcm, sr_in, sr_out)
    with torch._C._AutoDispatchBelowAutograd():
        return torch.ops.orcai.resample(pcm, sr_in, sr_out)


_register("resample", "(Tensor pcm, SymInt sr_in, SymInt sr_out) -> Tensor", _resample_impl, _resample_fake, _resample_autograd)


# ---------------------------------------------------------------------------------------------------------------- orcai::decode_pcm
# The sample decode `orcai predict` runs on the bytes of a recording's data chunk (orcai_amd/wavio.py: decode_device).  The kernel reads aligned 16-byte
# words, so the bytes it is given are padded to a multiple of 16 when they are not one (a copy; wavio.upload_and_decode allocates padded and makes none).
# Integer input: nothing to differentiate, the Autograd key runs the kernel.
def _pcm_frames(nbytes, channels: int, sample_format: int, who: str):
    from orcai_amd.wavio import BYTES_PER_SAMPLE, MAX_DEVICE_CHANNELS

    if not 0 <= sample_format < len(BYTES_PER_SAMPLE):
        raise ValueError(f"{who}: format must be 0 U8, 1 S16, 2 S24, 3 S32, 4 F32 or 5 F64, got {sample_format}")
    if not 1 <= channels <= MAX_DEVICE_CHANNELS:
        raise ValueError(f"{who}: channels must be 1 .. {MAX_DEVICE_CHANNELS}, got {channels}")
    return nbytes // (channels * BYTES_PER_SAMPLE[sample_format])


def decode_pcm(frames: Tensor, channels: int, channel: int, format: int) -> Tensor:
    """The f32 samples of 0-based `channel` from uint8 frames[nbytes], the interleaved little-endian frames of a WAV data chunk (whole frames are
    decoded, trailing bytes ignored)."""
    return torch.ops.orcai.decode_pcm(frames, channels, channel, format)


def _decode_pcm_impl(frames, channels, channel, format):
    from orcai_amd.wavio import BYTES_PER_SAMPLE, decode_device

    if frames.dim() != 1 or frames.dtype != torch.uint8 or not frames.is_cuda:
        raise ValueError("orcai::decode_pcm: frames must be a 1-d uint8 cuda tensor")
    n = _pcm_frames(frames.shape[0], channels, format, "orcai::decode_pcm")
    if not 0 <= channel < channels:
        raise ValueError(f"orcai::decode_pcm: channel must be in [0, {channels}), got {channel}")
    if n == 0:
        return frames.new_empty((0,), dtype=torch.float32)
    need = -(-n * channels * BYTES_PER_SAMPLE[format] // 16) * 16
    if frames.shape[0] < need or frames.data_ptr() % 16 or not frames.is_contiguous():
        padded = frames.new_empty((need,))
        padded[: min(need, frames.shape[0])].copy_(frames[:need])
        frames = padded
    return decode_device(frames, n, channels, channel, format)


def _decode_pcm_fake(frames, channels, channel, format):
    return frames.new_empty((_pcm_frames(frames.shape[0], channels, format, "orcai::decode_pcm"),), dtype=torch.float32)


def _decode_pcm_autograd(frames, channels, channel, format):
    with torch._C._AutoDispatchBelowAutograd():
        return torch.ops.orcai.decode_pcm(frames, channels, channel, format)


_register("decode_pcm", "(Tensor frames, SymInt channels, SymInt channel, SymInt format) -> Tensor", _decode_pcm_impl, _decode_pcm_fake, _decode_pcm_autograd)


class _WaveformFrontEnd(torch.nn.Module):
    """What the four front-end modules share: forward(pcm f32[n] at native_rate) = orcai::<_op>(resample(pcm, native_rate, sampling_rate), sampling_rate,
    nfft, hop, *_args, q_lo, q_hi).  A subclass names its op, refuses in _route what is not its route and keeps there what _args and extra_repr read.
    Only the subclass whose op takes the denoise quantile (_denoised) accepts a parameter with ``denoise`` set."""

    _op: str
    _denoised = False

    def __init__(self, spectrogram_parameter: dict, native_rate: int):
        super().__init__()
        sp = spectrogram_parameter
        if not self._denoised:
            _no_denoise(sp, type(self).__name__)
        self._route(sp)
        self.native_rate = int(native_rate)
        self.sampling_rate, self.nfft, self.hop = int(sp["sampling_rate"]), int(sp["nfft"]), int(sp["n_overlap"])
        self.q_lo, self.q_hi = (float(q) for q in sp["quantiles"])
        _check_rates(self.native_rate, self.sampling_rate, type(self).__name__)

    def forward(self, pcm: Tensor) -> Tensor:
        at_rate = torch.ops.orcai.resample(pcm, self.native_rate, self.sampling_rate)
        return getattr(torch.ops.orcai, self._op)(at_rate, self.sampling_rate, self.nfft, self.hop, *self._args, self.q_lo, self.q_hi)

    def extra_repr(self) -> str:
        return f"{self.native_rate} Hz -> {self.sampling_rate} Hz, nfft={self.nfft}, hop={self.hop}, "

    def _linear_or_mel(self, sp: dict, cfg: dict | None) -> tuple:
        """(freq_hi, n_mels, fmin, fmax, htk, slaney_norm) of an op that chooses its route by n_mels, from cfg = mel.mel_config(sp)."""
        if cfg is not None:
            return (0.0, cfg["n_mels"], cfg["fmin"], cfg["fmax"], cfg["htk"], cfg["norm"] == "slaney")
        if float(sp["freq_range"][0]) != 0.0:
            raise ValueError(f"{type(self).__name__}: freq_range must start at 0 (orcai::{self._op.removesuffix('_wrt_pcm')} keeps the leading bins), "
                             f"got {sp['freq_range']}")
        return (float(sp["freq_range"][1]), 0, 0.0, 0.0, False, True)


class WaveformFrontEnd(_WaveformFrontEnd):
    """A recording at the rate it was made at -> the [T, K] spectrogram the detector reads, differentiable down to those samples:
    forward(pcm f32[n] at native_rate) = spectrogram_wrt_pcm(resample(pcm, native_rate, sampling_rate), ...), the two stages `orcai predict` runs in
    front of the model (same bits).  spectrogram_parameter is the "spectrogram" section of a model's parameter file (sampling_rate, nfft,
    n_overlap = the hop, freq_range = [0, freq_hi], quantiles).  The three normalisation statistics are held constant in the backward."""

    _op = "spectrogram_wrt_pcm"

    def _route(self, sp: dict) -> None:
        _no_pcen(sp, "WaveformFrontEnd")
        if sp.get("mel") is not None:
            raise NotImplementedError("WaveformFrontEnd: spectrogram parameter mel is set and this class is the linear front end; "
                                      "torch_ops.waveform_front_end(spectrogram_parameter, native_rate) returns MelWaveformFrontEnd for it")
        if float(sp["freq_range"][0]) != 0.0:
            raise ValueError(f"WaveformFrontEnd: freq_range must start at 0 (orcai::spectrogram keeps the leading bins), got {sp['freq_range']}")
        self.freq_hi = float(sp["freq_range"][1])

    @property
    def _args(self) -> tuple:
        return (self.freq_hi,)

    def extra_repr(self) -> str:
        return super().extra_repr() + f"freq_hi={self.freq_hi}"


class MelWaveformFrontEnd(_WaveformFrontEnd):
    """WaveformFrontEnd for a spectrogram parameter whose ``mel`` key is set: forward(pcm f32[n] at native_rate) =
    mel_spectrogram_wrt_pcm(resample(pcm, native_rate, sampling_rate), ...) -> [T, n_mels], differentiable down to those samples.  The parameter is
    validated as mel.mel_config does (ValueError names the key, NotImplementedError an nfft the mel route does not take)."""

    _op = "mel_spectrogram_wrt_pcm"

    def _route(self, sp: dict) -> None:
        from orcai_amd import mel

        _no_pcen(sp, "MelWaveformFrontEnd")
        cfg = mel.mel_config(sp)
        if cfg is None:
            raise ValueError("MelWaveformFrontEnd: spectrogram parameter mel is absent or null; torch_ops.waveform_front_end(spectrogram_parameter, "
                             "native_rate) returns WaveformFrontEnd for it")
        self.n_mels, self.fmin, self.fmax, self.htk, self.slaney_norm = cfg["n_mels"], cfg["fmin"], cfg["fmax"], cfg["htk"], cfg["norm"] == "slaney"

    @property
    def _args(self) -> tuple:
        return (self.n_mels, self.fmin, self.fmax, self.htk, self.slaney_norm)

    def extra_repr(self) -> str:
        return super().extra_repr() + f"n_mels={self.n_mels}, fmin={self.fmin}, fmax={self.fmax}, htk={self.htk}, slaney_norm={self.slaney_norm}"


class PcenWaveformFrontEnd(_WaveformFrontEnd):
    """WaveformFrontEnd for a spectrogram parameter whose ``pcen`` key is set, on either route (the mel one when ``mel`` is set as well):
    forward(pcm f32[n] at native_rate) = pcen_spectrogram_wrt_pcm(resample(pcm, native_rate, sampling_rate), ...) -> [T, K], differentiable down to those
    samples.  The parameter is validated as pcen.pcen_config and mel.mel_config do; p_lo and p_hi are held constant in the backward."""

    _op = "pcen_spectrogram_wrt_pcm"

    def _route(self, sp: dict) -> None:
        from orcai_amd import mel, pcen

        pc = pcen.pcen_config(sp)
        if pc is None:
            raise ValueError("PcenWaveformFrontEnd: spectrogram parameter pcen is absent or null; torch_ops.waveform_front_end(spectrogram_parameter, "
                             "native_rate) returns the dB front end for it")
        self.route = self._linear_or_mel(sp, mel.mel_config(sp))
        self.pcen = tuple(pc[k] for k in pcen.PCEN_KEYS)  # time_constant, gain, bias, power, eps, scale: the op's order

    @property
    def _args(self) -> tuple:
        return (*self.route, *self.pcen)

    def extra_repr(self) -> str:
        freq_hi, n_mels = self.route[:2]
        return (super().extra_repr() + (f"n_mels={n_mels}" if n_mels else f"freq_hi={freq_hi}")
                + f", time_constant={self.pcen[0]}, gain={self.pcen[1]}, bias={self.pcen[2]}, power={self.pcen[3]}, eps={self.pcen[4]}, scale={self.pcen[5]}")


class DenoisedWaveformFrontEnd(_WaveformFrontEnd):
    """WaveformFrontEnd for a spectrogram parameter whose ``denoise`` key is set, on either route (the mel one when ``mel`` is set as well):
    forward(pcm f32[n] at native_rate) = denoised_spectrogram_wrt_pcm(resample(pcm, native_rate, sampling_rate), ...) -> [T, K], differentiable down to
    those samples.  The parameter is validated as denoise.denoise_config (which refuses ``pcen`` beside it) and mel.mel_config do; ref_db, p_lo, p_hi and
    the per-channel floor are held constant in the backward."""

    _op = "denoised_spectrogram_wrt_pcm"
    _denoised = True

    def _route(self, sp: dict) -> None:
        from orcai_amd import denoise, mel
        from orcai_amd.frontend import FrontEnd

        dn = denoise.denoise_config(sp)
        if dn is None:
            raise ValueError("DenoisedWaveformFrontEnd: spectrogram parameter denoise is absent or null; torch_ops.waveform_front_end(spectrogram_parameter, "
                             "native_rate) returns the dB front end for it")
        denoise.no_segment_gradient(sp, "DenoisedWaveformFrontEnd")
        cfg = mel.mel_config(sp)
        if cfg is None:
            FrontEnd._check_nfft_backward(sp["nfft"])
        self.route = self._linear_or_mel(sp, cfg)
        self.quantile = dn["quantile"]

    @property
    def _args(self) -> tuple:
        return (*self.route, self.quantile)

    def extra_repr(self) -> str:
        freq_hi, n_mels = self.route[:2]
        return super().extra_repr() + (f"n_mels={n_mels}" if n_mels else f"freq_hi={freq_hi}") + f", denoise.quantile={self.quantile}"


def waveform_front_end(spectrogram_parameter: dict, native_rate: int) -> torch.nn.Module:
    """The differentiable dB front end of a parameter file's "spectrogram" section: MelWaveformFrontEnd when its ``mel`` key is set, WaveformFrontEnd
    when it is absent or null.  A parameter whose ``pcen`` key is set is refused by both (NotImplementedError): PcenWaveformFrontEnd is its class.  A
    parameter whose ``denoise`` key is set is refused here and by all three (NotImplementedError that names denoise and DenoisedWaveformFrontEnd, its
    class: these run the plain dB ops, whose forward and gradient know no floor)."""
    _no_denoise(spectrogram_parameter, "waveform_front_end")
    if spectrogram_parameter.get("mel") is not None:
        return MelWaveformFrontEnd(spectrogram_parameter, native_rate)
    return WaveformFrontEnd(spectrogram_parameter, native_rate)


# ---------------------------------------------------------------------------------------------------------------- orcai::detect_wrt_input
# The inference network with the gradient w.r.t. the snippets (orcai_amd/eval_grad.py), built the way spectrogram_wrt_pcm is: an inner op that
# also returns what the backward reads (`saved`, owned by the autograd graph: no "one open step" rule), and a functional backward op.  Weights
# and statistics get no gradient; nothing is mutated.
def _eval_grad(config: str, device: torch.device):
    eng = _engine(config, device)
    if getattr(eng, "_eval_grad", None) is None:
        from orcai_amd.eval_grad import EvalGrad

        eng._eval_grad = EvalGrad(eng.model)
    return eng, eng._eval_grad


@functools.lru_cache(maxsize=None)
def _saved_per_snippet(config: str) -> int:
    from orcai_amd.eval_grad import saved_layout

    return saved_layout(_skeleton(config))[1]


@torch.library.custom_op("orcai::detect_with_saved", mutates_args=())
def detect_with_saved(x: Tensor, weights: list[Tensor], stats: list[Tensor], config: str) -> tuple[Tensor, Tensor]:
    """EvalGrad.forward: the eval-mode probabilities f32[B, steps, labels] and the flat f32 tensor of stored activations its backward reads."""
    _check_x(config, x, "orcai::detect_wrt_input")
    _check_vars(config, weights, stats)
    eng, eg = _eval_grad(config, x.device)
    if x.shape[0] == 0:
        return _probs_fake(x, weights, stats, config), x.new_empty((0,))
    with torch.cuda.device(x.device):
        return eg.forward(x.detach().contiguous(), params=eng.flat(weights, stats))


@detect_with_saved.register_fake
def _detect_with_saved_fake(x, weights, stats, config):
    return _probs_fake(x, weights, stats, config), x.new_empty((x.shape[0] * _saved_per_snippet(config),), dtype=torch.float32)


@torch.library.custom_op("orcai::detect_backward", mutates_args=())
def detect_backward(grad: Tensor, saved: Tensor, weights: list[Tensor], stats: list[Tensor], config: str) -> Tensor:
    """EvalGrad.backward: dL/dx f32[B, H, W] from grad = dL/dprobs and the `saved` tensor orcai::detect_with_saved returned for the same weights."""
    cfg = _parse(config)
    H, W = int(cfg["input_shape"][0]), int(cfg["input_shape"][1])
    _check_vars(config, weights, stats)
    eng, eg = _eval_grad(config, grad.device)
    if grad.shape[0] == 0:
        return grad.new_empty((0, H, W))
    with torch.cuda.device(grad.device):
        return eg.backward(grad, saved, params=eng.flat(weights, stats))


@detect_backward.register_fake
def _detect_backward_fake(grad, saved, weights, stats, config):
    H, W = (int(v) for v in _parse(config)["input_shape"][:2])
    return grad.new_empty((grad.shape[0], H, W), dtype=torch.float32)


def detect_wrt_input(x: Tensor, weights: list[Tensor], stats: list[Tensor], config: str) -> Tensor:
    """The model in eval mode on snippets x[B][H][W]; its backward returns dL/dx when x requires grad (never a weight gradient)."""
    return torch.ops.orcai.detect_wrt_input(x, weights, stats, config)


def _detect_impl(x, weights, stats, config):
    return torch.ops.orcai.detect_with_saved(x, weights, stats, config)[0]


class _DetectFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, config, n_weights, *variables):
        weights, stats = list(variables[:n_weights]), list(variables[n_weights:])
        with torch._C._AutoDispatchBelowAutograd():
            probs, saved = torch.ops.orcai.detect_with_saved(x, weights, stats, config)
        ctx.config, ctx.n_weights = config, n_weights
        ctx.save_for_backward(saved, *[t.detach() for t in variables])
        return probs

    @staticmethod
    def backward(ctx, grad):
        saved, *variables = ctx.saved_tensors
        n = ctx.n_weights
        dx = torch.ops.orcai.detect_backward(grad.contiguous(), saved, list(variables[:n]), list(variables[n:]), ctx.config)
        return (dx, None, None, *([None] * len(variables)))


def _detect_autograd(x, weights, stats, config):
    if torch.is_grad_enabled() and x.requires_grad:
        return _DetectFunction.apply(x, config, len(weights), *weights, *stats)
    with torch._C._AutoDispatchBelowAutograd():
        return torch.ops.orcai.detect_wrt_input(x, weights, stats, config)


_register("detect_wrt_input", "(Tensor x, Tensor[] weights, Tensor[] stats, str config) -> Tensor", _detect_impl, _probs_fake, _detect_autograd)


# ---------------------------------------------------------------------------------------------------------------- orcai::detect_wrt_params
# The predict-time network with the gradient w.r.t. its weights as well: fine-tuning a pretrained detector with BatchNorm frozen on its moving
# statistics (EvalGrad.backward(wgrad=True)).  Built as detect_wrt_input is: the same inner forward op (orcai::detect_with_saved), and a functional
# backward op that returns dx and the flat weight gradient in ParamLayout order; the autograd kernel splits it per variable (layout().split_w, the
# inverse of _Engine.flat).  The statistics get None; nothing is mutated.
@torch.library.custom_op("orcai::detect_backward_params", mutates_args=())
def detect_backward_params(grad: Tensor, saved: Tensor, weights: list[Tensor], stats: list[Tensor], config: str) -> tuple[Tensor, Tensor]:
    """EvalGrad.backward(wgrad=True): (dL/dx f32[B, H, W], the flat f32 gradient w.r.t. the trainable variables in variable_spec() order) from grad = dL/dprobs
    and the `saved` tensor orcai::detect_with_saved returned for the same weights."""
    cfg = _parse(config)
    H, W = int(cfg["input_shape"][0]), int(cfg["input_shape"][1])
    _check_vars(config, weights, stats)
    eng, eg = _eval_grad(config, grad.device)
    if grad.shape[0] == 0:
        return grad.new_empty((0, H, W)), grad.new_zeros((eng.model.layout().n_w,))
    with torch.cuda.device(grad.device):
        return eg.backward(grad, saved, params=eng.flat(weights, stats), wgrad=True)


@detect_backward_params.register_fake
def _detect_backward_params_fake(grad, saved, weights, stats, config):
    return _detect_backward_fake(grad, saved, weights, stats, config), _flat_grad_fake(grad, config)


def detect_wrt_params(x: Tensor, weights: list[Tensor], stats: list[Tensor], config: str) -> Tensor:
    """The model in eval mode on snippets x[B][H][W]; its backward returns a gradient per weight (BatchNorm frozen on `stats`, which get none) and dL/dx when
    x requires grad."""
    return torch.ops.orcai.detect_wrt_params(x, weights, stats, config)


class _DetectParamsFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, config, n_weights, *variables):
        weights, stats = list(variables[:n_weights]), list(variables[n_weights:])
        with torch._C._AutoDispatchBelowAutograd():
            probs, saved = torch.ops.orcai.detect_with_saved(x, weights, stats, config)
        ctx.config, ctx.n_weights = config, n_weights
        ctx.save_for_backward(saved, *[t.detach() for t in variables])
        return probs

    @staticmethod
    def backward(ctx, grad):
        saved, *variables = ctx.saved_tensors
        n = ctx.n_weights
        dx, flat = torch.ops.orcai.detect_backward_params(grad.contiguous(), saved, list(variables[:n]), list(variables[n:]), ctx.config)
        need = ctx.needs_input_grad
        wgrads = [g if want else None for g, want in zip(_skeleton(ctx.config).layout().split_w(flat), need[3 : 3 + n])]
        return (dx if need[0] else None, None, None, *wgrads, *([None] * (len(variables) - n)))


def _detect_params_autograd(x, weights, stats, config):
    if torch.is_grad_enabled() and (x.requires_grad or any(w.requires_grad for w in weights)):
        return _DetectParamsFunction.apply(x, config, len(weights), *weights, *stats)
    with torch._C._AutoDispatchBelowAutograd():
        return torch.ops.orcai.detect_wrt_params(x, weights, stats, config)


_register("detect_wrt_params", "(Tensor x, Tensor[] weights, Tensor[] stats, str config) -> Tensor", _detect_impl, _probs_fake, _detect_params_autograd)


# ---------------------------------------------------------------------------------------------------------------- orcai::detect_recording
# The recording-level function of `orcai predict` (snippets -> predict-time network -> 50 %-overlap average) with the gradient w.r.t. the spectrogram
# (orcai_amd/eval_grad.py: RecordingGrad), wired as detect_wrt_input / detect_wrt_params are: the forward keeps nothing but its arguments, the backward is a
# functional op that recomputes the detector in chunks of `chunk` snippets.  One EvalGrad per (config, device) serves both families of ops.
def _recording_grad(config: str, device: torch.device, chunk: int):
    from orcai_amd.eval_grad import RecordingGrad

    eng, eg = _eval_grad(config, device)
    return eng, RecordingGrad(eng.model, int(chunk), eval_grad=eg)  # host bookkeeping only: the engine's EvalGrad holds the workspaces


def _check_spec(config: str, spec: Tensor, who: str) -> None:
    W = int(_parse(config)["input_shape"][1])
    if spec.dim() != 2 or spec.shape[1] != W or spec.dtype != torch.float32:
        raise ValueError(f"{who}: spec must be f32 [T, {W}], got {spec.dtype} {tuple(spec.shape)}")


def _avg_fake(spec, weights, stats, config, chunk):
    cfg = _parse(config)
    return spec.new_empty((spec.shape[0] // 2 ** len(cfg["filters"]), cfg["num_labels"]), dtype=torch.float32)


def detect_recording(spec: Tensor, weights: list[Tensor], stats: list[Tensor], config: str, chunk: int = 64) -> Tensor:
    """The overlap-averaged probabilities f32[T // tpo, labels] of the recording spec[T][W] (what `orcai predict` thresholds, rounded to f32); its backward
    returns dL/dspec when spec requires grad (never a weight gradient).  A recording shorter than one snippet raises."""
    return torch.ops.orcai.detect_recording(spec, weights, stats, config, chunk)


def detect_recording_wrt_params(spec: Tensor, weights: list[Tensor], stats: list[Tensor], config: str, chunk: int = 64) -> Tensor:
    """detect_recording whose backward also returns a gradient per weight (BatchNorm frozen on `stats`, which get none)."""
    return torch.ops.orcai.detect_recording_wrt_params(spec, weights, stats, config, chunk)


def _detect_recording_impl(spec, weights, stats, config, chunk):
    _check_spec(config, spec, "orcai::detect_recording")
    _check_vars(config, weights, stats)
    eng, rg = _recording_grad(config, spec.device, chunk)
    with torch.cuda.device(spec.device):
        return rg.forward(spec.detach(), params=eng.flat(weights, stats))


@torch.library.custom_op("orcai::detect_recording_bwd", mutates_args=())
def detect_recording_bwd(grad: Tensor, spec: Tensor, weights: list[Tensor], stats: list[Tensor], config: str, chunk: int) -> Tensor:
    """RecordingGrad.backward: dL/dspec f32[T, W] from grad = dL/davg f32[T // tpo, labels] and the spectrogram of the forward."""
    _check_spec(config, spec, "orcai::detect_recording_bwd")
    _check_vars(config, weights, stats)
    eng, rg = _recording_grad(config, spec.device, chunk)
    with torch.cuda.device(spec.device):
        return rg.backward(spec.detach(), grad.contiguous(), params=eng.flat(weights, stats))


@detect_recording_bwd.register_fake
def _detect_recording_bwd_fake(grad, spec, weights, stats, config, chunk):
    return spec.new_empty(spec.shape, dtype=torch.float32)


@torch.library.custom_op("orcai::detect_recording_bwd_params", mutates_args=())
def detect_recording_bwd_params(grad: Tensor, spec: Tensor, weights: list[Tensor], stats: list[Tensor], config: str, chunk: int) -> tuple[Tensor, Tensor]:
    """RecordingGrad.backward(wgrad=True): (dL/dspec f32[T, W], the flat f32 gradient w.r.t. the trainable variables in variable_spec() order)."""
    _check_spec(config, spec, "orcai::detect_recording_bwd_params")
    _check_vars(config, weights, stats)
    eng, rg = _recording_grad(config, spec.device, chunk)
    with torch.cuda.device(spec.device):
        return rg.backward(spec.detach(), grad.contiguous(), params=eng.flat(weights, stats), wgrad=True)


@detect_recording_bwd_params.register_fake
def _detect_recording_bwd_params_fake(grad, spec, weights, stats, config, chunk):
    return spec.new_empty(spec.shape, dtype=torch.float32), _flat_grad_fake(grad, config)


def _recording_autograd(name: str, with_params: bool):
    """The Autograd kernel of orcai::<name>: spec and the variables are all the backward needs (it recomputes); with_params: the weights get gradients too."""

    class Function(torch.autograd.Function):
        @staticmethod
        def forward(ctx, spec, config, chunk, n_weights, *variables):
            with torch._C._AutoDispatchBelowAutograd():
                avg = getattr(torch.ops.orcai, name)(spec, list(variables[:n_weights]), list(variables[n_weights:]), config, chunk)
            ctx.config, ctx.chunk, ctx.n_weights = config, chunk, n_weights
            ctx.save_for_backward(spec.detach(), *[t.detach() for t in variables])
            return avg

        @staticmethod
        def backward(ctx, grad):
            spec, *variables = ctx.saved_tensors
            n = ctx.n_weights
            args = (grad.contiguous(), spec, list(variables[:n]), list(variables[n:]), ctx.config, ctx.chunk)
            need = ctx.needs_input_grad
            if not with_params:
                return (torch.ops.orcai.detect_recording_bwd(*args), None, None, None, *([None] * len(variables)))
            dspec, flat = torch.ops.orcai.detect_recording_bwd_params(*args)
            wgrads = [g if want else None for g, want in zip(_skeleton(ctx.config).layout().split_w(flat), need[4 : 4 + n])]
            return (dspec if need[0] else None, None, None, None, *wgrads, *([None] * (len(variables) - n)))

    Function.__name__ = Function.__qualname__ = "_" + "".join(part.capitalize() for part in name.split("_")) + "Function"

    def autograd(spec, weights, stats, config, chunk):
        if torch.is_grad_enabled() and (spec.requires_grad or (with_params and any(w.requires_grad for w in weights))):
            return Function.apply(spec, config, chunk, len(weights), *weights, *stats)
        with torch._C._AutoDispatchBelowAutograd():
            return getattr(torch.ops.orcai, name)(spec, weights, stats, config, chunk)

    return autograd


_RECORDING_SCHEMA = "(Tensor spec, Tensor[] weights, Tensor[] stats, str config, SymInt chunk) -> Tensor"
_register("detect_recording", _RECORDING_SCHEMA, _detect_recording_impl, _avg_fake, _recording_autograd("detect_recording", False))
_register("detect_recording_wrt_params", _RECORDING_SCHEMA, _detect_recording_impl, _avg_fake, _recording_autograd("detect_recording_wrt_params", True))


# ---------------------------------------------------------------------------------------------------------------- orcai::predict_spectrogram
@torch.library.custom_op("orcai::predict_spectrogram", mutates_args=())
def predict_spectrogram(spec: Tensor, weights: list[Tensor], stats: list[Tensor], config: str) -> Tensor:
    """All 50 %-overlapping snippets of spec[T][W] (model.predict_spectrogram: blocks 1-2 shared between overlapping snippets), eval mode."""
    cfg = _parse(config)
    if spec.dim() != 2 or spec.shape[1] != int(cfg["input_shape"][1]) or spec.dtype != torch.float32:
        raise ValueError(f"orcai::predict_spectrogram: spec must be f32 [T, {cfg['input_shape'][1]}], got {spec.dtype} {tuple(spec.shape)}")
    _check_vars(config, weights, stats)
    with torch.cuda.device(spec.device):
        return _engine(config, spec.device).predict(spec, weights, stats)


@predict_spectrogram.register_fake
def _predict_spectrogram_fake(spec, weights, stats, config):
    H = int(_parse(config)["input_shape"][0])
    n = torch.sym_max((spec.shape[0] - H) // (H // 2) + 1, 0)
    return spec.new_empty((n, _out_steps(config), _parse(config)["num_labels"]), dtype=torch.float32)


# ---------------------------------------------------------------------------------------------------------------- nn.Module
def param_name(keras_name: str) -> str:
    """Module attribute of a Keras variable name: '/' -> '__' (reversible: no variable name holds '__')."""
    return keras_name.replace("/", "__")


class OrcaiModule(torch.nn.Module):
    """A ResNetLSTM / ResNet1DConv as a torch.nn.Module: the trainable variables are parameters, the BatchNorm moving statistics buffers,
    both named after the Keras variables (param_name).  forward(x f32[B, H, W]) follows self.training; gradients reach the parameters
    only, and an x that requires grad raises -- unless input_grad=True: the module then calls orcai::forward_wrt_input, whose training-mode
    backward also returns dL/dx (not in eval mode, not for f16 models).  input_grad="eval": as input_grad=True in .train(); in .eval() the
    module calls orcai::detect_wrt_input, the predict-time network with a backward w.r.t. x (the parameters get no gradient, the statistics are
    not touched).  frozen_bn=True: fine-tuning of the PREDICT-TIME network -- the module calls orcai::detect_wrt_params whether in .train() or .eval():
    BatchNorm with the moving statistics (never written: bit-identical after any number of steps), no Dropout, gradients for every parameter and
    for an x that requires grad; input_grad="eval" is implied, input_grad=True (the training-mode input gradient) contradicts it and raises.
    Built from a model object or a model directory (io.load_orcai_model).  dropout_seed of the n-th training forward:
    seed * 1000003 + n."""

    def __init__(self, model, seed: int = 0, input_grad: bool | str = False, frozen_bn: bool = False):
        super().__init__()
        if frozen_bn and input_grad is not False and input_grad != "eval":
            raise ValueError("OrcaiModule: frozen_bn=True runs the eval-mode network, whose input gradient is input_grad='eval' (implied); "
                             f"input_grad={input_grad!r} asks for the training-mode one")
        if isinstance(model, (str, os.PathLike)):
            from orcai_amd.io import load_orcai_model

            model = load_orcai_model(Path(model))[0]
        self.config = model_config(model)  # raises for f16 models
        self._model = model
        self._trainable, self._stats = [], []
        for name, _, _, trainable in model.variable_spec():
            t = torch.from_numpy(model.weights[name].copy())
            if trainable:
                self.register_parameter(param_name(name), torch.nn.Parameter(t))
                self._trainable.append(name)
            else:
                self.register_buffer(param_name(name), t)
                self._stats.append(name)
        self.seed = int(seed)
        if isinstance(input_grad, str) and input_grad != "eval":
            raise ValueError(f"OrcaiModule: input_grad must be False, True or 'eval', got {input_grad!r}")
        self.input_grad = input_grad if input_grad == "eval" else bool(input_grad)
        self.frozen_bn = bool(frozen_bn)
        if self.frozen_bn:
            self.input_grad = "eval"
        self.dropout_draws = 0

    def weights_list(self) -> list:
        return [getattr(self, param_name(n)) for n in self._trainable]

    def stats_list(self) -> list:
        return [getattr(self, param_name(n)) for n in self._stats]

    def forward(self, x: Tensor) -> Tensor:
        if self.frozen_bn:
            return torch.ops.orcai.detect_wrt_params(x, self.weights_list(), self.stats_list(), self.config)
        if self.input_grad == "eval" and not self.training:
            return torch.ops.orcai.detect_wrt_input(x, self.weights_list(), self.stats_list(), self.config)
        seed = 0
        if self.training:
            seed = (self.seed * 1000003 + self.dropout_draws) & 0x7FFFFFFFFFFFFFFF
            self.dropout_draws += 1
        op = torch.ops.orcai.forward_wrt_input if self.input_grad else torch.ops.orcai.forward
        return op(x, self.weights_list(), self.stats_list(), self.config, self.training, seed)

    def predict_spectrogram(self, spec: Tensor) -> Tensor:
        return torch.ops.orcai.predict_spectrogram(spec, self.weights_list(), self.stats_list(), self.config)

    def detect_recording(self, spec: Tensor, chunk: int = 64) -> Tensor:
        """The overlap-averaged probabilities f32[T // tpo, labels] of the recording spec f32[T, W] -- always the PREDICT-TIME network, whatever
        self.training says (orcai::detect_recording).  input_grad="eval": a spec that requires grad gets dL/dspec; frozen_bn=True: so does every parameter
        (orcai::detect_recording_wrt_params); otherwise a spec that requires grad raises.  The backward recomputes the detector `chunk` snippets at a time."""
        if self.frozen_bn:
            return torch.ops.orcai.detect_recording_wrt_params(spec, self.weights_list(), self.stats_list(), self.config, chunk)
        if self.input_grad != "eval" and torch.is_grad_enabled() and spec.requires_grad:
            raise NotImplementedError("OrcaiModule.detect_recording: the gradient w.r.t. the spectrogram is that of the predict-time network: build the module with "
                                      "input_grad='eval' (or frozen_bn=True for the weight gradients as well)")
        return torch.ops.orcai.detect_recording(spec, self.weights_list(), self.stats_list(), self.config, chunk)

    def to_model(self):
        """Writes the parameters and buffers back into the model object (for .save, predict, `orcai predict`) and returns it."""
        self._model.set_weights_dict({n: getattr(self, param_name(n)).detach().cpu().numpy() for n in self._trainable + self._stats})
        return self._model
