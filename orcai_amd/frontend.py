"""Device-side front-end engine: PCM on the GPU -> normalised spectrogram on the GPU.

Wraps the C ABI calls of include/orcai_hip.h that replace reference
``src/orcAI/spectrogram.py:34-87``.  Host logic restated here: the crop indices
(spectrogram.py:62-67) and numpy's float32 "nearest" virtual index (spectrogram.py:70-75).
"""

from __future__ import annotations

import ctypes as C
from typing import NamedTuple

import numpy as np
import torch

from orcai_amd import _native as N
from orcai_amd import denoise
from orcai_amd import mel
from orcai_amd import pcen

TOP_DB = 80.0  # librosa.amplitude_to_db default, spectrogram.py:51-53


def fft_frequencies(sampling_rate: float, n_fft: int) -> np.ndarray:
    """``librosa.fft_frequencies`` (spectrogram.py:41-43)."""
    return np.fft.rfftfreq(n=n_fft, d=1.0 / sampling_rate)


def frames_to_time(n_frames: int, sampling_rate: float, hop: int) -> np.ndarray:
    """``librosa.frames_to_time(range(T))`` (spectrogram.py:45-49)."""
    return (np.arange(n_frames) * hop).astype(int) / float(sampling_rate)


def crop_indices(frequencies: np.ndarray, freq_range) -> tuple[int, int]:
    """spectrogram.py:62-67: first bin with f <= lo, first bin with f >= hi."""
    lo = int(np.argwhere(frequencies <= freq_range[0])[0][0])
    hi = int(np.argwhere(frequencies >= freq_range[1])[0][0])
    return lo, hi


def nearest_rank_index(n: int, q_fraction: float) -> int:
    """Index into the sorted flattened float32 data that ``np.percentile(a, 100*q, method="nearest")``
    picks: numpy >= 2 divides by float32(100) and rounds (n-1)*q half-to-even in float32."""
    q = np.true_divide(np.float32(100 * q_fraction), np.float32(100))
    return int(np.around(np.float32(n - 1) * q))


def n_frames(n, nfft, hop):
    """Frames of a signal of n samples -- librosa, center=True: 1 + (n + 2 (nfft // 2) - nfft) // hop.  Plain integer arithmetic: n may be a SymInt."""
    return 1 + (n - (nfft & 1)) // hop


class Route(NamedTuple):
    """What a spectrogram parameter asks of the front end (resolve_route): the transform, K of the [T, K] result and which of the three C entry points
    serves it -- pcen set: the PCEN one, on the mel bands when mel is set too; else mel set: the mel one; else the linear one."""

    nfft: int
    hop: int
    K: int
    mel: dict | None  # mel.mel_config's result
    pcen: dict | None  # pcen.pcen_config's result


def resolve_route(spectrogram_parameter: dict) -> Route:
    """The parameter's route, and its own refusals: pcen's, mel's, the transform size and the crop, in that order."""
    pc = pcen.pcen_config(spectrogram_parameter)
    cfg = mel.mel_config(spectrogram_parameter)
    n_fft = int(spectrogram_parameter["nfft"])
    if cfg is not None:  # the mel route: K = n_mels, no frequency crop
        K = cfg["n_mels"]
    else:
        FrontEnd._check_nfft(n_fft)
        freqs = fft_frequencies(spectrogram_parameter["sampling_rate"], n_fft)
        f_lo, K = crop_indices(freqs, spectrogram_parameter["freq_range"])
        if f_lo != 0:
            raise NotImplementedError("HIP front end keeps leading bins only (reference crop start is always bin 0)")
    return Route(n_fft, int(spectrogram_parameter["n_overlap"]), K, cfg, pc)


class FrontEnd:
    """Owns the selection workspace; one instance per device/stream."""

    def __init__(self, device: torch.device | str = "cuda"):
        self.lib = N.lib()
        self.device = torch.device(device)
        nbytes = self.lib.orcai_frontend_workspace_bytes()
        self.workspace = torch.zeros(nbytes, dtype=torch.uint8, device=self.device)
        self._mel_tables: dict = {}
        # grown on demand: "pcen" orcai_pcen's partials and carries, "pcen_bwd" orcai_pcen_spectrogram_bwd's energies, planes and carries, "column_select"
        # orcai_column_select's histograms and per-column state
        self._scratch: dict = {}

    @staticmethod
    def _check_nfft(n_fft: int) -> None:
        """The reference reads nfft from the parameter file (spectrogram.py:34-39).  512 -- orcai-V1 and default_orcai_parameter.json -- runs the
        tuned STFT kernel, any other power of two from 32 to 4096 a plain radix-2 kernel, every other size from 2 to 4096 a direct transform (slow,
        exact); say what is not covered instead of a bare error code."""
        n = int(n_fft)
        if n < 2 or n > 4096:
            raise NotImplementedError(f"spectrogram parameter nfft = {n_fft}: the MI355X front end implements transform sizes from 2 to 4096 "
                                      "(512, the value of orcai-V1 and of default_orcai_parameter.json, on the tuned kernel); larger transforms "
                                      "need the reference's CPU path")

    # -- the whole of make_spectrogram after decode (spectrogram.py:90-147) -----------------
    def _kept_bins(self, spectrogram_parameter: dict) -> int:
        """K of make_spectrogram's [T, K]; the parameter's own refusals."""
        return resolve_route(spectrogram_parameter).K

    def _mel_table(self, spectrogram_parameter: dict, cfg: dict):
        """(host band table, packed weights on this device) of a mel parameter: uploaded once per (device, parameter) and kept."""
        key = (float(spectrogram_parameter["sampling_rate"]), int(spectrogram_parameter["nfft"]), *(cfg[k] for k in mel.MEL_KEYS))
        if key not in self._mel_tables:
            t = mel.table_for(spectrogram_parameter, cfg)
            self._mel_tables[key] = (t, torch.from_numpy(t["weights"].copy()).to(self.device))
        return self._mel_tables[key]

    def _bands(self, spectrogram_parameter: dict, cfg: dict | None) -> tuple:
        """The band arguments (lo, hi, off, weights, n_weights) of the C calls; the five nulls of a parameter without mel."""
        if cfg is None:
            return (None, None, None, None, 0)
        t, weights = self._mel_table(spectrogram_parameter, cfg)
        return (t["lo"].ctypes.data, t["hi"].ctypes.data, t["off"].ctypes.data, N.ptr(weights), weights.numel())

    def _grown(self, name: str, need: int) -> torch.Tensor:
        """The f32 scratch tensor `name` of this front end, replaced by a larger one when it holds fewer than need floats."""
        if name not in self._scratch or self._scratch[name].numel() < need:
            self._scratch[name] = torch.empty(need, dtype=torch.float32, device=self.device)
        return self._scratch[name]

    def _stats_dev(self) -> torch.Tensor:
        """The last run's six statistics as a device tensor f32[6] (no host synchronisation)."""
        stats = torch.empty(6, dtype=torch.float32, device=self.device)
        N.check(self.lib.orcai_frontend_stats_dev(N.ptr(self.workspace), N.ptr(stats), N.stream_ptr()), "orcai_frontend_stats_dev")
        return stats

    def spectrogram_shape(self, n_samples: int, spectrogram_parameter: dict) -> tuple[int, int]:
        """(T, K) of make_spectrogram's result for a signal of n_samples at the parameter's rate: host arithmetic only."""
        route = resolve_route(spectrogram_parameter)
        return n_frames(n_samples, route.nfft, route.hop), route.K

    def make_spectrogram(self, pcm: torch.Tensor, spectrogram_parameter: dict, return_stats: bool = False, out: torch.Tensor | None = None,
                         return_profile: bool = False):
        """pcm: f32[N] on the device, already at spectrogram_parameter['sampling_rate'].
        With the parameter's pcen key set the values are PCEN (orcai_amd/pcen.py) of the magnitudes -- of the mel band powers when mel is set too --
        clipped and normalised by the same quantiles; the statistics then hold p_lo / p_hi as PCEN values, pmax and ref_db 0.
        Returns f32[T, K] on the device, values in [0, 1]; with return_stats also the run's statistics {pmax, ref_db, p_lo, p_hi, sel_lo_raw,
        sel_hi_raw} as a device tensor f32[6] (orcai_frontend_stats_dev: no host synchronisation), which backward needs -- the
        workspace itself is overwritten by the next recording.  out: a contiguous f32[T, K] of this device to write into (a recording's rows of a
        batch buffer, predict.predict_wavs) instead of a new tensor.
        With the parameter's denoise key set (orcai_amd/denoise.py; linear or mel route) every channel of the referenced dB spectrogram loses its own
        noise floor -- the order statistic denoise.quantile of the channel over the recording, the median by default -- before the quantile clip, which
        then runs on the denoised values (orcai_make_denoised_spectrogram); the statistics hold p_lo / p_hi as denoised values, pmax of the STFT and
        ref_db 0.  return_profile (denoise only): the f32[K] device tensor of the subtracted floors, in referenced dB, is returned last.  The statistics
        and the profile together are what denoised_spectrogram_backward, the gradient of this route, reads (it recomputes ref_db from pmax).
        With denoise.segment set as well the floor is time-varying (orcai_make_segment_denoised_spectrogram; denoise.segment_denoise_ref is its
        definition) and the profile is f32[S, K], one row per segment.  Forward only."""
        n_fft, hop, K, cfg, pc = resolve_route(spectrogram_parameter)
        dn = denoise.denoise_config(spectrogram_parameter)  # beside the route: Route keeps its five fields
        if return_profile and dn is None:
            raise ValueError("make_spectrogram: return_profile needs the spectrogram parameter denoise (the profile is the per-channel floor it subtracts)")
        pcm = self._check_pcm(pcm)
        n = pcm.numel()
        T = n_frames(n, n_fft, hop)
        if out is None:
            out = torch.empty((T, K), dtype=torch.float32, device=self.device)
        elif not (out.is_cuda and out.dtype == torch.float32 and tuple(out.shape) == (T, K) and out.is_contiguous()):
            raise ValueError(f"make_spectrogram: out must be a contiguous float32 CUDA tensor [{T}, {K}]")
        total = T * K
        r_lo = nearest_rank_index(total, spectrogram_parameter["quantiles"][0])
        r_hi = nearest_rank_index(total, spectrogram_parameter["quantiles"][1])
        signal = (N.ptr(pcm), n, n_fft, hop, T, K)
        profile = None
        if dn is not None:  # the dB spectrogram, linear or mel, minus every channel's own floor
            if T < 1:
                raise ValueError(f"make_spectrogram: spectrogram parameter denoise needs at least one frame, got {T}")
            if "segment" in dn:  # the time-varying floor: one order statistic per (segment, channel), interpolated between the segment centres
                W = denoise.segment_rows(dn["segment"], spectrogram_parameter["sampling_rate"], hop)
                S = denoise.segment_count(T, W)
                profile = torch.empty((S, K), dtype=torch.float32, device=self.device) if return_profile else None
                scratch = self._grown("column_select", self.lib.orcai_segment_column_select_scratch_bytes(T, K, W) // 4)
                rc = self.lib.orcai_make_segment_denoised_spectrogram(*signal, *self._bands(spectrogram_parameter, cfg), W, nearest_rank_index(W, dn["quantile"]),
                                                                      nearest_rank_index(T - (S - 1) * W, dn["quantile"]), r_lo, r_hi, TOP_DB, N.ptr(out),
                                                                      None if profile is None else N.ptr(profile), N.ptr(scratch), N.ptr(self.workspace),
                                                                      N.stream_ptr())
                N.check(rc, "orcai_make_segment_denoised_spectrogram")
            else:
                profile = torch.empty(K, dtype=torch.float32, device=self.device) if return_profile else None
                scratch = self._grown("column_select", self.lib.orcai_column_select_scratch_bytes(K) // 4)
                rc = self.lib.orcai_make_denoised_spectrogram(*signal, *self._bands(spectrogram_parameter, cfg), nearest_rank_index(T, dn["quantile"]), r_lo, r_hi,
                                                              TOP_DB, N.ptr(out), None if profile is None else N.ptr(profile), N.ptr(scratch),
                                                              N.ptr(self.workspace), N.stream_ptr())
                N.check(rc, "orcai_make_denoised_spectrogram")
        elif pc is not None:  # PCEN of the magnitudes, or of the mel band powers when mel is set as well
            a, b = pcen.smoother(pc["time_constant"], spectrogram_parameter["sampling_rate"], hop)
            scratch = self._grown("pcen", self.lib.orcai_pcen_scratch_bytes(T, K) // 4)
            rc = self.lib.orcai_make_pcen_spectrogram(*signal, *self._bands(spectrogram_parameter, cfg), a, b, pc["scale"], pc["gain"], pc["bias"], pc["power"],
                                                      pc["eps"], r_lo, r_hi, N.ptr(out), N.ptr(scratch), N.ptr(self.workspace), N.stream_ptr())
            N.check(rc, "orcai_make_pcen_spectrogram")
        elif cfg is not None:
            rc = self.lib.orcai_make_mel_spectrogram(*signal, *self._bands(spectrogram_parameter, cfg), r_lo, r_hi, TOP_DB, N.ptr(out), N.ptr(self.workspace),
                                                     N.stream_ptr())
            N.check(rc, "orcai_make_mel_spectrogram")
        else:
            N.check(self.lib.orcai_make_spectrogram(*signal, r_lo, r_hi, TOP_DB, N.ptr(out), N.ptr(self.workspace), N.stream_ptr()), "orcai_make_spectrogram")
        res = (out,) + ((self._stats_dev(),) if return_stats else ()) + ((profile,) if return_profile else ())
        return res if len(res) > 1 else out

    # -- the gradient of make_spectrogram w.r.t. the audio (the statistics are held constant) -----------------
    @staticmethod
    def _check_nfft_backward(n_fft: int) -> None:
        n = int(n_fft)
        if n < 32 or n > 4096 or n & (n - 1):
            raise NotImplementedError(f"spectrogram parameter nfft = {n_fft}: the gradient w.r.t. the audio is implemented for powers of two from 32 to "
                                      "4096 (512, the value of orcai-V1, included); the forward runs every size from 2 to 4096")

    def _backward(self, pcm: torch.Tensor, grad: torch.Tensor, stats: torch.Tensor, spectrogram_parameter: dict, who: str, profile: torch.Tensor | None = None):
        """The one body behind backward and denoised_spectrogram_backward: the parameter's and the tensors' refusals under the name who, then the C call
        of the route -- orcai_denoised_spectrogram_bwd with denoise set (the only route that reads profile), else orcai_pcen_spectrogram_bwd with pcen
        set, orcai_mel_spectrogram_bwd with mel alone, orcai_spectrogram_bwd otherwise.  denoise.denoise_config has already run in either caller's own
        refusal; running it here again is what keeps the order of the refusals with one body."""
        dn = denoise.denoise_config(spectrogram_parameter)  # before the route: {denoise, pcen} is refused, not resolved as a PCEN route
        n_fft, hop, K, cfg, pc = resolve_route(spectrogram_parameter)
        if cfg is None:  # (mel.mel_config has refused what the mel route does not differentiate)
            self._check_nfft_backward(n_fft)
        if hop < 1:
            raise ValueError(f"spectrogram parameter n_overlap = {hop} (the hop) must be positive; nfft = {n_fft}")
        pcm = self._check_pcm(pcm)
        n = pcm.numel()
        T = n_frames(n, n_fft, hop)
        sizes = f"nfft = {n_fft}" if cfg is None else f"nfft = {n_fft}, n_mels = {K}"
        if not (isinstance(grad, torch.Tensor) and grad.is_cuda and grad.dtype == torch.float32 and tuple(grad.shape) == (T, K)):
            raise ValueError(f"{who}: grad must be a float32 CUDA tensor [{T}, {K}] ({sizes}, hop = {hop}, {n} samples), got "
                             f"{getattr(grad, 'dtype', None)} {tuple(getattr(grad, 'shape', ()))}")
        if not (isinstance(stats, torch.Tensor) and stats.is_cuda and stats.dtype == torch.float32 and tuple(stats.shape) == (6,)):
            raise ValueError(f"{who} ({sizes}): stats must be the float32 CUDA tensor [6] of make_spectrogram(..., return_stats=True)")
        if dn is not None and not (isinstance(profile, torch.Tensor) and profile.is_cuda and profile.dtype == torch.float32 and tuple(profile.shape) == (K,)):
            raise ValueError(f"{who} ({sizes}): profile must be the float32 CUDA tensor [{K}] of make_spectrogram(..., return_profile=True)")
        dpcm = torch.empty(n, dtype=torch.float32, device=self.device)
        if n == 0:
            return dpcm
        signal = (N.ptr(pcm), n, n_fft, hop, T, K)
        grad, stats = grad.contiguous(), stats.contiguous()
        if dn is not None:
            profile = profile.contiguous()
            rc = self.lib.orcai_denoised_spectrogram_bwd(*signal, *self._bands(spectrogram_parameter, cfg), N.ptr(grad), N.ptr(stats), N.ptr(profile), TOP_DB,
                                                         N.ptr(dpcm), N.stream_ptr())
            N.check(rc, "orcai_denoised_spectrogram_bwd")
        elif pc is not None:
            a, b = pcen.smoother(pc["time_constant"], spectrogram_parameter["sampling_rate"], hop)
            scratch = self._grown("pcen_bwd", self.lib.orcai_pcen_spectrogram_bwd_scratch_bytes(T, K) // 4)
            rc = self.lib.orcai_pcen_spectrogram_bwd(*signal, *self._bands(spectrogram_parameter, cfg), a, b, pc["scale"], pc["gain"], pc["bias"], pc["power"],
                                                     pc["eps"], N.ptr(grad), N.ptr(stats), N.ptr(dpcm), N.ptr(scratch), N.stream_ptr())
            N.check(rc, "orcai_pcen_spectrogram_bwd")
        elif cfg is not None:
            rc = self.lib.orcai_mel_spectrogram_bwd(*signal, *self._bands(spectrogram_parameter, cfg), N.ptr(grad), N.ptr(stats), TOP_DB, N.ptr(dpcm),
                                                    N.stream_ptr())
            N.check(rc, "orcai_mel_spectrogram_bwd")
        else:
            N.check(self.lib.orcai_spectrogram_bwd(*signal, N.ptr(grad), N.ptr(stats), TOP_DB, N.ptr(dpcm), N.stream_ptr()), "orcai_spectrogram_bwd")
        return dpcm

    def backward(self, pcm: torch.Tensor, grad: torch.Tensor, stats: torch.Tensor, spectrogram_parameter: dict, who: str = "backward") -> torch.Tensor:
        """dL/dpcm f32[N] from grad = dL/d(make_spectrogram(pcm)) f32[T, K] and the f32[6] statistics make_spectrogram(..., return_stats=True)
        returned for the same pcm, on the route the parameter asks for: orcai_pcen_spectrogram_bwd with pcen set (on the mel bands when mel is set
        too), orcai_mel_spectrogram_bwd with mel alone, orcai_spectrogram_bwd otherwise.  ref_db, p_lo and p_hi are constants of the backward; the
        filterbank weights and the PCEN parameters get no gradient (include/orcai_hip.h).  who: the name the refusals carry.  A parameter with denoise
        set is refused first (denoise.no_gradient): its gradient is denoised_spectrogram_backward, which also takes the profile."""
        denoise.no_gradient(spectrogram_parameter, who)
        return self._backward(pcm, grad, stats, spectrogram_parameter, who)

    # The named entries: each insists on its own route and is `_backward` otherwise.
    @staticmethod
    def _no_pcen_gradient(spectrogram_parameter: dict, who: str) -> None:
        if pcen.pcen_config(spectrogram_parameter) is not None:
            raise NotImplementedError(f"{who} is a dB front end's gradient and the spectrogram parameter pcen is set: "
                                      "FrontEnd.pcen_spectrogram_backward is the gradient of the PCEN front end")

    def spectrogram_backward(self, pcm: torch.Tensor, grad: torch.Tensor, stats: torch.Tensor, spectrogram_parameter: dict) -> torch.Tensor:
        """backward for the linear dB front end only (orcai_spectrogram_bwd): a parameter whose mel or pcen key is set is refused."""
        denoise.no_gradient(spectrogram_parameter, "spectrogram_backward")
        self._no_pcen_gradient(spectrogram_parameter, "spectrogram_backward")
        if mel.mel_config(spectrogram_parameter) is not None:
            raise NotImplementedError("spectrogram_backward is the linear front end's gradient and the spectrogram parameter mel is set: "
                                      "FrontEnd.mel_spectrogram_backward is the gradient of the mel front end")
        return self.backward(pcm, grad, stats, spectrogram_parameter, who="spectrogram_backward")

    def mel_spectrogram_backward(self, pcm: torch.Tensor, grad: torch.Tensor, stats: torch.Tensor, spectrogram_parameter: dict) -> torch.Tensor:
        """backward for the mel dB front end only (orcai_mel_spectrogram_bwd): grad is f32[T, n_mels]; a parameter without mel, or with pcen, is
        refused.  The parameter's refusals are mel.mel_config's."""
        denoise.no_gradient(spectrogram_parameter, "mel_spectrogram_backward")
        self._no_pcen_gradient(spectrogram_parameter, "mel_spectrogram_backward")
        if mel.mel_config(spectrogram_parameter) is None:
            raise ValueError("mel_spectrogram_backward: the spectrogram parameter mel is absent or null; FrontEnd.spectrogram_backward is the gradient "
                             "of the linear front end")
        return self.backward(pcm, grad, stats, spectrogram_parameter, who="mel_spectrogram_backward")

    def pcen_spectrogram_backward(self, pcm: torch.Tensor, grad: torch.Tensor, stats: torch.Tensor, spectrogram_parameter: dict) -> torch.Tensor:
        """backward for the PCEN front end only, on either route (orcai_pcen_spectrogram_bwd): a parameter without pcen is refused."""
        denoise.no_gradient(spectrogram_parameter, "pcen_spectrogram_backward")
        if pcen.pcen_config(spectrogram_parameter) is None:
            raise ValueError("pcen_spectrogram_backward: the spectrogram parameter pcen is absent or null; FrontEnd.spectrogram_backward and "
                             "FrontEnd.mel_spectrogram_backward are the gradients of the dB front ends")
        return self.backward(pcm, grad, stats, spectrogram_parameter, who="pcen_spectrogram_backward")

    def denoised_spectrogram_backward(self, pcm: torch.Tensor, grad: torch.Tensor, stats: torch.Tensor, profile: torch.Tensor,
                                      spectrogram_parameter: dict) -> torch.Tensor:
        """The gradient of the denoised front end (orcai_denoised_spectrogram_bwd), on the linear or the mel route: dL/dpcm f32[N] from grad =
        dL/d(make_spectrogram(pcm)) f32[T, K] and the f32[6] statistics and f32[K] profile that make_spectrogram(..., return_stats=True,
        return_profile=True) returned for the same pcm and parameter.  ref_db (recomputed from the statistics' pmax), p_lo, p_hi and the per-channel
        floor are constants of the backward (include/orcai_hip.h).  A parameter without denoise is refused (ValueError naming the plain entries), one
        with pcen as denoise.denoise_config refuses it."""
        who = "denoised_spectrogram_backward"
        if denoise.denoise_config(spectrogram_parameter) is None:
            raise ValueError(f"{who}: the spectrogram parameter denoise is absent or null; FrontEnd.spectrogram_backward and FrontEnd.mel_spectrogram_backward "
                             "are the gradients of the plain dB front ends (FrontEnd.pcen_spectrogram_backward of the PCEN one)")
        denoise.no_segment_gradient(spectrogram_parameter, who)  # the time-varying floor has no gradient yet: never the global floor's in its place
        return self._backward(pcm, grad, stats, spectrogram_parameter, who, profile=profile)

    # -- calculate_spectrogram (spectrogram.py:15-55): dB of all bins, referenced and floored ----
    def calculate_db(self, pcm: torch.Tensor, n_fft: int, hop: int) -> torch.Tensor:
        """Returns f32[T, 1 + n_fft//2] (time-major) = amplitude_to_db(|stft|, ref=max)."""
        self._check_nfft(n_fft)
        pcm = self._check_pcm(pcm)
        n = pcm.numel()
        T = n_frames(n, n_fft, hop)
        K = 1 + n_fft // 2
        out = torch.empty((T, K), dtype=torch.float32, device=self.device)
        s = N.stream_ptr()
        ws = N.ptr(self.workspace)
        N.check(self.lib.orcai_frontend_reset(ws, s), "orcai_frontend_reset")
        N.check(self.lib.orcai_stft_db(N.ptr(pcm), n, n_fft, hop, T, K, N.ptr(out), ws, s), "orcai_stft_db")
        N.check(self.lib.orcai_frontend_finalize(1, TOP_DB, ws, s), "orcai_frontend_finalize")
        N.check(self.lib.orcai_db_reference(N.ptr(out), T * K, ws, s), "orcai_db_reference")
        return out

    # -- preprocess_spectrogram on a caller-supplied dB array (spectrogram.py:58-87) ------------
    def preprocess_db(self, db_ft: torch.Tensor, f_lo: int, f_hi: int, quantiles) -> torch.Tensor:
        """db_ft: f32[F, T] on the device (the reference's [freq, time] layout). Returns f32[T, f_hi-f_lo]."""
        assert db_ft.dtype == torch.float32 and db_ft.is_cuda and db_ft.dim() == 2
        db_ft = db_ft.contiguous()
        F, T = db_ft.shape
        K = f_hi - f_lo
        out = torch.empty((T, K), dtype=torch.float32, device=self.device)
        s = N.stream_ptr()
        ws = N.ptr(self.workspace)
        N.check(self.lib.orcai_crop_transpose(N.ptr(db_ft), F, T, f_lo, f_hi, N.ptr(out), s), "orcai_crop_transpose")
        self.normalize_inplace(out, quantiles)
        return out

    def _select_into_workspace(self, x: torch.Tensor, rank_lo: int, rank_hi: int, method: str) -> None:
        """The two order statistics of x into the workspace.  method "level1": reset + orcai_hist_level1 + orcai_quantile_select, whose cost depends on
        where the values lie (tuned for dB); "radix": orcai_quantile_select_radix, three reads of x for any values.  Both are exact: same bytes."""
        total = x.numel()
        s = N.stream_ptr()
        ws = N.ptr(self.workspace)
        if method == "level1":
            N.check(self.lib.orcai_frontend_reset(ws, s), "orcai_frontend_reset")
            N.check(self.lib.orcai_hist_level1(N.ptr(x), total, ws, s), "orcai_hist_level1")
            N.check(self.lib.orcai_quantile_select(N.ptr(x), total, rank_lo, rank_hi, ws, s), "orcai_quantile_select")
        elif method == "radix":
            N.check(self.lib.orcai_quantile_select_radix(N.ptr(x), total, rank_lo, rank_hi, ws, s), "orcai_quantile_select_radix")
        else:
            raise ValueError(f"method must be 'level1' or 'radix', got {method!r}")
        N.check(self.lib.orcai_frontend_finalize(0, TOP_DB, ws, s), "orcai_frontend_finalize")

    def normalize_inplace(self, x: torch.Tensor, quantiles, method: str = "level1") -> None:
        """Exact percentile clip + min-max normalise of a final-dB array, in place.  method: _select_into_workspace's."""
        total = x.numel()
        r_lo = nearest_rank_index(total, quantiles[0])
        r_hi = nearest_rank_index(total, quantiles[1])
        self._select_into_workspace(x, r_lo, r_hi, method)
        N.check(self.lib.orcai_clip_normalize(N.ptr(x), total, N.ptr(self.workspace), N.stream_ptr()), "orcai_clip_normalize")

    def select(self, x: torch.Tensor, rank_lo: int, rank_hi: int, method: str = "level1") -> tuple[float, float]:
        """Exact rank_lo-th / rank_hi-th smallest of a device f32 array (test hook for the selection kernels).  method: _select_into_workspace's."""
        self._select_into_workspace(x, rank_lo, rank_hi, method)
        st = self.stats()
        return st["sel_lo_raw"], st["sel_hi_raw"]

    def percentiles(self, x: torch.Tensor, q, dim: int | None = None, segment_rows: int | None = None) -> torch.Tensor:
        """Exact percentiles of any contiguous f32 CUDA tensor, taken flat: element i is the nearest_rank_index(x.numel(), q[i])-th smallest value, what
        ``np.percentile(x, 100 * q[i], method="nearest")`` returns for float32 data.  q: a sequence of fractions in [0, 1].  Returns f32[len(q)] on
        the device with no host synchronisation.  The ranks go through the radix select two at a time (a single one twice).
        dim=0: per column instead -- x of at least two dimensions is read as [R, C], C the product of the others (at most 4096), and the result is
        f32[len(q), *x.shape[1:]], what ``np.percentile(x, 100 * q, axis=0, method="nearest")`` returns: one orcai_column_select per q with rank
        nearest_rank_index(R, q[i]).  No other dim is implemented.
        segment_rows=W (dim=0 only): per column inside every segment of W rows -- S = max(1, R // W) segments, the last one taking the remainder -- by
        orcai_segment_column_select: f32[len(q), S, *x.shape[1:]], or f32[S, *x.shape[1:]] when q is a single number instead of a sequence."""
        if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32):
            raise TypeError("percentiles: x must be a float32 CUDA tensor")
        if not x.is_contiguous():
            raise ValueError("percentiles: x must be contiguous")
        one_q = segment_rows is not None and isinstance(q, (int, float, np.integer, np.floating))  # a single fraction: no leading q axis (segment_rows only)
        q = [float(q)] if one_q else [float(v) for v in q]
        total = x.numel()
        if not q or total == 0 or not all(0.0 <= v <= 1.0 for v in q):
            raise ValueError(f"percentiles: q must be a non-empty sequence of fractions in [0, 1] and x non-empty, got q = {q}, {total} values")
        if segment_rows is not None and dim is None:
            raise ValueError("percentiles: segment_rows needs dim=0 (segments are runs of rows)")
        if dim is not None:
            if dim != 0 or isinstance(dim, bool):
                raise ValueError(f"percentiles: dim must be None (flat) or 0 (per column of [R, C]), got {dim!r}; selects along other dimensions are not implemented")
            if x.dim() < 2:
                raise ValueError(f"percentiles: dim=0 needs a tensor of at least two dimensions, got shape {tuple(x.shape)}")
            R, cols = x.shape[0], total // x.shape[0]
            if cols > 4096:
                raise ValueError(f"percentiles: dim=0 takes at most 4096 columns (orcai_column_select), got {cols} for shape {tuple(x.shape)}")
            if segment_rows is not None:
                W = int(segment_rows)
                if isinstance(segment_rows, bool) or W != segment_rows or W < 1:
                    raise ValueError(f"percentiles: segment_rows must be a positive integer, got {segment_rows!r}")
                S = denoise.segment_count(R, W)
                res = torch.empty((len(q), S, *x.shape[1:]), dtype=torch.float32, device=self.device)
                scratch = self._grown("column_select", self.lib.orcai_segment_column_select_scratch_bytes(R, cols, W) // 4)
                for i, v in enumerate(q):
                    rc = self.lib.orcai_segment_column_select(N.ptr(x), R, cols, W, nearest_rank_index(W, v), nearest_rank_index(R - (S - 1) * W, v), N.ptr(res[i]),
                                                              N.ptr(scratch), N.stream_ptr())
                    N.check(rc, "orcai_segment_column_select")
                return res[0] if one_q else res
            res = torch.empty((len(q), *x.shape[1:]), dtype=torch.float32, device=self.device)
            scratch = self._grown("column_select", self.lib.orcai_column_select_scratch_bytes(cols) // 4)
            for i, v in enumerate(q):
                rc = self.lib.orcai_column_select(N.ptr(x), R, cols, nearest_rank_index(R, v), N.ptr(res[i]), N.ptr(scratch), N.stream_ptr())
                N.check(rc, "orcai_column_select")
            return res
        ranks = [nearest_rank_index(total, v) for v in q]
        pairs = torch.empty((len(ranks) + 1) // 2, 6, dtype=torch.float32, device=self.device)
        s = N.stream_ptr()
        ws = N.ptr(self.workspace)
        for i in range(0, len(ranks), 2):
            r_lo, r_hi = ranks[i], ranks[min(i + 1, len(ranks) - 1)]
            N.check(self.lib.orcai_quantile_select_radix(N.ptr(x), total, r_lo, r_hi, ws, s), "orcai_quantile_select_radix")
            N.check(self.lib.orcai_frontend_finalize(0, TOP_DB, ws, s), "orcai_frontend_finalize")
            N.check(self.lib.orcai_frontend_stats_dev(ws, N.ptr(pairs[i // 2]), s), "orcai_frontend_stats_dev")
        return pairs[:, 4:6].reshape(-1)[:len(ranks)].contiguous()  # sel_lo_raw, sel_hi_raw of each pair

    def stats(self) -> dict:
        """Synchronises; {pmax, ref_db, p_lo, p_hi, sel_lo_raw, sel_hi_raw} of the last run."""
        buf = (C.c_float * 6)()
        N.check(self.lib.orcai_frontend_stats_host(N.ptr(self.workspace), buf, N.stream_ptr()), "orcai_frontend_stats_host")
        keys = ["pmax", "ref_db", "p_lo", "p_hi", "sel_lo_raw", "sel_hi_raw"]
        return {k: float(np.float32(v)) for k, v in zip(keys, buf)}

    def _check_pcm(self, pcm: torch.Tensor) -> torch.Tensor:
        if not (isinstance(pcm, torch.Tensor) and pcm.is_cuda and pcm.dtype == torch.float32 and pcm.dim() == 1):
            raise TypeError("pcm must be a 1-D float32 CUDA tensor")
        return pcm.contiguous()


_FRONTENDS: dict = {}


def get_frontend(device: torch.device | str | None = None) -> FrontEnd:
    if not torch.cuda.is_available():
        raise RuntimeError("orcai_amd needs a ROCm GPU: there is no CPU fallback for the front end")
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    key = (dev.type, dev.index if dev.index is not None else torch.cuda.current_device())
    if key not in _FRONTENDS:
        _FRONTENDS[key] = FrontEnd(torch.device("cuda", key[1]))
    return _FRONTENDS[key]
