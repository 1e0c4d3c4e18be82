"""Sampling-rate conversion on the GPU (the resampling half of ``librosa.load(sr=...)``, reference
``src/orcAI/spectrogram.py:23-27``).

librosa's default ``res_type="soxr_hq"`` cannot be matched bit-for-bit (libsoxr is absent: parity unpinned,
SURVEY 8c).  This is an exact rational polyphase Kaiser-windowed-sinc filter; the table is designed here in
float64 and applied by ``csrc/resample.hip``.  ``resample_backward_device`` is its adjoint with the same table (the resampler is linear: that is
its whole gradient); ``orcai_amd.torch_ops`` wraps both as ``torch.ops.orcai.resample`` with autograd.
"""

from __future__ import annotations

import math
from functools import lru_cache

import numpy as np
import torch

from orcai_amd import _native as N

NUM_ZEROS = 64
KAISER_BETA = 14.769656459379492
ROLLOFF = 0.9475937167399596


def ratio(sr_in: int, sr_out: int) -> tuple[int, int]:
    g = math.gcd(int(sr_in), int(sr_out))
    return int(sr_out) // g, int(sr_in) // g  # L (up), M (down)


def output_length(n_in: int, sr_in: int, sr_out: int) -> int:
    """``librosa.resample`` output length: ceil(n * sr_out / sr_in)."""
    return int(math.ceil(n_in * sr_out / sr_in))


@lru_cache(maxsize=8)
def design_table(L: int, M: int) -> np.ndarray:
    """float32 [L][ntaps]: tap j of phase p weighs input sample i0 - ntaps/2 + 1 + j for output time i0 + p/L."""
    scale = min(1.0, L / M)
    half = int(math.ceil(NUM_ZEROS / scale))
    ntaps = 2 * half
    ntaps += (-ntaps) % 4
    j = np.arange(ntaps, dtype=np.float64)[None, :]
    p = np.arange(L, dtype=np.float64)[:, None]
    t = j - (ntaps // 2 - 1) - p / L  # input offset relative to the output instant
    fc = scale * ROLLOFF
    u = t * scale / NUM_ZEROS
    inside = np.abs(u) < 1.0
    win = np.where(inside, np.i0(KAISER_BETA * np.sqrt(np.clip(1.0 - u * u, 0.0, 1.0))) / np.i0(KAISER_BETA), 0.0)
    return np.ascontiguousarray((fc * np.sinc(fc * t) * win).astype(np.float32))


_DEVICE_TABLES: dict = {}


def device_table(L: int, M: int, device: torch.device) -> torch.Tensor:
    """design_table(L, M) on `device`, uploaded once per (L, M, device): the forward and the backward read the same tensor."""
    index = device.index if device.index is not None else torch.cuda.current_device()
    key = (L, M, index)
    table = _DEVICE_TABLES.get(key)
    if table is None:
        table = _DEVICE_TABLES[key] = torch.from_numpy(design_table(L, M)).to(torch.device("cuda", index))
    return table


def resample_device(pcm: torch.Tensor, sr_in: int, sr_out: int) -> torch.Tensor:
    """f32 cuda [N] at sr_in -> f32 cuda [ceil(N*sr_out/sr_in)] at sr_out."""
    if sr_in == sr_out:
        return pcm
    if not (pcm.is_cuda and pcm.dtype == torch.float32 and pcm.dim() == 1):
        raise TypeError("pcm must be a 1-D float32 CUDA tensor")
    L, M = ratio(sr_in, sr_out)
    table = device_table(L, M, pcm.device)
    n_in = pcm.numel()
    n_out = output_length(n_in, sr_in, sr_out)
    out = torch.empty(n_out, dtype=torch.float32, device=pcm.device)
    x = pcm.contiguous()
    with torch.cuda.device(pcm.device):
        N.check(N.lib().orcai_resample_polyphase(N.ptr(x), n_in, N.ptr(out), n_out, L, M, N.ptr(table), table.shape[1], N.stream_ptr()), "orcai_resample_polyphase")
    return out


def resample_backward_device(dout: torch.Tensor, n_in: int, sr_in: int, sr_out: int) -> torch.Tensor:
    """The adjoint of resample_device: dout f32 cuda [ceil(n_in*sr_out/sr_in)] = dL/d(resampled) -> f32 cuda [n_in] = dL/dpcm (orcai_resample_polyphase_bwd)."""
    if not (dout.is_cuda and dout.dtype == torch.float32 and dout.dim() == 1):
        raise TypeError("dout must be a 1-D float32 CUDA tensor")
    n_in = int(n_in)
    if dout.numel() != output_length(n_in, sr_in, sr_out):
        raise ValueError(f"dout has {dout.numel()} samples; {n_in} samples at {sr_in} Hz resample to {output_length(n_in, sr_in, sr_out)} at {sr_out} Hz")
    if sr_in == sr_out:
        return dout
    L, M = ratio(sr_in, sr_out)
    table = device_table(L, M, dout.device)
    dx = torch.empty(n_in, dtype=torch.float32, device=dout.device)
    g = dout.contiguous()
    with torch.cuda.device(dout.device):
        N.check(N.lib().orcai_resample_polyphase_bwd(N.ptr(g), g.numel(), N.ptr(dx), n_in, L, M, N.ptr(table), table.shape[1], N.stream_ptr()), "orcai_resample_polyphase_bwd")
    return dx
