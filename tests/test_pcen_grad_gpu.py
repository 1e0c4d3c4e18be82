"""The gradient of the PCEN front end w.r.t. the audio on the GPU: the reverse scan orcai_pcen_bwd against the float64 specification
pcen.pcen_bwd_ref, its gates against the forward's clip bit for bit, the two energy epilogues of the STFT backward, the one call
orcai_pcen_spectrogram_bwd against the float64 reference of tests/pcen_grad_ref.py, the launchers' contracts and refusals, the torch ops and the chain
native-rate pcm -> PcenWaveformFrontEnd -> snippets -> OrcaiModule(input_grad="eval") -> loss differentiated down to the waveform."""

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import pcen_grad_ref as R  # noqa: E402
import orcai_amd.torch_ops  # noqa: E402, F401  (registers the ops)
from orcai_amd import pcen  # noqa: E402

# Measured on the CPU for exactly these inputs (tests/pcen_grad_ref.py run as a script prints the three tables).  The bar for a kernel is 8 x the value of
# its case (the f32 evaluation of the same formula is what the hardware can be asked for, 8 covers another legitimate summation order).
# The scan alone: a float32 numpy restatement of the sequential formulas (R.pcen_bwd_f32) against pcen_bwd_ref, as a share of max|dE|.
# Key: (parameter set, index into R.SCAN_SHAPES).
SCAN_F32_DEVIATION = {
    ("default", 0): 8.37e-07,  # T 1 K 171: tie share 0.0e+00, clipped 0.07 / 0.12
    ("default", 1): 1.61e-07,  # T 2 K 1: tie share 0.0e+00, clipped 0.00 / 0.00
    ("default", 2): 3.13e-07,  # T 255 K 64: tie share 0.0e+00, clipped 0.10 / 0.10
    ("default", 3): 2.96e-07,  # T 256 K 65: tie share 0.0e+00, clipped 0.10 / 0.09
    ("default", 4): 2.59e-06,  # T 257 K 171: tie share 0.0e+00, clipped 0.10 / 0.10
    ("default", 5): 1.95e-07,  # T 513 K 63: tie share 0.0e+00, clipped 0.10 / 0.11
    ("default", 6): 3.61e-07,  # T 1030 K 171: tie share 0.0e+00, clipped 0.10 / 0.10
    ("default", 7): 5.91e-07,  # T 4501 K 8: tie share 0.0e+00, clipped 0.10 / 0.10
    ("long", 0): 1.95e-06,  # T 1 K 171: tie share 0.0e+00, clipped 0.08 / 0.13
    ("long", 1): 2.76e-07,  # T 2 K 1: tie share 0.0e+00, clipped 0.00 / 0.00
    ("long", 2): 9.78e-07,  # T 255 K 64: tie share 0.0e+00, clipped 0.10 / 0.12
    ("long", 3): 7.08e-07,  # T 256 K 65: tie share 0.0e+00, clipped 0.10 / 0.08
    ("long", 4): 5.79e-08,  # T 257 K 171: tie share 0.0e+00, clipped 0.10 / 0.10
    ("long", 5): 6.04e-07,  # T 513 K 63: tie share 0.0e+00, clipped 0.10 / 0.10
    ("long", 6): 6.62e-07,  # T 1030 K 171: tie share 0.0e+00, clipped 0.10 / 0.10
    ("long", 7): 1.43e-06,  # T 4501 K 8: tie share 0.0e+00, clipped 0.10 / 0.10
    ("gain0", 0): 4.58e-08,  # T 1 K 171: tie share 0.0e+00, clipped 0.09 / 0.09
    ("gain0", 1): 1.01e-07,  # T 2 K 1: tie share 0.0e+00, clipped 0.00 / 0.00
    ("gain0", 2): 6.23e-08,  # T 255 K 64: tie share 0.0e+00, clipped 0.07 / 0.10
    ("gain0", 3): 5.80e-08,  # T 256 K 65: tie share 0.0e+00, clipped 0.07 / 0.10
    ("gain0", 4): 9.89e-08,  # T 257 K 171: tie share 0.0e+00, clipped 0.07 / 0.09
    ("gain0", 5): 7.64e-08,  # T 513 K 63: tie share 0.0e+00, clipped 0.07 / 0.11
    ("gain0", 6): 9.24e-08,  # T 1030 K 171: tie share 0.0e+00, clipped 0.07 / 0.07
    ("gain0", 7): 9.30e-08,  # T 4501 K 8: tie share 0.0e+00, clipped 0.08 / 0.07
    ("power1", 0): 1.11e-06,  # T 1 K 171: tie share 0.0e+00, clipped 0.08 / 0.09
    ("power1", 1): 2.36e-07,  # T 2 K 1: tie share 0.0e+00, clipped 0.00 / 0.00
    ("power1", 2): 3.62e-07,  # T 255 K 64: tie share 0.0e+00, clipped 0.10 / 0.11
    ("power1", 3): 3.74e-07,  # T 256 K 65: tie share 0.0e+00, clipped 0.10 / 0.10
    ("power1", 4): 1.62e-07,  # T 257 K 171: tie share 0.0e+00, clipped 0.10 / 0.11
    ("power1", 5): 2.46e-07,  # T 513 K 63: tie share 0.0e+00, clipped 0.10 / 0.11
    ("power1", 6): 7.64e-07,  # T 1030 K 171: tie share 0.0e+00, clipped 0.10 / 0.10
    ("power1", 7): 2.74e-07,  # T 4501 K 8: tie share 0.0e+00, clipped 0.10 / 0.10
    ("bias0", 0): 2.83e-06,  # T 1 K 171: tie share 0.0e+00, clipped 0.08 / 0.07
    ("bias0", 1): 1.75e-07,  # T 2 K 1: tie share 0.0e+00, clipped 0.00 / 0.00
    ("bias0", 2): 2.57e-07,  # T 255 K 64: tie share 0.0e+00, clipped 0.08 / 0.11
    ("bias0", 3): 3.81e-07,  # T 256 K 65: tie share 0.0e+00, clipped 0.11 / 0.10
    ("bias0", 4): 4.13e-07,  # T 257 K 171: tie share 0.0e+00, clipped 0.09 / 0.10
    ("bias0", 5): 2.83e-07,  # T 513 K 63: tie share 0.0e+00, clipped 0.09 / 0.10
    ("bias0", 6): 3.09e-07,  # T 1030 K 171: tie share 0.0e+00, clipped 0.07 / 0.10
    ("bias0", 7): 7.06e-07,  # T 4501 K 8: tie share 0.0e+00, clipped 0.08 / 0.10
    ("a0", 0): 2.04e-06,  # T 1 K 171: tie share 0.0e+00, clipped 0.07 / 0.09
    ("a0", 1): 1.53e-06,  # T 2 K 1: tie share 0.0e+00, clipped 0.00 / 0.00
    ("a0", 2): 2.21e-06,  # T 255 K 64: tie share 0.0e+00, clipped 0.10 / 0.10
    ("a0", 3): 3.72e-06,  # T 256 K 65: tie share 0.0e+00, clipped 0.10 / 0.10
    ("a0", 4): 2.67e-06,  # T 257 K 171: tie share 0.0e+00, clipped 0.10 / 0.10
    ("a0", 5): 2.55e-06,  # T 513 K 63: tie share 0.0e+00, clipped 0.10 / 0.10
    ("a0", 6): 2.90e-06,  # T 1030 K 171: tie share 0.0e+00, clipped 0.10 / 0.10
    ("a0", 7): 3.27e-06,  # T 4501 K 8: tie share 0.0e+00, clipped 0.10 / 0.10
}
# End to end: torch's float32 evaluation of the whole chain against its float64 one, as a share of max|dpcm|.  Key: (recording, index into R.CASES).
F32_REFERENCE_DEVIATION = {
    ("a", 0): 1.06e-06,  # linear 512 / 256: tie share 2.1e-04
    ("a", 1): 2.54e-06,  # linear 1024 / 512: tie share 2.2e-04
    ("a", 2): 2.53e-05,  # linear 2048 / 300: tie share 1.6e-04
    ("a", 3): 4.67e-06,  # linear 32 / 16: tie share 1.6e-04
    ("a", 4): 5.30e-07,  # mel 512 / 256 / 64: tie share 5.0e-04
    ("a", 5): 5.12e-06,  # mel 128 / 32 / 8: tie share 3.6e-04
    ("a", 6): 4.19e-07,  # mel 4096 / 1000 / 64: tie share 3.2e-04
    ("b", 0): 2.04e-06,  # linear 512 / 256: tie share 3.1e-04
    ("b", 1): 1.60e-06,  # linear 1024 / 512: tie share 2.7e-04
    ("b", 2): 2.08e-05,  # linear 2048 / 300: tie share 3.0e-04
    ("b", 3): 6.45e-06,  # linear 32 / 16: tie share 1.8e-04
    ("b", 4): 4.00e-07,  # mel 512 / 256 / 64: tie share 5.8e-04
    ("b", 5): 3.12e-06,  # mel 128 / 32 / 8: tie share 3.1e-04
    ("b", 6): 6.17e-07,  # mel 4096 / 1000 / 64: tie share 4.3e-04
}
# The energy backwards alone, likewise.  Key: index into R.ENERGY_CASES.
ENERGY_F32_DEVIATION = {
    0: 4.26e-06,  # linear 512 / 256
    1: 5.52e-06,  # linear 2048 / 300
    2: 1.50e-07,  # mel 512 / 256 / 64
    3: 2.53e-07,  # mel 2048 / 300 / 64
}
LIN = (48000, 512, 256, 16000.0, 0, 0.0, 0.0, False, True, 0.4, 0.98, 2.0, 0.5, 1e-6, 2.0**31, 0.01, 0.999)
MEL = (48000, 512, 256, 0.0, 64, 0.0, 24000.0, False, True, 0.4, 0.98, 2.0, 0.5, 1e-6, 2.0**31, 0.30, 0.999)
SP_LIN = R.parameter(R.CASES[0], "a")
SP_MEL = R.parameter(R.CASES[4], "a")


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(torch.int32), b.view(torch.int32))


def _fe():
    from orcai_amd.frontend import get_frontend

    return get_frontend()


def _lib():
    from orcai_amd import _native as N

    return N.lib(), N


def _p(t):
    return 0 if t is None else t.data_ptr()


def _stats(p_lo, p_hi):
    return torch.tensor([0.0, 0.0, p_lo, p_hi, p_lo, p_hi], dtype=torch.float32, device="cuda")


def _scalars(cfg, sr, hop):
    a, b = pcen.smoother(cfg["time_constant"], sr, hop)
    return [a, b, cfg["scale"], cfg["gain"], cfg["bias"], cfg["power"], cfg["eps"]]


def _scan(E, g, stats, T, K, scalars, dE, scratch="own"):
    """orcai_pcen_bwd itself (return code, no exception)."""
    lib, N = _lib()
    if isinstance(scratch, str):
        scratch = torch.empty(lib.orcai_pcen_bwd_scratch_bytes(T, K) // 4, dtype=torch.float32, device="cuda")
        assert scratch.numel() == 4 * ((T + 255) // 256) * K + 2 * T * K
    return lib.orcai_pcen_bwd(_p(E), _p(g), _p(stats), T, K, *scalars, _p(dE), _p(scratch), N.stream_ptr())


# ------------------------------------------------------------------------------------------------------------------ 1. the scan against its specification
@pytest.mark.parametrize("name", list(R.SCAN_PARAMETERS))
@pytest.mark.parametrize("shape", range(len(R.SCAN_SHAPES)))
def test_scan_against_the_float64_specification(shape, name):
    c = R.scan_case(shape, name)
    T, K = R.SCAN_SHAPES[shape]
    if name == "long":
        assert pcen.smoother(c["cfg"]["time_constant"], c["sr"], c["hop"])[0] ** 256 > 0.5  # carries across chunks matter
    if name == "a0":
        assert pcen.smoother(c["cfg"]["time_constant"], c["sr"], c["hop"]) == (0.0, 1.0)
    E = torch.tensor(c["E"], device="cuda")
    dE = torch.full((T, K), float("nan"), device="cuda")
    assert _scan(E, torch.tensor(c["g"], device="cuda"), _stats(*c["stats"]), T, K, _scalars(c["cfg"], c["sr"], c["hop"]), dE) == 0
    assert torch.isfinite(dE).all()
    ref = c["dE64"]
    share = float(np.abs(dE.cpu().numpy().astype(np.float64) - ref).max() / np.abs(ref).max())
    dev = SCAN_F32_DEVIATION[(name, shape)]
    print(f"orcai_pcen_bwd T={T} K={K} {name}: kernel error {share:.2e} of max|dE|; float32 restatement {dev:.2e}; bar {8 * dev:.2e}")
    assert share <= 8 * dev, (share, dev)


# ------------------------------------------------------------------------------------------------------------------ 2. the gates are the forward's
def test_gates_agree_with_the_forwards_clip_exactly():
    """gain = 0: no coupling in time, dE[t] = scale d[t].  dE is exactly 0 wherever orcai_pcen followed by the percentile clip gave 0.0 or 1.0, and
    non-zero wherever out lies strictly inside (0, 1) and g is not zero."""
    lib, N = _lib()
    fe = _fe()
    for shape in (4, 6):  # 257 x 171: a chunk of one frame; 1030 x 171
        c = R.scan_case(shape, "gain0")
        T, K = R.SCAN_SHAPES[shape]
        sc = _scalars(c["cfg"], c["sr"], c["hop"])
        E = torch.tensor(c["E"], device="cuda")
        out = E.clone()
        scratch = torch.empty(lib.orcai_pcen_scratch_bytes(T, K) // 4, dtype=torch.float32, device="cuda")
        assert lib.orcai_pcen(out.data_ptr(), T, K, *sc, scratch.data_ptr(), N.stream_ptr()) == 0
        fe.normalize_inplace(out, (0.1, 0.9))
        stats = torch.empty(6, device="cuda")
        assert lib.orcai_frontend_stats_dev(N.ptr(fe.workspace), stats.data_ptr(), N.stream_ptr()) == 0
        g = torch.randn((T, K), device="cuda", generator=torch.Generator("cuda").manual_seed(5))
        g[::7, ::3] = 0.0
        dE = torch.full((T, K), float("nan"), device="cuda")
        assert _scan(E, g, stats, T, K, sc, dE) == 0
        clipped = (out == 0.0) | (out == 1.0)
        assert 0.15 < float(clipped.float().mean()) < 0.25
        assert not dE[clipped].view(torch.int32).bitwise_and(0x7FFFFFFF).any()  # +0.0 or -0.0, nothing else
        inside = (out > 0.0) & (out < 1.0) & (g != 0.0)
        assert bool((dE[inside] != 0.0).all()) and torch.isfinite(dE).all()


# ------------------------------------------------------------------------------------------------------------------ 3. determinism and coverage
def test_scan_twice_gives_identical_bits_writes_every_element_and_leaves_E_alone():
    c = R.scan_case(6, "long")
    T, K = R.SCAN_SHAPES[6]
    E = torch.tensor(c["E"], device="cuda")
    before = E.clone()
    g, stats, sc = torch.tensor(c["g"], device="cuda"), _stats(*c["stats"]), _scalars(c["cfg"], c["sr"], c["hop"])
    outs = []
    for _ in range(2):
        dE = torch.full((T, K), float("nan"), device="cuda")
        assert _scan(E, g, stats, T, K, sc, dE) == 0
        outs.append(dE)
    assert torch.isfinite(outs[0]).all() and same_bits(outs[0], outs[1]) and same_bits(E, before)


@pytest.mark.parametrize("index", [0, 2, 6])  # linear 512 / 256; linear 2048 / 300 (workgroup per run); mel 4096 / 1000 / 64 (more than 64 KiB of LDS)
def test_one_call_twice_gives_identical_bits_and_writes_every_element(index):
    pc = R.CASES[index]
    c = R.case("b", index)
    outs = []
    for _ in range(2):
        dpcm = torch.full((c["pcm"].numel(),), float("nan"), device="cuda")
        assert _one_call(c["pcm"].cuda(), R.parameter(pc, "b"), c["g"].cuda(), R.stats_tensor(c, "cuda"), dpcm) == 0
        outs.append(dpcm)
    assert torch.isfinite(outs[0]).all() and float(outs[0].abs().max()) > 0 and same_bits(outs[0], outs[1])


def test_one_call_twice_mel_2048():
    """2048 / 300 with 64 mel bands: the workgroup-per-run mel kernel below the LDS opt-in."""
    mc = R.MG.CASES[4]
    pc = ("mel", mc)
    sp = R.parameter(pc, "b")
    pcm = torch.from_numpy(R.G.recording("b").copy()).cuda()
    T = 1 + pcm.numel() // mc[1]
    g = torch.randn((T, mc[2]), device="cuda", generator=torch.Generator("cuda").manual_seed(3))
    spec, stats = _fe().make_spectrogram(pcm, sp, return_stats=True)
    outs = []
    for _ in range(2):
        dpcm = torch.full((pcm.numel(),), float("nan"), device="cuda")
        assert _one_call(pcm, sp, g, stats, dpcm) == 0
        outs.append(dpcm)
    assert torch.isfinite(outs[0]).all() and float(outs[0].abs().max()) > 0 and same_bits(outs[0], outs[1])


def _one_call(pcm, sp, g, stats, dpcm, scratch="own", n_frames=None, hop=None, nfft=None, scalars=None, null_pcm=False):
    """orcai_pcen_spectrogram_bwd itself (return code, no exception), its arguments derived from a spectrogram parameter as FrontEnd does."""
    from orcai_amd import mel

    lib, N = _lib()
    fe = _fe()
    cfg = pcen.pcen_config(sp)
    mcfg = mel.mel_config(sp)
    hop = int(sp["n_overlap"]) if hop is None else hop
    n = pcm.numel()
    T = (1 + n // int(sp["n_overlap"])) if n_frames is None else n_frames
    K = fe._kept_bins(sp)
    if mcfg is not None:
        t, w = fe._mel_table(sp, mcfg)
        bands = (t["lo"].ctypes.data, t["hi"].ctypes.data, t["off"].ctypes.data, N.ptr(w), w.numel())
    else:
        bands = (None, None, None, None, 0)
    if isinstance(scratch, str):
        scratch = torch.empty(lib.orcai_pcen_spectrogram_bwd_scratch_bytes(max(T, 1), K) // 4, dtype=torch.float32, device="cuda")
    sc = _scalars(cfg, sp["sampling_rate"], int(sp["n_overlap"])) if scalars is None else scalars
    return lib.orcai_pcen_spectrogram_bwd(0 if null_pcm else _p(pcm), n, int(sp["nfft"]) if nfft is None else nfft, hop, T, K, *bands, *sc, _p(g), _p(stats), _p(dpcm), _p(scratch),
                                          N.stream_ptr())


# ------------------------------------------------------------------------------------------------------------------ 4. dpcm against float64, end to end
@pytest.mark.parametrize("which", ["a", "b"])
@pytest.mark.parametrize("index", range(len(R.CASES)))
def test_dpcm_against_the_float64_reference(which, index):
    pc = R.CASES[index]
    c = R.case(which, index)
    dpcm = _fe().pcen_spectrogram_backward(c["pcm"].cuda(), c["g"].cuda(), R.stats_tensor(c, "cuda"), R.parameter(pc, which))
    ref = c["dpcm64"]
    share = float((dpcm.cpu().double() - ref).abs().max() / ref.abs().max())
    dev = F32_REFERENCE_DEVIATION[(which, index)]
    print(f"({which}) {R.label(pc)}: kernel error {share:.2e} of max|dpcm|; torch f32 {dev:.2e}; bar {8 * dev:.2e}")
    assert torch.isfinite(dpcm).all()
    assert share <= 8 * dev, (share, dev)


def test_a_recording_shorter_than_one_window():
    """100 samples, one frame of 512: T = 1, the scan's chain of one element.  The bar is 8 x the float32 deviation of this very case."""
    pc = R.CASES[0]
    pcm = torch.from_numpy(R.G.recording("a")[:100].copy())
    c = R.build_case(pcm, pc, (0.01, 0.999), seed=9)
    ref = c["dpcm64"]
    dev = R.f32_error_share(c, pc)
    dpcm = _fe().pcen_spectrogram_backward(pcm.cuda(), c["g"].cuda(), R.stats_tensor(c, "cuda"), SP_LIN)
    share = float((dpcm.cpu().double() - ref).abs().max() / ref.abs().max())
    print(f"100 samples: kernel error {share:.2e} of max|dpcm|; torch f32 {dev:.2e}")
    assert c["out64"].shape == (1, 171) and dpcm.shape == (100,) and float(ref.abs().max()) > 0 and share <= 8 * dev, (share, dev)


# ------------------------------------------------------------------------------------------------------------------ 5. the coupling in time
@pytest.mark.parametrize("index, columns", [(0, (0, 31, 63)), (4, (31, 40, 63))], ids=["linear", "mel"])  # columns whose value at frame 20 lies inside the clip
def test_one_element_reaches_its_own_frame_and_the_earlier_ones_only(index, columns):
    """g zero but for (frame 20, one column): the value depends on frame 20's energy and, through the smoother, on every EARLIER frame's -- on none
    after it.  dpcm is zero from 20 hop + nfft/2 on, non-zero before frame 20's own window, and equals the float64 gradient of that single element."""
    pc = R.CASES[index]
    nfft, hop = R.sizes(pc)
    c = R.case("a", index)
    pcm = c["pcm"][:20000].contiguous()
    p_lo, p_hi = c["stats"]
    sp = R.parameter(pc, "a")
    for k in columns:
        x = pcm.double().requires_grad_()
        out, aux = R.forward(x, pc, None, stats=c["stats"])
        y = float(aux["y"][20, k])
        assert p_lo + 0.01 < y < p_hi - 0.01, (k, y, p_lo, p_hi)  # the element's gate is open, away from ties
        g = torch.zeros(out.shape)
        g[20, k] = 1.0
        (ref,) = torch.autograd.grad(out, x, g.double())
        dpcm = _fe().pcen_spectrogram_backward(pcm.cuda(), g.cuda(), R.stats_tensor(c, "cuda"), sp).cpu()
        a, b = 20 * hop - nfft // 2, 20 * hop + nfft // 2
        assert not dpcm[b:].any(), k
        assert dpcm[:a].any() and float(ref[:a].abs().max()) > 0, k
        assert float((dpcm.double() - ref).abs().max() / ref.abs().max()) <= 1e-4, k


# ------------------------------------------------------------------------------------------------------------------ 6. the energy backwards alone
@pytest.mark.parametrize("index", range(len(R.ENERGY_CASES)))
def test_energy_backward_against_float64(index):
    from orcai_amd import mel

    lib, N = _lib()
    pc = R.ENERGY_CASES[index]
    c = R.energy_case(index)
    nfft, hop = R.sizes(pc)
    pcm, gE = c["pcm"].cuda(), c["gE"].cuda()
    n = pcm.numel()
    T, K = gE.shape
    dpcm = torch.full((n,), float("nan"), device="cuda")
    if pc[0] == "mel":
        sp = R.parameter(pc, "b")
        t, w = _fe()._mel_table(sp, mel.mel_config(sp))
        rc = lib.orcai_stft_mel_energy_bwd(pcm.data_ptr(), n, nfft, hop, T, K, t["lo"].ctypes.data, t["hi"].ctypes.data, t["off"].ctypes.data, w.data_ptr(), w.numel(),
                                           gE.data_ptr(), dpcm.data_ptr(), N.stream_ptr())
    else:
        rc = lib.orcai_stft_energy_bwd(pcm.data_ptr(), n, nfft, hop, T, K, gE.data_ptr(), dpcm.data_ptr(), N.stream_ptr())
    assert rc == 0 and torch.isfinite(dpcm).all()
    ref = c["dpcm64"]
    share = float((dpcm.cpu().double() - ref).abs().max() / ref.abs().max())
    dev = ENERGY_F32_DEVIATION[index]
    print(f"energy backward {R.label(pc)}: kernel error {share:.2e} of max|dpcm|; torch f32 {dev:.2e}; bar {8 * dev:.2e}")
    assert share <= 8 * dev, (share, dev)


# ------------------------------------------------------------------------------------------------------------------ 7. refusals
def test_refusals_leave_the_outputs_untouched():
    lib, N = _lib()
    # the scan
    T, K = 300, 8
    E = torch.rand((T, K), device="cuda")
    g = torch.ones((T, K), device="cuda")
    stats = _stats(0.1, 1.0)
    good = [0.99, 0.01, 2.0**31, 0.98, 2.0, 0.5, 1e-6]
    ok = torch.full((T, K), float("nan"), device="cuda")
    assert _scan(E, g, stats, T, K, good, ok) == 0 and torch.isfinite(ok).all()
    dE = torch.full((T, K), float("nan"), device="cuda")
    for what, a in (("E", (None, g, stats)), ("gout", (E, None, stats)), ("stats_dev", (E, g, None))):
        assert _scan(*a, T, K, good, dE) == N.E_BADARG and torch.isnan(dE).all(), what
    assert _scan(E, g, stats, T, K, good, None) == N.E_BADARG
    assert _scan(E, g, stats, T, K, good, dE, scratch=None) == N.E_BADARG and torch.isnan(dE).all()
    assert _scan(E, g, stats, 0, K, good, dE) == N.E_BADARG and _scan(E, g, stats, T, 0, good, dE) == N.E_BADARG and torch.isnan(dE).all()
    bad = {0: (-0.1, 1.0), 1: (0.0, 1.5), 2: (0.0, -1.0), 3: (-0.1, 1.5), 4: (-1.0,), 5: (0.0, 1.5), 6: (0.0, -1e-6)}  # a, b, scale, gain, bias, power, eps
    for i, values in bad.items():
        for v in values + (float("nan"),):
            sc = list(good)
            sc[i] = v
            assert _scan(E, g, stats, T, K, sc, dE) == N.E_BADARG and torch.isnan(dE).all(), (i, v)
    assert lib.orcai_pcen_bwd_scratch_bytes(0, 8) == 0 and lib.orcai_pcen_spectrogram_bwd_scratch_bytes(8, 0) == 0
    # the two energy backwards and the one call
    pcm = torch.from_numpy(R.G.recording("a")[:4000].copy()).cuda()
    n = pcm.numel()
    T = 1 + n // 256
    for sp, K in ((SP_LIN, 171), (SP_MEL, 64)):
        g = torch.zeros((T + 1, K), device="cuda")
        stats = _stats(0.1, 1.0)
        ok = torch.full((n,), float("nan"), device="cuda")
        assert _one_call(pcm, sp, g, stats, ok) == 0 and torch.isfinite(ok).all()
        dpcm = torch.full((n,), float("nan"), device="cuda")

        def refused(want, what, *a, **k):
            assert _one_call(*a, **k) == want, (what, K)
            assert torch.isnan(dpcm).all(), (what, K)

        refused(N.E_BADARG, "pcm", pcm, sp, g, stats, dpcm, null_pcm=True)
        refused(N.E_BADARG, "gout", pcm, sp, None, stats, dpcm)
        refused(N.E_BADARG, "stats_dev", pcm, sp, g, None, dpcm)
        refused(N.E_BADARG, "scratch", pcm, sp, g, stats, dpcm, scratch=None)
        assert _one_call(pcm, sp, g, stats, None) == N.E_BADARG
        refused(N.E_BADARG, "n_frames + 1", pcm, sp, g, stats, dpcm, n_frames=T + 1)
        refused(N.E_BADARG, "hop 0", pcm, sp, g, stats, dpcm, hop=0)
        for nfft in (500, 16, 8192):  # (171 bins are more than 16 / 2 + 1: that is refused first)
            refused(N.E_BADARG if (nfft, K) == (16, 171) else N.E_UNSUPPORTED, nfft, pcm, sp, g, stats, dpcm, nfft=nfft)
        for i, values in bad.items():
            for v in values:
                sc = list(good)
                sc[i] = v
                refused(N.E_BADARG, (i, v), pcm, sp, g, stats, dpcm, scalars=sc)
    # the energy backwards themselves: null pointers, the frame count, the sizes
    gE = torch.zeros((T, 171), device="cuda")
    dpcm = torch.full((n,), float("nan"), device="cuda")
    s = N.stream_ptr()
    assert lib.orcai_stft_energy_bwd(pcm.data_ptr(), n, 512, 256, T, 171, gE.data_ptr(), dpcm.data_ptr(), s) == 0 and not dpcm.any()
    dpcm.fill_(float("nan"))
    assert lib.orcai_stft_energy_bwd(0, n, 512, 256, T, 171, gE.data_ptr(), dpcm.data_ptr(), s) == N.E_BADARG
    assert lib.orcai_stft_energy_bwd(pcm.data_ptr(), n, 512, 256, T, 171, 0, dpcm.data_ptr(), s) == N.E_BADARG
    assert lib.orcai_stft_energy_bwd(pcm.data_ptr(), n, 512, 256, T, 171, gE.data_ptr(), 0, s) == N.E_BADARG
    assert lib.orcai_stft_energy_bwd(pcm.data_ptr(), n, 512, 256, T + 1, 171, gE.data_ptr(), dpcm.data_ptr(), s) == N.E_BADARG
    assert lib.orcai_stft_energy_bwd(pcm.data_ptr(), n, 512, 0, T, 171, gE.data_ptr(), dpcm.data_ptr(), s) == N.E_BADARG
    assert lib.orcai_stft_energy_bwd(pcm.data_ptr(), n, 512, 256, T, 258, gE.data_ptr(), dpcm.data_ptr(), s) == N.E_BADARG
    for nfft in (500, 16, 8192):
        assert lib.orcai_stft_energy_bwd(pcm.data_ptr(), n, nfft, 256, T, 8, gE.data_ptr(), dpcm.data_ptr(), s) == N.E_UNSUPPORTED
    from orcai_amd import mel

    t, w = _fe()._mel_table(SP_MEL, mel.mel_config(SP_MEL))
    tab = (t["lo"].ctypes.data, t["hi"].ctypes.data, t["off"].ctypes.data, w.data_ptr(), w.numel())
    assert lib.orcai_stft_mel_energy_bwd(pcm.data_ptr(), n, 512, 256, T, 64, *tab, 0, dpcm.data_ptr(), s) == N.E_BADARG
    assert lib.orcai_stft_mel_energy_bwd(pcm.data_ptr(), n, 512, 256, T, 64, 0, *tab[1:], gE.data_ptr(), dpcm.data_ptr(), s) == N.E_BADARG
    assert lib.orcai_stft_mel_energy_bwd(pcm.data_ptr(), n, 64, 256, T, 64, *tab, gE.data_ptr(), dpcm.data_ptr(), s) == N.E_UNSUPPORTED
    assert torch.isnan(dpcm).all()
    # the Python layer
    fe = _fe()
    g = torch.zeros((T, 171), device="cuda")
    with pytest.raises(ValueError, match="pcen is absent"):
        fe.pcen_spectrogram_backward(pcm, g, stats, {k: v for k, v in SP_LIN.items() if k != "pcen"})
    with pytest.raises(ValueError, match=r"\[16, 171\]"):
        fe.pcen_spectrogram_backward(pcm, g[:-1], stats, SP_LIN)
    with pytest.raises(NotImplementedError, match="nfft"):
        fe.pcen_spectrogram_backward(pcm, g, stats, dict(SP_LIN, nfft=500))
    with pytest.raises(ValueError, match="stats"):
        fe.pcen_spectrogram_backward(pcm, g, stats[:4], SP_LIN)


# ------------------------------------------------------------------------------------------------------------------ 8. the ops
@pytest.mark.parametrize("args, sp", [(LIN, SP_LIN), (MEL, SP_MEL)], ids=["linear", "mel"])
def test_op_forward_bits_gradient_bits_and_stats_survive_another_recording(args, sp):
    fe = _fe()
    pcm1 = torch.from_numpy(R.G.recording("a")[:48000 + 16].copy()).cuda()
    pcm2 = torch.from_numpy(R.G.recording("b")[40000:100000].copy()).cuda()
    want = torch.ops.orcai.pcen_spectrogram(pcm1, *args)
    with torch.no_grad():
        assert same_bits(torch.ops.orcai.pcen_spectrogram_wrt_pcm(pcm1, *args), want)
    x1, x2 = pcm1.clone().requires_grad_(), pcm2.clone().requires_grad_()
    s1 = torch.ops.orcai.pcen_spectrogram_wrt_pcm(x1, *args)
    s2 = torch.ops.orcai.pcen_spectrogram_wrt_pcm(x2, *args)  # another recording overwrites the front end's workspace before s1's backward
    assert same_bits(s1.detach(), want) and s1.requires_grad
    g = torch.randn(s1.shape, device="cuda", generator=torch.Generator("cuda").manual_seed(1))
    (d1,) = torch.autograd.grad(s1, x1, g)
    spec1, st1 = fe.make_spectrogram(pcm1, sp, return_stats=True)
    assert same_bits(spec1, want)
    assert same_bits(d1, fe.pcen_spectrogram_backward(pcm1, g, st1, sp))
    assert torch.isfinite(d1).all() and float(d1.abs().max()) > 0
    (d2,) = torch.autograd.grad(s2.sum(), x2)
    assert same_bits(d2, fe.pcen_spectrogram_backward(pcm2, torch.ones_like(s2), fe.make_spectrogram(pcm2, sp, return_stats=True)[1], sp))


def test_opcheck_new_ops():
    from torch.library import opcheck

    pcm = torch.from_numpy(R.G.recording("a")[:24000].copy()).cuda()
    for args in (LIN, MEL):
        opcheck(torch.ops.orcai.pcen_spectrogram_wrt_pcm.default, (pcm, *args))
        opcheck(torch.ops.orcai.pcen_spectrogram_wrt_pcm.default, (pcm.clone().requires_grad_(), *args))
        opcheck(torch.ops.orcai.pcen_spectrogram_with_stats.default, (pcm, *args))
        spec, stats = torch.ops.orcai.pcen_spectrogram_with_stats(pcm, *args)
        opcheck(torch.ops.orcai.pcen_spectrogram_backward.default, (torch.ones_like(spec), pcm, stats, *args[:-2]))


# ------------------------------------------------------------------------------------------------------------------ 9. end to end
def test_waveform_gradient_through_the_detector():
    """pcm at 96 kHz -> PcenWaveformFrontEnd (resample, pcen_spectrogram_wrt_pcm on the mel route) -> snippets -> OrcaiModule(input_grad="eval") of input
    width n_mels -> scalar loss -> backward: pcm.grad is finite, non-zero and, bit for bit, the chain composed by hand -- resample_backward of
    pcen_spectrogram_backward of the snippet gradients scattered back onto the spectrogram (the construction of tests/test_mel_grad_gpu.py's last test)."""
    from orcai_amd.architectures import ResNet1DConv
    from orcai_amd.resample import resample_device
    from orcai_amd.torch_ops import OrcaiModule, PcenWaveformFrontEnd

    H, W, B = 64, 64, 2
    model = ResNet1DConv((H, W, 1), 4, [12, 20], 3, dropout_rate=0.0, seed=4)
    m = OrcaiModule(model, input_grad="eval").cuda().eval()
    front = PcenWaveformFrontEnd(SP_MEL, 96000)
    rng = np.random.default_rng(7)
    t = np.arange(96000) / 96000.0
    pcm0 = torch.from_numpy((0.1 * rng.uniform(-1, 1, t.size) + 0.3 * np.sin(2 * np.pi * (3000.0 * t + 4000.0 * t * t))).astype(np.float32)).cuda()
    pcm = pcm0.clone().requires_grad_()
    spec = front(pcm)
    assert spec.shape[1] == W and spec.shape[0] >= B * H
    x = spec[: B * H].view(B, H, W)
    x.retain_grad()
    loss = (m(x) ** 2).sum()
    loss.backward()
    assert torch.isfinite(pcm.grad).all() and float(pcm.grad.abs().max()) > 0
    fe = _fe()
    at_rate = resample_device(pcm0, 96000, 48000)
    spec0, st = fe.make_spectrogram(at_rate, SP_MEL, return_stats=True)
    assert same_bits(spec0, spec.detach())
    gspec = torch.zeros_like(spec0)
    gspec[: B * H] = x.grad.view(B * H, W)
    d_rate = fe.pcen_spectrogram_backward(at_rate, gspec, st, SP_MEL)
    assert same_bits(pcm.grad, torch.ops.orcai.resample_backward(d_rate, pcm0.numel(), 96000, 48000))
    # and the linear route through detect_recording
    lin = PcenWaveformFrontEnd(SP_LIN, 96000)
    assert lin(pcm0).shape[1] == 171
