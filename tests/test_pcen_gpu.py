"""The PCEN front end on the GPU: orcai_pcen alone against the float64 specification orcai_amd.pcen.pcen_ref, the two energy epilogues of the STFT
kernels against tests/stft_ref.py / tests/mel_ref.py, FrontEnd.make_spectrogram with the pcen key end to end against the numpy composition, no change
when the key is off, and the public surface (torch op, predict).

Tolerance of the recursion (measured against the reference, not fixed): the largest deviation of a float32 numpy restatement of the SEQUENTIAL
recurrence (pcen_f32 below; it knows nothing of the kernel's chunks) from the float64 one, relative to max(|out|, bias^power), and the kernel gets 8 times
that: it chains three hardware transcendentals of about one ulp each where numpy's are correctly rounded, and associates the carry differently.  The
deviation is taken over all of this file's inputs for a smoother, not case by case: a case of one element (T = 1, K = 1) has whatever deviation its one
rounding happens to leave, which bounds nothing.  Each case prints its own error as a multiple of the float32 restatement's."""

import numpy as np
import pytest

import mel_ref as MR
import stft_ref as R
from orcai_amd import mel, pcen

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

SR, HOP = 48000, 256
CASES = [(1, 1), (2, 8), (255, 64), (256, 171), (257, 257), (513, 8), (1030, 171)]  # (T, K): every K of {1, 8, 64, 171, 257} appears
SMOOTHERS = {"default": 0.4, "long": 2.5}  # seconds at 48 kHz / hop 256: t = 75 frames; t = 468.75 frames, a^256 = 0.58
FAMILIES = ("random", "constant", "impulse", "zero", "step")


def energies(T, K, case):
    """f32[T, K]: column k is of family (k + case) % 5 -- log-uniform random in 1e-9 .. 1, a constant, an impulse at frame 300 (the last frame of a
    shorter input), all zero, a step at the chunk boundary (frame 256; the middle of a shorter input)."""
    rng = np.random.default_rng(100 + case)
    E = np.zeros((T, K), dtype=np.float32)
    for k in range(K):
        fam = FAMILIES[(k + case) % 5]
        if fam == "random":
            E[:, k] = 10.0 ** rng.uniform(-9, 0, T)
        elif fam == "constant":
            E[:, k] = 10.0 ** rng.uniform(-6, -1)
        elif fam == "impulse":
            E[:, k] = 1e-7
            E[min(300, T - 1), k] = 0.5
        elif fam == "step":
            E[:, k] = 1e-6
            E[(256 if T > 256 else T // 2):, k] = 1e-2
    return E


def cfg_for(smoother):
    return pcen.pcen_config({"nfft": 512, "pcen": {"time_constant": SMOOTHERS[smoother]}})


def pcen_f32(E, cfg, sampling_rate, hop):
    """pcen_ref with every operation in float32, sequential over time: the tolerance's yardstick."""
    f = np.float32
    a, b = (f(v) for v in pcen.smoother(cfg["time_constant"], sampling_rate, hop))
    S = f(cfg["scale"]) * np.asarray(E, dtype=f)
    M = np.empty_like(S)
    M[0] = S[0]
    for t in range(1, S.shape[0]):
        M[t] = a * M[t - 1] + b * S[t]
    out = pcen.pcen_values(S, M, cfg)
    assert out.dtype == f
    return out


def rel_dev(got, want, cfg):
    return np.abs(np.asarray(got, dtype=np.float64) - want) / np.maximum(np.abs(want), cfg["bias"] ** cfg["power"])


_REF = {}


def reference(smoother):
    """{case: (E, out64)} and the float32 restatement's largest deviation over all cases, computed once per smoother."""
    if smoother not in _REF:
        cfg = cfg_for(smoother)
        per_case, worst = {}, 0.0
        for i, (T, K) in enumerate(CASES):
            E = energies(T, K, i)
            want = pcen.pcen_ref(E, cfg, SR, HOP)
            dev = float(rel_dev(pcen_f32(E, cfg, SR, HOP), want, cfg).max())
            worst = max(worst, dev)
            E.setflags(write=False)
            want.setflags(write=False)
            per_case[i] = (E, want, dev)
        _REF[smoother] = (per_case, worst)
    return _REF[smoother]


def run_pcen(E, cfg, sampling_rate=SR, hop=HOP):
    from orcai_amd import _native as N

    lib = N.lib()
    T, K = E.shape
    a, b = pcen.smoother(cfg["time_constant"], sampling_rate, hop)
    x = torch.tensor(E, device="cuda")
    scratch = torch.empty(lib.orcai_pcen_scratch_bytes(T, K) // 4, dtype=torch.float32, device="cuda")
    assert scratch.numel() == 2 * ((T + 255) // 256) * K
    rc = lib.orcai_pcen(x.data_ptr(), T, K, a, b, cfg["scale"], cfg["gain"], cfg["bias"], cfg["power"], cfg["eps"], scratch.data_ptr(), N.stream_ptr())
    assert rc == 0, rc
    return x.cpu().numpy()


# ------------------------------------------------------------------------------------------------ 1. the recursion
@pytest.mark.parametrize("smoother", list(SMOOTHERS))
@pytest.mark.parametrize("case", range(len(CASES)))
def test_pcen_against_float64(case, smoother):
    cfg = cfg_for(smoother)
    per_case, dev32 = reference(smoother)
    E, want, dev_case = per_case[case]
    if smoother == "long":
        assert pcen.smoother(cfg["time_constant"], SR, HOP)[0] ** 256 > 0.5  # carries across four chunks matter
    got = run_pcen(E, cfg)
    again = run_pcen(E, cfg)
    assert np.array_equal(got.view(np.int32), again.view(np.int32)), "the same call twice gave other bytes"
    assert np.isfinite(got).all()
    err = float(rel_dev(got, want, cfg).max())
    T, K = CASES[case]
    print(f"orcai_pcen T={T} K={K} {smoother}: error {err:.3e} = {err / dev32:.2f} x the float32 restatement's {dev32:.3e} (this case's own: {dev_case:.3e})")
    assert err <= 8.0 * dev32, (T, K, smoother, err, dev32)
    for k in range(K):
        if FAMILIES[(k + case) % 5] == "zero":
            assert not got[:, k].view(np.int32).any(), (k, got[:, k][got[:, k] != 0][:4])  # exactly +0.0


def test_pcen_refusals():
    from orcai_amd import _native as N

    lib = N.lib()
    x = torch.ones(8, device="cuda")
    s = torch.empty(2, device="cuda")
    ok = (x.data_ptr(), 8, 1, 0.9, 0.1, 1.0, 0.98, 2.0, 0.5, 1e-6, s.data_ptr(), N.stream_ptr())
    for i, bad in ((0, None), (1, 0), (2, 0), (3, 1.0), (4, 0.0), (5, 0.0), (6, 1.5), (7, -1.0), (8, 0.0), (9, 0.0), (10, None)):
        args = list(ok)
        args[i] = bad
        assert lib.orcai_pcen(*args) == N.E_BADARG, i
    assert torch.equal(x.cpu(), torch.ones(8))


# ------------------------------------------------------------------------------------------------ 2. the energies
N_SAMPLES = 6000


def _noise(n_fft, hop):
    x = R.make_input("noise", N_SAMPLES, n_fft, hop)
    x.setflags(write=False)
    return x


@pytest.mark.parametrize("n_fft,hop,k_crops", [(512, 256, (171, 257, 40)), (128, 64, (65, 43))])
def test_stft_energy(n_fft, hop, k_crops):
    """|X[k]| within the bound tests/test_stft_gpu.py:105 grants the amplitude before the logarithm, |a_gpu - a_ref| <= gamma(N) S[t] + rho a_ref
    (stft_ref.amp_ratio <= 1), here against the unclamped |X|."""
    from orcai_amd import _native as N

    lib = N.lib()
    x = _noise(n_fft, hop)
    P, S1 = MR.power_ref(x, n_fft, hop)
    a_ref = np.sqrt(P)
    T = R.num_frames(x.size, n_fft, hop)
    xd = torch.tensor(x, device="cuda")
    for k in k_crops:
        out = torch.full((T * k + 67,), float("nan"), device="cuda")
        assert lib.orcai_stft_energy(xd.data_ptr(), x.size, n_fft, hop, T, k, out.data_ptr(), N.stream_ptr()) == 0
        assert bool(torch.isnan(out[T * k:]).all()), "written behind n_frames * k_crop"
        E = out[: T * k].cpu().numpy().reshape(T, k)
        ratio = R.amp_ratio(E, a_ref[:, :k], S1, R.gamma(n_fft, "radix2"))
        print(f"orcai_stft_energy N={n_fft} hop={hop} k_crop={k}: ratio {ratio.max():.4f}")
        assert np.isfinite(E).all() and (E >= 0).all() and ratio.max() <= 1.0
    assert lib.orcai_stft_energy(xd.data_ptr(), x.size, 500, hop, R.num_frames(x.size, 500, hop), 40, out.data_ptr(), N.stream_ptr()) == N.E_UNSUPPORTED


@pytest.mark.parametrize("n_fft,hop,n_mels", [(512, 256, 8), (512, 256, 64), (128, 64, 8), (1024, 256, 64)])
def test_stft_mel_energy(n_fft, hop, n_mels):
    """The band power within mel_ref.mel_bound's dM: the bound tests/test_mel_gpu.py derives for the power before the logarithm."""
    from orcai_amd import _native as N

    lib = N.lib()
    x = _noise(n_fft, hop)
    t = mel.band_table(SR, n_fft, n_mels, 0.0, 16000.0)
    W = MR.weights_f64(SR, n_fft, n_mels, 0.0, 16000.0, False, "slaney")
    P, S1 = MR.power_ref(x, n_fft, hop)
    _, M, dM = MR.mel_bound(P, S1, W, n_fft)
    T = R.num_frames(x.size, n_fft, hop)
    xd = torch.tensor(x, device="cuda")
    w = torch.tensor(t["weights"], device="cuda")
    out = torch.full((T * n_mels + 67,), float("nan"), device="cuda")
    rc = lib.orcai_stft_mel_energy(xd.data_ptr(), x.size, n_fft, hop, T, n_mels, t["lo"].ctypes.data, t["hi"].ctypes.data, t["off"].ctypes.data, w.data_ptr(), w.numel(),
                                   out.data_ptr(), N.stream_ptr())
    assert rc == 0, rc
    assert bool(torch.isnan(out[T * n_mels:]).all())
    E = out[: T * n_mels].cpu().numpy().reshape(T, n_mels).astype(np.float64)
    ratio = np.abs(E - M) / dM
    print(f"orcai_stft_mel_energy N={n_fft} hop={hop} n_mels={n_mels}: ratio {ratio.max():.4f}")
    assert ratio.max() <= 1.0


# ------------------------------------------------------------------------------------------------ 3. end to end
def _signal(n, seed=3):
    rng = np.random.default_rng(seed)
    t = np.arange(n) / SR
    x = 0.05 * rng.standard_normal(n) * (1.0 + 0.8 * np.sin(2 * np.pi * 3.0 * t)) + 0.2 * np.sin(2 * np.pi * 2500.0 * t) * (t > 0.2)
    return x.astype(np.float32)


def _pcen_slack(S, dS, cfg, a, b):
    """First-order bound on |d pcen| for energies known to within dS (both scaled): M is a convex combination of S, so dM obeys the same recurrence;
    d out <= power (S r + bias)^(power - 1) r (dS + gain S dM / (eps + M)), r = (eps + M)^-gain."""
    M, dM = np.empty_like(S), np.empty_like(S)
    M[0], dM[0] = S[0], dS[0]
    for t in range(1, S.shape[0]):
        M[t] = a * M[t - 1] + b * S[t]
        dM[t] = a * dM[t - 1] + b * dS[t]
    r = (cfg["eps"] + M) ** -cfg["gain"]
    return 1.01 * cfg["power"] * (S * r + cfg["bias"]) ** (cfg["power"] - 1.0) * r * (dS + cfg["gain"] * S * dM / (cfg["eps"] + M))


E2E = {
    "linear-128": dict(sampling_rate=SR, nfft=128, n_overlap=64, freq_range=[0, 16000], quantiles=[0.01, 0.999], pcen={}),
    "mel16-128": dict(sampling_rate=8000, nfft=128, n_overlap=64, freq_range=[0, 4000], quantiles=[0.01, 0.999], mel={"n_mels": 16}, pcen={"time_constant": 0.1}),
    "linear-512": dict(sampling_rate=SR, nfft=512, n_overlap=256, freq_range=[0, 16000], quantiles=[0.01, 0.999], pcen={}),
    "mel16-512": dict(sampling_rate=SR, nfft=512, n_overlap=256, freq_range=[0, 16000], quantiles=[0.01, 0.999], mel={"n_mels": 16}, pcen={"time_constant": 0.1}),
}


@pytest.mark.parametrize("name", list(E2E))
def test_make_spectrogram_with_pcen(name):
    from orcai_amd.frontend import get_frontend, nearest_rank_index

    sp = E2E[name]
    n_fft, hop, sr = sp["nfft"], sp["n_overlap"], sp["sampling_rate"]
    x = _signal(20000)
    fe = get_frontend()
    xd = torch.tensor(x, device="cuda")
    T, K = fe.spectrogram_shape(x.size, sp)
    assert T == 1 + x.size // hop and (n_fft != 128 or T > 256)  # crosses a chunk boundary at hop 64
    big = torch.full((T + 8, K), -7.0, device="cuda")  # four rows in front: the output stays 16-byte aligned whatever K is
    got, stats = fe.make_spectrogram(xd, sp, return_stats=True, out=big[4 : T + 4])
    assert got.data_ptr() == big[4].data_ptr() and bool((big[:4] == -7.0).all()) and bool((big[T + 4 :] == -7.0).all())
    fresh = fe.make_spectrogram(xd, sp)
    assert tuple(fresh.shape) == (T, K) and torch.equal(fresh.view(torch.int32), got.view(torch.int32))
    out = got.cpu().numpy()
    assert out.min() >= 0.0 and out.max() <= 1.0 and out.min() == 0.0 and out.max() == 1.0
    _, _, p_lo, p_hi, sel_lo, sel_hi = (float(v) for v in stats.cpu().numpy())
    assert (p_lo, p_hi) == (sel_lo, sel_hi) and p_lo < p_hi

    # the numpy composition: reference energies -> pcen_ref -> nearest-rank percentiles -> clip and normalise
    cfg = pcen.pcen_config(sp)
    mcfg = mel.mel_config(sp)
    P, S1 = MR.power_ref(x, n_fft, hop)
    if mcfg is None:
        E = np.sqrt(P)[:, :K]
        dE = (R.gamma(n_fft, "radix2") * S1)[:, None] + R.RHO * E  # tests/test_stft_gpu.py:105
    else:
        W = MR.weights_f64(sr, n_fft, mcfg["n_mels"], mcfg["fmin"], mcfg["fmax"], mcfg["htk"], mcfg["norm"])
        _, E, dE = MR.mel_bound(P, S1, W, n_fft)
    a, b = pcen.smoother(cfg["time_constant"], sr, hop)
    v = pcen.pcen_ref(E, cfg, sr, hop)
    dev32 = float(rel_dev(pcen_f32(E, cfg, sr, hop), v, cfg).max())
    tol = 8.0 * dev32 * np.maximum(np.abs(v), cfg["bias"] ** cfg["power"]) + _pcen_slack(cfg["scale"] * E, cfg["scale"] * dE, cfg, a, b)
    order = np.argsort(v, axis=None)
    srt, srt_tol = v.ravel()[order], tol.ravel()[order]
    for q, bound in zip(sp["quantiles"], (p_lo, p_hi)):
        r = nearest_rank_index(T * K, q)
        # the bound may be another element than the reference's r-th when values lie within the tolerance of each other: the value is what is held
        w = slice(max(r - 8, 0), r + 9)
        print(f"{name}: q={q} rank {r}: reported {bound:.6g}, reference {srt[r]:.6g}, tolerance {srt_tol[w].max():.3g}")
        assert abs(bound - srt[r]) <= srt_tol[w].max(), (q, bound, srt[r])
    want = (np.clip(v, p_lo, p_hi) - p_lo) / (p_hi - p_lo)  # with the bounds the GPU reports
    err = np.abs(out - want) - (tol / (p_hi - p_lo) + 4 * 2.0**-24)
    print(f"{name}: T={T} K={K}, largest |out - want| {np.abs(out - want).max():.3e}, float32 restatement's deviation {dev32:.3e}")
    assert err.max() <= 0.0, (float(err.max()), np.unravel_index(err.argmax(), err.shape))


# ------------------------------------------------------------------------------------------------ 4. no change when off
@pytest.mark.parametrize("extra", [{}, {"mel": {"n_mels": 64}}], ids=["linear", "mel"])
def test_no_change_when_off(extra):
    from orcai_amd.frontend import get_frontend

    sp = dict(sampling_rate=SR, nfft=512, n_overlap=256, freq_range=[0, 16000], quantiles=[0.01, 0.999], **extra)
    fe = get_frontend()
    xd = torch.tensor(_signal(20000, seed=4), device="cuda")
    base, st0 = fe.make_spectrogram(xd, sp, return_stats=True)
    off, st1 = fe.make_spectrogram(xd, dict(sp, pcen=None), return_stats=True)
    assert torch.equal(base.view(torch.int32), off.view(torch.int32)) and torch.equal(st0.view(torch.int32), st1.view(torch.int32))
    on = fe.make_spectrogram(xd, dict(sp, pcen={}))
    assert on.shape == base.shape and not torch.equal(on, base)
    again = fe.make_spectrogram(xd, sp)  # and the PCEN run in between left nothing behind
    assert torch.equal(base.view(torch.int32), again.view(torch.int32))


# ------------------------------------------------------------------------------------------------ 5. the surface
def test_backward_entry_points_refuse_pcen():
    from orcai_amd.frontend import get_frontend

    fe = get_frontend()
    sp = dict(E2E["linear-512"])
    xd = torch.tensor(_signal(4096), device="cuda")
    spec, stats = fe.make_spectrogram(xd, sp, return_stats=True)
    with pytest.raises(NotImplementedError, match="pcen"):
        fe.spectrogram_backward(xd, torch.ones_like(spec), stats, sp)
    with pytest.raises(NotImplementedError, match="pcen"):
        fe.mel_spectrogram_backward(xd, torch.ones_like(spec), stats, dict(E2E["mel16-512"]))


def test_torch_op_returns_make_spectrograms_bytes_and_has_no_gradient():
    import orcai_amd.torch_ops  # noqa: F401  (registers the ops)
    from orcai_amd.frontend import get_frontend
    from torch._subclasses.fake_tensor import FakeTensorMode

    fe = get_frontend()
    xd = torch.tensor(_signal(20000), device="cuda")
    lin = (SR, 512, 256, 16000.0, 0, 0.0, 0.0, False, True, 0.4, 0.98, 2.0, 0.5, 1e-6, 2.0**31, 0.01, 0.999)
    got = torch.ops.orcai.pcen_spectrogram(xd, *lin)
    assert torch.equal(got.view(torch.int32), fe.make_spectrogram(xd, E2E["linear-512"]).view(torch.int32))
    m = (SR, 512, 256, 0.0, 16, 0.0, 16000.0, False, True, 0.1, 0.98, 2.0, 0.5, 1e-6, 2.0**31, 0.01, 0.999)
    got_m = torch.ops.orcai.pcen_spectrogram(xd, *m)
    assert torch.equal(got_m.view(torch.int32), fe.make_spectrogram(xd, E2E["mel16-512"]).view(torch.int32))
    with FakeTensorMode():
        fake = torch.ops.orcai.pcen_spectrogram(torch.empty(xd.numel(), device="cuda"), *lin)
    assert tuple(fake.shape) == tuple(got.shape) and fake.dtype == torch.float32
    xg = xd.clone().requires_grad_(True)
    y = torch.ops.orcai.pcen_spectrogram(xg, *lin)
    assert y.requires_grad and torch.equal(y.detach(), got)
    with pytest.raises(NotImplementedError, match="pcen"):
        y.sum().backward()
    with pytest.raises(NotImplementedError, match="pcen"):
        orcai_amd.torch_ops.waveform_front_end(E2E["linear-512"], SR)


def test_predict_runs_with_a_pcen_parameter(tmp_path):
    import json
    from pathlib import Path

    from orcai_amd import wavio
    from orcai_amd.architectures import ResNetLSTM
    from orcai_amd.io import read_json
    from orcai_amd.predict import predict
    from orcai_amd.synthetic import synth_recording

    root = Path(__file__).resolve().parent.parent
    param = read_json(root / "orcai_amd" / "models" / "orcai-V1" / "orcai_parameter.json")
    param["name"] = "tiny"
    param["calls"] = ["A", "B", "C"]
    param["model"].update(filters=[10, 20], kernel_size=3, lstm_units=64)
    param["spectrogram"]["mel"] = {"n_mels": 16}
    param["spectrogram"]["pcen"] = {"time_constant": 0.2}
    folder = tmp_path / "tiny"
    folder.mkdir()
    (folder / "orcai_parameter.json").write_text(json.dumps(param))
    (folder / "model_shape.json").write_text(json.dumps({"input_shape": [32, 16, 1], "num_labels": 3}))
    ResNetLSTM((32, 16, 1), 3, [10, 20], 3, 0.0, 64, seed=5).save_weights(folder / "tiny.weights.npz")  # seeded initial weights
    wav = tmp_path / "rec.wav"
    wavio.write_wav_pcm16(wav, synth_recording(0.25, 48000, seed=11), 48000)  # 47 frames: one snippet of 32
    predict(wav, channel=1, model_dir=folder, output_path=tmp_path / "labels.txt", verbosity=0)
    assert (tmp_path / "labels.txt").exists()
