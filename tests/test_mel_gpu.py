"""orcai_stft_mel_db / orcai_make_mel_spectrogram (csrc/frontend.hip) through the C ABI against the float64 contract and the DERIVED bound of
tests/mel_ref.py, on the tuned 512-point kernel's three launch routes and the workgroup-per-frame kernel; the composition against the clip and
normalise computed on the CPU from the GPU's own dB values; identical bytes on a second run; every refusal; and the wiring up to predict() and the
torch op.  Each accuracy test prints the largest error-to-bound ratio it saw."""

import ctypes as C

import numpy as np
import pytest

import mel_ref as MR
import stft_ref as R
from orcai_amd import mel

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

GUARD = 64 + 3
SENTINEL_BITS = 0x7FC12345
TOP_DB = 80.0


class Harness:
    def __init__(self):
        from orcai_amd import _native as N

        self.lib = N.lib()
        self.ws = torch.zeros(self.lib.orcai_frontend_workspace_bytes(), dtype=torch.uint8, device="cuda")
        self.wsp = self.ws.data_ptr()
        self.s = N.stream_ptr()
        self._tables = {}

    def table(self, n_fft, n_mels, fmin, fmax, htk, norm):
        key = (n_fft, n_mels, fmin, fmax, htk, norm)
        if key not in self._tables:
            t = mel.band_table(MR.SR, n_fft, n_mels, fmin, fmax, htk, norm)
            self._tables[key] = (t, torch.tensor(t["weights"], device="cuda"))
        return self._tables[key]

    def buffer(self, count):
        return torch.full((count + GUARD,), SENTINEL_BITS, dtype=torch.int32, device="cuda")

    @staticmethod
    def untouched(buf, start=0):
        return bool((buf[start:] == SENTINEL_BITS).all().item())

    def stats(self):
        st = (C.c_float * 6)()
        assert self.lib.orcai_frontend_stats_host(self.wsp, st, self.s) == 0
        return [np.float32(v) for v in st]

    def args(self, xd, n_fft, hop, t, wd, buf, T=None, n_mels=None):
        n = xd.numel()
        return [xd.data_ptr(), n, n_fft, hop, R.num_frames(n, n_fft, hop) if T is None else T, t["lo"].size if n_mels is None else n_mels,
                t["lo"].ctypes.data, t["hi"].ctypes.data, t["off"].ctypes.data, wd.data_ptr(), wd.numel(), buf.data_ptr(), self.wsp, self.s]

    def stft_mel(self, xd, n_fft, hop, t, wd):
        """reset + orcai_stft_mel_db: (L f32[T, n_mels] on the host, max M from the workspace, the device buffer with its guard)."""
        T, n_mels = R.num_frames(xd.numel(), n_fft, hop), t["lo"].size
        buf = self.buffer(T * n_mels)
        assert self.lib.orcai_frontend_reset(self.wsp, self.s) == 0
        rc = self.lib.orcai_stft_mel_db(*self.args(xd, n_fft, hop, t, wd, buf))
        assert rc == 0, rc
        pmax = self.stats()[0]
        assert self.untouched(buf, T * n_mels), "the guard behind n_frames * n_mels was written"
        body = buf[: T * n_mels]
        assert not bool((body == SENTINEL_BITS).any().item()), "an output element was never written"
        L = body.view(torch.float32).cpu().numpy().reshape(T, n_mels)
        assert np.isfinite(L).all()
        return L, pmax, buf


@pytest.fixture(scope="module")
def h():
    return Harness()


_REF = {}


def reference(family, case):
    """(x, A_ref, M_ref, dM) once per (input, filterbank); read-only."""
    n_fft, hop, n, n_mels, fmin, fmax, htk, norm = case
    edge = MR.edge_frequency(n_mels, fmin, fmax, htk) if family == "band_edge_tone" else 0.0
    kx = (family, n, n_fft, hop, edge)
    if kx not in _REF:
        x = MR.make_input(family, n, n_fft, hop, MR.SR, edge)
        _REF[kx] = (x, *MR.power_ref(x, n_fft, hop))
    x, P, S1 = _REF[kx]
    kb = kx + case[3:]
    if kb not in _REF:
        out = MR.mel_bound(P, S1, MR.weights_f64(MR.SR, n_fft, n_mels, fmin, fmax, htk, norm), n_fft)
        for a in (x, *out):
            a.setflags(write=False)
        _REF[kb] = out
    return (x, *_REF[kb])


# ------------------------------------------------------------------------------------------------ 1. values, every band of every frame
@pytest.mark.parametrize("family", MR.FAMILIES)
@pytest.mark.parametrize("case", MR.cases(), ids=lambda c: "N{}-hop{}-n{}-m{}-{}-{}-{}-{}".format(*c))
def test_values_within_the_derived_bound(h, case, family):
    n_fft, hop, n, n_mels, fmin, fmax, htk, norm = case
    x, A_ref, M_ref, dM = reference(family, case)
    t, wd = h.table(n_fft, n_mels, fmin, fmax, htk, norm)
    L, pmax, _ = h.stft_mel(torch.tensor(x, device="cuda"), n_fft, hop, t, wd)
    ratio = MR.ratio_from_db(L, A_ref, dM)
    fr, b = np.unravel_index(ratio.argmax(), ratio.shape)
    print(f"N={n_fft} hop={hop} n={n} n_mels={n_mels} htk={htk} norm={norm} {family}: ratio {ratio.max():.4f} at frame {fr} band {b}")
    assert ratio.max() <= 1.0, (case, family, float(ratio.max()), int(fr), int(b))
    # the workspace maximum is the maximum of the GPU's own band powers: L is monotone in M, so the largest L is 10 log10(max(max M, 1e-10)) to the bit
    # (orcai_frontend_finalize evaluates the same expression on the workspace's maximum)
    assert h.lib.orcai_frontend_finalize(1, TOP_DB, h.wsp, h.s) == 0
    assert h.stats()[1] == np.float32(L.max()), (pmax, h.stats()[1], L.max())
    assert abs(float(pmax) - M_ref.max()) <= dM.max(), (pmax, M_ref.max())  # |max a - max b| <= max |a - b|
    if family == "silence":
        assert pmax == 0.0 and np.unique(L.view(np.int32)).size == 1 and abs(float(L.flat[0]) + 100.0) <= R.CLAMP_DB_TOL


# ------------------------------------------------------------------------------------------------ 2. the composition, exactly; 3. the same bytes twice
@pytest.mark.parametrize("case", [c for c in MR.cases() if c[3] in (8, 40, 256) or c[0] == 512], ids=lambda c: "N{}-hop{}-n{}-m{}-{}-{}-{}-{}".format(*c))
def test_make_mel_spectrogram_is_its_steps_and_repeats_its_bytes(h, case):
    from orcai_amd.frontend import nearest_rank_index

    n_fft, hop, n, n_mels, fmin, fmax, htk, norm = case
    x = MR.make_input("noise", n, n_fft, hop)
    xd = torch.tensor(x, device="cuda")
    t, wd = h.table(n_fft, n_mels, fmin, fmax, htk, norm)
    L, pmax, raw = h.stft_mel(xd, n_fft, hop, t, wd)
    L2, pmax2, raw2 = h.stft_mel(xd, n_fft, hop, t, wd)
    assert torch.equal(raw, raw2) and pmax == pmax2, "two runs of orcai_stft_mel_db differ"
    T = L.shape[0]
    total = T * n_mels
    q = (0.01, 0.999)
    r_lo, r_hi = nearest_rank_index(total, q[0]), nearest_rank_index(total, q[1])
    outs = []
    for _ in range(2):
        buf = h.buffer(total)
        a = h.args(xd, n_fft, hop, t, wd, buf)
        rc = h.lib.orcai_make_mel_spectrogram(*a[:11], r_lo, r_hi, TOP_DB, *a[11:])
        assert rc == 0 and h.untouched(buf, total)
        outs.append(buf)
    assert torch.equal(outs[0], outs[1]), "two runs of orcai_make_mel_spectrogram differ"
    got = outs[0][:total].view(torch.float32).cpu().numpy().reshape(T, n_mels)
    want, (ref, p_lo, p_hi) = MR.clip_normalize_ref(L, *q)
    st = h.stats()
    # (the clip bounds themselves may differ from the CPU's in the last place: orcai_frontend_finalize subtracts the reference level with a fused
    # multiply-add; what is held to 2 ulp is the output)
    assert st[1] == ref and abs(float(st[2]) - float(p_lo)) <= 1e-5 and abs(float(st[3]) - float(p_hi)) <= 1e-5, (st, ref, p_lo, p_hi)
    ulp = np.abs(got.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))
    print(f"N={n_fft} hop={hop} n_mels={n_mels}: composition differs from the CPU's by at most {ulp.max()} ulp")
    assert ulp.max() <= 2 and got.min() == 0.0 and got.max() == 1.0


# ------------------------------------------------------------------------------------------------ 4. refusals leave everything untouched
def test_refusals(h):
    n_fft, hop, n = 512, 256, 4100
    t, wd = h.table(512, *MR.MELS[512][1])
    n_mels = t["lo"].size
    xd = torch.tensor(MR.make_input("noise", n, n_fft, hop), device="cuda")
    T = R.num_frames(n, n_fft, hop)
    buf = h.buffer(T * n_mels)
    assert h.lib.orcai_frontend_reset(h.wsp, h.s) == 0
    torch.cuda.synchronize()
    ws_before = h.ws.clone()
    good = h.args(xd, n_fft, hop, t, wd, buf)

    def bad_table(key, m, v):
        b = {k: a.copy() for k, a in t.items()}
        b[key][m] = v
        return b

    cases = []
    for i, what in ((0, "pcm"), (6, "band_lo"), (7, "band_hi"), (8, "band_off"), (9, "weights"), (11, "out_db"), (12, "workspace")):
        a = list(good)
        a[i] = None
        cases.append((a, R.E_BADARG, f"null {what}"))
    for i, what in ((0, "pcm"), (9, "weights"), (11, "out_db")):
        a = list(good)
        a[i] = good[i] + 4
        cases.append((a, R.E_BADARG, f"misaligned {what}"))
    for i, v, what in ((1, 0, "n_samples 0"), (3, 0, "hop 0"), (4, T + 1, "n_frames + 1"), (4, T - 1, "n_frames - 1"), (5, 7, "n_mels 7"), (5, 257, "n_mels 257"),
                       (10, 0, "n_weights 0"), (10, 65536, "n_weights 65536"), (10, int(t["off"][-1]), "n_weights short of the last band")):
        a = list(good)
        a[i] = v
        cases.append((a, R.E_BADARG, what))
    keep = []
    for key, m, v, what in (("lo", 3, -1, "band_lo < 0"), ("hi", 5, 258, "band_hi > 1 + n_fft / 2"), ("hi", 2, int(t["lo"][2]) - 1, "band_hi < band_lo"),
                            ("off", 0, -4, "band_off < 0"), ("off", n_mels - 1, wd.numel(), "band_off past the weights")):
        b = bad_table(key, m, v)
        keep.append(b)
        a = list(good)
        a[6], a[7], a[8] = b["lo"].ctypes.data, b["hi"].ctypes.data, b["off"].ctypes.data
        cases.append((a, R.E_BADARG, what))
    for nf in (64, 500, 384, 8192):
        a = list(good)
        a[2] = nf
        a[4] = R.num_frames(n, nf, hop)
        cases.append((a, R.E_UNSUPPORTED, f"n_fft {nf}"))
    for a, want, what in cases:
        assert h.lib.orcai_stft_mel_db(*a) == want, what
    r_lo, r_hi = 10, T * n_mels - 10
    for a, want, what in cases:
        if a[12] is not None:
            assert h.lib.orcai_make_mel_spectrogram(*a[:11], r_lo, r_hi, TOP_DB, *a[11:]) == want, what
    assert h.lib.orcai_make_mel_spectrogram(*good[:11], r_lo, T * n_mels, TOP_DB, *good[11:]) == R.E_BADARG  # rank past the end
    torch.cuda.synchronize()
    assert h.untouched(buf), "a refused call wrote to the output"
    # the composition zeroes the workspace before its first check of the STFT arguments, as orcai_make_spectrogram does; nothing else may change it
    assert torch.equal(h.ws, ws_before)
    assert h.lib.orcai_stft_mel_occupancy() >= 2


# ------------------------------------------------------------------------------------------------ 5. wiring
SP = {"sampling_rate": 48000, "nfft": 512, "n_overlap": 256, "freq_range": [0, 16000], "quantiles": [0.01, 0.999], "duration": 4}


def test_frontend_routes_on_the_mel_key(h):
    from orcai_amd.frontend import get_frontend
    from orcai_amd.synthetic import pcm16_to_float, synth_recording

    fe = get_frontend()
    y = torch.from_numpy(pcm16_to_float(synth_recording(2.0, 48000, seed=3))).cuda()
    plain = fe.make_spectrogram(y, SP)
    assert torch.equal(fe.make_spectrogram(y, dict(SP, mel=None)).view(torch.int32), plain.view(torch.int32)) and plain.shape[1] == 171
    sp = dict(SP, mel={"n_mels": 64})
    got = fe.make_spectrogram(y, sp)
    assert tuple(got.shape) == fe.spectrogram_shape(y.numel(), sp) == (1 + y.numel() // 256, 64)
    # the same through the C ABI with the table built by hand
    t, wd = h.table(512, 64, 0.0, 16000.0, False, "slaney")
    L, _, _ = h.stft_mel(y, 512, 256, t, wd)
    want, _ = MR.clip_normalize_ref(L, 0.01, 0.999)
    assert np.abs(got.cpu().numpy().view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64)).max() <= 2
    assert len(fe._mel_tables) >= 1 and fe.make_spectrogram(y, sp).data_ptr() != got.data_ptr()
    n_tables = len(fe._mel_tables)
    fe.make_spectrogram(y, dict(sp))
    assert len(fe._mel_tables) == n_tables, "the band table is uploaded once per (device, parameter)"
    out, stats = fe.make_spectrogram(y, sp, return_stats=True)
    assert torch.equal(out, got) and stats.shape == (6,)
    with pytest.raises(NotImplementedError, match="mel"):
        fe.spectrogram_backward(y, torch.ones_like(got), stats, sp)
    # the torch op
    import orcai_amd.torch_ops  # noqa: F401

    op = torch.ops.orcai.mel_spectrogram(y, 48000, 512, 256, 64, 0.0, 16000.0, False, True, 0.01, 0.999)
    assert torch.equal(op.view(torch.int32), got.view(torch.int32))
    from torch._subclasses.fake_tensor import FakeTensorMode

    with FakeTensorMode():
        fake = torch.ops.orcai.mel_spectrogram(torch.empty(y.numel(), device="cuda"), 48000, 512, 256, 64, 0.0, 16000.0, False, True, 0.01, 0.999)
    assert tuple(fake.shape) == tuple(got.shape) and fake.dtype == torch.float32
    op_htk = torch.ops.orcai.mel_spectrogram(y, 48000, 1024, 256, 40, 0.0, 16000.0, True, False, 0.01, 0.999)
    assert torch.equal(op_htk, fe.make_spectrogram(y, dict(SP, nfft=1024, mel={"n_mels": 40, "htk": True, "norm": None})))


def _tiny_model_dir(folder, width, n_mels):
    import json

    from orcai_amd.architectures import ResNetLSTM
    from orcai_amd.io import read_json
    from pathlib import Path

    root = Path(__file__).resolve().parent.parent
    param = read_json(root / "orcai_amd" / "models" / "orcai-V1" / "orcai_parameter.json")
    param["name"] = "tiny"
    param["calls"] = ["A", "B", "C"]
    param["model"].update(filters=[10, 20], kernel_size=3, lstm_units=64)
    param["spectrogram"]["mel"] = {"n_mels": n_mels}
    folder.mkdir()
    (folder / "orcai_parameter.json").write_text(json.dumps(param))
    (folder / "model_shape.json").write_text(json.dumps({"input_shape": [32, width, 1], "num_labels": 3}))
    ResNetLSTM((32, width, 1), 3, [10, 20], 3, 0.0, 64, seed=5).save_weights(folder / "tiny.weights.npz")
    return folder


def test_predict_runs_a_mel_model_and_refuses_another_width(tmp_path):
    from orcai_amd import wavio
    from orcai_amd.frontend import get_frontend
    from orcai_amd.io import load_orcai_model
    from orcai_amd.predict import compute_aggregated_predictions, predict, predict_wav_finish, save_predictions
    from orcai_amd.spectrogram import make_spectrogram
    from orcai_amd.synthetic import pcm16_to_float, synth_recording

    pcm = synth_recording(1.5, 48000, seed=11)
    wav = tmp_path / "rec.wav"
    wavio.write_wav_pcm16(wav, pcm, 48000)
    model_dir = _tiny_model_dir(tmp_path / "tiny", 16, 16)
    predict(wav, channel=1, model_dir=model_dir, output_path=tmp_path / "got.txt", verbosity=0)
    # by hand: FrontEnd.make_spectrogram + the model on that spectrogram
    model, param, shape = load_orcai_model(model_dir)
    sp = param["spectrogram"]
    spec = get_frontend().make_spectrogram(torch.from_numpy(pcm16_to_float(pcm)).cuda(), sp)
    assert tuple(spec.shape) == (1 + pcm.size // 256, 16)
    delta_t = 256 / 48000
    pending = compute_aggregated_predictions(recording_path=wav, spectrogram=spec, model=model, orcai_parameter=param, shape=shape, wait=False, delta_t=delta_t)
    labels, agg, dt = predict_wav_finish({"pending": pending, "delta_t": delta_t, "orcai_parameter": param})
    save_predictions(labels, tmp_path / "want.txt", dt)
    assert (tmp_path / "got.txt").read_bytes() == (tmp_path / "want.txt").read_bytes()
    assert agg.shape == (spec.shape[0] // 4, 3) and np.isfinite(agg).all()
    # the public host API returns the band centres as its frequencies
    s, f, times = make_spectrogram(wav, 1, param, verbosity=0)
    assert s.shape == tuple(spec.shape) and np.array_equal(s, spec.cpu().numpy()) and times.size == s.shape[0]
    assert f.dtype == np.float64 and np.array_equal(f, mel.band_table(48000, 512, 16, 0.0, 16000.0)["centres"])
    # the same parameter file with a model of another width
    wide = _tiny_model_dir(tmp_path / "wide", 171, 16)
    with pytest.raises(ValueError, match=r"not equal to input shape \(171\).*mel"):
        predict(wav, channel=1, model_dir=wide, output_path=tmp_path / "never.txt", verbosity=0)
    assert not (tmp_path / "never.txt").exists()
