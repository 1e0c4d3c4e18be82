"""Several recordings, or every channel of one, in one detector pass, on the GPU.  Exact equality throughout: the two new launchers
against the launchers they generalise, predict_spectrograms against predict_spectrogram per recording (orcai-V1-shaped model and seed of
test_two_level_share_gpu), predict_wavs against predict_wav per item, and the files of predict(channel="all") / predict(batch_frames=N) against the
files of the one-by-one calls, byte for byte."""

import numpy as np
import pandas as pd
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from test_predict_e2e_gpu import _model_dir  # noqa: E402
from test_two_level_share_gpu import H, W, _model  # noqa: E402
from test_wav_decode import FORMATS, riff, sample_bytes  # noqa: E402

from orcai_amd import _native as N  # noqa: E402
from orcai_amd import batch as B  # noqa: E402
from orcai_amd import wavio  # noqa: E402

P, STEP = 46, 23


def bits(t):
    return t.contiguous().view(torch.int32)


def content(path):
    """The bytes of an output file; of a .gz the bytes inside (its header carries the time of writing)."""
    import gzip

    data = path.read_bytes()
    return gzip.decompress(data) if path.suffix == ".gz" else data


# ------------------------------------------------------------------ 1. orcai_overlap_average_ragged
def _ragged_case(recordings, L, integer, seed=0):
    """recordings = [(n_r, uncovered trailing steps, snippets skipped before it)].  Returns (pred, table rows, [S_r])."""
    table, first, row = [], 0, 0
    for n, trailing, skipped in recordings:
        first += skipped
        S = (n - 1) * STEP + P + trailing
        table.append((first, n, S, row))
        first, row = first + n, row + S
    g = torch.Generator(device="cuda").manual_seed(seed)
    if integer:
        pred = torch.randint(-9, 10, (first, P, L), generator=g, device="cuda").to(torch.float32)
    else:
        pred = torch.rand((first, P, L), generator=g, device="cuda", dtype=torch.float32)
    return pred, table, row


def _ragged(pred, table, S_total, L):
    dev = torch.tensor(table, dtype=torch.int64, device="cuda")
    agg = torch.full((S_total, L), -7.0, dtype=torch.float64, device="cuda")
    cnt = torch.full((S_total,), -7.0, dtype=torch.float64, device="cuda")
    N.check(N.lib().orcai_overlap_average_ragged(N.ptr(pred), P, L, STEP, N.ptr(dev), len(table), S_total, N.ptr(agg), N.ptr(cnt), N.stream_ptr()),
            "orcai_overlap_average_ragged")
    return agg, cnt


@pytest.mark.parametrize("integer", [False, True])
@pytest.mark.parametrize("recordings,L", [
    ([(1, 0, 0), (2, 13, 2), (3, 0, 1), (29, 13, 2), (1, 13, 1), (29, 0, 2)], 7),
    ([(29, 13, 0)], 7),
    ([(3, 13, 0), (1, 0, 1), (2, 13, 2)], 1),
])
def test_ragged_average_equals_the_launcher_per_recording(recordings, L, integer):
    pred, table, S_total = _ragged_case(recordings, L, integer, seed=len(recordings) + L)
    agg, cnt = _ragged(pred, table, S_total, L)
    lib, st = N.lib(), N.stream_ptr()
    for first, n, S, row in table:
        a = torch.empty((S, L), dtype=torch.float64, device="cuda")
        c = torch.empty((S,), dtype=torch.float64, device="cuda")
        assert lib.orcai_overlap_average(N.ptr(pred[first:]), n, P, L, STEP, S, N.ptr(a), N.ptr(c), st) == 0
        assert torch.equal(agg[row : row + S].view(torch.int64), a.view(torch.int64)) and torch.equal(cnt[row : row + S], c), (first, n, S)
        covered = (n - 1) * STEP + P
        assert bool((c[:covered] >= 1).all()) and bool((c[covered:] == 0).all()) and bool((a[covered:] == 0).all())
        if integer:  # sums of at most two small integers, halved: exact by hand
            p = pred[first : first + n].double().cpu().numpy()
            want, k = np.zeros((S, L)), np.zeros(S)
            for i in range(n):
                want[i * STEP : i * STEP + P] += p[i]
                k[i * STEP : i * STEP + P] += 1
            want[k > 0] /= k[k > 0][:, None]
            assert np.array_equal(a.cpu().numpy(), want) and np.array_equal(c.cpu().numpy(), k)


def test_ragged_average_refusals():
    pred, table, S_total = _ragged_case([(2, 0, 0)], 7, True)
    dev = torch.tensor(table, dtype=torch.int64, device="cuda")
    out = torch.full((S_total * 8,), -7.0, dtype=torch.float64, device="cuda")
    p, t, a, s = N.ptr(pred), N.ptr(dev), N.ptr(out), N.stream_ptr()
    call = N.lib().orcai_overlap_average_ragged
    assert call(None, P, 7, STEP, t, 1, S_total, a, a, s) == N.E_BADARG and call(p, P, 7, STEP, None, 1, S_total, a, a, s) == N.E_BADARG
    assert call(p, P, 7, STEP, t, 1, S_total, None, a, s) == N.E_BADARG and call(p, P, 7, STEP, t, 1, S_total, a, None, s) == N.E_BADARG
    assert call(p, P, 7, STEP, t, 0, S_total, a, a, s) == N.E_BADARG and call(p, P, 7, STEP, t, -1, S_total, a, a, s) == N.E_BADARG
    assert call(p, P, 7, STEP, t, 1, 0, a, a, s) == N.E_BADARG and call(p, P, 0, STEP, t, 1, S_total, a, a, s) == N.E_BADARG
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())  # nothing was launched


# ------------------------------------------------------------------ 2. orcai_pcm_decode_planar
def _upload(payload: bytes):
    n = len(payload)
    dev = torch.full((-(-n // 16) * 16,), 0xA5, dtype=torch.uint8, device="cuda")
    dev[:n] = torch.frombuffer(bytearray(payload), dtype=torch.uint8).cuda()
    return dev


@pytest.mark.parametrize("channels", [1, 2, 3, 5, 64])
@pytest.mark.parametrize("fmt", FORMATS)
def test_planar_decode_equals_read_wav_and_the_one_channel_decode(tmp_path, fmt, channels):
    """Frames: 1, 3, one more than the 256 threads of a workgroup cover in one pass, one more than the largest tile (4096 frames), a few thousand;
    sample_bytes puts the extreme codes of the format first."""
    sample_format = FORMATS.index(fmt)
    path = tmp_path / "a.wav"
    for frames in (1, 3, 257, 4097, 5003):
        payload = sample_bytes(fmt, channels * frames, seed=100 * channels + frames)
        path.write_bytes(riff(fmt, channels, 8000, payload))
        with np.errstate(over="ignore", under="ignore", invalid="ignore"):
            ref = torch.from_numpy(wavio.read_wav(path)[0]).cuda()
        dev = _upload(payload)
        stride = -(-frames // 4) * 4
        out = torch.full((channels, stride), -7.0, device="cuda")
        N.check(N.lib().orcai_pcm_decode_planar(N.ptr(dev), frames, channels, sample_format, N.ptr(out), stride, N.stream_ptr()), "orcai_pcm_decode_planar")
        assert torch.equal(bits(out[:, :frames]), bits(ref)), (fmt, channels, frames)
        assert bool((out[:, frames:] == -7.0).all())  # the pad floats of a plane are not written
        for channel in range(channels):
            one = wavio.decode_device(dev, frames, channels, channel, sample_format)
            assert torch.equal(bits(out[channel, :frames]), bits(one)), (fmt, channels, frames, channel)
        planes = wavio.decode_device_planar(dev, frames, channels, sample_format)
        assert planes.shape == (channels, frames) and torch.equal(bits(planes), bits(ref))
        assert all(planes[c].is_contiguous() and planes[c].data_ptr() % 16 == 0 for c in range(channels))


def test_planar_decode_refusals_and_upload(tmp_path):
    dev = _upload(sample_bytes("S16", 64, seed=0))
    out = torch.full((64,), -7.0, device="cuda")
    f, o, s = N.ptr(dev), N.ptr(out), N.stream_ptr()
    cases = {"null frames": (None, 16, 2, 1, o, 16), "null out": (f, 16, 2, 1, None, 16), "misaligned frames": (f + 4, 16, 2, 1, o, 16),
             "misaligned out": (f, 16, 2, 1, o + 4, 16), "no frames": (f, 0, 2, 1, o, 16), "no channels": (f, 16, 0, 1, o, 16),
             "65 channels": (f, 1, 65, 0, o, 4), "format 6": (f, 16, 2, 6, o, 16), "format -1": (f, 16, 2, -1, o, 16),
             "stride below frames": (f, 16, 2, 1, o, 12), "stride not a multiple of 4": (f, 14, 2, 1, o, 14)}
    for name, args in cases.items():
        assert N.lib().orcai_pcm_decode_planar(*args, s) == N.E_BADARG, name
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())
    # upload_and_decode_all: the page-locked route of a 3-channel PCM24 file, against the host decode
    path = tmp_path / "b.wav"
    path.write_bytes(riff("S24", 3, 22050, sample_bytes("S24", 3 * 7001, seed=4)))
    planes = wavio.upload_and_decode_all(wavio.read_wav_raw(path, pin=True))
    assert torch.equal(bits(planes), bits(torch.from_numpy(wavio.read_wav(path)[0]).cuda()))


# ------------------------------------------------------------------ 3. predict_spectrograms
T_LIST = [736, 737, 1104, 1471, 2944 + 5]  # 1 + 1 + 2 + 2 + 7 real snippets


def _specs(seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return [torch.rand((T, W), generator=g, device="cuda", dtype=torch.float32) for T in T_LIST]


@pytest.fixture(scope="module")
def singles():
    """predict_spectrogram per recording, f32: computed once, shared, never changed."""
    model = _model()
    return [model.predict_spectrogram(s).clone() for s in _specs()]


def test_predict_spectrograms_f32_one_batch_and_three(singles):
    model = _model()
    specs = _specs()
    assert [s.shape[0] for s in singles] == [1, 1, 2, 2, 7]
    plan = B.plan_batches(T_LIST, H, B.DEFAULT_MAX_FRAMES)
    assert len(plan) == 1 and plan[0].n_total == 19 and plan[0].junk == 6
    got = model.predict_spectrograms(specs)
    assert all(torch.equal(bits(g), bits(s)) for g, s in zip(got, singles))
    assert [len(b.items) for b in B.plan_batches(T_LIST, H, 2600)] == [2, 2, 1]  # max_frames small enough to force three batches
    got = model.predict_spectrograms(specs, max_frames=2600)
    assert all(torch.equal(bits(g), bits(s)) for g, s in zip(got, singles))
    short = model.predict_spectrograms([specs[0][:735].contiguous(), specs[1]])
    assert short[0].shape == (0, model.out_steps, 7) and torch.equal(bits(short[1]), bits(singles[1]))


def test_predict_spectrograms_f16():
    from orcai_amd.architectures import ResNetLSTM

    model = ResNetLSTM((H, W, 1), 7, [30, 40, 50, 60], 3, 0.0, 128, seed=1, precision="f16")
    specs = _specs(seed=1)
    want = [model.predict_spectrogram(s).clone() for s in specs]
    got = model.predict_spectrograms(specs)
    assert all(torch.equal(bits(g), bits(w)) for g, w in zip(got, want))


def test_a_nan_recording_in_the_middle_leaves_its_neighbours_alone(singles):
    """A constant spectrogram is all NaN after normalisation (0 / 0, as in the reference).  In the middle of the batch its rows lie inside the
    super-images its neighbours' rows lie in: their bits must not change, and its own result is the single call's NaN pattern."""
    from orcai_amd.frontend import get_frontend

    model = _model()
    specs = _specs()
    nan = torch.full((T_LIST[2], W), -100.0, device="cuda")
    get_frontend().normalize_inplace(nan, [0.01, 0.999])
    assert bool(torch.isnan(nan).all())
    specs[2] = nan
    want = model.predict_spectrogram(nan).clone()
    got = model.predict_spectrograms(specs)
    for r in (0, 1, 3, 4):
        assert torch.equal(bits(got[r]), bits(singles[r])), r
    assert torch.equal(torch.isnan(got[2]), torch.isnan(want)) and torch.equal(got[2].nan_to_num(7.0), want.nan_to_num(7.0))
    assert torch.allclose(got[2], want, rtol=0, atol=0, equal_nan=True)


# ------------------------------------------------------------------ 4. - 6. from the files
@pytest.fixture(scope="module")
def loaded(tmp_path_factory):
    from orcai_amd.io import load_orcai_model

    model_dir, _ = _model_dir(tmp_path_factory.mktemp("batch_model"))
    return (model_dir, *load_orcai_model(model_dir))


def _clips(folder):
    from orcai_amd.synthetic import synth_recording

    folder.mkdir()
    clips = [("a", 12.0, 48000), ("b", 9.0, 22050), ("c", 3.0, 48000), ("d", 4.5, 48000), ("e", 8.0, 48000)]  # c: shorter than one snippet (3.93 s)
    for i, (name, seconds, rate) in enumerate(clips):
        wavio.write_wav_pcm16(folder / f"{name}.wav", synth_recording(seconds, rate, seed=30 + i), rate)
    return [folder / f"{name}.wav" for name, _, _ in clips]


def test_predict_wavs_equals_predict_wav_per_item(tmp_path, loaded):
    from orcai_amd.predict import predict_wav, predict_wavs

    _, model, param, shape = loaded
    paths = _clips(tmp_path / "clips")
    got = predict_wavs([(p, 1) for p in paths], model, param, shape)
    assert len(got) == 5
    for i, p in enumerate(paths):
        if i == 2:
            with pytest.raises(ValueError, match="recording too short") as single:
                predict_wav(p, 1, model, param, shape)
            assert isinstance(got[i], ValueError) and str(got[i]) == str(single.value)
            continue
        labels, agg, delta_t = predict_wav(p, 1, model, param, shape)
        assert isinstance(got[i], tuple), got[i]
        assert got[i][0].equals(labels) and list(got[i][0].columns) == list(labels.columns)
        assert got[i][1].dtype == np.float64 and np.array_equal(got[i][1], agg) and got[i][2] == delta_t
    # two batches (the host half of the first beside the GPU half of the second): the same results
    again = predict_wavs([(p, 1) for p in paths], model, param, shape, max_frames=4000)
    for a, b in zip(got, again):
        assert type(a) is type(b) and (isinstance(a, Exception) or (a[0].equals(b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]))


def test_predict_all_channels_writes_the_single_channel_files(tmp_path, loaded):
    from orcai_amd.predict import predict
    from orcai_amd.synthetic import synth_recording

    model_dir = loaded[0]
    rate, seconds = 22050, 8.0
    pcm = np.stack([synth_recording(seconds, rate, seed=40 + c) for c in range(3)]).astype(np.int32)  # [3][n]
    v = (pcm.T << 8) | (np.arange(pcm.size, dtype=np.int32).reshape(-1, 3) & 0xFF)
    payload = np.ascontiguousarray(v).view(np.uint8).reshape(-1, 4)[:, :3].tobytes()
    want = {}
    for mode in ("single", "all"):
        folder = tmp_path / mode
        folder.mkdir()
        (folder / "array.wav").write_bytes(riff("S24", 3, rate, payload))
        if mode == "single":
            for c in (1, 2, 3):
                predict(folder / "array.wav", channel=c, model_dir=model_dir, save_probabilities=True, verbosity=0)
        else:
            predict(folder / "array.wav", channel="all", model_dir=model_dir, save_probabilities=True, verbosity=0)
        files = sorted(f.name for f in folder.iterdir() if f.name != "array.wav")
        assert files == sorted([f"array_c{c}_orcai-v1_predicted.txt" for c in (1, 2, 3)] + [f"array_c{c}_orcai-v1_predicted_probabilities.csv.gz" for c in (1, 2, 3)])
        want[mode] = {name: content(folder / name) for name in files}
    assert want["all"] == want["single"]
    assert len({want["all"][f"array_c{c}_orcai-v1_predicted_probabilities.csv.gz"] for c in (1, 2, 3)}) == 3  # three different channels
    with pytest.raises(FileExistsError):
        predict(tmp_path / "all" / "array.wav", channel="all", model_dir=model_dir, verbosity=0)


def test_predict_table_with_batch_frames_writes_the_same_files(tmp_path, loaded, capsys):
    from orcai_amd.predict import predict

    model_dir = loaded[0]
    paths = _clips(tmp_path / "clips")
    names = ["a", "b", "d", "e", "missing"]
    table = pd.DataFrame({"recording": names, "base_dir_recording": [str(tmp_path / "clips")] * 5,
                          "rel_recording_path": ["a.wav", "b.wav", "d.wav", "e.wav", "nope.wav"], "channel": [1] * 5})
    table.to_csv(tmp_path / "table.csv", index=False)
    out = {}
    for mode, batch_frames in (("one_by_one", 0), ("batched", 3000), ("one_batch", 675000)):
        folder = tmp_path / mode
        folder.mkdir()
        predict(tmp_path / "table.csv", model_dir=model_dir, output_path=folder, save_probabilities=True, verbosity=1, batch_frames=batch_frames)
        text = capsys.readouterr()
        assert "Error predicting missing" in text.out + text.err, mode  # the unreadable fifth row is logged and the run goes on
        out[mode] = {f.name: content(f) for f in sorted(folder.iterdir())}
        assert sorted(out[mode]) == sorted([f"{n}_model_predicted.txt" for n in names[:4]] + [f"{n}_model_predicted_probabilities.csv.gz" for n in names[:4]])
    assert out["batched"] == out["one_by_one"] and out["one_batch"] == out["one_by_one"]
    assert paths[0].exists()
