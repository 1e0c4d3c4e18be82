"""LSTM widths 32..256 (multiples of 32) and 9..64 call labels on the HIP path: the recurrence kernels against float64, the dense + sigmoid
head, the model forward and training steps (f32, f16, ResNet1DConv) against the oracle, and the workflows: the training loop replayed as a
hipGraph at U = 256, `train`, `hyperparameter_search` over lstm_units [32, 256], and `predict` with a 12-call `init-weights` model."""

import json
from pathlib import Path

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from oracle import model_ref as M  # noqa: E402
from oracle import train_ref as T  # noqa: E402

from lstm_ref import _bwd_ref, _fwd_ref, sig  # noqa: E402

ROOT = Path(__file__).resolve().parent.parent
CALLS12 = [f"C{i:02d}" for i in range(12)]

@pytest.mark.parametrize("U", [32, 96, 160, 256])
@pytest.mark.parametrize("B,Tn", [(7, 46), (20, 9), (65, 9)])
def test_lstm_recurrence_widths_vs_float64(U, B, Tn):
    """orcai_lstm_train_fwd (both orcai_lstm_split settings) and orcai_lstm_recurrent against a float64 recurrence: h, gates and cell states
    within 1e-5 over all dependent steps, and the inference entry equal to the training entry's h."""
    from orcai_amd import _native as N

    lib, st = N.lib(), N.stream_ptr()
    rng = np.random.default_rng(U + B + Tn)
    xz = rng.standard_normal((B, Tn, 2, 4 * U)).astype(np.float32)
    Uw = (rng.standard_normal((2, U, 4 * U)) * (0.8 / np.sqrt(U))).astype(np.float32)
    xd, ud = torch.from_numpy(xz).cuda(), torch.from_numpy(Uw).cuda()
    href, gref, cref = _fwd_ref(xz, Uw)
    prev = lib.orcai_lstm_split(-1)
    try:
        for split in (0, 1):
            lib.orcai_lstm_split(split)
            h = torch.full((B + 1, Tn, 2 * U), -7.0, device="cuda")
            g = torch.full((B + 1, Tn, 2, 4 * U), -7.0, device="cuda")
            c = torch.full((B + 1, Tn, 2, U), -7.0, device="cuda")
            N.check(lib.orcai_lstm_train_fwd(N.ptr(xd), N.ptr(ud), B, Tn, U, N.ptr(h), N.ptr(g), N.ptr(c), st), "lstm_train_fwd")
            hi = torch.full((B + 1, Tn, 2 * U), -7.0, device="cuda")
            N.check(lib.orcai_lstm_recurrent(N.ptr(xd), N.ptr(ud), B, Tn, U, N.ptr(hi), st), "lstm_recurrent")
            torch.cuda.synchronize()
            h, g, c, hi = (a.cpu().numpy() for a in (h, g, c, hi))
            errs = [float(np.abs(a[:B] - b).max()) for a, b in ((h, href), (g, gref), (c, cref))]
            print(f"U {U} B {B} T {Tn} split {split}: max |h, gates, c - float64| = {errs}")
            assert max(errs) <= 1e-5, (split, errs)
            assert (h[B] == -7.0).all() and (g[B] == -7.0).all() and (c[B] == -7.0).all() and (hi[B] == -7.0).all()  # nothing past the last row
            assert np.abs(hi[:B] - h[:B]).max() <= 1e-6 if U <= 128 else np.array_equal(hi, h)  # the wide family: one kernel body for both entries
    finally:
        lib.orcai_lstm_split(prev)


@pytest.mark.parametrize("U", [32, 96, 160, 256])
@pytest.mark.parametrize("B,Tn,gscale", [(20, 46, 1e-4), (7, 9, 3.0), (65, 9, 1e-9)])
def test_lstm_backward_widths_vs_float64(U, B, Tn, gscale):
    """orcai_lstm_bwd (both split settings) against the float64 backward through time, relative to the largest dxz, at incoming gradient scales
    1e-9 .. 3: the bar of the split kernel's test against the f32 kernel (5e-6)."""
    from orcai_amd import _native as N

    lib, st = N.lib(), N.stream_ptr()
    rng = np.random.default_rng(U + Tn + B)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)  # noqa: E731
    gates = sig(f(B, Tn, 2, 4 * U)).astype(np.float32)
    gv = gates.reshape(B, Tn, 2, U // 8, 4, 8)
    gv[..., 2, :] = np.tanh(f(B, Tn, 2, U // 8, 8))
    cst = f(B, Tn, 2, U) * 0.7
    dH = (f(B, Tn, 2 * U) * gscale).astype(np.float32)
    Uw = (f(2, U, 4 * U) * (0.8 / np.sqrt(U))).astype(np.float32)
    ref = _bwd_ref(dH, gates, cst, Uw)
    scale = np.abs(ref).max()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    gd, cd, hd, ud = dev(gates), dev(cst), dev(dH), dev(Uw)
    prev = lib.orcai_lstm_split(-1)
    try:
        for split in (0, 1):
            lib.orcai_lstm_split(split)
            dxz = torch.full((B + 1, Tn, 2, 4 * U), -7.0, device="cuda")
            N.check(lib.orcai_lstm_bwd(N.ptr(hd), N.ptr(gd), N.ptr(cd), N.ptr(ud), B, Tn, U, N.ptr(dxz), st), "lstm_bwd")
            torch.cuda.synchronize()
            got = dxz.cpu().numpy()
            assert (got[B] == -7.0).all()
            err = float(np.abs(got[:B] - ref).max()) / scale
            print(f"LSTM backward U {U} B {B} T {Tn} |dH| ~ {gscale:g} split {split}: max |dxz - float64| / max |dxz| = {err:.2e}")
            assert np.isfinite(got).all() and err <= 5e-6, (split, err)
    finally:
        lib.orcai_lstm_split(prev)


@pytest.mark.parametrize("N_", [9, 16, 33, 64])
@pytest.mark.parametrize("M_,K", [(2944, 128), (33, 36), (7, 6)])
def test_dense_sigmoid_wide_vs_float64(M_, K, N_):
    from orcai_amd import _native as N

    lib, st = N.lib(), N.stream_ptr()
    rng = np.random.default_rng(K + N_ + M_)
    x, w, b = rng.standard_normal((M_, K)).astype(np.float32), (rng.standard_normal((K, N_)) / np.sqrt(K)).astype(np.float32), rng.standard_normal(N_).astype(np.float32)
    xd, wd, bd = (torch.from_numpy(a).cuda() for a in (x, w, b))
    out = torch.full((M_ + 1, N_), -1.0, device="cuda")
    N.check(lib.orcai_dense_sigmoid(N.ptr(xd), N.ptr(wd), N.ptr(bd), M_, K, N_, N.ptr(out), st), "dense_sigmoid")
    want = 1.0 / (1.0 + np.exp(-(x.astype(np.float64) @ w.astype(np.float64) + b)))
    got = out.cpu().numpy()
    assert np.abs(got[:M_] - want).max() <= 1e-6 and (got[M_] == -1.0).all()


def test_dense_sigmoid_refuses_more_than_64_labels():
    from orcai_amd import _native as N

    lib = N.lib()
    x = torch.zeros((4, 8), device="cuda")
    w, b = torch.zeros((8, 65), device="cuda"), torch.zeros(65, device="cuda")
    out = torch.zeros((4, 65), device="cuda")
    assert lib.orcai_dense_sigmoid(N.ptr(x), N.ptr(w), N.ptr(b), 4, 8, 65, N.ptr(out), N.stream_ptr()) != 0


def _cfg(rng, train):
    nb = int(rng.integers(1, 4))
    H = int(rng.integers(2, 6)) * 2**nb
    W = int(rng.choice([11, 20, 31, 60, 65]))
    filters = tuple(int(rng.integers(3, 40)) for _ in range(nb))
    return dict(input_shape=(H, W, 1), filters=filters, kernel_size=int(rng.choice([3, 5])), lstm_units=int(rng.choice([32, 96, 192, 256])),
                num_labels=int(rng.integers(9, 65)))


@pytest.mark.parametrize("seed", range(4))
def test_wide_head_inference_configs(seed):
    from orcai_amd.architectures import ResNetLSTM

    rng = np.random.default_rng(3000 + seed)
    cfg = _cfg(rng, train=False)
    p = M.calibrated_params(seed=seed, **cfg)
    model = ResNetLSTM(cfg["input_shape"], cfg["num_labels"], list(cfg["filters"]), cfg["kernel_size"], 0.0, cfg["lstm_units"])
    model.set_weights_dict(p)
    B = int(rng.choice([1, 15, 17, 33]))
    x = rng.random((B, *cfg["input_shape"]), dtype=np.float32)
    ref = M.forward_ref(p, x)
    out = model.predict(x, batch_size=B)
    assert out.shape == ref.shape, cfg
    assert np.abs(out - ref).max() <= 1e-5, (cfg, B, float(np.abs(out - ref).max()))


def test_wide_head_half_forward():
    """The f16 engine at U = 256 and 40 labels (its recurrences run on the f32 kernels) at the f16 forward's bar."""
    from orcai_amd.architectures import ResNetLSTM

    cfg = dict(input_shape=(64, 61, 1), num_labels=40, filters=(30, 40, 50, 60), kernel_size=3, lstm_units=256)
    p = M.calibrated_params(seed=8, **cfg)
    model = ResNetLSTM(cfg["input_shape"], 40, list(cfg["filters"]), 3, 0.0, 256, precision="f16")
    model.set_weights_dict(p)
    x = np.random.default_rng(9).random((5, 64, 61, 1), dtype=np.float32)
    got = model.predict(x, batch_size=5)
    assert got.shape == (5, 4, 40)
    assert np.abs(got - M.forward_ref(p, x)).max() <= 5e-3


def test_wide_labels_resnet_1dconv_forward():
    from test_model_gpu import make_1dconv

    model, p = make_1dconv(7, (96, 20, 1), (10, 20), 3, num_labels=12)
    x = np.random.default_rng(2).random((3, 96, 20, 1), dtype=np.float32)
    ref = M.forward_ref_1dconv(p, x)
    xd = torch.from_numpy(x[..., 0].copy()).cuda()
    out = torch.empty((3, 24, 12), dtype=torch.float32, device="cuda")
    model.forward_device(xd.view(-1), 96 * 20, 3, out)
    assert np.abs(out.cpu().numpy() - ref).max() <= 1e-5


@pytest.mark.parametrize("u,L,B", [(256, 12, 3), (32, 40, 5)])
def test_wide_head_training_step(u, L, B):
    from orcai_amd.architectures import ResNetLSTM
    from orcai_amd.training import Trainer

    rng = np.random.default_rng(4000 + u)
    cfg = dict(input_shape=(32, 20, 1), filters=(10, 20, 30), kernel_size=3, lstm_units=u, num_labels=L)
    p = M.calibrated_params(seed=u, **cfg)
    for k in p:
        if k.endswith(("gamma", "beta")):
            p[k] = (p[k] + 0.2 * rng.standard_normal(p[k].shape)).astype(np.float32)
    H, W, _ = cfg["input_shape"]
    steps = H // 8
    x = rng.random((B, H, W, 1), dtype=np.float32)
    y = (rng.random((B, steps, L)) > 0.5).astype(np.float32)
    y[0, :, 0] = -1.0
    ref = T.loss_and_grads(p, x, y, None, 0.0)
    model = ResNetLSTM(cfg["input_shape"], L, list(cfg["filters"]), 3, 0.0, u)
    model.set_weights_dict(p)
    tr = Trainer(model, learning_rate=1e-3)
    out = tr.forward_backward(torch.from_numpy(np.ascontiguousarray(x[..., 0])).cuda().view(-1), H * W, B, torch.from_numpy(y).cuda(), masks=None)
    acc = out["acc"].cpu().numpy()
    assert np.abs(out["probs"].cpu().numpy() - ref["probs"]).max() <= 5e-6
    assert abs(acc[0] / acc[1] + acc[3] - ref["loss"]) <= 2e-6 * max(1.0, abs(ref["loss"]))
    bad = {}
    for name, g in ref["grads"].items():
        got = tr.P.G(name).cpu().numpy()
        zero_mean_bias = name.endswith("/bias") and not name.startswith(("dense2", "lstm", "dense1")) and "res" not in name
        scale = max(1e-3, float(np.abs(g).max())) if not zero_mean_bias else 1.0
        err = float(np.abs(got - g).max()) / scale
        if err > (5e-4 if not zero_mean_bias else 1e-4):
            bad[name] = err
    assert not bad, bad


@pytest.mark.parametrize("u", [32, 96, 256])
def test_wide_head_half_training_step(u):
    """One f16 training step at 12 labels, held to the bars of tests/test_half_gpu.py's step test: U = 32 and 96 run the f16 recurrence
    kernels (orcai_h_lstm_train_fwd / orcai_h_lstm_bwd, the U = 96 backward with its > 64 KiB LDS opt-in), U = 256 the f32 wide family."""
    from test_half_gpu import _check_half_step, _train_setup

    cfg = dict(input_shape=(32, 12, 1), filters=(10, 20), kernel_size=3, lstm_units=u, num_labels=12)
    ref, tr, out = _train_setup(cfg, 3, seed=5, rate=0.5, precision="f16")
    _check_half_step(cfg, 3, ref, tr, out, seed=5)


def test_wide_labels_resnet_1dconv_training_step():
    """Conv1DHeadTrainer end to end at 12 labels: forward + masked BCE + full backward against torch autograd (float64)."""
    from orcai_amd.architectures import FINAL_FILTERS, ResNet1DConv
    from orcai_amd.training import Trainer

    L = 12
    cfg = dict(input_shape=(48, 21, 1), filters=(12, 30, 40), kernel_size=3, lstm_units=64, num_labels=L)
    p = M.calibrated_params(seed=6, **cfg)
    p = {k: v for k, v in p.items() if not k.startswith(("lstm", "dense", "bn_d"))}
    rng = np.random.default_rng(16)
    for k in p:
        if k.endswith(("gamma", "beta")):
            p[k] = (p[k] + 0.2 * rng.standard_normal(p[k].shape)).astype(np.float32)
    p["conv1d/kernel"] = (0.1 * rng.standard_normal((FINAL_FILTERS, FINAL_FILTERS, L))).astype(np.float32)
    p["conv1d/bias"] = (0.1 * rng.standard_normal(L)).astype(np.float32)
    B, (H, W, _) = 3, cfg["input_shape"]
    x = rng.random((B, H, W, 1), dtype=np.float32)
    y = (rng.random((B, H // 8, L)) > 0.5).astype(np.float32)
    y[1, :, 10] = -1.0
    model = ResNet1DConv(cfg["input_shape"], L, list(cfg["filters"]), 3, 0.0)
    model.set_weights_dict(p)
    ref = T.loss_and_grads_1dconv(p, x, y, None, 0.0)
    tr = Trainer(model, learning_rate=1e-3)
    out = tr.forward_backward(torch.from_numpy(np.ascontiguousarray(x[..., 0])).cuda().view(-1), H * W, B, torch.from_numpy(y).cuda(), masks=None)
    acc = out["acc"].cpu().numpy()
    assert out["probs"].shape == (B, H // 8, L)
    assert np.abs(out["probs"].cpu().numpy() - ref["probs"]).max() <= 5e-6
    assert abs(acc[0] / acc[1] - ref["loss"]) <= 2e-6 * max(1.0, abs(ref["loss"]))
    bad = {}
    for name, g in ref["grads"].items():
        got = tr.P.G(name).cpu().numpy()
        zero_mean_bias = name.endswith("/bias") and "res" not in name and not name.startswith("conv1d")
        scale = max(1e-3, float(np.abs(g).max())) if not zero_mean_bias else 1.0
        err = float(np.abs(got - g).max()) / scale
        if err > (5e-4 if not zero_mean_bias else 1e-4):
            bad[name] = err
    assert not bad, bad


# ---------------------------------------------------------------------------------------------------------------------------------
# Workflows at the new shapes
def _param12(**model_over):
    from orcai_amd.io import read_json

    p = read_json(ROOT / "orcai_amd" / "defaults" / "default_orcai_parameter.json")
    p["calls"] = list(CALLS12)
    p["seed"] = 1234
    p["model"].update({"filters": [10, 20], "lstm_units": 256, "batch_size": 8, "epochs": 2, "learning_rate": 3e-3, "dropout_rate": 0.0})
    p["model"].update(model_over)
    return p


def _data12(tmp_path, n_train=32, n_val=16):
    from orcai_amd.datasets import make_synthetic_dataset

    d = tmp_path / "data"
    d.mkdir()
    make_synthetic_dataset(d / "train_dataset", n_train, seed=4, input_shape=(32, 12), out_steps=8, n_labels=12)
    make_synthetic_dataset(d / "val_dataset", n_val, seed=5, input_shape=(32, 12), out_steps=8, n_labels=12)
    (d / "dataset_shapes.json").write_text(json.dumps({"spectrogram": [32, 12, 1], "labels": [8, 12]}))
    return d


def test_wide_head_fit_loop_on_a_replayed_graph(tmp_path):
    """Two epochs of FitLoop at U = 256 and 12 labels with the step replayed as one hipGraph against eager launches: the wide recurrence
    kernels (and their LDS opt-in, done in the eager warm-up) inside a captured graph give the eager run's losses, up to the float-atomic
    reordering bar of tests/test_train_workflow_gpu.py's graph test."""
    from orcai_amd.architectures import ResNetLSTM
    from orcai_amd.datasets import SnippetDataset
    from orcai_amd.fit import FitLoop
    from orcai_amd.training import Trainer

    d = _data12(tmp_path)
    runs = {}
    for graph in (False, True):
        model = ResNetLSTM((32, 12, 1), 12, [10, 20], 3, 0.0, 256, seed=3)
        tr = Trainer(model, learning_rate=3e-3, seed=1)
        loop = FitLoop(model, tr, graph_step=graph)
        assert loop.graph_step == graph
        train = SnippetDataset(d / "train_dataset", 8, seed=[1, 2], shuffle=True)
        val = SnippetDataset(d / "val_dataset", 8, seed=[3, 4], shuffle=False)
        h = loop.fit(train, validation_data=val, epochs=2).history
        runs[graph] = (h, tr.P.w.clone(), tr._graph is not None)
        tr.release_graph()
    (eh, ew, eg), (gh, gw, gg) = runs[False], runs[True]
    assert not eg and gg  # the graphed loop really replayed a graph
    assert len(eh["loss"]) == len(gh["loss"]) == 2 and np.isfinite(gh["loss"]).all()
    for k in ("loss", "val_loss", "MBA", "val_MBA"):
        assert np.allclose(eh[k], gh[k], rtol=0, atol=2e-3), (k, eh[k], gh[k])
    assert float((ew - gw).abs().max()) <= 2e-3


def test_train_api_at_256_units_and_12_calls(tmp_path):
    """`train` (graph_step on by default) for two epochs with 12 calls and lstm_units 256: outputs written, reloadable, 12 label columns."""
    from orcai_amd.io import load_orcai_model
    from orcai_amd.train import train

    d = _data12(tmp_path)
    out = tmp_path / "out"
    out.mkdir()
    train(d, out, _param12(), verbosity=0)
    mdir = out / "orcai-v1"
    hist = json.loads((mdir / "training_history.json").read_text())
    assert len(hist["loss"]) == 2 and np.isfinite(hist["loss"]).all() and np.isfinite(hist["val_loss"]).all()
    assert json.loads((mdir / "model_shape.json").read_text()) == {"input_shape": [32, 12, 1], "num_labels": 12}
    model, p2, _ = load_orcai_model(mdir)
    assert model.lstm_units == 256 and p2["calls"] == CALLS12
    x = np.random.default_rng(0).random((3, 32, 12, 1), dtype=np.float32)
    probs = model.predict(x)
    assert probs.shape == (3, 8, 12)
    assert np.abs(probs - M.forward_ref(model.weights, x)).max() <= 1e-5


def test_hyperparameter_search_over_32_and_256_units(tmp_path):
    """hyperparameter_search with lstm_units [32, 256] (12 calls): with this seed Hyperband draws both widths, and every trial completes."""
    import pandas as pd

    from orcai_amd.hpsearch import hyperparameter_search

    d = _data12(tmp_path, n_train=16, n_val=8)
    hps = {"filters": {"set1": [10, 20]}, "lstm_units": [32, 256], "dropout_rate": [0.0], "kernel_size": [3], "batch_size": [8]}
    out = tmp_path / "hps_out"
    out.mkdir()
    hyperparameter_search(d, out, _param12(), hps, verbosity=0, max_epochs=3)
    trials = pd.read_csv(out / "hps_logs" / "all_trials.csv")
    assert set(trials["lstm_units"].astype(int)) == {32, 256}
    assert (trials["status"] == "COMPLETED").all() and np.isfinite(trials["score"].astype(float)).all()
    best = json.loads((out / "hps_logs" / "best_hyperparameters.json").read_text())
    assert best["lstm_units"] in (32, 256)


def test_predict_with_a_12_call_init_weights_model(tmp_path):
    """`orcai init-weights` on a 12-call, U = 256 model directory, then `predict` on a short wav: the probability table's columns are the 12
    calls, and every label of the label table is one of them."""
    import pandas as pd
    from click.testing import CliRunner

    from orcai_amd.cli import cli
    from orcai_amd.predict import predict
    from orcai_amd.synthetic import synth_recording
    from orcai_amd.wavio import write_wav_pcm16

    v1 = ROOT / "orcai_amd" / "models" / "orcai-V1"
    param, shape = json.loads((v1 / "orcai_parameter.json").read_text()), json.loads((v1 / "model_shape.json").read_text())
    param["calls"] = list(CALLS12)
    param["model"]["lstm_units"] = 256
    shape["num_labels"] = 12
    mdir = tmp_path / "model"
    mdir.mkdir()
    (mdir / "orcai_parameter.json").write_text(json.dumps(param))
    (mdir / "model_shape.json").write_text(json.dumps(shape))
    res = CliRunner().invoke(cli, ["init-weights", str(mdir), "--seed", "3"], catch_exceptions=False)
    assert res.exit_code == 0, res.output
    wav = tmp_path / "rec.wav"
    write_wav_pcm16(wav, synth_recording(9.0, 48000, seed=5), 48000)
    out = tmp_path / "rec_predicted.txt"
    predict(wav, model_dir=mdir, output_path=out, save_probabilities=True, verbosity=0)
    probs = pd.read_csv(tmp_path / "rec_predicted_probabilities.csv.gz", index_col="time")
    assert list(probs.columns) == CALLS12 and len(probs) > 0 and np.isfinite(probs.to_numpy()).all()
    labels = pd.read_csv(out, sep="\t")
    assert list(labels.columns) == ["start", "stop", "label"]
    assert set(labels["label"].str.rstrip("*")) <= set(CALLS12)
