"""The orcai torch custom ops on the GPU against the package's own paths: orcai_sigmoid_bwd against aten::sigmoid_backward, the device-side
inference preparation against ResNetLSTM.prepare(), the eval forward / predict against forward_device / predict_spectrogram (all bit for
bit), the training forward against Trainer.forward_backward + apply (bit for bit), the weight gradients from a torch-written loss against
the trainer's fused loss (1e-5 of each tensor's max-abs), opcheck, a torch.optim loop against the Trainer, torch.compile, misuse."""

import math

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from oracle import model_ref as M  # noqa: E402

SMALL = [
    ("lstm_k3", dict(input_shape=(32, 12, 1), filters=(10, 20), kernel_size=3, lstm_units=64, num_labels=3), 3),
    ("lstm_k5", dict(input_shape=(32, 16, 1), filters=(10, 20), kernel_size=5, lstm_units=64, num_labels=2), 2),
    ("lstm_k7", dict(input_shape=(48, 21, 1), filters=(12, 30, 40), kernel_size=7, lstm_units=32, num_labels=7), 2),
    ("conv1d_k3", dict(input_shape=(48, 21, 1), filters=(12, 30, 40), kernel_size=3, num_labels=5), 2),
]


def make(cfg, seed=5, rate=0.0):
    """A model with calibrated weights and non-trivial BatchNorm moving statistics and affine parameters."""
    from orcai_amd.architectures import FINAL_FILTERS, ResNet1DConv, ResNetLSTM

    conv1d = "lstm_units" not in cfg
    p = M.calibrated_params(seed=seed, input_shape=cfg["input_shape"], num_labels=cfg["num_labels"], filters=cfg["filters"], kernel_size=cfg["kernel_size"],
                            lstm_units=cfg.get("lstm_units", 64))
    rng = np.random.default_rng(seed)
    if conv1d:
        p = {k: v for k, v in p.items() if not k.startswith(("lstm", "dense", "bn_d"))}
        lim = np.sqrt(6.0 / (FINAL_FILTERS * FINAL_FILTERS + FINAL_FILTERS * cfg["num_labels"]))
        p["conv1d/kernel"] = rng.uniform(-lim, lim, (FINAL_FILTERS, FINAL_FILTERS, cfg["num_labels"])).astype(np.float32)
        p["conv1d/bias"] = (0.1 * rng.standard_normal(cfg["num_labels"])).astype(np.float32)
        model = ResNet1DConv(cfg["input_shape"], cfg["num_labels"], list(cfg["filters"]), cfg["kernel_size"], rate)
    else:
        model = ResNetLSTM(cfg["input_shape"], cfg["num_labels"], list(cfg["filters"]), cfg["kernel_size"], rate, cfg["lstm_units"])
    for k in p:
        if k.endswith(("gamma", "beta", "/mean", "/bias")):
            p[k] = (p[k] + 0.2 * rng.standard_normal(p[k].shape)).astype(np.float32)
        elif k.endswith("/var"):
            p[k] = (p[k] * rng.uniform(0.5, 2.0, p[k].shape)).astype(np.float32)
    model.set_weights_dict(p)
    return model


def flat(model):
    spec = model.variable_spec()
    w = torch.cat([torch.from_numpy(model.weights[n]).reshape(-1) for n, _, _, t in spec if t]).cuda()
    s = torch.cat([torch.from_numpy(model.weights[n]).reshape(-1) for n, _, _, t in spec if not t]).cuda()
    return w, s


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def test_sigmoid_bwd_equals_aten_bit_for_bit():
    from orcai_amd import _native as N

    g = torch.Generator(device="cuda").manual_seed(3)
    for n, off in ((1, 0), (7, 0), (4099, 1), (100003, 0), (100003, 3)):
        p = torch.sigmoid(4 * torch.randn(n + off, device="cuda", generator=g))[off:]
        up = torch.randn(n + off, device="cuda", generator=g)[off:] * 3
        dz = torch.empty(n + off, device="cuda")[off:]
        N.check(N.lib().orcai_sigmoid_bwd(p.data_ptr(), up.data_ptr(), n, dz.data_ptr(), N.stream_ptr()), "sigmoid_bwd")
        assert same_bits(dz, torch.ops.aten.sigmoid_backward(up, p)), (n, off)


@pytest.mark.parametrize("name,cfg,B", SMALL, ids=[s[0] for s in SMALL])
def test_device_preparation_equals_prepare(name, cfg, B):
    model = make(cfg)
    ref = model.prepare()
    got = model.prepare_device(*flat(model))
    assert sorted(got) == sorted(ref)
    for k in ref:
        assert same_bits(got[k], ref[k]), k
        assert got[k].data_ptr() % 256 == 0, k


def test_device_preparation_of_orcai_v1():
    model = make(dict(input_shape=(736, 171, 1), filters=(30, 40, 50, 60), kernel_size=3, lstm_units=128, num_labels=7))
    ref, got = model.prepare(), model.prepare_device(*flat(model))
    assert sorted(got) == sorted(ref) and all(same_bits(got[k], ref[k]) for k in ref)


@pytest.mark.parametrize("name,cfg,B", SMALL, ids=[s[0] for s in SMALL])
def test_eval_forward_equals_forward_device(name, cfg, B):
    from orcai_amd.torch_ops import OrcaiModule

    model = make(cfg)
    m = OrcaiModule(model).cuda().eval()
    H, W = model.input_hw
    x = torch.rand((B + 3, H, W), device="cuda")
    out = torch.empty((B + 3, model.out_steps, model.num_labels), device="cuda")
    model.forward_device(x.view(-1), H * W, B + 3, out)
    with torch.no_grad():
        assert same_bits(m(x), out)
    assert same_bits(m(x).detach(), out)  # with grad enabled (eval mode: no graph kept for a backward)


def test_predict_spectrogram_equals_model_orcai_v1():
    from orcai_amd.torch_ops import OrcaiModule

    model = make(dict(input_shape=(736, 171, 1), filters=(30, 40, 50, 60), kernel_size=3, lstm_units=128, num_labels=7), seed=2)
    m = OrcaiModule(model).cuda()
    spec = torch.rand((11250, 171), device="cuda")  # 60 s at 48 kHz, hop 256
    ref = model.predict_spectrogram(spec)
    with torch.no_grad():
        got = m.predict_spectrogram(spec)
    assert got.shape == (29, 46, 7) and same_bits(got, ref)
    x = spec[:736].clone().view(1, 736, 171)
    out = torch.empty((1, 46, 7), device="cuda")
    model.forward_device(x.view(-1), 736 * 171, 1, out)
    with torch.no_grad():
        assert same_bits(m.eval()(x), out)


def _trainer_step(model, x, y, seed):
    from orcai_amd.training import Trainer

    tr = Trainer(model, learning_rate=1e-3, seed=seed)
    H, W = model.input_hw
    out = tr.forward_backward(x.reshape(-1), H * W, x.shape[0], y)
    tr.apply()
    return tr, out


def _labels(model, B, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    y = (torch.rand((B, model.out_steps, model.num_labels), device="cuda", generator=g) > 0.5).float()
    y[0, :, 0] = -1.0
    return y


TRAIN = [SMALL[0], SMALL[1], SMALL[3]]


@pytest.mark.parametrize("rate", [0.0, 0.5])
@pytest.mark.parametrize("name,cfg,B", TRAIN, ids=[s[0] for s in TRAIN])
def test_training_forward_equals_trainer(name, cfg, B, rate):
    from orcai_amd.torch_ops import OrcaiModule, model_config

    model = make(cfg, rate=rate)
    m = OrcaiModule(model).cuda()
    H, W = model.input_hw
    x = torch.rand((B, H, W), device="cuda")
    tr, ref = _trainer_step(make(cfg, rate=rate), x, _labels(model, B, 1), seed=11)
    st = m.stats_list()
    with torch.no_grad():
        probs = torch.ops.orcai.forward(x, m.weights_list(), st, model_config(model), True, 11)
    assert same_bits(probs, ref["probs"])
    names = [n for n, _, _, t in model.variable_spec() if not t]
    for n, s in zip(names, st):
        assert same_bits(s, tr.P.stats[n].view(s.shape)), n


def _torch_loss(model, m, probs, y):
    """Masked BCE (Keras clipping, mean over the unmasked labels) + for ResNetLSTM the L2 penalty of architectures.py, written in torch."""
    q = probs.clamp(1e-7, 1.0 - 1e-7)
    mask = (y != -1.0).float()
    bce = -(y * torch.log(q) + (1.0 - y) * torch.log(1.0 - q))
    loss = (bce * mask).sum() / mask.sum()
    if model.architecture == "ResNetLSTM":
        for n in ["dense1/kernel"] + [f"lstm{i}/{d}/kernel" for i in (1, 2) for d in ("fwd", "bwd")]:
            loss = loss + 1e-3 * (m.get_parameter(n.replace("/", "__")) ** 2).sum()
    return loss


@pytest.mark.parametrize("rate", [0.0, 0.5])
@pytest.mark.parametrize("name,cfg,B", TRAIN, ids=[s[0] for s in TRAIN])
def test_gradients_match_the_trainer(name, cfg, B, rate):
    from orcai_amd.torch_ops import OrcaiModule, model_config

    model = make(cfg, rate=rate)
    m = OrcaiModule(model).cuda()
    H, W = model.input_hw
    x = torch.rand((B, H, W), device="cuda")
    y = _labels(model, B, 2)
    tr, _ = _trainer_step(make(cfg, rate=rate), x, y, seed=7)
    probs = torch.ops.orcai.forward(x, m.weights_list(), m.stats_list(), model_config(model), True, 7)
    _torch_loss(model, m, probs, y).backward()
    worst = 0.0
    for n, p in m.named_parameters():
        ref = tr.P.G(n.replace("__", "/"))
        scale = float(ref.abs().max())
        err = float((p.grad - ref).abs().max())
        if scale == 0.0:
            assert err == 0.0, n
            continue
        worst = max(worst, err / scale)
        assert err <= 1e-5 * scale, (n, err, scale)
    print(f"{name} rate {rate}: worst max|dgrad| / max|grad| = {worst:.2e}")


def test_opcheck():
    from torch.library import opcheck

    from orcai_amd.torch_ops import OrcaiModule, model_config

    name, cfg, B = SMALL[0]
    model = make(cfg)
    m = OrcaiModule(model).cuda()
    H, W = model.input_hw
    c = model_config(model)
    x = torch.rand((B, H, W), device="cuda")
    ws = [w.detach().clone() for w in m.weights_list()]
    opcheck(torch.ops.orcai.forward.default, (x, ws, [s.clone() for s in m.stats_list()], c, False, 0))
    # training mode: the schema and fake-tensor checks keep the results of two real calls alive at once, which with weights that require
    # grad is the misuse the op refuses (test_misuse_raises); they run on weights without grad, the autograd check on weights with
    wg = [w.detach().clone().requires_grad_() for w in m.weights_list()]
    opcheck(torch.ops.orcai.forward.default, (x, wg, [s.clone() for s in m.stats_list()], c, True, 3), test_utils=("test_autograd_registration",))
    opcheck(torch.ops.orcai.forward.default, (x, ws, [s.clone() for s in m.stats_list()], c, True, 3), test_utils=("test_schema", "test_faketensor"))
    spec = torch.rand((H * 3 + 5, W), device="cuda")
    opcheck(torch.ops.orcai.predict_spectrogram.default, (spec, ws, [s.clone() for s in m.stats_list()], c))
    pcm = torch.randn(48000, device="cuda") * 0.1
    opcheck(torch.ops.orcai.spectrogram.default, (pcm, 48000, 512, 256, 16000.0, 0.01, 0.999))


def test_adam_loop_follows_the_trainer():
    from orcai_amd.torch_ops import OrcaiModule
    from orcai_amd.training import Trainer

    name, cfg, B = SMALL[0]
    model = make(cfg)
    m = OrcaiModule(model).cuda().train()
    tr = Trainer(make(cfg), learning_rate=1e-3, seed=0)
    opt = torch.optim.Adam(m.parameters(), lr=1e-3, eps=1e-7)
    # the trainer's Adam is Keras': w -= lr sqrt(1 - b2^t) / (1 - b1^t) * m / (sqrt(v) + eps), epsilon BEFORE the bias correction; torch.optim.Adam
    # adds it after.  A second module follows the Keras rule written in torch, to separate the update rule from the gradients.
    mk = OrcaiModule(make(cfg)).cuda().train()
    mom = [(torch.zeros_like(p), torch.zeros_like(p)) for p in mk.parameters()]
    H, W = model.input_hw
    g = torch.Generator(device="cuda").manual_seed(9)
    ours, keras, theirs = [], [], []
    for step in range(20):
        x = torch.rand((B, H, W), device="cuda", generator=g)
        y = _labels(model, B, 100 + step)
        acc = tr.forward_backward(x.reshape(-1), H * W, B, y)["acc"]
        tr.apply()
        theirs.append(float(acc[0] / acc[1] + acc[3]))
        opt.zero_grad()
        loss = _torch_loss(model, m, m(x), y)
        loss.backward()
        opt.step()
        ours.append(float(loss.detach()))
        mk.zero_grad()
        loss = _torch_loss(model, mk, mk(x), y)
        loss.backward()
        keras.append(float(loss.detach()))
        with torch.no_grad():
            alpha = 1e-3 * math.sqrt(1.0 - 0.999 ** (step + 1)) / (1.0 - 0.9 ** (step + 1))
            for p, (m1, v1) in zip(mk.parameters(), mom):
                m1.add_((p.grad - m1) * (1.0 - 0.9))
                v1.add_((p.grad * p.grad - v1) * (1.0 - 0.999))
                p.sub_(alpha * m1 / (v1.sqrt() + 1e-7))
    rel = max(abs(a - b) / abs(b) for a, b in zip(ours, theirs))
    rel_k = max(abs(a - b) / abs(b) for a, b in zip(keras, theirs))
    print(f"20 Adam steps: loss {theirs[0]:.5f} -> {theirs[-1]:.5f}; max relative loss difference: torch.optim.Adam {rel:.2e}, the Keras rule in torch {rel_k:.2e}")
    assert rel_k <= 1e-4, (keras, theirs)
    assert rel <= 3e-2, (ours, theirs)


def test_compiled_front_end_and_predict_equal_eager():
    from orcai_amd.architectures import ResNetLSTM
    from orcai_amd.torch_ops import OrcaiModule

    model = ResNetLSTM((64, 171, 1), 3, [12, 20], 3, 0.0, 32, seed=4)
    m = OrcaiModule(model).cuda().eval()
    ws, st = m.weights_list(), m.stats_list()

    def f(pcm):
        spec = torch.ops.orcai.spectrogram(pcm, 48000, 512, 256, 16000.0, 0.01, 0.999)
        return torch.ops.orcai.predict_spectrogram(spec, ws, st, m.config)

    pcm = torch.randn(48000 * 3, device="cuda") * 0.1
    with torch.no_grad():
        eager = f(pcm)
        compiled = torch.compile(f, backend="aot_eager", fullgraph=True)(pcm)
    assert eager.shape[0] == (1 + 48000 * 3 // 256 - 64) // 32 + 1
    assert same_bits(compiled, eager)


def test_misuse_raises():
    from orcai_amd.torch_ops import OrcaiModule

    name, cfg, B = SMALL[0]
    model = make(cfg)
    m = OrcaiModule(model).cuda().train()
    H, W = model.input_hw
    x = torch.rand((B, H, W), device="cuda")
    first = m(x)
    with pytest.raises(RuntimeError, match="not been backpropagated"):
        m(x)
    first.sum().backward()  # the first step is still intact and closes here
    assert all(p.grad is not None for p in m.parameters())
    with pytest.raises(NotImplementedError, match="no gradient w.r.t. its input"):
        m(x.clone().requires_grad_())
    m(x).sum().backward()
    out = m.eval()(x)
    with pytest.raises(RuntimeError, match="training=False"):
        out.sum().backward()
    with torch.no_grad():  # no graph: the step closes at the next forward
        m.train()(x)
    m(x).sum().backward()
    assert math.isfinite(float(m.get_parameter("dense2__bias").grad.abs().sum()))
