"""ParamLayout and PreparePlan on the host: the layout against a loop over variable_spec() written out here, and the descriptor tables of
prepare_device and of EvalGrad's backward operands against the tables recorded before the two were built by one helper
(tests/golden/prepare_plans.json: lists of integers)."""

import json
from pathlib import Path

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from orcai_amd.architectures import ResNet1DConv, ResNetLSTM  # noqa: E402

GOLDEN = json.loads((Path(__file__).parent / "golden" / "prepare_plans.json").read_text())
MODELS = {"ResNetLSTM": lambda seed=1: ResNetLSTM((64, 40, 1), 4, [12, 20], 5, lstm_units=64, seed=seed),
          "ResNet1DConv": lambda seed=1: ResNet1DConv((48, 21, 1), 5, [12, 30], 3, seed=seed)}


@pytest.fixture(params=list(MODELS))
def model(request):
    return MODELS[request.param]()


def test_layout_follows_variable_spec(model):
    lay = model.layout()
    assert lay is model.layout()  # built once
    want = {True: {}, False: {}}
    off = {True: 0, False: 0}
    for name, shape, _, trainable in model.variable_spec():
        n = 1
        for d in shape:
            n *= int(d)
        want[trainable][name] = (off[trainable], n, tuple(shape))
        off[trainable] += n
    assert lay.w == want[True] and lay.s == want[False]
    assert lay.w_names == list(want[True]) and lay.s_names == list(want[False])  # spec order
    assert (lay.n_w, lay.n_s) == (off[True], off[False])
    assert lay.n_w + lay.n_s == model.count_params()


def test_flatten_and_split_round_trip(model):
    lay = model.layout()
    wflat, sflat = lay.flatten(model.weights, "cpu")
    for flat, n in ((wflat, lay.n_w), (sflat, lay.n_s)):
        assert flat.dtype == torch.float32 and flat.is_contiguous() and tuple(flat.shape) == (n,)
    spec = model.variable_spec()
    for flat, trainable in ((wflat, True), (sflat, False)):
        want = np.concatenate([model.weights[n].reshape(-1) for n, _, _, t in spec if t == trainable])
        assert np.array_equal(flat.numpy().view(np.int32), want.view(np.int32))
    parts = lay.split_w(wflat)
    assert len(parts) == len(lay.w_names)
    for name, part in zip(lay.w_names, parts):
        assert tuple(part.shape) == model.weights[name].shape
        assert np.array_equal(part.numpy().view(np.int32), model.weights[name].view(np.int32)), name
    tensors = {n: torch.from_numpy(a) for n, a in model.weights.items()}  # the ops pass tensors
    assert all(torch.equal(a, b) for a, b in zip(lay.flatten(tensors, "cpu"), (wflat, sflat)))


def _views(plan):
    return {key: [off, *shape] for key, (off, shape) in plan.views.items()}


def test_descriptor_tables_are_the_recorded_ones(model):
    from orcai_amd.eval_grad import EvalGrad

    want = GOLDEN[model.architecture]
    plan = model._device_plan()
    assert plan is model._device_plan()
    assert plan.desc == want["desc"] and plan.lstm == want["lstm"] and plan.size == want["size"]
    assert _views(plan) == want["views"] and list(plan.views) == list(want["views"])
    assert all(off % 64 == 0 for off, _ in plan.views.values())  # 256-byte aligned
    extra = EvalGrad(model)._extra_plan()
    assert extra.desc == want["extra_desc"] and extra.lstm == [] and extra.size == want["extra_size"]
    assert _views(extra) == want["extra_views"]


def test_set_weights_dict_bumps_the_version(model):
    before = model.weights_version
    model.set_weights_dict(MODELS[model.architecture](seed=2).weights)
    assert model.weights_version > before


def test_bound_restores_the_previous_binding(model):
    own, other = {"own": 1}, {"other": 2}
    model._dev = own
    with model.bound(other):
        assert model._dev is other
    assert model._dev is own
    with pytest.raises(KeyError):
        with model.bound(other):
            raise KeyError("inside")
    assert model._dev is own


def test_plane_shape_is_what_its_consumers_lay_out(model):
    """Against shapes written out for these two models by hand from "Padded plane layout" (csrc/model_fwd.hip): [ceil(c/4)][h + 2R][roundup4(w + R)][4], and
    against the first item of EvalGrad's saved layout (the entry activation: 16 channels at the input size)."""
    from orcai_amd.eval_grad import saved_layout

    want = {"ResNetLSTM": (4, 64 + 4, 44, 4), "ResNet1DConv": (4, 48 + 2, 24, 4)}[model.architecture]  # k 5: R 2, 40 + 2 -> 44; k 3: R 1, 21 + 1 -> 24
    H, W = model.input_hw
    assert model.plane_shape(16, H, W) == want
    assert saved_layout(model)[0][0] == ("y0", 0, want)
    assert model.plane_shape(13, 7, 9)[0] == 4 and model.plane_shape(17, 7, 9)[0] == 5
