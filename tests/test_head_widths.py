"""CPU side of LSTM widths 32..256 and up to 64 labels: the supported set named in the errors, the variable shapes and the Keras layout."""

import json
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]


@pytest.mark.parametrize("units", [48, 288, 16])
def test_unsupported_lstm_width_names_the_supported_set(units):
    from orcai_amd.architectures import ResNetLSTM

    with pytest.raises(NotImplementedError, match=r"multiple of 32 in \[32, 256\]"):
        ResNetLSTM((32, 12, 1), 7, [8, 12], 3, 0.0, units)


@pytest.mark.parametrize("labels", [65, 0])
def test_unsupported_label_count_names_the_supported_set(labels):
    from orcai_amd.architectures import ResNet1DConv, ResNetLSTM

    for build in (lambda: ResNetLSTM((32, 12, 1), labels, [8, 12], 3, 0.0, 64), lambda: ResNet1DConv((32, 12, 1), labels, [8, 12], 3, 0.0)):
        with pytest.raises(NotImplementedError, match="1 to 64 labels"):
            build()


@pytest.mark.parametrize("units,labels", [(32, 64), (96, 9), (160, 12), (256, 12), (256, 64)])
def test_wide_head_variable_shapes(units, labels):
    from oracle import model_ref as M
    from orcai_amd.architectures import ResNetLSTM

    model = ResNetLSTM((32, 12, 1), labels, [8, 12], 3, 0.0, units, seed=1)
    spec = {n: tuple(s) for n, s, *_ in model.variable_spec()}
    assert spec["lstm1/fwd/recurrent"] == (units, 4 * units) and spec["lstm2/bwd/kernel"] == (2 * units, 4 * units)
    assert spec["dense1/kernel"] == (2 * units, 128) and spec["dense2/kernel"] == (128, labels)
    assert model.output_shape == (None, 8, labels)
    ref = {n: tuple(s) for n, s, *_ in M.param_spec(input_shape=(32, 12, 1), num_labels=labels, filters=(8, 12), kernel_size=3, lstm_units=units)}
    assert {n: spec[n] for n in ref} == ref


def test_keras_layout_at_256_units_and_12_labels(tmp_path):
    """tools/keras_to_npz.py --layout on a 12-call, U = 256 model directory: every variable listed with its shape."""
    v1 = ROOT / "orcai_amd" / "models" / "orcai-V1"
    param = json.loads((v1 / "orcai_parameter.json").read_text())
    shape = json.loads((v1 / "model_shape.json").read_text())
    param["calls"] = [f"C{i}" for i in range(12)]
    param["model"]["lstm_units"] = 256
    shape["num_labels"] = 12
    (tmp_path / "orcai_parameter.json").write_text(json.dumps(param))
    (tmp_path / "model_shape.json").write_text(json.dumps(shape))
    out = subprocess.run([sys.executable, str(ROOT / "tools" / "keras_to_npz.py"), "--layout", str(tmp_path)], capture_output=True, text=True, cwd=ROOT, check=True).stdout
    rows = {line.split("->")[-1].strip(): line for line in out.splitlines() if "->" in line and "/" in line.split("->")[-1]}
    assert "(256, 1024)" in rows["lstm1/fwd/recurrent"] and "(512, 1024)" in rows["lstm2/fwd/kernel"]
    assert "(128, 12)" in rows["dense2/kernel"] and "(12,)" in rows["dense2/bias"]
