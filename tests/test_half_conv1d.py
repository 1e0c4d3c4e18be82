"""CPU side of ResNet1DConv on the f16 path: the architecture accepts the precision, build_model passes it through, anything else is refused."""

import pytest


def test_resnet_1dconv_constructs_in_f16():
    from orcai_amd.architectures import ResNet1DConv

    model = ResNet1DConv((32, 12, 1), 3, [10, 20], 3, 0.3, precision="f16")
    assert model.precision == "f16" and model.architecture == "ResNet1DConv"
    assert ResNet1DConv((32, 12, 1), 3, [10, 20], 3, 0.3).precision == "f32"
    names = {n for n, *_ in model.variable_spec()}
    assert "conv1d/kernel" in names and not any(n.startswith(("lstm", "dense")) for n in names)


def test_build_model_returns_an_f16_resnet_1dconv():
    from orcai_amd.architectures import build_model

    p = {"name": "m", "architecture": "ResNet1DConv", "calls": ["A", "B", "C"],
         "model": {"filters": [10, 20], "kernel_size": 3, "dropout_rate": 0.5, "precision": "f16"}}
    model = build_model((32, 12, 1), p)
    assert model.architecture == "ResNet1DConv" and model.precision == "f16" and model.output_shape == (None, 8, 3)


def test_resnet_1dconv_refuses_other_precisions():
    from orcai_amd.architectures import ResNet1DConv

    with pytest.raises(ValueError, match="precision"):
        ResNet1DConv((32, 12, 1), 3, [10, 20], 3, 0.3, precision="bf16")
