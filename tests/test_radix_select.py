"""The radix select's surface without a GPU: the library exports the symbol, orcai::percentile is registered with a fake implementation and an
autograd kernel, and its CPU kernel refuses.  What it computes is tests/test_radix_select_gpu.py's part."""

import pytest

torch = pytest.importorskip("torch")


def test_library_exports_the_radix_select():
    from orcai_amd import _native as N

    assert "orcai_quantile_select_radix" in N.exported_symbols()
    assert N._SIGNATURES["orcai_quantile_select_radix"] == N._SIGNATURES["orcai_quantile_select"]
    assert N.lib().orcai_quantile_select_radix is not None
    # refused before anything is launched, so no device is needed: null x, null workspace, n out of range
    assert N.lib().orcai_quantile_select_radix(None, 10, 0, 9, None, None) == N.E_BADARG
    assert N.lib().orcai_quantile_select_radix(16, 2**32, 0, 9, 16, None) == N.E_BADARG
    assert N.lib().orcai_quantile_select_radix(16, 0, 0, 0, 16, None) == N.E_BADARG


def test_percentile_op_shape_on_fake_tensors_and_cpu_refusal():
    import orcai_amd.torch_ops as O
    from torch._subclasses.fake_tensor import FakeTensorMode

    assert "orcai.percentile" in O.__doc__
    with FakeTensorMode():
        x = torch.empty((7, 9, 2))
        out = torch.ops.orcai.percentile(x, [0.0, 0.5, 1.0])
        assert tuple(out.shape) == (3,) and out.dtype == torch.float32 and out.device == x.device
        assert tuple(torch.ops.orcai.percentile(x.double(), [0.25]).shape) == (1,) and torch.ops.orcai.percentile(x.double(), [0.25]).dtype == torch.float32
    with pytest.raises(TypeError, match="CUDA"):
        torch.ops.orcai.percentile(torch.zeros(8), [0.5])
    schema = str(torch.ops.orcai.percentile.default._schema)
    assert "Tensor x" in schema and "float[] q" in schema
