"""The shared trunk stage of overlapping predict snippets gives the per-snippet path's bits: predict_spectrogram, which
computes blocks 1-2 once per recording row, against forward_device on materialised snippets (stride H*W: the per-snippet path)."""

import pytest
import torch

pytestmark = pytest.mark.gpu

H, W = 736, 171
P = H // 2


def _model(k=3, filters=(30, 40, 50, 60)):
    from orcai_amd.architectures import ResNetLSTM

    return ResNetLSTM((H, W, 1), 7, list(filters), k, 0.0, 128, seed=1)


def _spectrogram(n, extra=0, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.rand(((n + 1) * P + extra, W), generator=g, device="cuda", dtype=torch.float32)


def _per_snippet(model, spec, n, chunk=128):
    """Today's path: the n snippets copied out (stride H*W), so that no row is shared."""
    snippets = torch.stack([spec[i * P : i * P + H] for i in range(n)]).contiguous()
    out = torch.empty((n, model.out_steps, model.num_labels), dtype=torch.float32, device="cuda")
    model.forward_device(snippets.view(-1), H * W, n, out, chunk=chunk)
    return out


@pytest.mark.parametrize("n", [1, 2, 3, 17, 130, 305])
def test_shared_stage_matches_per_snippet_path(n):
    model = _model()
    assert model.shared_geometry(P * W) is not None and model.shared_geometry(H * W) is None
    spec = _spectrogram(n, extra=101, seed=n)
    got = model.predict_spectrogram(spec)
    assert got.shape == (n, model.out_steps, 7)
    assert torch.equal(got, _per_snippet(model, spec, n))


def test_ragged_last_super_snippet_and_two_tail_chunks():
    """305 snippets = 306 strides: 38 super-snippets of 8 strides and a ragged last one; with tail_chunk 128 the recording spans three
    tail chunks, each computing its own first and last stride.  A chunk of 40 snippets changes the launch grouping, not the bits."""
    n = 305
    model = _model()
    spec = _spectrogram(n, seed=7)
    want = _per_snippet(model, spec, n)
    assert torch.equal(model.predict_spectrogram(spec), want)
    model.tail_chunk = 128
    assert torch.equal(model.predict_spectrogram(spec), want)
    model.shared_strides = 3
    assert torch.equal(model.predict_spectrogram(spec, chunk=40), want)


def test_shard_style_range_starting_past_snippet_zero():
    """What predict_spectrogram(shard=True) hands each rank: a contiguous range of snippets starting at i0 > 0, read in place."""
    n, i0 = 61, 23
    model = _model()
    spec = _spectrogram(n, extra=5, seed=3)
    want = _per_snippet(model, spec, n)
    out = torch.empty((n - i0, model.out_steps, 7), dtype=torch.float32, device="cuda")
    model.forward_device(spec.view(-1)[i0 * P * W :], P * W, n - i0, out)
    assert torch.equal(out, want[i0:])


def test_kernel_size_5_shares_with_its_own_cones():
    model = _model(k=5)
    assert model.shared_geometry(P * W).patch_top == 4
    spec = _spectrogram(17, seed=5)
    assert torch.equal(model.predict_spectrogram(spec), _per_snippet(model, spec, 17))


def test_block_2_of_fused_width_takes_the_two_launch_tail():
    """Block-2 filters in 17..32 would run sep_b + pooling as one marching kernel; the shared stage's last block stores through the row
    map, so it takes the two launches, whose bits are the same."""
    model = _model(filters=(24, 32, 40, 48))
    spec = _spectrogram(9, seed=9)
    assert torch.equal(model.predict_spectrogram(spec), _per_snippet(model, spec, 9))


def test_refused_shape_keeps_the_per_snippet_path():
    """H/2 = 370 is not a multiple of 4 (a shared row would sit at two pooling phases): no sharing, the old path's bits."""
    from orcai_amd.architectures import ResNetLSTM

    Hr = 740
    model = ResNetLSTM((Hr, W, 1), 7, [30, 40, 50, 60], 3, 0.0, 128, seed=1)
    assert model.shared_geometry((Hr // 2) * W) is None
    n = 5
    spec = torch.rand(((n + 1) * (Hr // 2), W), device="cuda")
    snippets = torch.stack([spec[i * (Hr // 2) : i * (Hr // 2) + Hr] for i in range(n)]).contiguous()
    want = torch.empty((n, model.out_steps, 7), device="cuda")
    model.forward_device(snippets.view(-1), Hr * W, n, want)
    assert torch.equal(model.predict_spectrogram(spec), want)


def test_scatter_launcher_refuses_before_launching():
    from orcai_amd import _native as N

    lib = N.lib()
    buf = torch.zeros(1 << 16, device="cuda")
    p = N.ptr(buf)
    args = (p, p, 1, 40, 30, 16, 86, 3, p, p, p)
    rowmap = (184, 1, 92, 0, 0, 0, 4, 2, 181)
    assert lib.orcai_pool_res_add_scatter(*args, 0, *rowmap, N.stream_ptr()) == N.E_UNSUPPORTED  # not x-pooled: another kernel
    assert lib.orcai_pool_res_add_scatter(*args, 1, 184, 1, 92, 0, 0, 0, 4, 2, 185, N.stream_ptr()) == -1  # rows past the snippet
    assert lib.orcai_pool_res_add_scatter(*args, 1, 184, 1, 91, 0, 0, 0, 4, 2, 181, N.stream_ptr()) == -1  # not half overlapping
    torch.cuda.synchronize()
    assert int(torch.count_nonzero(buf)) == 0
