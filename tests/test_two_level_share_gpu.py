"""The two-level shared trunk of overlapping predict snippets gives the per-snippet path's bits: predict_spectrogram, which
computes blocks 1-4 once per recording row, against forward_device on materialised snippets (stride H*W: the per-snippet path)."""

import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

H, W = 736, 171
P = H // 2


def _model(k=3, filters=(30, 40, 50, 60), height=H):
    from orcai_amd.architectures import ResNetLSTM

    return ResNetLSTM((height, W, 1), 7, list(filters), k, 0.0, 128, seed=1)


def _spectrogram(n, extra=0, seed=0, height=H):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.rand(((n + 1) * (height // 2) + extra, W), generator=g, device="cuda", dtype=torch.float32)


def _per_snippet(model, spec, n, height=H):
    p = height // 2
    snippets = torch.stack([spec[i * p : i * p + height] for i in range(n)]).contiguous()
    out = torch.empty((n, model.out_steps, model.num_labels), dtype=torch.float32, device="cuda")
    model.forward_device(snippets.view(-1), height * W, n, out, chunk=128)
    return out


@pytest.mark.parametrize("n", [1, 2, 3, 17, 130, 305])
def test_two_levels_match_per_snippet_path(n):
    model = _model()
    assert model.tail_geometry(P * W) is not None and model.tail_geometry(H * W) is None
    spec = _spectrogram(n, extra=101, seed=n)
    got = model.predict_spectrogram(spec)
    assert got.shape == (n, model.out_steps, 7)
    assert torch.equal(got, _per_snippet(model, spec, n))


def test_ragged_last_super_image_and_three_tail_chunks():
    """305 snippets: ragged last super-images at both levels; tail_chunk 128 gives three tail chunks (128, 128, 49 snippets), each
    with its own two-level plan; 3 strides per super-image and a chunk of 40 change the launch grouping, not the bits."""
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
    n, i0 = 61, 23
    model = _model()
    spec = _spectrogram(n, extra=5, seed=3)
    want = _per_snippet(model, spec, n)
    out = torch.empty((n - i0, model.out_steps, 7), dtype=torch.float32, device="cuda")
    model.forward_device(spec.view(-1)[i0 * P * W :], P * W, n - i0, out)
    assert torch.equal(out, want[i0:])


def test_kernel_size_5_takes_the_cumulative_cones():
    model = _model(k=5)
    geo2 = model.tail_geometry(P * W)
    assert (geo2.patch_top, geo2.patch_bottom, geo2.crop) == (4, 5, 36)
    spec = _spectrogram(17, seed=5)
    assert torch.equal(model.predict_spectrogram(spec), _per_snippet(model, spec, 17))


def test_block_widths_24_to_48():
    model = _model(filters=(24, 32, 40, 48))
    assert model.tail_geometry(P * W) is not None
    spec = _spectrogram(9, seed=9)
    assert torch.equal(model.predict_spectrogram(spec), _per_snippet(model, spec, 9))


def test_layout_level_2_refuses_falls_back_to_one_level():
    """H/2 = 372: a multiple of 4 (blocks 1-2 shared) but not of 16 -- blocks 3-4 per snippet, the old bits."""
    Hr = 744
    model = _model(height=Hr)
    assert model.shared_geometry((Hr // 2) * W) is not None and model.tail_geometry((Hr // 2) * W) is None
    spec = _spectrogram(5, seed=11, height=Hr)
    assert torch.equal(model.predict_spectrogram(spec), _per_snippet(model, spec, 5, height=Hr))


def test_families_launcher_refuses_before_launching():
    from orcai_amd import _native as N

    lib = N.lib()
    buf = torch.zeros(1 << 16, device="cuda")
    p = N.ptr(buf)
    args = (p, p, 1, 40, 30, 16, 86, 3, p, p)

    def fams(*rows):
        return (N.RowFamily * len(rows))(*[N.RowFamily(p, *r) for r in rows])

    def call(xpooled, families, nfam=None):
        return lib.orcai_pool_res_add_scatter_families(*args, xpooled, 0, 1, 0, 8, ctypes.addressof(families), len(families) if nfam is None else nfam,
                                                       N.stream_ptr())

    ok = (20, 92, 0, 4, 0, 20)  # Hd, period, offset, count, keep_lo, keep_hi
    assert call(0, fams(ok)) == N.E_UNSUPPORTED  # not x-pooled: another kernel
    assert call(1, fams(ok, ok, ok, ok, ok)) == N.E_UNSUPPORTED  # more families than the kernel takes
    assert call(1, fams((760, 368, 0, 4, 0, 760))) == N.E_UNSUPPORTED  # a row in three images: past the kernel's destination loop
    assert call(1, fams((20, 92, 0, 4, 0, 21))) == -1  # kept rows past the image
    assert call(1, fams((20, 0, 0, 4, 0, 20))) == -1
    assert call(1, fams((20, 92, 0, 0, 0, 20))) == -1
    assert call(1, fams(ok), nfam=0) == -1
    torch.cuda.synchronize()
    assert int(torch.count_nonzero(buf)) == 0
