"""GPU parity of the HIP ResNetLSTM forward (through the C ABI) against the CPU oracle
(oracle/model_ref.py, torch-CPU restatement of the Keras layers; parity unpinned at the Keras boundary).

Tolerance: float32 throughout on both sides, different accumulation order:
  |delta| <= 2e-5 * max(1, max|ref|) per intermediate tensor, |delta p| <= 1e-5 on the output probabilities
  (BASELINE north_star: "within a stated fp32 tolerance"; SURVEY 8d states 1e-4 for the output).
"""

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from oracle import model_ref as M  # noqa: E402


def make_model(seed, input_shape=(736, 171, 1), filters=(30, 40, 50, 60), kernel_size=3, lstm_units=128, num_labels=7):
    from orcai_amd.architectures import ResNetLSTM

    p = M.calibrated_params(seed=seed, input_shape=input_shape, num_labels=num_labels, filters=filters, kernel_size=kernel_size, lstm_units=lstm_units)
    model = ResNetLSTM(input_shape, num_labels, list(filters), kernel_size, 0.0, lstm_units)
    model.set_weights_dict(p)
    return model, p


def close(a, b, rel=2e-5):
    scale = max(1.0, float(np.abs(b).max()))
    err = float(np.abs(a - b).max())
    assert err <= rel * scale, (err, scale)
    return err


def test_param_count_matches_reference_architecture():
    model, p = make_model(1)
    assert model.count_params() == 996039
    assert sum(int(w.size) for w in model.trainable_weights) == 994959
    assert sum(int(w.size) for w in model.non_trainable_weights) == 1080
    assert model.output_shape == (None, 46, 7) and model.input_shape == (None, 736, 171, 1)


def test_forward_intermediates_orcai_v1():
    model, p = make_model(3)
    rng = np.random.default_rng(0)
    x = rng.random((3, 736, 171, 1), dtype=np.float32)
    ref, inter = M.forward_ref(p, x, return_intermediates=True)
    xd = torch.from_numpy(x[..., 0].copy()).cuda()
    out = torch.empty((3, 46, 7), dtype=torch.float32, device="cuda")
    keep = {}
    model.forward_device(xd.view(-1), 736 * 171, 3, out, keep=keep)
    got = {k: v.cpu().numpy() for k, v in keep.items()}
    close(got["prev0"], inter["conv0"])
    for b in range(1, 5):
        close(got[f"a{b}"], inter[f"b{b}/a"])
        bref = inter[f"b{b}/b"]  # the kernel stores max over column pairs (2j, 2j+1), the first half of the (3,2) max-pool
        wx = (bref.shape[3] + 1) // 2
        pairs = np.full(bref.shape[:3] + (2 * wx,), -np.inf, dtype=np.float32)
        pairs[..., : bref.shape[3]] = bref
        close(got[f"b{b}"], pairs.reshape(bref.shape[:3] + (wx, 2)).max(axis=4))
        close(got[f"prev{b}"], inter[f"b{b}"])
    close(got["feat"], inter["features"])
    close(got["h1"], inter["lstm1"])
    close(got["h2"], inter["lstm2"])
    for name in ("prev0", "a1", "prev1", "a2", "prev4"):  # pad rows/columns/channels of the layout stay zero
        assert not got[name + "/pads"].any(), name
    o = out.cpu().numpy()
    assert np.abs(o - ref).max() <= 1e-5, np.abs(o - ref).max()
    ref64 = M.forward_ref(p, x, dtype=torch.float64)
    assert np.abs(o - ref64).max() <= 1e-5


@pytest.mark.parametrize("kernel_size", [5, 7])
def test_forward_intermediates_wide_kernels(kernel_size):
    """test_forward_intermediates_orcai_v1 for kernel sizes 5 and 7 at the sweep's width (171 columns: several 64-pixel windows per row of the
    flat padded planes, row pitch 176): every intermediate of the inference trunk, the pads, and the probabilities at the same bars."""
    H, W, B = 32, 171, 3
    model, p = make_model(3, input_shape=(H, W, 1), filters=(30, 40), kernel_size=kernel_size, lstm_units=64, num_labels=7)
    rng = np.random.default_rng(0)
    x = rng.random((B, H, W, 1), dtype=np.float32)
    ref, inter = M.forward_ref(p, x, return_intermediates=True)
    xd = torch.from_numpy(x[..., 0].copy()).cuda()
    out = torch.empty((B, H // 4, 7), dtype=torch.float32, device="cuda")
    keep = {}
    model.forward_device(xd.view(-1), H * W, B, out, keep=keep)
    got = {k: v.cpu().numpy() for k, v in keep.items()}
    close(got["prev0"], inter["conv0"])
    for b in range(1, 3):
        close(got[f"a{b}"], inter[f"b{b}/a"])
        bref = inter[f"b{b}/b"]  # the kernel stores max over column pairs (2j, 2j+1), the first half of the (3,2) max-pool
        wx = (bref.shape[3] + 1) // 2
        pairs = np.full(bref.shape[:3] + (2 * wx,), -np.inf, dtype=np.float32)
        pairs[..., : bref.shape[3]] = bref
        close(got[f"b{b}"], pairs.reshape(bref.shape[:3] + (wx, 2)).max(axis=4))
        close(got[f"prev{b}"], inter[f"b{b}"])
    close(got["feat"], inter["features"])
    close(got["h1"], inter["lstm1"])
    close(got["h2"], inter["lstm2"])
    for name in ("prev0", "a1", "prev1", "a2", "prev2"):  # pad rows/columns/channels of the layout stay zero
        assert not got[name + "/pads"].any(), name
    o = out.cpu().numpy()
    assert np.abs(o - ref).max() <= 1e-5, np.abs(o - ref).max()
    ref64 = M.forward_ref(p, x, dtype=torch.float64)
    assert np.abs(o - ref64).max() <= 1e-5


def test_predict_api_and_chunking():
    model, p = make_model(4)
    rng = np.random.default_rng(1)
    x = rng.random((5, 736, 171, 1), dtype=np.float32)
    ref = M.forward_ref(p, x)
    out = model.predict(x, batch_size=2, verbose=0)
    assert out.shape == (5, 46, 7) and out.dtype == np.float32
    assert np.abs(out - ref).max() <= 1e-5
    with pytest.raises(ValueError):
        model.predict(x[:, :700])


def test_sliding_view_equals_materialised_snippets():
    """Snippet indexing is bit-exact: reading snippets in place from the [T,171] spectrogram gives the same
    bits as predicting the materialised copies the reference builds (predict.py:253-261)."""
    from oracle.postprocess_ref import slice_snippets

    model, p = make_model(5)
    T = 736 + 368 * 3 + 100
    spec = np.random.default_rng(2).random((T, 171), dtype=np.float32)
    a = model.predict_spectrogram(torch.from_numpy(spec).cuda(), chunk=3).cpu().numpy()
    snippets = slice_snippets(spec, 736)
    assert snippets.shape[0] == a.shape[0] == 4
    b = model.predict(snippets, batch_size=4)
    assert np.array_equal(a, b)


@pytest.mark.parametrize(
    "cfg",
    [
        dict(input_shape=(64, 43, 1), filters=(10, 20, 30, 40), kernel_size=5, lstm_units=64, num_labels=3),
        dict(input_shape=(96, 37, 1), filters=(20, 30, 40, 50), kernel_size=7, lstm_units=128, num_labels=8),
        dict(input_shape=(48, 50, 1), filters=(30, 40), kernel_size=3, lstm_units=64, num_labels=7),
    ],
)
def test_forward_other_hyperparameters(cfg):
    """hpsearch variants (hps defaults: filters sets, kernel 3/5/7, lstm_units 64/128) and odd sizes."""
    model, p = make_model(7, **cfg)
    rng = np.random.default_rng(3)
    x = rng.random((18, *cfg["input_shape"]), dtype=np.float32)  # 18 > one LSTM batch tile of 16
    ref = M.forward_ref(p, x)
    out = model.predict(x, batch_size=18)
    assert out.shape == ref.shape
    assert np.abs(out - ref).max() <= 1e-5, np.abs(out - ref).max()


def test_overlap_average_bit_exact(golden_dir):
    from orcai_amd.predict import aggregate_predictions_device

    for T in [736, 1103, 1104, 1471, 1472, 11251]:
        g = np.load(golden_dir / f"aggregate_T{T}.npz")
        pred = torch.from_numpy(g["predictions"]).cuda()
        agg, cnt = aggregate_predictions_device(pred, T, 736, 4)
        assert np.array_equal(agg, g["aggregated"]) and np.array_equal(cnt, g["overlap_count"])


def make_1dconv(seed, input_shape, filters, kernel_size, num_labels=7):
    """Calibrated trunk parameters of the oracle + a glorot Conv1D head (architectures.py:107-115)."""
    from orcai_amd.architectures import FINAL_FILTERS, ResNet1DConv

    p = M.calibrated_params(seed=seed, input_shape=input_shape, num_labels=num_labels, filters=filters, kernel_size=kernel_size, lstm_units=64)
    p = {k: v for k, v in p.items() if not k.startswith(("lstm", "dense", "bn_d"))}
    rng = np.random.default_rng(seed + 100)
    lim = np.sqrt(6.0 / (FINAL_FILTERS * FINAL_FILTERS + FINAL_FILTERS * num_labels))
    p["conv1d/kernel"] = rng.uniform(-lim, lim, (FINAL_FILTERS, FINAL_FILTERS, num_labels)).astype(np.float32)
    p["conv1d/bias"] = (0.1 * rng.standard_normal(num_labels)).astype(np.float32)
    model = ResNet1DConv(input_shape, num_labels, list(filters), kernel_size, 0.3)
    model.set_weights_dict(p)
    return model, p


@pytest.mark.parametrize("input_shape,filters,k", [((736, 171, 1), (30, 40, 50, 60), 3), ((96, 20, 1), (10, 20), 5)])
def test_resnet_1dconv_forward(input_shape, filters, k):
    """ResNet1DConv = same trunk + ReduceFrequencyMean + Conv1D(k = 36, same, sigmoid); |delta p| <= 1e-5."""
    model, p = make_1dconv(7, input_shape, filters, k)
    H, W, _ = input_shape
    steps = H // 2 ** len(filters)
    assert model.output_shape == (None, steps, 7) and model.architecture == "ResNet1DConv"
    rng = np.random.default_rng(2)
    x = rng.random((3, H, W, 1), dtype=np.float32)
    ref, inter = M.forward_ref_1dconv(p, x, return_intermediates=True)
    xd = torch.from_numpy(x[..., 0].copy()).cuda()
    out = torch.empty((3, steps, 7), dtype=torch.float32, device="cuda")
    keep = {}
    model.forward_device(xd.view(-1), H * W, 3, out, keep=keep)
    close(keep["freq_mean"].cpu().numpy(), inter["freq_mean"])
    o = out.cpu().numpy()
    assert np.abs(o - ref).max() <= 1e-5, np.abs(o - ref).max()
    assert np.abs(o - M.forward_ref_1dconv(p, x, dtype=torch.float64)).max() <= 1e-5
    assert np.abs(model.predict(x, batch_size=2) - ref).max() <= 1e-5  # the keras-shaped entry point


@pytest.mark.parametrize("Cin,Cout,H,W,layout,relu_in,relu_out", [
    (16, 30, 736, 171, 0, 1, 1),   # orcai-V1 b1/sep_a
    (30, 30, 736, 171, 2, 0, 0),   # orcai-V1 b1/sep_b (x-pooled output, odd W)
    (13, 17, 9, 70, 0, 0, 1),      # ragged channels, few rows (tail windows), window crossing rows
    (32, 32, 5, 64, 2, 1, 0),      # even W; Wx % 4 == 0 -> the x-pooled buffer has no padding column
    (29, 32, 33, 118, 2, 1, 1),
    (32, 20, 2, 61, 0, 1, 0),
    (30, 40, 368, 86, 0, 1, 1),    # orcai-V1 b2/sep_a: three output tiles
    (40, 40, 64, 86, 2, 0, 0),     # b2/sep_b: 10 input quads
    (50, 50, 40, 43, 2, 0, 0),     # b3/sep_b: 13 quads, four output tiles
    (60, 60, 46, 22, 2, 0, 1),     # b4/sep_b: 15 quads
    (37, 64, 7, 100, 0, 1, 1),
    (16, 16, 20, 171, 0, 0, 0),    # one output tile (input-gradient pass of b1/sep_a)
    (7, 9, 3, 300, 0, 1, 0),       # 21 row chunks per quad: three LDS-DMAs per wave
])
def test_tile_sepconv_is_bit_identical(Cin, Cout, H, W, layout, relu_in, relu_out):
    """The LDS-shared-row kernels (sepconv_tile_kernel: 8-row x 64-column strip tiles; sepconv_ftile_kernel: 8 consecutive flat windows)
    perform the arithmetic of sepconv_kernel in the same order: outputs are equal bit for bit and plane pads stay zero, with the
    launcher's own choice (mode 1) and with the flat-range kernel forced for every shape (mode 2)."""
    from orcai_amd import _native as N

    lib = N.lib()
    dev = torch.device("cuda", 0)
    g = torch.Generator(device="cpu").manual_seed(Cin * 1000 + Cout * 10 + layout)
    B, CQ, CQo, WP = 3, (Cin + 3) // 4, (Cout + 3) // 4, lib.orcai_padded_width(W, 3)
    x = torch.zeros(B, CQ * 4, H + 2, WP)
    x[:, :Cin, 1:H + 1, :W] = torch.randn(B, Cin, H, W, generator=g)
    planes = x.view(B, CQ, 4, H + 2, WP).permute(0, 1, 3, 4, 2).contiguous().to(dev)
    dw = torch.randn(CQ, 9, 4, generator=g).to(dev)
    pw = (torch.randn(Cin, Cout, generator=g) / Cin ** 0.5).to(dev)
    scale, shift = torch.randn(Cout, generator=g).to(dev), torch.randn(Cout, generator=g).to(dev)
    Wx = (W + 1) // 2
    oshape = (B, CQo, H + 2, WP, 4) if layout == 0 else (B, CQo, H, (Wx + 3) // 4 * 4, 4)

    def run(tile):
        prev_tile = lib.orcai_sepconv_tile_mode(tile)
        try:
            out = torch.zeros(oshape, device=dev)
            rc = lib.orcai_sepconv_bn(N.ptr(planes), B, Cin, H, W, 3, relu_in, N.ptr(dw), N.ptr(pw), N.ptr(scale), N.ptr(shift), Cout, relu_out, layout,
                                      N.ptr(out), N.stream_ptr())
            assert rc == 0
            torch.cuda.synchronize()
            return out
        finally:
            lib.orcai_sepconv_tile_mode(prev_tile)

    ref = run(0)
    assert float(ref.abs().max()) > 0
    for tile in (1, 2):
        out = run(tile)
        assert torch.equal(out, ref), tile  # planes: pads included; x-pooled: the padding columns are never written either


@pytest.mark.parametrize("Cin,Cout,H,W,relu_in", [(16, 30, 736, 171, 0), (30, 30, 736, 171, 1), (29, 32, 33, 118, 1), (9, 17, 5, 130, 0)])
def test_tile_sepconv_training_forward_is_bit_identical(Cin, Cout, H, W, relu_in):
    """Training forward (the depthwise output u is stored next to the pre-BN output): the LDS-tile kernel against sepconv_kernel,
    both tensors equal bit for bit, pads of both stay zero."""
    from orcai_amd import _native as N

    lib = N.lib()
    dev = torch.device("cuda", 0)
    g = torch.Generator(device="cpu").manual_seed(Cin * 100 + Cout)
    B, CQ, CQo, WP = 2, (Cin + 3) // 4, (Cout + 3) // 4, lib.orcai_padded_width(W, 3)
    x = torch.zeros(B, CQ * 4, H + 2, WP)
    x[:, :Cin, 1:H + 1, :W] = torch.randn(B, Cin, H, W, generator=g)
    planes = x.view(B, CQ, 4, H + 2, WP).permute(0, 1, 3, 4, 2).contiguous().to(dev)
    dw = torch.randn(CQ, 9, 4, generator=g).to(dev)
    pw = (torch.randn(Cin, Cout, generator=g) / Cin ** 0.5).to(dev)
    scale, shift = torch.ones(Cout).to(dev), torch.randn(Cout, generator=g).to(dev)

    def run(tile):
        prev = lib.orcai_sepconv_tile_mode(tile)
        try:
            out = torch.zeros((B, CQo, H + 2, WP, 4), device=dev)
            u = torch.zeros((B, CQ, H + 2, WP, 4), device=dev)
            rc = lib.orcai_sepconv_planes_u(N.ptr(planes), B, Cin, H, W, 3, 3, relu_in, N.ptr(dw), N.ptr(pw), N.ptr(scale), N.ptr(shift), Cout, 0, 0, 0, 0,
                                            N.ptr(out), N.ptr(u), N.stream_ptr())
            assert rc == 0
            torch.cuda.synchronize()
            return out, u
        finally:
            lib.orcai_sepconv_tile_mode(prev)

    ref, uref = run(0)
    assert float(uref.abs().max()) > 0 and float(ref.abs().max()) > 0
    for mode in (1, 2):
        out, u = run(mode)
        assert torch.equal(out, ref) and torch.equal(u, uref), mode
        assert float(u[:, :, 0].abs().max()) == 0 and float(u[:, :, -1].abs().max()) == 0 and float(u[:, :, :, W:].abs().max()) == 0


@pytest.mark.parametrize("Cin,Cout,H,W,relu_in", [(16, 30, 21, 171, 1), (30, 30, 9, 171, 0), (20, 17, 8, 120, 0), (13, 32, 1, 230, 1), (16, 30, 16, 60, 1), (40, 30, 8, 171, 0),
                                                  (30, 40, 13, 86, 0), (50, 60, 7, 22, 1), (9, 10, 40, 43, 0), (16, 30, 4, 700, 1), (16, 40, 4, 700, 1)])
def test_sepconv_with_statistics_in_the_epilogue(Cin, Cout, H, W, relu_in):
    """orcai_sepconv_planes_stats + orcai_bn_finish_sharded (training forward of a separable conv with the BatchNorm batch statistics of
    its output reduced in the kernel's epilogue) against orcai_sepconv_planes_u + orcai_bn_planes_stats: both output tensors bit for
    bit, mean / variance to f32-partial-sum accuracy (and against float64 sums of the output itself), strip tiles and flat-range tiles,
    one to four output tiles; a plane too wide for either returns ORCAI_E_UNSUPPORTED and touches nothing."""
    from orcai_amd import _native as N

    lib = N.lib()
    dev = torch.device("cuda", 0)
    g = torch.Generator(device="cpu").manual_seed(Cin * 100 + Cout + W)
    B, CQ, CQo, WP = 3, (Cin + 3) // 4, (Cout + 3) // 4, lib.orcai_padded_width(W, 3)
    x = torch.zeros(B, CQ * 4, H + 2, WP)
    x[:, :Cin, 1:H + 1, :W] = torch.randn(B, Cin, H, W, generator=g) + 0.5
    planes = x.view(B, CQ, 4, H + 2, WP).permute(0, 1, 3, 4, 2).contiguous().to(dev)
    dw = torch.randn(CQ, 9, 4, generator=g).to(dev)
    pw = (torch.randn(Cin, Cout, generator=g) / Cin ** 0.5).to(dev)
    scale, shift = torch.ones(Cout).to(dev), (3.0 * torch.randn(Cout, generator=g)).to(dev)  # large biases: mean^2 >> variance for some channels
    st = N.stream_ptr()
    out_ref, u_ref = torch.zeros((B, CQo, H + 2, WP, 4), device=dev), torch.zeros((B, CQ, H + 2, WP, 4), device=dev)
    scratch = torch.zeros(8 * 16 * 32, dtype=torch.float64, device=dev)
    mean_ref, var_ref = torch.zeros(64, device=dev), torch.zeros(64, device=dev)
    assert lib.orcai_sepconv_planes_u(N.ptr(planes), B, Cin, H, W, 3, 3, relu_in, N.ptr(dw), N.ptr(pw), N.ptr(scale), N.ptr(shift), Cout, 0, 0, 0, 0, N.ptr(out_ref),
                                      N.ptr(u_ref), st) == 0
    assert lib.orcai_bn_planes_stats(N.ptr(out_ref), B, Cout, H, W, 3, N.ptr(scratch), N.ptr(mean_ref), N.ptr(var_ref), st) == 0
    out, u = torch.zeros_like(out_ref), torch.zeros_like(u_ref)
    shards = torch.full((8 * 16 * 32,), 7.0, dtype=torch.float64, device=dev)  # the launcher zeroes what it uses
    rc = lib.orcai_sepconv_planes_stats(N.ptr(planes), B, Cin, H, W, relu_in, N.ptr(dw), N.ptr(pw), N.ptr(scale), N.ptr(shift), Cout, N.ptr(out), N.ptr(u), N.ptr(shards), st)
    # every plane the LDS-tile kernels take: strip tiles at any width (two output tiles, <= 32 input channels), flat-range tiles up to ~500 columns
    supported = W < 600 or (16 < Cout <= 32 and Cin <= 32)
    if not supported:
        torch.cuda.synchronize()
        assert rc == N.E_UNSUPPORTED and float(out.abs().max()) == 0 and float(shards.min()) == 7.0
        return
    assert rc == 0
    mean, var = torch.zeros(64, device=dev), torch.zeros(64, device=dev)
    assert lib.orcai_bn_finish_sharded(N.ptr(shards), B, Cout, H, W, N.ptr(mean), N.ptr(var), st) == 0
    torch.cuda.synchronize()
    assert torch.equal(out, out_ref) and torch.equal(u, u_ref)
    v64 = out.double().permute(0, 1, 4, 2, 3).reshape(B, CQo * 4, H + 2, WP)[:, :Cout, 1:H + 1, :W]
    m64, s64 = v64.mean(dim=(0, 2, 3)), v64.var(dim=(0, 2, 3), unbiased=False)
    for got_m, got_v in ((mean, var), (mean_ref, var_ref)):
        assert float((got_m[:Cout].double() - m64).abs().max()) <= 2e-6 * float(m64.abs().max())
        assert float(((got_v[:Cout].double() - s64).abs() / (s64 + 1e-3 * m64 * m64)).max()) <= 2e-5


@pytest.mark.parametrize("shape,filters", [((736, 171, 1), (30, 40, 50, 60)), ((33, 70, 1), (17, 20)), ((16, 64, 1), (64, 12)), ((50, 9, 1), (8, 8))])
def test_fused_entry_convolution_is_bit_identical(shape, filters):
    """orcai_conv0_sepconv (entry convolution computed inside block 1's first separable convolution, compact (2i, 2j) subsample for
    the residual branch) against orcai_conv0_bn_relu + orcai_sepconv_bn: the same fma chains in the same order, so the block-1
    activation, the subsample and the model output are equal bit for bit; odd and even H / W, rows shorter than a window."""
    from orcai_amd import _native as N

    model, p = make_model(21, input_shape=shape, filters=filters, kernel_size=3, lstm_units=64, num_labels=3)
    x = np.random.default_rng(6).random((3, *shape), dtype=np.float32)
    model.fuse_entry = False
    unfused = model.predict(x, batch_size=3)
    model.fuse_entry = True
    fused = model.predict(x, batch_size=3)
    assert np.array_equal(fused, unfused), np.abs(fused - unfused).max()
    assert np.abs(fused - M.forward_ref(p, x)).max() <= 1e-5

    # the two outputs of the fused kernel themselves
    lib, d = N.lib(), model.prepare()
    dev = torch.device("cuda", 0)
    H, W = shape[:2]
    f, B = filters[0], 3
    WP, CQo = lib.orcai_padded_width(W, 3), (f + 3) // 4
    xs = torch.from_numpy(x).to(dev).contiguous()
    prev0 = torch.zeros((B, 4, H + 2, WP, 4), device=dev)
    a_ref, a_fused = torch.zeros((B, CQo, H + 2, WP, 4), device=dev), torch.zeros((B, CQo, H + 2, WP, 4), device=dev)
    sub = torch.zeros((B, 4, (H + 1) // 2, (W + 1) // 2, 4), device=dev)
    st = N.stream_ptr()
    w = lambda k: N.ptr(d[k])  # noqa: E731
    assert lib.orcai_conv0_bn_relu(xs.data_ptr(), H * W, B, H, W, 3, w("conv0/w"), w("conv0/scale"), w("conv0/shift"), N.ptr(prev0), st) == 0
    assert lib.orcai_sepconv_bn(N.ptr(prev0), B, 16, H, W, 3, 1, w("b1/sep_a/dw"), w("b1/sep_a/pw"), w("b1/sep_a/scale"), w("b1/sep_a/shift"), f, 1, 0,
                                N.ptr(a_ref), st) == 0
    assert lib.orcai_conv0_sepconv(xs.data_ptr(), H * W, B, H, W, w("conv0/w"), w("conv0/scale"), w("conv0/shift"), w("b1/sep_a/dw"), w("b1/sep_a/pw"),
                                   w("b1/sep_a/scale"), w("b1/sep_a/shift"), f, 1, N.ptr(a_fused), N.ptr(sub), st) == 0
    torch.cuda.synchronize()
    assert torch.equal(a_fused, a_ref)  # pads included
    assert torch.equal(sub, prev0[:, :, 1:H + 1:2, 0:W:2, :])


def test_tile_sepconv_random_shapes():
    """Seeded sweep over shapes the launcher hands to the LDS-shared-row kernels: every quad count and output tile count, widths from
    narrower than a window to several windows per row, one-row planes, both output layouts; launcher's choice and flat-range kernel
    forced, each against sepconv_kernel."""
    from orcai_amd import _native as N

    lib = N.lib()
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(11)
    g = torch.Generator(device="cpu").manual_seed(11)
    for case in range(24):
        Cout = int(rng.integers(1, 65))
        Cin = int(rng.integers(1, 16 * ((Cout + 15) // 16) + 1))
        H, W = int(rng.integers(1, 24)), int(rng.integers(3, 190))
        layout = int(rng.integers(0, 2)) * 2
        relu_in, relu_out = int(rng.integers(0, 2)), int(rng.integers(0, 2))
        B, CQ, CQo, WP = 2, (Cin + 3) // 4, (Cout + 3) // 4, lib.orcai_padded_width(W, 3)
        x = torch.zeros(B, CQ * 4, H + 2, WP)
        x[:, :Cin, 1:H + 1, :W] = torch.randn(B, Cin, H, W, generator=g)
        planes = x.view(B, CQ, 4, H + 2, WP).permute(0, 1, 3, 4, 2).contiguous().to(dev)
        dw = torch.randn(CQ, 9, 4, generator=g).to(dev)
        pw = (torch.randn(Cin, Cout, generator=g) / Cin ** 0.5).to(dev)
        scale, shift = torch.randn(Cout, generator=g).to(dev), torch.randn(Cout, generator=g).to(dev)
        Wx = (W + 1) // 2
        oshape = (B, CQo, H + 2, WP, 4) if layout == 0 else (B, CQo, H, (Wx + 3) // 4 * 4, 4)
        outs = []
        for mode in (0, 1, 2):
            prev = lib.orcai_sepconv_tile_mode(mode)
            try:
                out = torch.zeros(oshape, device=dev)
                assert lib.orcai_sepconv_bn(N.ptr(planes), B, Cin, H, W, 3, relu_in, N.ptr(dw), N.ptr(pw), N.ptr(scale), N.ptr(shift), Cout, relu_out, layout,
                                            N.ptr(out), N.stream_ptr()) == 0
                torch.cuda.synchronize()
            finally:
                lib.orcai_sepconv_tile_mode(prev)
            outs.append(out)
        assert torch.equal(outs[1], outs[0]) and torch.equal(outs[2], outs[0]), (case, Cin, Cout, H, W, layout)


def test_fused_entry_random_shapes():
    """orcai_conv0_sepconv against orcai_conv0_bn_relu + orcai_sepconv_bn on seeded random shapes and windows-per-wave settings:
    planes narrower than a window, single rows, odd / even sizes, every output tile count; overlapping snippet views."""
    from orcai_amd import _native as N

    lib = N.lib()
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(12)
    g = torch.Generator(device="cpu").manual_seed(12)
    for case in range(16):
        H, W, Cout = int(rng.integers(1, 40 if case < 12 else 150)), int(rng.integers(2, 200)), int(rng.integers(1, 65))
        if case % 2 == 0:  # shapes of the strip-tile variant: two output tiles, at least two 62-column strips
            W, Cout = int(rng.integers(106, 260)), int(rng.integers(17, 33))
        B = 3
        stride = (H // 2 + 1) * W  # overlapping snippets of one long array, as predict uses them
        src = torch.randn((B - 1) * stride + H * W, generator=g).to(dev)
        w0, sc0, sh0 = torch.randn(9, 16, generator=g).to(dev), torch.randn(16, generator=g).to(dev), torch.randn(16, generator=g).to(dev)
        dw, pw = torch.randn(4, 9, 4, generator=g).to(dev), (0.25 * torch.randn(16, Cout, generator=g)).to(dev)
        sc, sh = torch.randn(Cout, generator=g).to(dev), torch.randn(Cout, generator=g).to(dev)
        WP, CQo = lib.orcai_padded_width(W, 3), (Cout + 3) // 4
        relu_out = int(rng.integers(0, 2))
        st = N.stream_ptr()
        prev0 = torch.zeros((B, 4, H + 2, WP, 4), device=dev)
        a_ref = torch.zeros((B, CQo, H + 2, WP, 4), device=dev)
        assert lib.orcai_conv0_bn_relu(N.ptr(src), stride, B, H, W, 3, N.ptr(w0), N.ptr(sc0), N.ptr(sh0), N.ptr(prev0), st) == 0
        assert lib.orcai_sepconv_bn(N.ptr(prev0), B, 16, H, W, 3, 1, N.ptr(dw), N.ptr(pw), N.ptr(sc), N.ptr(sh), Cout, relu_out, 0, N.ptr(a_ref), st) == 0
        for nw, tile in ((1, 0), (2, 0), (5, 0), (4, 10), (4, 16)):
            prev = lib.orcai_entry_windows(nw)
            prev_tile = lib.orcai_entry_tile(tile)
            try:
                a = torch.zeros_like(a_ref)
                sub = torch.zeros((B, 4, (H + 1) // 2, (W + 1) // 2, 4), device=dev)
                assert lib.orcai_conv0_sepconv(N.ptr(src), stride, B, H, W, N.ptr(w0), N.ptr(sc0), N.ptr(sh0), N.ptr(dw), N.ptr(pw), N.ptr(sc), N.ptr(sh), Cout, relu_out,
                                               N.ptr(a), N.ptr(sub), st) == 0
                torch.cuda.synchronize()
            finally:
                lib.orcai_entry_windows(prev)
                lib.orcai_entry_tile(prev_tile)
            assert torch.equal(a, a_ref), (case, H, W, Cout, nw, tile)
            assert torch.equal(sub, prev0[:, :, 1:H + 1:2, 0:W:2, :]), (case, H, W, Cout, nw, tile)


def test_forward_is_hip_graph_capturable():
    """include/orcai_hip.h promises that nothing in the C ABI allocates, frees or synchronises, so a sequence of calls can be captured
    into a hipGraph.  Proof: front end + ResNetLSTM forward + overlap average of a recording captured ONCE on a side stream (after a
    warm-up that sizes the workspaces) and replayed on new audio written into the same input buffer, bit-identical to eager."""
    from orcai_amd import _native as N
    from orcai_amd.frontend import get_frontend
    from orcai_amd.synthetic import pcm16_to_float, synth_recording

    model, _ = make_model(3, input_shape=(64, 171, 1), filters=(12, 20), kernel_size=3, lstm_units=64, num_labels=3)
    sp = {"sampling_rate": 48000, "nfft": 512, "n_overlap": 256, "freq_range": [0, 16000], "quantiles": [0.01, 0.999]}
    fe = get_frontend()
    clips = [torch.from_numpy(pcm16_to_float(synth_recording(1.5, 48000, seed=s))).cuda() for s in (1, 2, 3)]
    static_in = clips[0].clone()

    def run():
        spec = fe.make_spectrogram(static_in, sp)
        return model.predict_spectrogram(spec)

    eager = []
    for c in clips:
        static_in.copy_(c)
        eager.append(run().clone())
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        static_in.copy_(clips[0])
        run()  # warm-up on the capture stream
        torch.cuda.current_stream().synchronize()
        with torch.cuda.graph(g, stream=side):
            assert N.stream_ptr() == side.cuda_stream  # the launchers are handed the capturing stream
            static_out = run()
    for c, want in zip(clips, eager):
        static_in.copy_(c)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(static_out, want)


@pytest.mark.parametrize("C,Cp,H,W,compact", [(30, 16, 736, 171, 1), (40, 30, 368, 86, 0), (30, 16, 37, 171, 0), (40, 30, 9, 87, 0), (50, 40, 21, 80, 0), (20, 9, 5, 161, 1)])
def test_pooling_on_stacked_tiles_is_bit_identical(C, Cp, H, W, compact):
    """pool_res_add_x_kernel<MT, true> (a wave = 4 output rows x 16 columns, the input row two pooling windows share loaded once) against the
    flat-window instantiation: the same maxima and sums, bit for bit, pads of the output untouched -- orcai-V1's blocks 1 and 2, odd heights and
    widths (clamped last rows / columns), a partial last row group, the compact (2i, 2j) subsample of the entry fusion as residual input."""
    from orcai_amd import _native as N

    lib = N.lib()
    dev = torch.device("cuda", 0)
    g = torch.Generator(device="cpu").manual_seed(C * 100 + W)
    B, k = 2, 3
    CQ, CQp = (C + 3) // 4, (Cp + 3) // 4
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    assert Wo >= 40  # the launcher's rule for the stacked tiles
    WPx = (Wo + 3) // 4 * 4
    s = torch.randn(B, CQ, H, WPx, 4, generator=g).to(dev)  # x-pooled conv output
    if compact:
        prev = torch.randn(B, CQp, Ho, Wo, 4, generator=g).to(dev)
    else:
        WP = lib.orcai_padded_width(W, k)
        prev = torch.zeros(B, CQp, H + 2, WP, 4)
        prev[:, :, 1:H + 1, :W] = torch.randn(B, CQp, H, W, 4, generator=g)
        prev = prev.to(dev)
    wr = (torch.randn(Cp, C, generator=g) / Cp ** 0.5).to(dev)
    br = torch.randn(C, generator=g).to(dev)
    WPo = lib.orcai_padded_width(Wo, k)
    outs = {}
    before = lib.orcai_pool_vertical(-1)
    try:
        for vert in (0, 1):
            lib.orcai_pool_vertical(vert)
            out = torch.full((B, CQ, Ho + 2, WPo, 4), 3.0, device=dev)
            rc = lib.orcai_pool_res_add(N.ptr(s), N.ptr(prev), B, C, Cp, H, W, k, N.ptr(wr), N.ptr(br), N.ptr(out), 1 | (2 if compact else 0), N.stream_ptr())
            assert rc == 0
            torch.cuda.synchronize()
            outs[vert] = out
    finally:
        lib.orcai_pool_vertical(before)
    assert torch.equal(outs[0], outs[1])
    pads = outs[1].clone()
    pads[:, :, 1:Ho + 1, :Wo] = 3.0
    assert float((pads - 3.0).abs().max()) == 0.0  # only the interior is written


@pytest.mark.parametrize("C,Cp,H,W,compact,relu_in,nt", [(30, 16, 736, 171, 1, 0, 8), (30, 16, 62, 171, 0, 0, 2), (32, 16, 16, 120, 0, 1, 1), (20, 9, 30, 104, 1, 0, 3), (24, 12, 8, 171, 0, 0, 8),
                                                       (28, 16, 54, 230, 0, 1, 4), (30, 16, 2, 171, 1, 0, 8), (30, 16, 130, 171, 1, 0, 64)])
def test_fused_block_tail_is_bit_identical(C, Cp, H, W, compact, relu_in, nt):
    """orcai_sepconv_pool_res (sepconv_pool_march_kernel: a block's second separable conv with the vertical max-pool, the strided residual 1x1 conv and the
    add in its epilogue; workgroups march down a column strip and carry the row two pooling windows of neighbouring tiles share) against the two launches
    it replaces, orcai_sepconv_bn(out_layout = 2) + orcai_pool_res_add: the same bits, pads of the output untouched.  orcai-V1 block 1 at full size, ragged
    segment / tile counts (H = 62: 4 tiles in segments of 2; H = 54, 30, 130), a single tile and a two-row image, every quad count the launcher instantiates
    (5 .. 8), both residual-input layouts, ReLU on load, strips with a partial last strip (W = 104, 230)."""
    from orcai_amd import _native as N

    lib = N.lib()
    dev = torch.device("cuda", 0)
    g = torch.Generator(device="cpu").manual_seed(C * 1000 + H + W)
    B, k = 2, 3
    CQ, CQp, CQo = (C + 3) // 4, (Cp + 3) // 4, (C + 3) // 4
    Ho, Wo = H // 2, (W + 1) // 2
    WP, WPo, WPx = lib.orcai_padded_width(W, k), lib.orcai_padded_width(Wo, k), (Wo + 3) // 4 * 4
    a = torch.zeros(B, CQ, H + 2, WP, 4)
    a[:, :, 1:H + 1, :W] = torch.randn(B, CQ, H, W, 4, generator=g)
    chan = torch.arange(CQ * 4).view(CQ, 4) < C  # channels past C inside the last quad are kept at zero
    a = (a * chan.view(1, CQ, 1, 1, 4)).to(dev)
    if compact:
        prev = torch.randn(B, CQp, Ho, Wo, 4, generator=g).to(dev)
    else:
        prev = torch.zeros(B, CQp, H + 2, WP, 4)
        prev[:, :, 1:H + 1, :W] = torch.randn(B, CQp, H, W, 4, generator=g)
        prev = prev.to(dev)
    dw = (torch.randn(CQ, 9, 4, generator=g) / 3).to(dev)
    pw = (torch.randn(C, C, generator=g) / C ** 0.5).to(dev)
    scale, shift = (0.5 + torch.rand(C, generator=g)).to(dev), torch.randn(C, generator=g).to(dev)
    scale[::3] *= -1.0  # negative folded BatchNorm scales: BatchNorm must come BEFORE the maxima
    wr = (torch.randn(Cp, C, generator=g) / Cp ** 0.5).to(dev)
    br = torch.randn(C, generator=g).to(dev)
    st = N.stream_ptr()
    xp = torch.zeros(B, CQo, H, WPx, 4, device=dev)
    assert lib.orcai_sepconv_bn(N.ptr(a), B, C, H, W, k, relu_in, N.ptr(dw), N.ptr(pw), N.ptr(scale), N.ptr(shift), C, 0, 2, N.ptr(xp), st) == 0
    want = torch.full((B, CQo, Ho + 2, WPo, 4), 3.0, device=dev)
    assert lib.orcai_pool_res_add(N.ptr(xp), N.ptr(prev), B, C, Cp, H, W, k, N.ptr(wr), N.ptr(br), N.ptr(want), 1 | (2 if compact else 0), st) == 0
    got = torch.full((B, CQo, Ho + 2, WPo, 4), 3.0, device=dev)
    before = lib.orcai_pool_fused(nt)
    try:
        rc = lib.orcai_sepconv_pool_res(N.ptr(a), N.ptr(prev), B, C, C, Cp, H, W, k, relu_in, N.ptr(dw), N.ptr(pw), N.ptr(scale), N.ptr(shift), 0, N.ptr(wr), N.ptr(br),
                                        N.ptr(got), compact, st)
    finally:
        lib.orcai_pool_fused(before)
    assert rc == 0, rc
    torch.cuda.synchronize()
    diff = (got - want).abs()
    assert torch.equal(got, want), (float(diff.max()), int((diff > 0).sum()), [int(v) for v in torch.nonzero(diff > 0)[0]] if (diff > 0).any() else None)
    pads = got.clone()
    pads[:, :, 1:Ho + 1, :Wo] = 3.0
    assert float((pads - 3.0).abs().max()) == 0.0  # only the interior is written


def test_fused_block_tail_refuses_other_shapes():
    """The launcher answers ORCAI_E_UNSUPPORTED before touching anything for shapes the marching kernel does not have: the caller's two launches follow."""
    from orcai_amd import _native as N

    lib = N.lib()
    t = torch.zeros(1 << 20, device="cuda")
    p = N.ptr(t)
    for C, Cp, H, W, k in ((40, 30, 368, 86, 3), (30, 16, 737, 171, 3), (30, 16, 736, 60, 3), (30, 16, 736, 171, 5), (16, 16, 736, 171, 3), (30, 20, 736, 171, 3)):
        assert lib.orcai_sepconv_pool_res(p, p, 1, C, C, Cp, H, W, k, 0, p, p, p, p, 0, p, p, p, 0, N.stream_ptr()) == N.E_UNSUPPORTED, (C, Cp, H, W, k)
    torch.cuda.synchronize()
    assert float(t.abs().max()) == 0.0
