"""The whole-recording gradient on the GPU: the two adjoint launchers alone on exact integers, their adjointness to orcai_overlap_average, RecordingGrad's
forward against the predict path (bit for bit) and its backward against float64 autograd of the eval-mode oracle under a numpy overlap average, the
independence of the chunking, the torch ops, the chain down to the recorded samples, and the memory bound the chunked recompute exists for.

The small model: ResNetLSTM((32, 12, 1), 3, [10, 20], 3, 0.0, 64) and the ResNet1DConv of the same shape -- H 32, shift 16, tpo 4, P 8, step 4."""

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import eval_grad_ref as R  # noqa: E402

CFG = R.STEP_CONFIGS[0][0]  # input_shape (32, 12, 1), filters (10, 20), k 3, 64 LSTM units, 3 labels
H, W, L, SHIFT, P, STEP, TPO = 32, 12, 3, 16, 8, 4, 4
CHUNKS = ((0, 5), (0, 2), (2, 2), (4, 1))  # (i0, nb) of a recording of 5 snippets: the whole, and three chunks with a ragged last one
ARCHS = ("lstm", "conv1d")


def _bits(a):
    return a.contiguous().view(torch.int32)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _lib():
    from orcai_amd import _native as N

    return N, N.lib(), N.stream_ptr()


def _cover(n, S):
    """c(s) by the reference's loop (predict.py:276-293)."""
    cnt = np.zeros(S)
    for i in range(n):
        cnt[i * STEP : i * STEP + P] += 1
    return cnt


def _average_np(pred, S):
    """predict.py:276-293 in float64."""
    agg, cnt = np.zeros((S, pred.shape[2])), np.zeros(S)
    for i in range(pred.shape[0]):
        agg[i * STEP : i * STEP + P] += pred[i]
        cnt[i * STEP : i * STEP + P] += 1
    agg[cnt > 0] /= cnt[cnt > 0, None]
    return agg, cnt


# ------------------------------------------------------------------------------------------------------------------ the kernels alone, exact integers
def _integer_dagg():
    """Integer dagg [25][3] for n = 5 snippets: even wherever two snippets cover the step, so dagg / c is an integer; step 24 is covered by none."""
    cnt = _cover(5, 25)
    assert list(cnt[:4]) == [1] * 4 and list(cnt[4:20]) == [2] * 16 and list(cnt[20:24]) == [1] * 4 and cnt[24] == 0
    dagg = np.random.default_rng(11).integers(-40, 41, (25, L)).astype(np.float32)
    dagg[cnt == 2] *= 2
    dagg[24] = (7, -9, 11)  # never read
    return dagg, cnt


def _avg_bwd(dagg_dev, i0, nb, spare=1, fill=777.0):
    N, lib, st = _lib()
    out = torch.full((nb + spare, P, L), fill, device="cuda")
    rc = lib.orcai_overlap_average_bwd(N.ptr(dagg_dev), 5, P, L, STEP, 25, i0, nb, N.ptr(out), st)
    torch.cuda.synchronize()
    return rc, out


@pytest.mark.parametrize("i0,nb", CHUNKS)
def test_overlap_average_bwd_exact(i0, nb):
    dagg, cnt = _integer_dagg()
    rc, out = _avg_bwd(_dev(dagg), i0, nb)
    assert rc == 0
    want = np.empty((nb, P, L), dtype=np.float32)
    for i in range(i0, i0 + nb):
        for off in range(P):
            want[i - i0, off] = dagg[i * STEP + off] / cnt[i * STEP + off]
    got = out.cpu().numpy()
    assert np.array_equal(got[:nb], want)
    assert (got[nb:] == 777.0).all()  # the spare row behind the chunk is not touched


def _overlap_add_np(dx, T):
    out = np.zeros((T, dx.shape[2]), dtype=np.float64)
    for i in range(dx.shape[0]):
        out[i * SHIFT : i * SHIFT + H] += dx[i]
    return out


@pytest.mark.parametrize("Wd", [12, 171])
def test_snippets_overlap_add_exact(Wd):
    """Integer dx of 5 snippets into dspec [101][Wd], once as one chunk and once as the chunks (0, 2), (2, 2), (4, 1) in sequence: both are the numpy
    overlap-add exactly; rows 96-100 (behind the last full snippet) stay zero, and so does a spare row behind dspec.  dspec is cleared by orcai_zero_fill."""
    N, lib, st = _lib()
    T = 101
    dx = np.random.default_rng(12 + Wd).integers(-50, 51, (5, H, Wd)).astype(np.float32)
    want = _overlap_add_np(dx, T)
    dxd = _dev(dx)
    for chunks in (CHUNKS[:1], CHUNKS[1:]):
        buf = torch.full((T + 1, Wd), 3.0e30, device="cuda")
        assert lib.orcai_zero_fill(N.ptr(buf), 4 * T * Wd, st) == 0
        for i0, nb in chunks:
            assert lib.orcai_snippets_overlap_add(N.ptr(dxd[i0 : i0 + nb]), i0, nb, H, Wd, SHIFT, T, N.ptr(buf), st) == 0
        torch.cuda.synchronize()
        got = buf.cpu().numpy()
        assert np.array_equal(got[:T].astype(np.float64), want), chunks
        assert not got[96:T].any() and (got[T] == np.float32(3.0e30)).all()


def test_bad_arguments_launch_nothing():
    N, lib, st = _lib()
    dagg, _ = _integer_dagg()
    dg = _dev(dagg)
    out = torch.full((6, P, L), 777.0, device="cuda")
    a = lambda dagg_p, n, P_, L_, step, S, i0, nb, out_p: lib.orcai_overlap_average_bwd(dagg_p, n, P_, L_, step, S, i0, nb, out_p, st)  # noqa: E731
    d, o = N.ptr(dg), N.ptr(out)
    for args in ((None, 5, P, L, STEP, 25, 0, 5, o), (d, 5, P, L, STEP, 25, 0, 5, None), (d, 5, P, L, STEP, 25, 0, 0, o), (d, 5, P, L, STEP, 25, -1, 2, o),
                 (d, 5, P, L, STEP, 25, 4, 2, o), (d, 0, P, L, STEP, 25, 0, 1, o), (d, 5, 0, L, STEP, 25, 0, 5, o), (d, 5, P, 0, STEP, 25, 0, 5, o),
                 (d, 5, P, L, 0, 25, 0, 5, o), (d, 5, P, L, STEP, 23, 0, 5, o)):
        assert a(*args) == N.E_BADARG, args
    dx = torch.ones((5, H, W), device="cuda")
    dspec = torch.zeros((101, W), device="cuda")
    b = lambda dx_p, i0, nb, H_, W_, shift, T, ds_p: lib.orcai_snippets_overlap_add(dx_p, i0, nb, H_, W_, shift, T, ds_p, st)  # noqa: E731
    x, s = N.ptr(dx), N.ptr(dspec)
    for args in ((None, 0, 5, H, W, SHIFT, 101, s), (x, 0, 5, H, W, SHIFT, 101, None), (x, 0, 0, H, W, SHIFT, 101, s), (x, 0, -1, H, W, SHIFT, 101, s),
                 (x, -1, 2, H, W, SHIFT, 101, s), (x, 0, 5, H, W, SHIFT, 95, s), (x, 4, 2, H, W, SHIFT, 101, s), (x, 0, 5, 0, W, SHIFT, 101, s),
                 (x, 0, 5, H, 0, SHIFT, 101, s), (x, 0, 5, H, W, 0, 101, s)):
        assert b(*args) == N.E_BADARG, args
    assert lib.orcai_zero_fill(None, 16, st) == N.E_BADARG and lib.orcai_zero_fill(s, 6, st) == N.E_BADARG and lib.orcai_zero_fill(s + 2, 8, st) == N.E_BADARG
    assert lib.orcai_zero_fill(s, -4, st) == N.E_BADARG
    torch.cuda.synchronize()
    assert bool((out == 777.0).all()) and not bool(dspec.any())


def test_adjointness_exact():
    """<overlap_average(pred), dagg> = <pred, overlap_average_bwd(dagg)> in float64, exactly, on integer data (sums of halves of integers: no rounding)."""
    N, lib, st = _lib()
    dagg, _ = _integer_dagg()
    pred = np.random.default_rng(13).integers(-30, 31, (5, P, L)).astype(np.float32)
    pd = _dev(pred)
    agg = torch.empty((25, L), dtype=torch.float64, device="cuda")
    cnt = torch.empty((25,), dtype=torch.float64, device="cuda")
    assert lib.orcai_overlap_average(N.ptr(pd), 5, P, L, STEP, 25, N.ptr(agg), N.ptr(cnt), st) == 0
    rc, dpred = _avg_bwd(_dev(dagg), 0, 5, spare=0)
    assert rc == 0
    want_agg, want_cnt = _average_np(pred.astype(np.float64), 25)
    assert np.array_equal(agg.cpu().numpy(), want_agg) and np.array_equal(cnt.cpu().numpy(), want_cnt)
    lhs = float((agg.cpu().numpy() * dagg.astype(np.float64)).sum())
    rhs = float((pred.astype(np.float64) * dpred.cpu().numpy().astype(np.float64)).sum())
    print(f"<A pred, dagg> = {lhs}, <pred, A^T dagg> = {rhs}")
    assert lhs == rhs and lhs != 0.0


# ------------------------------------------------------------------------------------------------------------------ the recording-level function
_CACHE = {}


def _case(arch):
    """The small model of `arch` with the calibrated weights of tests/eval_grad_ref.py, built once."""
    if arch in _CACHE:
        return _CACHE[arch]
    from orcai_amd.architectures import ResNet1DConv, ResNetLSTM

    conv1d = arch == "conv1d"
    p, _, _ = R.e2e_inputs(CFG, 1, conv1d, 6 if conv1d else 5)
    if conv1d:
        model = ResNet1DConv(CFG["input_shape"], CFG["num_labels"], list(CFG["filters"]), CFG["kernel_size"], 0.0)
    else:
        model = ResNetLSTM(CFG["input_shape"], CFG["num_labels"], list(CFG["filters"]), CFG["kernel_size"], 0.0, CFG["lstm_units"])
    model.set_weights_dict(p)
    _CACHE[arch] = dict(model=model, p=p, conv1d=conv1d)
    return _CACHE[arch]


def _recording(T, Wd=W):
    """A seeded spectrogram [T][Wd] in [0, 1) and the weights r [T // 4][3] of the loss sum(avg * r)."""
    rng = np.random.default_rng(1000 + T)
    return rng.random((T, Wd), dtype=np.float32), rng.standard_normal((T // TPO, L)).astype(np.float32)


def _reference(arch):
    """T = 101, loss sum(avg * r) in float64: the eval-mode oracle on every snippet, the numpy overlap average (as a constant matrix, so that autograd
    passes through it), float64 autograd.  (avg, dspec, the largest |gradient w.r.t. a snippet|), computed once per architecture."""
    c = _case(arch)
    if "ref" in c:
        return c["ref"]
    T = 101
    spec, r = _recording(T)
    n, S = (T - H) // SHIFT + 1, T // TPO
    A = np.zeros((S, n * P))
    for j in range(n * P):  # column j of the average = the average of a unit prediction
        e = np.zeros((n * P, 1))
        e[j] = 1.0
        A[:, j] = _average_np(e.reshape(n, P, 1), S)[0][:, 0]
    st = torch.tensor(spec, dtype=torch.float64, requires_grad=True)
    snippets = torch.stack([st[i * SHIFT : i * SHIFT + H] for i in range(n)])[..., None]
    snippets.retain_grad()
    probs = R.forward_eval(c["p"], snippets, c["conv1d"])
    avg = torch.tensor(A) @ probs.reshape(n * P, L)
    (avg * torch.tensor(r, dtype=torch.float64)).sum().backward()
    assert np.allclose(avg.detach().numpy(), _average_np(probs.detach().numpy(), S)[0], rtol=0, atol=1e-15)  # the matrix IS the numpy loop
    c["ref"] = dict(avg=avg.detach().numpy(), dspec=st.grad.numpy(), dx_max=float(snippets.grad.abs().max()))
    return c["ref"]


@pytest.mark.parametrize("arch", ARCHS)
@pytest.mark.parametrize("T", [32, 101, 112])
def test_forward_is_the_predict_path_bit_for_bit(arch, T):
    from orcai_amd.eval_grad import RecordingGrad
    from orcai_amd.predict import aggregate_predictions_device

    model = _case(arch)["model"]
    spec = _dev(_recording(T)[0])
    avg = RecordingGrad(model, chunk=2).forward(spec)
    want = aggregate_predictions_device(model.predict_spectrogram(spec), T, H, len(model.filters))[0].astype(np.float32)
    assert avg.shape == (T // TPO, L) and avg.dtype == torch.float32
    assert np.array_equal(avg.cpu().numpy().view(np.int32), want.view(np.int32))
    lay = model.layout()
    again = RecordingGrad(model).forward(spec, params=lay.flatten(model.weights, spec.device))  # flat device weights: the same bits
    assert torch.equal(_bits(avg), _bits(again))


def test_a_recording_shorter_than_one_snippet_raises():
    from orcai_amd.eval_grad import RecordingGrad, recording_saliency

    model = _case("lstm")["model"]
    rg = RecordingGrad(model)
    short = torch.zeros((31, W), device="cuda")
    with pytest.raises(ValueError, match="recording too short: 31 spectrogram frames, one snippet needs 32"):
        rg.forward(short)
    with pytest.raises(ValueError, match="recording too short"):
        rg.backward(short, torch.zeros((7, L), device="cuda"))
    with pytest.raises(ValueError, match="recording too short"):
        recording_saliency(model, short)
    with pytest.raises(ValueError, match="davg must be"):
        rg.backward(torch.zeros((48, W), device="cuda"), torch.zeros((11, L), device="cuda"))


@pytest.mark.parametrize("arch", ARCHS)
@pytest.mark.parametrize("chunk", [2, 64])
def test_gradient_vs_float64_autograd(arch, chunk):
    """T = 101 (5 snippets; chunk 2: a ragged last chunk, chunk 64: one chunk), loss sum(avg * r).  The project's bar for a snippet gradient is
    5e-4 max|ref| (tests/test_eval_grad_gpu.py); at most two snippets add into a row of dspec, so max|dspec - ref| <= 2 * 5e-4 * max_i max|dx_ref_i|.
    The averaged probabilities of the forward lie within 5e-6 of the oracle's (the bar of the per-snippet probabilities: an average does not widen it)."""
    from orcai_amd.eval_grad import RecordingGrad

    c, ref = _case(arch), _reference(arch)
    spec, r = _recording(101)
    rg = RecordingGrad(c["model"], chunk=chunk)
    sd = _dev(spec)
    avg = rg.forward(sd)
    dspec = rg.backward(sd, _dev(r))
    torch.cuda.synchronize()
    got = dspec.cpu().numpy().astype(np.float64)
    err, bar = float(np.abs(got - ref["dspec"]).max()), 2 * 5e-4 * ref["dx_max"]
    davg = float(np.abs(avg.cpu().numpy().astype(np.float64) - ref["avg"]).max())
    print(f"{arch} chunk {chunk}: max|dspec - ref| = {err:.3e}, bar {bar:.3e} (max|dx_ref| {ref['dx_max']:.3e}, max|ref| {np.abs(ref['dspec']).max():.3e}); avg vs float64 {davg:.1e}")
    assert dspec.shape == (101, W) and np.isfinite(got).all() and err <= bar, (err, bar)
    assert not got[96:].any() and np.abs(got[:96]).max(axis=1).min() > 0  # frames behind the last full snippet get zero, every covered frame a gradient
    assert davg <= 5e-6


@pytest.mark.parametrize("arch", ARCHS)
def test_chunking_is_the_composition_bit_for_bit(arch):
    """chunk 2 on T = 101: dspec and dw are, bit for bit, the same composition written here -- per chunk EvalGrad.forward / backward(wgrad=True) on the
    materialised snippets, the average's adjoint by torch indexing, torch index_add_ into a zeroed [T, W] in ascending snippet order, dw added in chunk
    order.  A row of dspec receives at most two f32 addends and f32 addition is commutative, so the order inside a row does not matter.

    What each identity rests on.  dspec: EvalGrad's dx has no float atomics, so two runs of a chunk give the same bits and the identity is unconditional.
    dw: the weight-gradient launchers add with float atomics (orcai_dw_wgrad, the entry conv, split-K GEMMs), so a chunk's dw is reproducible between two
    runs only as far as the atomics arrive in the same order; the two runs compared here are the same launches on the same data with the same grids (batch 2
    of the small model: a handful of workgroups per launch), and they have given the same bits in every run so far (difference 0.0, printed below).  That
    part of the identity is therefore checked twice: first on the per-chunk (dx, dw) that RecordingGrad's own EvalGrad returned, recorded in passing --
    no second run, no atomics between the two sides: what RecordingGrad itself adds (the two adjoints, the chunk order of dw) is exact without
    condition -- and then against the independent runs.  If only the last assertion ever fails, the arrival order of a weight-gradient launcher changed, not the
    chunking."""
    from orcai_amd.eval_grad import EvalGrad, RecordingGrad

    model = _case(arch)["model"]
    T = 101
    spec, r = _recording(T)
    sd, rd = _dev(spec), _dev(r)
    rg = RecordingGrad(model, chunk=2)
    recorded, inner = [], rg.eg.backward

    def recording_backward(*a, **kw):
        res = inner(*a, **kw)
        recorded.append(tuple(t.clone() for t in res))
        return res

    rg.eg.backward = recording_backward
    dspec, dw = rg.backward(sd, rd, wgrad=True)
    del rg.eg.backward
    n, S = 5, T // TPO
    assert [int(dx.shape[0]) for dx, _ in recorded] == [2, 2, 1]
    own, own_dw = torch.zeros((T, W), device="cuda"), torch.zeros(model.layout().n_w, device="cuda")
    for c, (dx, dwc) in enumerate(recorded):
        for j in range(dx.shape[0]):
            i = 2 * c + j
            own.index_add_(0, torch.arange(i * SHIFT, i * SHIFT + H, device="cuda"), dx[j])
        own_dw.add_(dwc)
    assert torch.equal(_bits(dspec), _bits(own)) and torch.equal(_bits(dw), _bits(own_dw))
    eg = EvalGrad(model)
    cnt = _dev(_cover(n, S).astype(np.float32))
    want, want_dw = torch.zeros((T, W), device="cuda"), torch.zeros(model.layout().n_w, device="cuda")
    for i0 in range(0, n, 2):
        nb = min(2, n - i0)
        x = torch.stack([sd[i * SHIFT : i * SHIFT + H] for i in range(i0, i0 + nb)])
        _, saved = eg.forward(x)
        dpred = torch.stack([rd[i * STEP : i * STEP + P] / cnt[i * STEP : i * STEP + P, None] for i in range(i0, i0 + nb)])
        dx, dwc = eg.backward(dpred, saved, wgrad=True)
        for i in range(i0, i0 + nb):
            want.index_add_(0, torch.arange(i * SHIFT, i * SHIFT + H, device="cuda"), dx[i - i0])
        want_dw.add_(dwc)
    torch.cuda.synchronize()
    print(f"{arch}: max|dspec - composition| = {float((dspec - want).abs().max()):.3e}, max|dw - composition| = {float((dw - want_dw).abs().max()):.3e} "
          f"(max|dw| {float(dw.abs().max()):.3e})")
    assert torch.equal(_bits(dspec), _bits(want))
    assert torch.equal(_bits(RecordingGrad(model, chunk=2).backward(sd, rd)), _bits(dspec))  # the input gradient does not depend on wgrad
    assert torch.equal(_bits(dw), _bits(want_dw))


@pytest.mark.parametrize("arch", ARCHS)
def test_a_spectrogram_that_is_a_view_into_a_larger_tensor(arch):
    """spec = big[7 : 7 + T], a contiguous row slice with a storage offset (one recording of a stack, the tail of a longer one): forward and backward read
    THOSE rows -- avg, dspec and the ops' gradient have the bits of the same calls on spec.clone(), and the rows of `big` around the slice do not matter."""
    from orcai_amd.eval_grad import RecordingGrad, recording_saliency

    model = _case(arch)["model"]
    T = 101
    spec, r = _recording(T)
    rd = _dev(r)
    big = torch.full((T + 20, W), 0.25, device="cuda")
    big[7 : 7 + T] = _dev(spec)
    view, own = big[7 : 7 + T], big[7 : 7 + T].clone()
    assert view.is_contiguous() and view.storage_offset() == 7 * W and own.storage_offset() == 0
    for chunk in (2, 64):
        rg = RecordingGrad(model, chunk=chunk)
        assert torch.equal(_bits(rg.forward(view)), _bits(rg.forward(own)))
        want = rg.backward(own, rd)
        assert torch.equal(_bits(rg.backward(view, rd)), _bits(want))
        big[:7], big[7 + T :] = -3.0, 9.0  # what lies around the slice is not read
        assert torch.equal(_bits(rg.backward(view, rd)), _bits(want))
    assert torch.equal(_bits(recording_saliency(model, view, chunk=2)), _bits(recording_saliency(model, own, chunk=2)))
    m = _module(arch, frozen_bn=True)
    grads = []
    for x in (view, own):
        x = x.detach().requires_grad_()
        (m.detect_recording(x, chunk=2) * rd).sum().backward()
        grads.append(x.grad)
        m.zero_grad()
    assert torch.equal(_bits(grads[0]), _bits(grads[1])) and torch.equal(_bits(grads[0]), _bits(RecordingGrad(model, chunk=2).backward(own, rd)))


def test_recording_saliency():
    from orcai_amd.eval_grad import RecordingGrad, recording_saliency

    model = _case("lstm")["model"]
    sd = _dev(_recording(101)[0])
    g = torch.zeros((25, L), device="cuda")
    g[:, 1] = 1.0
    assert torch.equal(_bits(recording_saliency(model, sd, label=1)), _bits(RecordingGrad(model).backward(sd, g)))
    assert torch.equal(_bits(recording_saliency(model, sd, chunk=2)), _bits(RecordingGrad(model, chunk=2).backward(sd, torch.ones((25, L), device="cuda"))))


# ------------------------------------------------------------------------------------------------------------------ torch ops
def _module(arch="lstm", **kw):
    from orcai_amd.torch_ops import OrcaiModule

    return OrcaiModule(_case(arch)["model"], **kw).cuda().eval()


def test_opcheck():
    from torch.library import opcheck

    m = _module(frozen_bn=True)
    ws, st, cfg = [w.detach().clone() for w in m.weights_list()], [s.clone() for s in m.stats_list()], m.config
    spec, r = (_dev(a) for a in _recording(101))
    opcheck(torch.ops.orcai.detect_recording.default, (spec, ws, st, cfg, 2))
    opcheck(torch.ops.orcai.detect_recording.default, (spec.clone().requires_grad_(), ws, st, cfg, 2))
    opcheck(torch.ops.orcai.detect_recording_bwd.default, (r, spec, ws, st, cfg, 2))
    # the weight gradients go through float atomics (EvalGrad.backward(wgrad=True)): the checks that compare two runs bit for bit are left out, as in
    # tests/test_frozen_grad_gpu.py
    partial = ("test_schema", "test_autograd_registration", "test_faketensor")
    opcheck(torch.ops.orcai.detect_recording_wrt_params.default, (spec, ws, st, cfg, 2))
    opcheck(torch.ops.orcai.detect_recording_wrt_params.default, (spec.clone().requires_grad_(), [w.clone().requires_grad_() for w in ws], st, cfg, 2), test_utils=partial)
    opcheck(torch.ops.orcai.detect_recording_bwd_params.default, (r, spec, ws, st, cfg, 2), test_utils=partial)


@pytest.mark.parametrize("arch", ARCHS)
def test_module_gradient_is_recording_grad(arch):
    """OrcaiModule(input_grad="eval").detect_recording: avg is RecordingGrad.forward, x.grad RecordingGrad.backward, bit for bit and the same bits in a
    second call; the parameters get no gradient and nothing of the module changes."""
    from orcai_amd.eval_grad import RecordingGrad

    model = _case(arch)["model"]
    m = _module(arch, input_grad="eval")
    before = {n: t.detach().clone() for n, t in list(m.named_parameters()) + list(m.named_buffers())}
    spec, r = (_dev(a) for a in _recording(101))
    rg = RecordingGrad(model, chunk=2)
    grads = []
    for _ in range(2):
        x = spec.clone().requires_grad_()
        avg = m.detect_recording(x, chunk=2)
        assert torch.equal(_bits(avg.detach()), _bits(rg.forward(spec)))
        (avg * r).sum().backward()
        grads.append(x.grad)
    assert torch.equal(_bits(grads[0]), _bits(rg.backward(spec, r))) and torch.equal(_bits(grads[0]), _bits(grads[1]))
    assert all(p.grad is None for p in m.parameters())
    for n, t in list(m.named_parameters()) + list(m.named_buffers()):
        assert torch.equal(_bits(t.detach()), _bits(before[n])), n
    with torch.no_grad():
        assert torch.equal(_bits(m.detect_recording(spec)), _bits(rg.forward(spec)))
    with pytest.raises(NotImplementedError, match="input_grad='eval'"):
        _module(arch).detect_recording(spec.clone().requires_grad_())


@pytest.mark.parametrize("arch", ARCHS)
def test_frozen_bn_module_gets_weight_gradients(arch):
    """frozen_bn=True: every parameter gets a finite, non-zero .grad that is the flat dw of RecordingGrad.backward(wgrad=True) split per variable (to 1e-5 of
    the variable's largest gradient: the weight-gradient launchers add with float atomics, tests/test_frozen_grad_gpu.py), the spectrogram its gradient bit
    for bit, and the moving statistics stay what they were."""
    from orcai_amd.eval_grad import RecordingGrad

    model = _case(arch)["model"]
    m = _module(arch, frozen_bn=True)
    stats = {n: t.detach().clone() for n, t in m.named_buffers()}
    spec, r = (_dev(a) for a in _recording(101))
    x = spec.clone().requires_grad_()
    (m.detect_recording(x, chunk=2) * r).sum().backward()
    dspec, dw = RecordingGrad(model, chunk=2).backward(spec, r, wgrad=True)
    assert torch.equal(_bits(x.grad), _bits(dspec))
    lay = model.layout()
    for n, g in zip(lay.w_names, lay.split_w(dw)):
        got = getattr(m, n.replace("/", "__")).grad
        assert got is not None and got.shape == g.shape and bool(torch.isfinite(got).all()) and float(got.abs().max()) > 0, n
        assert float((got - g).abs().max()) <= 1e-5 * float(g.abs().max()), n
    for n, t in m.named_buffers():
        assert torch.equal(_bits(t), _bits(stats[n])), n


def test_end_to_end_gradient_reaches_the_recorded_samples():
    """pcm at 22.05 kHz -> WaveformFrontEnd -> OrcaiModule(input_grad="eval").detect_recording -> sum(avg * r): pcm.grad is, bit for bit, the chain composed
    by hand -- RecordingGrad.backward, orcai::spectrogram_backward, orcai::resample_backward -- and it is not zero."""
    from orcai_amd.architectures import ResNetLSTM
    from orcai_amd.eval_grad import RecordingGrad
    from orcai_amd.resample import resample_device
    from orcai_amd.torch_ops import OrcaiModule, WaveformFrontEnd, _bins

    sp = {"sampling_rate": 48000, "nfft": 512, "n_overlap": 256, "freq_range": [0, 16000.0], "quantiles": [0.01, 0.999]}
    args = (48000, 512, 256, 16000.0, 0.01, 0.999)
    K = _bins(48000, 512, 16000.0)
    model = ResNetLSTM((H, K, 1), L, [10, 20], 3, 0.0, 64, seed=3)
    m = OrcaiModule(model, input_grad="eval").cuda().eval()
    front = WaveformFrontEnd(sp, 22050)
    n = 8000
    pcm0 = (torch.rand(n, device="cuda", generator=torch.Generator("cuda").manual_seed(5)) * 2 - 1) * 0.3
    pcm = pcm0.clone().requires_grad_()
    avg = m.detect_recording(front(pcm), chunk=2)
    T = 1 + int(resample_device(pcm0, 22050, 48000).shape[0]) // 256
    assert T >= H + 2 * SHIFT and avg.shape == (T // TPO, L)  # at least three snippets: two chunks
    r = torch.randn(avg.shape, device="cuda", generator=torch.Generator("cuda").manual_seed(6))
    (avg * r).sum().backward()
    assert pcm.grad.shape == (n,) and bool(torch.isfinite(pcm.grad).all()) and float(pcm.grad.abs().max()) > 0
    at48 = resample_device(pcm0, 22050, 48000)
    spec, stats = torch.ops.orcai.spectrogram_with_stats(at48, *args)
    dspec = RecordingGrad(model, chunk=2).backward(spec, r)
    d48 = torch.ops.orcai.spectrogram_backward(dspec, at48, stats, *args[:4])
    assert torch.equal(_bits(pcm.grad), _bits(torch.ops.orcai.resample_backward(d48, n, 22050, 48000)))


# ------------------------------------------------------------------------------------------------------------------ memory
@pytest.mark.parametrize("snippets", [40, 42])
def test_backward_memory_does_not_grow_with_the_recording(snippets):
    """T = 32 + 16 * 39 (40 snippets: ten chunks of 4) and 32 + 16 * 41 (42 snippets: a ragged last chunk of 2), chunk 4: what backward allocates at its
    peak, beyond what is alive when it starts, stays below 8 snippets' stored activations (8 x per_snippet floats) plus dspec -- spec itself is alive before
    the call and is not counted twice.  All snippets at once store 40 (42) x per_snippet.  A condition, not a measurement.  Before the peak counter is
    reset a backward on a one-snippet recording has bound the weights (they are no activations and do not depend on T), and EvalGrad's gradient planes of
    that call are dropped, so the planes of the measured call count in full.  The ragged chunk works in the head of the full chunks' planes
    (EvalGrad._workspace): it adds nothing to the peak.  Measured at 40 snippets: 8.12 snippets' activations at the peak (4 stored + 2.96 of gradient planes
    + the head's temporaries + dspec) of the 8.18 the bound allows."""
    from orcai_amd.eval_grad import RecordingGrad

    model = _case("lstm")["model"]
    rg = RecordingGrad(model, chunk=4)
    rg.backward(torch.rand((H, W), device="cuda"), torch.ones((P, L), device="cuda"))
    rg.eg._ws = {}
    T = H + SHIFT * (snippets - 1)
    spec, r = (_dev(a) for a in _recording(T))
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    dspec = rg.backward(spec, r)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    bound = 4 * 8 * rg.eg.per_snippet + 4 * dspec.numel()
    print(f"{snippets} snippets: peak beyond the start {peak} bytes = {peak / (4 * rg.eg.per_snippet):.2f} snippets' activations (dspec {4 * dspec.numel()} bytes); "
          f"bound {bound} bytes; all snippets at once would store {4 * snippets * rg.eg.per_snippet}")
    assert dspec.shape == (T, W) and peak < bound, (peak, bound)
    planes = {b for (b, _), w in rg.eg._ws.items() if "_parent" not in w}
    assert planes == {4}  # one set of gradient planes, the full chunks'; the ragged chunk took its head
