"""The gradient of the PREDICT-TIME network w.r.t. its input snippets: BatchNorm with the moving statistics (the folded scale / shift of the
inference path), no Dropout, nothing written to the model -- saliency / attribution, robustness probes, training something in front of the
detector that will be deployed.  f32 models, both architectures, kernel sizes 3, 5 and 7; no autograd is needed:

    eg = EvalGrad(model)
    probs, saved = eg.forward(x)          # x f32 cuda [B, H, W]
    dx = eg.backward(dprobs, saved)       # f32 [B, H, W]

The forward runs the INFERENCE launchers on the weights ``prepare_device`` folds (the unfused sequence of ``trunk_device(keep=...)``:
orcai_conv0_bn_relu, orcai_sepconv_bn with plane output, orcai_pool_res_add on the full-resolution tensor) and leaves what the backward reads in
ONE flat tensor ``saved`` the caller owns -- y0, every block's y_a, pre-pool s_b and output prev_b, the features, the LSTM gates / cell states
and Dense-128's ReLU output (or the frequency mean of ResNet1DConv), the probabilities and the snippets themselves -- so any number of forwards
may be alive at once (integrated gradients, several losses).  The backward runs no weight-gradient launcher and stores no depthwise output:
every separable conv is ONE orcai_sepconv_dgrad (k = 3; for k = 5 / 7 that launcher refuses and ``compose_dgrad`` runs the existing launchers, as
it does for the large launches beyond 32 input channels where the fused kernel measured slower: EvalGrad.fused),
the pooling is orcai_pool_bwd, the residual 1x1 stride-2 gradient is scatter-added by orcai_sepconv_planes(out_layout = 3), the heads use the
training kernels' data-gradient halves (orcai_lstm_bwd, orcai_conv1d_bwd into a scratch weight gradient) and dgrad GEMMs on the forward GEMM
kernel (no split-K atomics: two runs give the same bits).

    dx, dwflat = eg.backward(dprobs, saved, wgrad=True)    # + f32 [layout().n_w]: the gradient w.r.t. every trainable variable, ParamLayout order

adds the weight gradients of that same network -- fine-tuning with BatchNorm FROZEN on its moving statistics (OrcaiModule(frozen_bn=True)):
per separable conv ONE orcai_sepconv_wgrad_frozen (k = 3; it refuses k = 5 / 7, and ``compose_wgrad`` -- the training step's reduction launchers on a
recomputed depthwise output -- runs instead, as it does where the fused kernel measured slower: EvalGrad.fused_wgrad), finished by orcai_frozen_bn_finish, the residual convs by orcai_outer_reduce(a_stride2) / orcai_planes_sum, the entry conv by orcai_conv0_bn_bwd_x[_ready] with
the moving statistics, the heads by the training step's weight-gradient GEMMs on LSTM outputs rebuilt from the features.  dx keeps its launches and bits;
the weight gradients go through float atomics (orcai_dw_wgrad, split-K GEMMs) and are reproducible to rounding only.

RecordingGrad is the same gradient for a whole RECORDING: the function `orcai predict` reports, spectrogram [T, W] -> the 50 %-overlap average [T // tpo, labels]
of the snippets' probabilities, differentiated w.r.t. the spectrogram (and the weights) in chunks of snippets, so that the stored activations do not grow with T
(DESIGN 4.9):

    rg = RecordingGrad(model, chunk=64)
    avg = rg.forward(spec)                # f32 [T // tpo, L]: predict_spectrogram + orcai_overlap_average, bit for bit what `orcai predict` averages
    dspec = rg.backward(spec, davg)       # f32 [T, W]; with wgrad=True (dspec, dwflat)

The entry conv REUSES orcai_conv0_bn_bwd_dx: called with the moving statistics and zeroed sums it evaluates the eval-mode formula
(dv = gamma * rsqrt(var + eps) * dy where the ReLU fired).  Its ReLU decision is formed from the unfolded BatchNorm, the forward's from the folded
one; the two can only differ for a pre-activation within rounding of zero, and dr1 is already zero where the stored y0 is (x_gate of block 1's
first conv), so a differing decision can only zero a residual-branch term at such a pixel.
"""

from __future__ import annotations

import numpy as np
import torch

from orcai_amd import _native as N
from orcai_amd.architectures import BN_EPS, DENSE_UNITS, ENTRY_FILTERS, FINAL_FILTERS, PreparePlan

Tensor = torch.Tensor


def compose_dgrad(lib, g: Tensor, y_gate, x_gate, B: int, Cin: int, Cout: int, H: int, W: int, k: int, wts: Tensor, dw_rev: Tensor, dr: Tensor, du: Tensor, st) -> None:
    """orcai_sepconv_dgrad's result from the launchers that existed before it (what the launcher's refusal for k = 5 / 7 falls back to, and what its
    tests and tools/time_eval_grad.py compare it with): ReLU gate of g IN PLACE, pointwise pass with wts, depthwise pass with the reversed taps and an
    identity pointwise factor, ReLU gate of dr.  g, du (planes of Cin channels, scratch) and dr need zero pads."""
    dev = g.device
    ones, zeros = torch.ones(64, device=dev), torch.zeros(64, device=dev)
    eye = torch.eye(Cin, device=dev).contiguous()
    if y_gate is not None:
        N.check(lib.orcai_planes_relu_bwd(g.data_ptr(), y_gate.data_ptr(), g.numel(), g.data_ptr(), st), "orcai_planes_relu_bwd")
    N.check(lib.orcai_sepconv_planes(g.data_ptr(), B, Cout, H, W, k, 1, 0, ones.data_ptr(), wts.data_ptr(), ones.data_ptr(), zeros.data_ptr(), Cin, 0, 0, 0, 0,
                                     du.data_ptr(), st), "orcai_sepconv_planes")
    N.check(lib.orcai_sepconv_planes(du.data_ptr(), B, Cin, H, W, k, k, 0, dw_rev.data_ptr(), eye.data_ptr(), ones.data_ptr(), zeros.data_ptr(), Cin, 0, 0, 0, 0,
                                     dr.data_ptr(), st), "orcai_sepconv_planes")
    if x_gate is not None:
        N.check(lib.orcai_planes_relu_bwd(dr.data_ptr(), x_gate.data_ptr(), dr.numel(), dr.data_ptr(), st), "orcai_planes_relu_bwd")



def compose_wgrad(lib, g: Tensor, y_gate, x: Tensor, relu_in: int, B: int, Cin: int, Cout: int, H: int, W: int, k: int, dw: Tensor, wts: Tensor, pw: Tensor, bias, gamma: Tensor,
                  mean: Tensor, var: Tensor, u: Tensor, du: Tensor, G: Tensor, sums: Tensor, scratch: Tensor, partials: Tensor, dWdw: Tensor, dWpw: Tensor, dbias, dgamma: Tensor,
                  dbeta: Tensor, st, consts: dict | None = None) -> None:
    """The weight gradients of one folded separable conv y = [relu](scale (.) (pw . u + bias) + shift), u = dw(relu_in ? relu(x) : x), of the eval path from the
    launchers of the training step: ReLU gate of g IN PLACE (idempotent: compose_dgrad and orcai_sepconv_dgrad form the same gg), u recomputed by the
    forward taps with an identity pointwise factor, G = sum gg (x) u (orcai_outer_reduce), sum gg (orcai_planes_sum), du = wts^T gg, the depthwise gradient
    sum r (.) du accumulated in Keras layout into dWdw (orcai_dw_wgrad), and orcai_frozen_bn_finish for dWpw / dbias / dgamma / dbeta.  g, x, u, du (planes of Cin
    channels, scratch) need zero pads; G [Cout][Cin] and dWdw must be zero on entry (both launchers accumulate); scratch: f64[64]; partials: orcai_outer_reduce's
    workspace.  dw: the forward taps [ceil(Cin/4)][k*k][4]; pw / bias / gamma / mean / var: the layer's variables (Keras layouts).  consts (optional): a dict
    that keeps the constant operands ("ones", "zeros", ("eye", Cin)) between calls."""
    dev = g.device
    consts = {} if consts is None else consts
    for key, make in (("ones", lambda: torch.ones(64, device=dev)), ("zeros", lambda: torch.zeros(64, device=dev)), (("eye", Cin), lambda: torch.eye(Cin, device=dev).contiguous())):
        if key not in consts:
            consts[key] = make()
    ones, zeros, eye = consts["ones"], consts["zeros"], consts[("eye", Cin)]
    if y_gate is not None:
        N.check(lib.orcai_planes_relu_bwd(g.data_ptr(), y_gate.data_ptr(), g.numel(), g.data_ptr(), st), "orcai_planes_relu_bwd")
    N.check(lib.orcai_sepconv_planes(x.data_ptr(), B, Cin, H, W, k, k, relu_in, dw.data_ptr(), eye.data_ptr(), ones.data_ptr(), zeros.data_ptr(), Cin, 0, 0, 0, 0,
                                     u.data_ptr(), st), "orcai_sepconv_planes")
    N.check(lib.orcai_outer_reduce(g.data_ptr(), Cout, u.data_ptr(), Cin, B, H, W, k, 0, 0, 0, G.data_ptr(), partials.data_ptr(), partials.numel(), st), "orcai_outer_reduce")
    N.check(lib.orcai_planes_sum(g.data_ptr(), B, Cout, H, W, k, scratch.data_ptr(), sums.data_ptr(), 0, st), "orcai_planes_sum")
    N.check(lib.orcai_sepconv_planes(g.data_ptr(), B, Cout, H, W, k, 1, 0, ones.data_ptr(), wts.data_ptr(), ones.data_ptr(), zeros.data_ptr(), Cin, 0, 0, 0, 0,
                                     du.data_ptr(), st), "orcai_sepconv_planes")
    N.check(lib.orcai_dw_wgrad(x.data_ptr(), du.data_ptr(), B, Cin, H, W, k, k, relu_in, dWdw.data_ptr(), st), "orcai_dw_wgrad")
    N.check(lib.orcai_frozen_bn_finish(G.data_ptr(), sums.data_ptr(), pw.data_ptr(), None if bias is None else bias.data_ptr(), gamma.data_ptr(), mean.data_ptr(),
                                       var.data_ptr(), BN_EPS, Cin, Cout, dWpw.data_ptr(), None if dbias is None else dbias.data_ptr(), dgamma.data_ptr(), dbeta.data_ptr(), st),
            "orcai_frozen_bn_finish")


def saved_layout(model) -> tuple[list, int]:
    """[(name, offset, shape)] per snippet and the floats per snippet of ``saved``: tensor `name` of a batch of B snippets is
    saved[B * offset : B * (offset + prod(shape))] viewed as [B, *shape].  Host arithmetic only (the fake implementations use it)."""
    planes = model.plane_shape
    shapes = model.stage_shapes()
    H, W = model.input_hw
    items = [("y0", planes(ENTRY_FILTERS, H, W))]
    for b, f in enumerate(model.filters, start=1):
        h, w, _ = shapes[b - 1]
        items += [(f"a{b}", planes(f, h, w)), (f"s{b}", planes(f, h, w)), (f"prev{b}", planes(f, shapes[b][0], shapes[b][1]))]
    T, wd, _ = shapes[-1]
    items.append(("feat", (T, wd * FINAL_FILTERS)))
    if model.architecture == "ResNet1DConv":
        items.append(("fm", (T, FINAL_FILTERS)))
    else:
        u = model.lstm_units
        for layer in (1, 2):
            items += [(f"gates{layer}", (T, 2, 4 * u)), (f"cs{layer}", (T, 2, u))]
        items.append(("pre1", (T, DENSE_UNITS)))
    items += [("probs", (T, model.num_labels)), ("x", (H, W))]  # the snippets last: H * W need not be a multiple of 4 floats
    out, off = [], 0
    for name, shape in items:
        out.append((name, off, shape))
        off += int(np.prod(shape))
    return out, off


class EvalGrad:
    """Eval-mode forward that keeps what its backward needs, and that backward (module docstring).  `params` of forward / backward: (wflat, sflat),
    the trainable variables and the BatchNorm moving statistics as flat f32 cuda tensors in variable_spec() order; None: the model's own weights."""

    # Where the fused kernel loses to the composition (tools/time_eval_grad.py, DESIGN 4.7: beyond 32 input channels its LDS ring leaves one workgroup of
    # four waves per compute unit, and planes narrower than a 62-column strip idle most of its lanes) the composition runs -- unless the launch is so
    # small that the number of launches decides.
    FUSED_MAX_CHANNELS = 32
    FUSED_ANY_CHANNELS_BELOW_PIXELS = 1 << 14

    def __init__(self, model):
        precision = getattr(model, "precision", "f32")
        if precision != "f32":
            raise NotImplementedError(f"EvalGrad: precision {precision!r} computes no gradient w.r.t. the input (f32 models only)")
        self.model = model
        self.conv1d = model.architecture == "ResNet1DConv"
        self.layout, self.per_snippet = saved_layout(model)
        self.lib = None
        self._own = None
        self._ws = {}
        self._plan = None

    # ------------------------------------------------------------------ weights
    def _lib(self):
        if self.lib is None:
            self.lib = N.lib()
        return self.lib

    def _extra_plan(self) -> PreparePlan:
        """The backward's own operands from flat device weights (orcai_prepare_inference kinds 3, 4, 5): per separable conv wts = scale (.) pointwise^T
        and the reversed taps, per block the transposed residual kernel."""
        if self._plan is not None:
            return self._plan
        m, lay = self.model, self.model.layout()
        plan = PreparePlan(lay)
        convs, c = [], ENTRY_FILTERS
        for b, f in enumerate(m.filters, start=1):
            convs += [(f"b{b}/sep_a", f"b{b}/bn_a", c, f), (f"b{b}/sep_b", f"b{b}/bn_b", f, f)]
            plan.add(5, f"b{b}/res/wT", (f, c), c * f, lay.w[f"b{b}/res/kernel"][0], c, f)
            c = f
        convs.append(("sep_f", "bn_f", c, FINAL_FILTERS))
        for name, bn, cin, cout in convs:
            plan.add(3, name + "/wts", (cout, cin), cout, lay.w[bn + "/gamma"][0], lay.s[bn + "/var"][0], lay.w[name + "/pointwise"][0], cin)
            plan.dw(name + "/dw_rev", name + "/depthwise", kind=4)
        self._plan = plan
        return plan

    def bind(self, wflat: Tensor, sflat: Tensor) -> dict:
        """Everything forward and backward read, from flat device weights: prepare_device's folded inference tensors, the backward's operands
        (one more orcai_prepare_inference launch) and views of the raw entry-conv variables."""
        d = dict(self.model.prepare_device(wflat, sflat))
        d.update(self._extra_plan().run(wflat, sflat))
        # the heads' data-gradient GEMMs run on the forward GEMM kernel with transposed operands: orcai_gemm_strided splits K with float atomics
        # for these shapes, and this gradient is bit-reproducible
        for key in ("dense2/W", "dense1/W", "lstm1/W", "lstm2/W"):
            if key in d:
                d[key + "T"] = d[key].t().contiguous()
        lay = self.model.layout()
        for flat, table, names in ((wflat, lay.w, ("conv0/kernel", "conv0/bias", "bn0/gamma", "bn0/beta")), (sflat, lay.s, ("bn0/mean", "bn0/var"))):
            for name in names:
                o, n, _ = table[name]
                d["raw/" + name] = flat[o : o + n]
        d["flat/w"], d["flat/s"] = wflat, sflat  # the weight gradient reads the variables themselves (Keras layouts)
        return d

    def _params(self, params, device) -> dict:
        if isinstance(params, dict):  # already bound (RecordingGrad binds once for all its chunks)
            return params
        if params is not None:
            return self.bind(*params)
        m = self.model
        if self._own is None or self._own[0] != (device, m.weights_version):  # set_weights_dict bumps the version: never the old network
            self._own = ((device, m.weights_version), self.bind(*m.layout().flatten(m.weights, device)))
        return self._own[1]

    def invalidate(self) -> None:
        """Forget the device copies of the model's own weights (set_weights_dict does it too; this is for weights edited in place)."""
        self._own = None

    # ------------------------------------------------------------------ saved
    def views(self, saved: Tensor) -> dict:
        if saved.dim() != 1 or saved.dtype != torch.float32 or not saved.is_cuda or not saved.is_contiguous() or saved.numel() % self.per_snippet:
            raise ValueError(f"EvalGrad: saved must be the contiguous f32 cuda tensor forward() returned ({self.per_snippet} floats per snippet)")
        B = saved.numel() // self.per_snippet
        return {name: saved[B * off : B * (off + int(np.prod(shape)))].view(B, *shape) for name, off, shape in self.layout}

    # ------------------------------------------------------------------ forward
    def forward(self, x: Tensor, params=None) -> tuple[Tensor, Tensor]:
        m = self.model
        H, W = m.input_hw
        if x.dim() != 3 or tuple(x.shape[1:]) != (H, W) or x.dtype != torch.float32 or not x.is_cuda:
            raise ValueError(f"EvalGrad.forward: x must be an f32 cuda tensor [B, {H}, {W}], got {x.dtype} {tuple(x.shape)} on {x.device}")
        B = int(x.shape[0])
        if B == 0:
            raise ValueError("EvalGrad.forward: empty batch")
        with torch.cuda.device(x.device):
            return self._forward(x, B, params)

    def _forward(self, x, B, params):
        m, lib, st = self.model, self._lib(), N.stream_ptr()
        d = self._params(params, x.device)
        H, W = m.input_hw
        k = m.kernel_size
        shapes = m.stage_shapes()
        saved = torch.zeros(B * self.per_snippet, dtype=torch.float32, device=x.device)  # zero pads of every plane tensor
        v = self.views(saved)
        v["x"].copy_(x.detach())
        p = N.ptr
        N.check(lib.orcai_conv0_bn_relu(p(v["x"]), H * W, B, H, W, k, p(d["conv0/w"]), p(d["conv0/scale"]), p(d["conv0/shift"]), p(v["y0"]), st), "orcai_conv0_bn_relu")
        prev, c = v["y0"], ENTRY_FILTERS
        for b, f in enumerate(m.filters, start=1):
            h, w, _ = shapes[b - 1]
            pa, pb = f"b{b}/sep_a", f"b{b}/sep_b"
            N.check(lib.orcai_sepconv_bn(p(prev), B, c, h, w, k, 1, p(d[pa + "/dw"]), p(d[pa + "/pw"]), p(d[pa + "/scale"]), p(d[pa + "/shift"]), f, 1, 0, p(v[f"a{b}"]), st),
                    "orcai_sepconv_bn")
            N.check(lib.orcai_sepconv_bn(p(v[f"a{b}"]), B, f, h, w, k, 0, p(d[pb + "/dw"]), p(d[pb + "/pw"]), p(d[pb + "/scale"]), p(d[pb + "/shift"]), f, 0, 0, p(v[f"s{b}"]), st),
                    "orcai_sepconv_bn")
            N.check(lib.orcai_pool_res_add(p(v[f"s{b}"]), p(prev), B, f, c, h, w, k, p(d[f"b{b}/res/w"]), p(d[f"b{b}/res/b"]), p(v[f"prev{b}"]), 0, st), "orcai_pool_res_add")
            prev, c = v[f"prev{b}"], f
        T, wd, _ = shapes[-1]
        N.check(lib.orcai_sepconv_bn(p(prev), B, c, T, wd, k, 0, p(d["sep_f/dw"]), p(d["sep_f/pw"]), p(d["sep_f/scale"]), p(d["sep_f/shift"]), FINAL_FILTERS, 1, 1, p(v["feat"]), st),
                "orcai_sepconv_bn")
        M, L = B * T, m.num_labels
        f32 = dict(dtype=torch.float32, device=x.device)
        if self.conv1d:
            N.check(lib.orcai_freq_mean(p(v["feat"]), M, wd, FINAL_FILTERS, p(v["fm"]), st), "orcai_freq_mean")
            N.check(lib.orcai_conv1d_sigmoid(p(v["fm"]), p(d["conv1d/W"]), p(d["conv1d/b"]), B, T, FINAL_FILTERS, FINAL_FILTERS, L, p(v["probs"]), st), "orcai_conv1d_sigmoid")
        else:
            u = m.lstm_units
            xin, fin = v["feat"], wd * FINAL_FILTERS
            xz = torch.empty((B, T, 2, 4 * u), **f32)
            for layer in (1, 2):
                N.check(lib.orcai_gemm_bias_act(p(xin), p(d[f"lstm{layer}/W"]), p(d[f"lstm{layer}/b"]), None, None, p(xz), M, 8 * u, fin, 0, st), "orcai_gemm_bias_act")
                hout = torch.empty((B, T, 2 * u), **f32)
                N.check(lib.orcai_lstm_train_fwd(p(xz), p(d[f"lstm{layer}/U"]), B, T, u, p(hout), p(v[f"gates{layer}"]), p(v[f"cs{layer}"]), st), "orcai_lstm_train_fwd")
                xin, fin = hout, 2 * u
            # Dense-128: relu(h W + b) is kept for the backward, the folded BatchNorm behind it is a pass of its own
            N.check(lib.orcai_gemm_bias_act(p(xin), p(d["dense1/W"]), p(d["dense1/b"]), None, None, p(v["pre1"]), M, DENSE_UNITS, 2 * u, 1, st), "orcai_gemm_bias_act")
            d1 = torch.empty((M, DENSE_UNITS), **f32)
            N.check(lib.orcai_rows_affine(p(v["pre1"]), M, DENSE_UNITS, DENSE_UNITS, p(d["dense1/scale"]), p(d["dense1/shift"]), 0, p(d1), st), "orcai_rows_affine")
            N.check(lib.orcai_dense_sigmoid(p(d1), p(d["dense2/W"]), p(d["dense2/b"]), M, DENSE_UNITS, L, p(v["probs"]), st), "orcai_dense_sigmoid")
        return v["probs"].clone(), saved

    # ------------------------------------------------------------------ backward
    def _workspace(self, B: int, device) -> dict:
        """Gradient planes (zero pads; only interiors are ever written, so they persist) for a batch of B snippets.  One set is kept, sized for the largest
        batch seen on the device: planes are snippet-major, so a smaller batch (the ragged last chunk of RecordingGrad) works in the head of it."""
        key = (B, device)
        ws = self._ws.get(key)
        if ws is not None:
            return ws
        full = next((w for (b, dev), w in self._ws.items() if dev == device and b > B and "_parent" not in w), None)
        if full is not None:
            batched = full["_batched"]
            ws = {name: (t[:B] if name in batched else t) for name, t in full.items() if name not in ("_batched", "_B")}
            ws["_parent"] = full
            self._ws[key] = ws
            return ws
        m = self.model
        shapes = m.stage_shapes()

        def planes(c, h, w):
            return torch.zeros((B, *m.plane_shape(c, h, w)), dtype=torch.float32, device=device)

        ws = {"sums0": torch.zeros(32, dtype=torch.float64, device=device), "ones": torch.ones(64, device=device), "zeros": torch.zeros(64, device=device)}
        c = ENTRY_FILTERS
        for b, f in enumerate(m.filters, start=1):
            h, w, _ = shapes[b - 1]
            ws[f"dyb{b}"], ws[f"dya{b}"], ws[f"dr{b}"] = planes(f, h, w), planes(f, h, w), planes(c, h, w)
            c = f
        T, wd, _ = shapes[-1]
        ws["dvf"], ws["dprev_f"] = planes(FINAL_FILTERS, T, wd), planes(c, T, wd)
        ws["_B"], ws["_batched"] = B, {name for name in ws if name.startswith(("dy", "dr", "dvf", "dprev"))}
        self._ws = {key: ws}  # a larger batch replaces the set (and the heads taken from it)
        return ws

    @staticmethod
    def _lazy_planes(ws: dict, key, like: Tensor) -> Tensor:
        """Zero-padded scratch planes shaped like `like`, made on first use (only interiors are ever written); in a workspace that is the head of a larger one
        they are the head of the larger one's."""
        t = ws.get(key)
        if t is None:
            parent = ws.get("_parent")
            if parent is None:
                t = torch.zeros_like(like)
                if "_batched" in ws:
                    ws["_batched"].add(key)
            else:
                full = parent.get(key)
                if full is None:
                    full = parent[key] = torch.zeros((parent["_B"], *like.shape[1:]), dtype=like.dtype, device=like.device)
                    parent["_batched"].add(key)
                t = full[: like.shape[0]]
            ws[key] = t
        return t

    def fused(self, B: int, Cin: int, h: int, w: int) -> bool:
        """Whether this separable conv's backward asks orcai_sepconv_dgrad (k = 5 / 7 ask too: the launcher answers ORCAI_E_UNSUPPORTED)."""
        return self.model.kernel_size != 3 or Cin <= self.FUSED_MAX_CHANNELS or B * h * w < self.FUSED_ANY_CHANNELS_BELOW_PIXELS

    def _dgrad(self, d, ws, name, g, y_gate, x_gate, B, Cin, Cout, h, w, dr):
        lib, st, k = self._lib(), N.stream_ptr(), self.model.kernel_size
        wts, dw_rev = d[name + "/wts"], d[name + "/dw_rev"]
        if self.fused(B, Cin, h, w):
            rc = lib.orcai_sepconv_dgrad(g.data_ptr(), None if y_gate is None else y_gate.data_ptr(), None if x_gate is None else x_gate.data_ptr(), B, Cin, Cout, h, w, k,
                                         wts.data_ptr(), dw_rev.data_ptr(), dr.data_ptr(), st)
            if rc != N.E_UNSUPPORTED:
                N.check(rc, "orcai_sepconv_dgrad")
                return
        du = self._lazy_planes(ws, "du/" + name, dr)  # the pointwise product of the composed path (zero pads, interior rewritten by every call)
        compose_dgrad(lib, g, y_gate, x_gate, B, Cin, Cout, h, w, k, wts, dw_rev, dr, du, st)

    def _gemm(self, A, BT, C, M, Nn, K):
        """C[M][Nn] = A[M][K] BT[K][Nn] (a dgrad GEMM: BT = the layer's weight matrix transposed)."""
        N.check(self._lib().orcai_gemm_bias_act(A.data_ptr(), BT.data_ptr(), None, None, None, C.data_ptr(), M, Nn, K, 0, N.stream_ptr()), "orcai_gemm_bias_act")

    def backward(self, dprobs: Tensor, saved: Tensor, params=None, wgrad: bool = False):
        """dx f32 [B, H, W]; with wgrad=True (dx, dwflat): dwflat f32 [layout().n_w], the gradient w.r.t. every trainable variable of the PREDICT-TIME network
        (BatchNorm frozen on its moving statistics, which get no gradient) in ParamLayout order -- the flat order of Trainer and torch_ops.  dx is the same
        launches and the same bits either way."""
        v = self.views(saved)
        if tuple(dprobs.shape) != tuple(v["probs"].shape) or dprobs.dtype != torch.float32 or dprobs.device != saved.device:
            raise ValueError(f"EvalGrad.backward: dprobs must be f32 {tuple(v['probs'].shape)} on {saved.device}, got {dprobs.dtype} {tuple(dprobs.shape)} on {dprobs.device}")
        with torch.cuda.device(saved.device):
            return self._backward(dprobs.detach().contiguous(), v, params, wgrad)

    # ------------------------------------------------------------------ weight gradients (wgrad=True)
    def _wgrad_buffers(self, ws: dict, dev) -> None:
        if "partials" not in ws:
            ws["partials"] = torch.empty(512 * 64 * 64, dtype=torch.float32, device=dev)  # per-workgroup partial products (orcai_outer_reduce, orcai_conv0_bn_bwd_x)
            ws["sum_scratch"] = torch.zeros(64, dtype=torch.float64, device=dev)
            ws["sums_c0"] = torch.zeros(1024, dtype=torch.float64, device=dev)

    def _scratch_planes(self, ws: dict, key: str, like: Tensor) -> Tensor:
        """Zero-padded scratch planes shared by the layers of one shape (only interiors are ever written)."""
        return self._lazy_planes(ws, (key, tuple(like.shape[1:])), like)

    # Where orcai_sepconv_wgrad_frozen beats compose_wgrad (tools/time_frozen_grad.py, DESIGN 4.8: 1.30 x at 16 input channels, 0.41-0.66 x from 30 on -- its
    # tile of 64 pixels leaves the G contraction 16 MFMAs per output tile between barriers, and the LDS images of wider layers leave one or two workgroups per
    # compute unit); elsewhere, and where the launcher refuses (k = 5 / 7), the composition runs.
    WGRAD_FUSED_MAX_CHANNELS = 16
    WGRAD_WORKSPACE_FLOATS = 1024 * (64 * 64 + 64 + 9 * 64)  # serves every shape the launcher supports (include/orcai_hip.h)

    def fused_wgrad(self, B: int, Cin: int, h: int, w: int) -> bool:
        """Whether this separable conv's weight gradient asks orcai_sepconv_wgrad_frozen (k = 5 / 7 ask too: the launcher answers ORCAI_E_UNSUPPORTED)."""
        return self.model.kernel_size != 3 or Cin <= self.WGRAD_FUSED_MAX_CHANNELS

    def _wgrad_sep(self, d, ws, dw, name, bn, g, y_gate, x, relu_in, B, Cin, Cout, h, w):
        """The gradients of separable conv `name` and the frozen BatchNorm `bn` behind it into the flat gradient dw: the reductions by orcai_sepconv_wgrad_frozen
        where fused_wgrad() names the layer and the launcher accepts it, finished by orcai_frozen_bn_finish; otherwise compose_wgrad (g gated in place)."""
        lib, st, lay, wf, sf = self._lib(), N.stream_ptr(), self.model.layout(), d["flat/w"], d["flat/s"]
        W = lambda flat, n: flat[lay.w[n][0] : lay.w[n][0] + lay.w[n][1]]  # noqa: E731
        S = lambda n: sf[lay.s[n][0] : lay.s[n][0] + lay.s[n][1]]  # noqa: E731
        if ("wg/G", Cout, Cin) not in ws:
            ws[("wg/G", Cout, Cin)] = (torch.zeros(Cout * Cin, dtype=torch.float32, device=g.device), torch.empty(Cout, dtype=torch.float32, device=g.device))
        G, sums = ws[("wg/G", Cout, Cin)]
        pw, bias, gamma, mean, var = W(wf, name + "/pointwise"), W(wf, name + "/bias"), W(wf, bn + "/gamma"), S(bn + "/mean"), S(bn + "/var")
        if self.fused_wgrad(B, Cin, h, w):
            if "wg/partials" not in ws:
                ws["wg/partials"] = torch.empty(self.WGRAD_WORKSPACE_FLOATS, dtype=torch.float32, device=g.device)
            rc = lib.orcai_sepconv_wgrad_frozen(x.data_ptr(), g.data_ptr(), None if y_gate is None else y_gate.data_ptr(), relu_in, B, Cin, Cout, h, w, self.model.kernel_size,
                                                d[name + "/dw"].data_ptr(), d[name + "/wts"].data_ptr(), G.data_ptr(), sums.data_ptr(), W(dw, name + "/depthwise").data_ptr(),
                                                ws["wg/partials"].data_ptr(), ws["wg/partials"].numel(), st)
            if rc != N.E_UNSUPPORTED:
                N.check(rc, "orcai_sepconv_wgrad_frozen")
                N.check(lib.orcai_frozen_bn_finish(G.data_ptr(), sums.data_ptr(), pw.data_ptr(), bias.data_ptr(), gamma.data_ptr(), mean.data_ptr(), var.data_ptr(), BN_EPS, Cin,
                                                   Cout, W(dw, name + "/pointwise").data_ptr(), W(dw, name + "/bias").data_ptr(), W(dw, bn + "/gamma").data_ptr(),
                                                   W(dw, bn + "/beta").data_ptr(), st), "orcai_frozen_bn_finish")
                return
        G.zero_()  # orcai_outer_reduce accumulates
        compose_wgrad(lib, g, y_gate, x, relu_in, B, Cin, Cout, h, w, self.model.kernel_size, d[name + "/dw"], d[name + "/wts"], pw, bias, gamma, mean, var,
                      self._scratch_planes(ws, "wg/u", x), self._scratch_planes(ws, "wg/du", x), G, sums, ws["sum_scratch"], ws["partials"], W(dw, name + "/depthwise"),
                      W(dw, name + "/pointwise"), W(dw, name + "/bias"), W(dw, bn + "/gamma"), W(dw, bn + "/beta"), st, consts=ws)

    def _gemm_wgrad(self, A, lda, Bm, ldb, C, M, Nn, K):
        """C[M][Nn] = A^T Bm with A [K][lda] (its first M columns) and Bm [K][ldb] (its first Nn columns): the training step's weight-gradient GEMM."""
        N.check(self._lib().orcai_gemm_strided(A.data_ptr(), 1, lda, Bm.data_ptr(), ldb, 1, C.data_ptr(), M, Nn, K, 1.0, 0, None, 0.0, N.stream_ptr()), "orcai_gemm_strided")

    def _recompute_lstm_outputs(self, d, v, B, T):
        """h1, h2 [B][T][2u]: `saved` keeps the gates and cell states, not the layer outputs the weight gradients contract with -- the forward's two launches per
        layer again (the same bits), gates and cell states into scratch."""
        lib, st, u, p = self._lib(), N.stream_ptr(), self.model.lstm_units, N.ptr
        f32 = dict(dtype=torch.float32, device=v["feat"].device)
        M = B * T
        xin, fin, out = v["feat"], v["feat"].shape[-1], []
        xz, gates, cs = torch.empty((B, T, 2, 4 * u), **f32), torch.empty((B, T, 2, 4 * u), **f32), torch.empty((B, T, 2, u), **f32)
        for layer in (1, 2):
            N.check(lib.orcai_gemm_bias_act(p(xin), p(d[f"lstm{layer}/W"]), p(d[f"lstm{layer}/b"]), None, None, p(xz), M, 8 * u, fin, 0, st), "orcai_gemm_bias_act")
            hout = torch.empty((B, T, 2 * u), **f32)
            N.check(lib.orcai_lstm_train_fwd(p(xz), p(d[f"lstm{layer}/U"]), B, T, u, p(hout), p(gates), p(cs), st), "orcai_lstm_train_fwd")
            out.append(hout)
            xin, fin = hout, 2 * u
        return out

    def _backward(self, dprobs, v, params, wgrad=False):
        m, lib, st = self.model, self._lib(), N.stream_ptr()
        dev = dprobs.device
        d = self._params(params, dev)
        B = int(v["x"].shape[0])
        H, W = m.input_hw
        k = m.kernel_size
        shapes = m.stage_shapes()
        T, wd, c_last = shapes[-1]
        M, L = B * T, m.num_labels
        cols = wd * FINAL_FILTERS
        f32 = dict(dtype=torch.float32, device=dev)
        ws = self._workspace(B, dev)
        p = N.ptr
        dw = None
        if wgrad:
            # the flat gradient, zeroed: orcai_outer_reduce, orcai_dw_wgrad, orcai_conv1d_bwd and the entry conv's launchers accumulate
            lay = m.layout()
            dw = torch.zeros(lay.n_w, **f32)
            self._wgrad_buffers(ws, dev)
            Gw = lambda n: dw[lay.w[n][0] : lay.w[n][0] + lay.w[n][1]]  # noqa: E731
            Sv = lambda n: d["flat/s"][lay.s[n][0] : lay.s[n][0] + lay.s[n][1]]  # noqa: E731
        dz = torch.empty((M, L), **f32)
        N.check(lib.orcai_sigmoid_bwd(p(v["probs"]), p(dprobs), M * L, p(dz), st), "orcai_sigmoid_bwd")
        if self.conv1d:
            dfm = torch.empty((B, T, FINAL_FILTERS), **f32)
            # orcai_conv1d_bwd has no data-gradient-only form: without wgrad its weight gradient lands in a scratch tensor and is dropped
            dW = Gw("conv1d/kernel") if wgrad else torch.zeros((FINAL_FILTERS, FINAL_FILTERS, L), **f32)
            N.check(lib.orcai_conv1d_bwd(p(v["fm"]), p(d["conv1d/W"]), p(dz), B, T, FINAL_FILTERS, FINAL_FILTERS, L, p(dW), p(dfm), st), "orcai_conv1d_bwd")
            if wgrad:
                N.check(lib.orcai_colsum(p(dz), M, L, p(Gw("conv1d/bias")), 0, st), "orcai_colsum")
            dfeat = torch.empty((M, cols), **f32)
            N.check(lib.orcai_freq_mean_bwd(p(dfm), M, wd, FINAL_FILTERS, p(dfeat), st), "orcai_freq_mean_bwd")
        else:
            u = m.lstm_units
            dd1 = torch.empty((M, DENSE_UNITS), **f32)
            self._gemm(dz, d["dense2/WT"], dd1, M, DENSE_UNITS, L)
            if wgrad:
                # Dense(labels) from the BatchNorm output d1 (recomputed from the stored ReLU output), and bn_d from the gradient at its output -- before
                # orcai_rows_affine_relu_bwd turns dd1 into the gradient in front of the ReLU
                d1 = torch.empty((M, DENSE_UNITS), **f32)
                N.check(lib.orcai_rows_affine(p(v["pre1"]), M, DENSE_UNITS, DENSE_UNITS, p(d["dense1/scale"]), p(d["dense1/shift"]), 0, p(d1), st), "orcai_rows_affine")
                self._gemm_wgrad(d1, DENSE_UNITS, dz, L, Gw("dense2/kernel"), DENSE_UNITS, L, M)
                N.check(lib.orcai_colsum(p(dz), M, L, p(Gw("dense2/bias")), 0, st), "orcai_colsum")
                rows_ws = torch.empty(2 * DENSE_UNITS, **f32)
                N.check(lib.orcai_rows_bn_frozen_wgrad(p(dd1), p(v["pre1"]), M, DENSE_UNITS, DENSE_UNITS, p(Sv("bn_d/mean")), p(Sv("bn_d/var")), BN_EPS, p(Gw("bn_d/beta")),
                                                       p(Gw("bn_d/gamma")), p(rows_ws), st), "orcai_rows_bn_frozen_wgrad")
            N.check(lib.orcai_rows_affine_relu_bwd(p(dd1), p(v["pre1"]), M, DENSE_UNITS, DENSE_UNITS, p(d["dense1/scale"]), p(dd1), st), "orcai_rows_affine_relu_bwd")
            if wgrad:
                h1, h2 = self._recompute_lstm_outputs(d, v, B, T)
                self._gemm_wgrad(h2, 2 * u, dd1, DENSE_UNITS, Gw("dense1/kernel"), 2 * u, DENSE_UNITS, M)
                N.check(lib.orcai_colsum(p(dd1), M, DENSE_UNITS, p(Gw("dense1/bias")), 0, st), "orcai_colsum")
                unpack, alive = [], []  # kernel-order LSTM gradients -> Keras layout in the flat gradient: ONE launch for both layers at the end
            dh = torch.empty((M, 2 * u), **f32)
            self._gemm(dd1, d["dense1/WT"], dh, M, 2 * u, DENSE_UNITS)
            for layer, fin in ((2, 2 * u), (1, cols)):
                dxz = torch.empty((B, T, 2, 4 * u), **f32)
                N.check(lib.orcai_lstm_bwd(p(dh), p(v[f"gates{layer}"]), p(v[f"cs{layer}"]), p(d[f"lstm{layer}/U"]), B, T, u, p(dxz), st), "orcai_lstm_bwd")
                if wgrad:  # the training step's weight-gradient GEMMs on this dxz (both directions at once, permuted columns)
                    xin, hout = (h1, h2) if layer == 2 else (v["feat"], h1)
                    dWc, dbc, hp = torch.empty((fin, 8 * u), **f32), torch.empty(8 * u, **f32), torch.empty((B, T, 2, u), **f32)
                    self._gemm_wgrad(xin, fin, dxz, 8 * u, dWc, fin, 8 * u, M)
                    N.check(lib.orcai_colsum(p(dxz), M, 8 * u, p(dbc), 0, st), "orcai_colsum")
                    N.check(lib.orcai_lstm_hprev(p(hout), B, T, u, p(hp), st), "orcai_lstm_hprev")
                    for di, dname in enumerate(("fwd", "bwd")):
                        dU = torch.empty((u, 4 * u), **f32)
                        self._gemm_wgrad(hp.view(-1)[di * u :], 2 * u, dxz.view(-1)[di * 4 * u :], 8 * u, dU, u, 4 * u, M)
                        unpack += [N.UnpackDesc(dU.data_ptr(), 4 * u, 0, u, Gw(f"lstm{layer}/{dname}/recurrent").data_ptr(), None, 0.0),
                                   N.UnpackDesc(dWc.data_ptr(), 8 * u, di * 4 * u, fin, Gw(f"lstm{layer}/{dname}/kernel").data_ptr(), None, 0.0),
                                   N.UnpackDesc(dbc.data_ptr(), 8 * u, di * 4 * u, 1, Gw(f"lstm{layer}/{dname}/bias").data_ptr(), None, 0.0)]
                        alive += [dU, dWc, dbc]
                dxl = torch.empty((M, fin), **f32)
                self._gemm(dxz, d[f"lstm{layer}/WT"], dxl, M, fin, 8 * u)
                dh = dxl
            if wgrad:
                N.check(lib.orcai_unpack_lstm_grads((N.UnpackDesc * len(unpack))(*unpack), len(unpack), u, st), "orcai_unpack_lstm_grads")
                del alive
            dfeat = dh
        # the ReLU behind bn_f (its scale is inside sep_f's wts), then into planes
        N.check(lib.orcai_relu_bwd(p(dfeat), p(v["feat"]), M * cols, p(dfeat), st), "orcai_relu_bwd")
        N.check(lib.orcai_feat_to_planes(p(dfeat), B, FINAL_FILTERS, T, wd, k, p(ws["dvf"]), st), "orcai_feat_to_planes")
        nb = len(m.filters)
        dprev = ws["dprev_f"]
        if wgrad:
            self._wgrad_sep(d, ws, dw, "sep_f", "bn_f", ws["dvf"], None, v[f"prev{nb}"], 0, B, c_last, FINAL_FILTERS, T, wd)
        self._dgrad(d, ws, "sep_f", ws["dvf"], None, None, B, c_last, FINAL_FILTERS, T, wd, dprev)
        for b in range(nb, 0, -1):
            f = m.filters[b - 1]
            h, w, cprev = shapes[b - 1]
            ho, wo, _ = shapes[b]
            x_in = v["y0"] if b == 1 else v[f"prev{b - 1}"]
            dout = dprev
            dyb, dya, dr = ws[f"dyb{b}"], ws[f"dya{b}"], ws[f"dr{b}"]
            N.check(lib.orcai_pool_bwd(p(dout), p(v[f"s{b}"]), B, f, h, w, k, p(dyb), st), "orcai_pool_bwd")
            if wgrad:
                # the residual 1x1 stride-2 conv reads the block input at the even pixels; dout is the gradient at its output
                N.check(lib.orcai_outer_reduce(p(x_in), cprev, p(dout), f, B, ho, wo, k, 1, h, w, p(Gw(f"b{b}/res/kernel")), p(ws["partials"]), ws["partials"].numel(), st),
                        "orcai_outer_reduce")
                N.check(lib.orcai_planes_sum(p(dout), B, f, ho, wo, k, p(ws["sum_scratch"]), p(Gw(f"b{b}/res/bias")), 0, st), "orcai_planes_sum")
                self._wgrad_sep(d, ws, dw, f"b{b}/sep_b", f"b{b}/bn_b", dyb, None, v[f"a{b}"], 0, B, f, f, h, w)
            self._dgrad(d, ws, f"b{b}/sep_b", dyb, None, None, B, f, f, h, w, dya)
            if wgrad:
                self._wgrad_sep(d, ws, dw, f"b{b}/sep_a", f"b{b}/bn_a", dya, v[f"a{b}"], x_in, 1, B, cprev, f, h, w)
            self._dgrad(d, ws, f"b{b}/sep_a", dya, v[f"a{b}"], x_in, B, cprev, f, h, w, dr)
            # the residual 1x1 stride-2 conv reads the block input in front of the ReLU: its gradient joins at the even pixels
            N.check(lib.orcai_sepconv_planes(p(dout), B, f, ho, wo, k, 1, 0, p(ws["ones"]), p(d[f"b{b}/res/wT"]), p(ws["ones"]), p(ws["zeros"]), cprev, 0, 3, h, w, p(dr), st),
                    "orcai_sepconv_planes")
            dprev = dr
        dx = torch.empty((B, H, W), **f32)
        N.check(lib.orcai_conv0_bn_bwd_dx(p(v["x"]), H * W, p(dprev), B, H, W, k, p(d["raw/conv0/kernel"]), p(d["raw/conv0/bias"]), p(d["raw/bn0/mean"]), p(d["raw/bn0/var"]),
                                          p(d["raw/bn0/gamma"]), p(d["raw/bn0/beta"]), BN_EPS, p(ws["sums0"]), p(dx), st), "orcai_conv0_bn_bwd_dx")
        if not wgrad:
            return dx
        # The entry conv.  orcai_conv0_bn_bwd_x with the MOVING statistics: its sums sum g and sum g * xhat ARE the eval-mode dbeta0 and dgamma0; its weight gradient
        # is that of a batch-statistics BatchNorm and is dropped.  orcai_conv0_bn_bwd_x_ready on zeroed sums forms dv = gamma * inv * g exactly (the trick dx uses):
        # its weight gradient is the eval-mode dW0, and the (zero) sums it reports are dropped.  dbias0 = sum dv = scale0 * dbeta0 (orcai_frozen_bn_finish).
        c0 = (p(v["x"]), H * W, p(dprev), B, H, W, k, p(d["raw/conv0/kernel"]), p(d["raw/conv0/bias"]), p(d["raw/bn0/mean"]), p(d["raw/bn0/var"]), p(d["raw/bn0/gamma"]),
              p(d["raw/bn0/beta"]), BN_EPS)
        junk_w, junk_s = torch.zeros(k * k * ENTRY_FILTERS, **f32), torch.empty(2 * ENTRY_FILTERS, **f32)
        N.check(lib.orcai_conv0_bn_bwd_x(*c0, p(ws["sums_c0"]), p(Gw("bn0/beta")), p(Gw("bn0/gamma")), p(junk_w), p(ws["partials"]), ws["partials"].numel(), st), "orcai_conv0_bn_bwd_x")
        N.check(lib.orcai_conv0_bn_bwd_x_ready(*c0, p(ws["sums0"]), p(junk_s), p(junk_s[ENTRY_FILTERS:]), p(Gw("conv0/kernel")), p(ws["partials"]), ws["partials"].numel(), st),
                "orcai_conv0_bn_bwd_x_ready")
        N.check(lib.orcai_frozen_bn_finish(None, p(Gw("bn0/beta")), None, None, p(d["raw/bn0/gamma"]), None, p(d["raw/bn0/var"]), BN_EPS, 0, ENTRY_FILTERS, None,
                                           p(Gw("conv0/bias")), None, None, st), "orcai_frozen_bn_finish")
        return dx, dw


def saliency(model, x: Tensor, label: int | None = None) -> Tensor:
    """d(sum over snippets and steps of probs[:, t, label]) / dx of the predict-time network, f32 [B, H, W]; label=None sums over all labels."""
    eg = EvalGrad(model)
    probs, saved = eg.forward(x)
    g = torch.zeros_like(probs)
    if label is None:
        g.fill_(1.0)
    else:
        g[:, :, label] = 1.0
    return eg.backward(g, saved)


# ---------------------------------------------------------------------------------------------------------------------- the whole recording
def recording_geometry(H: int, n_filters: int, T: int) -> dict:
    """The snippet geometry of a recording of T spectrogram frames for snippets of H frames and a trunk of n_filters blocks (predict.py:244-293;
    aggregate_predictions_device): shift, tpo (time steps per output step), P (output steps per snippet), step (output steps between snippets), n (snippets,
    0 when the recording is shorter than one), S (output steps of the recording) and rows = (first, one past the last) spectrogram row a snippet covers --
    the frames from rows[1] on reach no snippet and get no gradient.  Host arithmetic only."""
    shift, tpo = H // 2, 2**n_filters
    n = max((T - H) // shift + 1, 0) if shift > 0 else 0
    return dict(H=H, shift=shift, tpo=tpo, P=H // tpo, step=shift // tpo, n=n, S=T // tpo, rows=(0, (n - 1) * shift + H if n > 0 else 0))


class RecordingGrad:
    """The recording-level function of `orcai predict` and its gradient (module docstring).  forward runs the shared-trunk predict path and
    keeps nothing; backward recomputes the per-snippet EvalGrad forward in chunks of at most `chunk` consecutive snippets -- chunk x EvalGrad.per_snippet
    floats of stored activations at a time, whatever T is -- and carries each chunk's gradient through the two adjoints orcai_overlap_average_bwd and
    orcai_snippets_overlap_add.  The gradient is therefore that of the per-snippet forward, whose probabilities lie within 5e-6 of the shared-trunk
    path's (tests/test_eval_grad_gpu.py), not bit-equal to them.  `params` as for EvalGrad.  chunk: 64 is the batch EvalGrad was timed at
    (profiles/eval_grad_mi355x.json)."""

    def __init__(self, model, chunk: int = 64, eval_grad: EvalGrad | None = None):
        """eval_grad: an EvalGrad of `model` to run the chunks on (its workspaces are then shared with its other callers); None: one of its own."""
        if int(chunk) <= 0:
            raise ValueError(f"RecordingGrad: chunk must be positive, got {chunk}")
        if eval_grad is not None and eval_grad.model is not model:
            raise ValueError("RecordingGrad: eval_grad belongs to another model")
        self.eg = EvalGrad(model) if eval_grad is None else eval_grad  # EvalGrad raises for f16 models
        self.model, self.chunk = model, int(chunk)

    def geometry(self, T: int) -> dict:
        H, _ = self.model.input_hw
        g = recording_geometry(H, len(self.model.filters), int(T))
        if g["P"] != self.model.out_steps or g["step"] * g["tpo"] != g["shift"]:
            raise NotImplementedError(f"RecordingGrad: snippets of {H} frames do not tile into output steps of {g['tpo']} frames (the overlap average assumes they do)")
        return g

    def _check_spec(self, spec: Tensor, who: str) -> dict:
        W = self.model.input_hw[1]
        if spec.dim() != 2 or spec.shape[1] != W or spec.dtype != torch.float32 or not spec.is_cuda:
            raise ValueError(f"RecordingGrad.{who}: spec must be an f32 cuda tensor [T, {W}], got {spec.dtype} {tuple(spec.shape)} on {spec.device}")
        g = self.geometry(spec.shape[0])
        if g["n"] <= 0:
            raise ValueError(f"recording too short: {int(spec.shape[0])} spectrogram frames, one snippet needs {g['H']}")
        return g

    def forward(self, spec: Tensor, params=None) -> Tensor:
        """avg f32 [T // tpo, L]: model.predict_spectrogram (the shared-trunk path) and orcai_overlap_average, rounded to f32 -- the bits of
        aggregate_predictions_device(...)[0].astype(np.float32).  Nothing is kept for the backward: it reads `spec` again."""
        g = self._check_spec(spec, "forward")
        m, lib = self.model, self.eg._lib()
        with torch.cuda.device(spec.device):
            x = spec.detach().contiguous()
            if params is None:
                pred = m.predict_spectrogram(x)
            else:
                with m.bound(m.prepare_device(*params)):
                    pred = m.predict_spectrogram(x)
            agg = torch.empty((g["S"], m.num_labels), dtype=torch.float64, device=spec.device)
            cnt = torch.empty((g["S"],), dtype=torch.float64, device=spec.device)
            N.check(lib.orcai_overlap_average(N.ptr(pred), g["n"], g["P"], m.num_labels, g["step"], g["S"], N.ptr(agg), N.ptr(cnt), N.stream_ptr()), "orcai_overlap_average")
            return agg.to(torch.float32)

    def backward(self, spec: Tensor, davg: Tensor, params=None, wgrad: bool = False):
        """dspec f32 [T, W] from davg = dL/davg f32 [T // tpo, L]; with wgrad=True (dspec, dwflat), dwflat as EvalGrad.backward's, added over the chunks in
        chunk order.  Frames behind the last full snippet get zero."""
        g = self._check_spec(spec, "backward")
        m, eg, lib = self.model, self.eg, self.eg._lib()
        H, W = m.input_hw
        T, L, n, shift = int(spec.shape[0]), m.num_labels, g["n"], g["shift"]
        if tuple(davg.shape) != (g["S"], L) or davg.dtype != torch.float32 or davg.device != spec.device:
            raise ValueError(f"RecordingGrad.backward: davg must be f32 {(g['S'], L)} on {spec.device}, got {davg.dtype} {tuple(davg.shape)} on {davg.device}")
        f32 = dict(dtype=torch.float32, device=spec.device)
        with torch.cuda.device(spec.device):
            st = N.stream_ptr()
            x, davg = spec.detach().contiguous(), davg.detach().contiguous()
            d = eg._params(params, spec.device)  # bound once: every chunk reads the same operands
            dspec = torch.empty((T, W), **f32)
            N.check(lib.orcai_zero_fill(N.ptr(dspec), 4 * dspec.numel(), st), "orcai_zero_fill")
            dw = torch.zeros(m.layout().n_w, **f32) if wgrad else None
            for i0 in range(0, n, self.chunk):
                nb = min(self.chunk, n - i0)
                snippets = torch.as_strided(x[i0 * shift :], (nb, H, W), (shift * W, W, 1)).contiguous()  # the row slice carries spec's own storage offset
                _, saved = eg.forward(snippets, params=d)
                del snippets  # `saved` holds its own copy
                dpred = torch.empty((nb, g["P"], L), **f32)
                N.check(lib.orcai_overlap_average_bwd(N.ptr(davg), n, g["P"], L, g["step"], g["S"], i0, nb, N.ptr(dpred), st), "orcai_overlap_average_bwd")
                res = eg.backward(dpred, saved, params=d, wgrad=wgrad)
                del saved, dpred
                dx = res[0] if wgrad else res
                N.check(lib.orcai_snippets_overlap_add(N.ptr(dx), i0, nb, H, W, shift, T, N.ptr(dspec), st), "orcai_snippets_overlap_add")
                if wgrad:
                    dw.add_(res[1])
                del res, dx
        return (dspec, dw) if wgrad else dspec


def recording_saliency(model, spec: Tensor, label: int | None = None, chunk: int = 64) -> Tensor:
    """d(sum over the recording's output steps of avg[:, label]) / dspec of the predict-time network, f32 [T, W]; label=None sums over all labels."""
    rg = RecordingGrad(model, chunk)
    g = rg._check_spec(spec, "forward")
    davg = torch.zeros((g["S"], model.num_labels), dtype=torch.float32, device=spec.device)
    if label is None:
        davg.fill_(1.0)
    else:
        davg[:, label] = 1.0
    return rg.backward(spec, davg)
