"""The predict-time driver of the conv trunk, one copy for both precisions: which route a layout takes -- two shared levels, one,
or the per-snippet loop -- and the launch groups of the shared routes, planned from the integer geometry of orcai_amd/overlap.py.

An engine is the f32 model itself (ResNetLSTM) or the f16 HalfEngine.  What the driver asks of it:
  model                       the ResNetLSTM: input_hw, filters, kernel_size, stage_shapes, tail_from_block, tail_chunk, shared_strides, share_overlap
  fits(shapes, blocks)        whether the engine's launchers accept `blocks` on images with these stage shapes (their own index bounds)
  two_phase_unshared          how the route that shares nothing is chunked (see forward_device)
  _buffers(B, first, last, need_input, height)
  trunk_device(src, snippet_stride, B, feat, keep, first, last, ws, height, scatter), head_device(feat, out, keep)
scatter = [(b0, count, destination)]: block `last`'s tail of images b0 .. b0 + count - 1 stores through a RowMap or a Families destination; the
engine formats the C arguments of its own launchers from it.  Nothing here touches a device: tensors are only sliced and passed on.
"""

from __future__ import annotations

from typing import NamedTuple

import torch

from orcai_amd import _native as N
from orcai_amd import overlap


class RowMap(NamedTuple):
    """One destination (orcai_[h_]pool_res_add_scatter): image b's row r is recording row base + b * img_step + r, kept for r in [r_lo, r_hi) and
    stored into rows [keep_lo, keep_hi) of the `nsnip` snippets of `rows` rows, `period` apart, in `planes`.  Fields after `planes` in C order."""

    planes: torch.Tensor
    rows: int
    nsnip: int
    period: int
    base: int
    img_step: int
    r_lo: int
    r_hi: int
    keep_lo: int
    keep_hi: int


class Families(NamedTuple):
    """Several destinations (orcai_[h_]pool_res_add_scatter_families): the window as in RowMap, `array` a ctypes array of _native.RowFamily that
    the launcher reads during the call."""

    base: int
    img_step: int
    r_lo: int
    r_hi: int
    array: object


def _row_map(planes, geo, nsnip: int, w, b0: int = 0) -> RowMap:
    return RowMap(planes, geo.rows, nsnip, geo.period, w.base + b0 * w.img_step, w.img_step, w.r_lo, w.r_hi, w.keep_lo, w.keep_hi)


# ------------------------------------------------------------------ which layouts share
def shared_geometry(engine, snippet_stride: int):
    """overlap.SharedStage for the blocks before tail_from_block when the snippets overlap by half (predict_spectrogram), None for every layout or
    shape that takes the per-snippet path.  Refuses what the engine's launchers would refuse at the tallest image."""
    m = engine.model
    H, W = m.input_hw
    S = m.tail_from_block - 1
    if not 1 <= S <= len(m.filters) or not m.share_overlap:
        return None
    geo = overlap.shared_stage(H, W, m.kernel_size, S, snippet_stride)
    if geo is None:
        return None
    hi = m.shared_strides * (H // 2) + 2 * geo.halo  # the tallest super-snippet
    return geo if engine.fits(m.stage_shapes(hi), range(1, S + 1)) else None


def tail_geometry(engine, snippet_stride: int):
    """overlap.tail_stage for blocks tail_from_block .. last (level 2 of the shared trunk) where shared_geometry applies, None where only the
    blocks before tail_from_block are shared."""
    m = engine.model
    if shared_geometry(engine, snippet_stride) is None:
        return None
    H, W = m.input_hw
    nb, split = len(m.filters), m.tail_from_block
    geo2 = overlap.tail_stage(H, W, m.kernel_size, split, nb, snippet_stride)
    if geo2 is None:
        return None
    P2 = H // 2 // 2 ** (split - 1)  # level-1 output rows per snippet stride
    m2 = max(m.shared_strides, -(-2 * geo2.halo // P2))
    hi = (m2 * P2 + 2 * geo2.halo) * 2 ** (split - 1)  # the tallest level-2 image, in spectrogram rows
    return geo2 if engine.fits(m.stage_shapes(hi), range(split, nb + 1)) else None


# ------------------------------------------------------------------ the shared stages of one tail chunk
def _level1(engine, src, nt: int, geo, chunk: int, groups) -> None:
    """The entry conv and blocks 1 .. geo.blocks on the level-1 windows, in launch groups of at most `chunk` snippets' worth of rows (activation
    memory stays within what `chunk` snippets use on the per-snippet path).  groups = [(window, is a crop, destination(window, first image))]."""
    H, W = engine.model.input_hw
    budget = chunk * H
    n_crop = max(1, min(nt, budget // (4 * geo.crop)))
    n_super = max(1, (budget - n_crop * geo.crop) // max(w.height for w, crop, _ in groups if not crop))
    for w, crop, destination in groups:
        per = n_crop if crop else n_super
        for b0 in range(0, w.count, per):
            B = min(per, w.count - b0)
            ws = engine._buffers(min(per, w.count), 1, geo.blocks, height=w.height)
            engine.trunk_device(src[(w.start + b0 * w.step) * W :], w.step * W, B, None, first=0, last=geo.blocks, ws=ws, height=w.height,
                                scatter=[(0, B, destination(w, b0))])


def _one_level(engine, src, nt: int, carry, geo, chunk: int) -> None:
    """Entry conv and blocks 1 .. geo.blocks of nt consecutive 50 %-overlapping snippets (snippet 0 at src), once per recording row: super-snippets
    for the rows away from snippet edges, crops of every snippet's first / last rows for its edge patches (overlap.plan_windows).  Every row of
    every snippet lands in carry[0:nt] exactly once."""
    m = engine.model
    supers, crops = overlap.plan_windows(geo, m.input_hw[0], nt, m.shared_strides)

    def destination(w, b0):
        return _row_map(carry, geo, nt, w, b0)

    _level1(engine, src, nt, geo, chunk, [(w, False, destination) for w in supers] + [(w, True, destination) for w in crops])


def _two_level(engine, src, nt: int, carry, geo, geo2, chunk: int) -> None:
    """Entry conv and blocks 1 .. last of nt consecutive 50 %-overlapping snippets, once per recording row in two levels (overlap.plan_two_level).
    Level 1 (blocks 1 .. geo.blocks) stores into the level-2 images: super-images of level-1 output rows and crops of every snippet's first / last
    rows.  Level 2 runs the remaining blocks on those images, its last tail storing every snippet's rows into carry[0:nt] exactly once."""
    m = engine.model
    S, nb = geo.blocks, len(m.filters)
    plan = overlap.plan_two_level(geo, geo2, m.input_hw[0], nt, m.shared_strides)
    up = geo.scale  # spectrogram rows per level-1 output row
    planes = {"super": engine._buffers(plan.super_images, S + 1, S, height=plan.super_height * up)[f"prev{S}"],
              "crop": engine._buffers(2 * nt, S + 1, S, height=plan.crop_height * up)[f"prev{S}"]}
    img_bytes = {key: t[0].numel() * t.element_size() for key, t in planes.items()}
    groups = []
    for i, (w, fams) in enumerate(plan.level1):  # the last two windows are the crops
        arr = (N.RowFamily * len(fams))(*[N.RowFamily(N.ptr(planes[f.planes]) + f.image * img_bytes[f.planes], f.height, f.period, f.offset, f.count,
                                                      f.keep_lo, f.keep_hi) for f in fams])
        groups.append((w, i >= len(plan.level1) - 2, lambda w, b0, arr=arr: Families(w.base + b0 * w.img_step, w.img_step, w.r_lo, w.r_hi, arr)))
    _level1(engine, src, nt, geo, chunk, groups)

    # level 2: all super-images in one launch group, all crops in another; the last tail once per window
    for key, windows, height in (("super", plan.supers, plan.super_height), ("crop", plan.crops, plan.crop_height)):
        count = sum(w.count for w, _ in windows)
        ws = dict(engine._buffers(count, S + 1, nb, need_input=False, height=height * up))
        ws[f"prev{S}"] = planes[key]
        engine.trunk_device(None, 0, count, None, first=S + 1, last=nb, ws=ws, height=height * up,
                            scatter=[(j, w.count, _row_map(carry, geo2, nt, w)) for w, j in windows])


# ------------------------------------------------------------------ the route
def forward_device(engine, src, snippet_stride: int, n: int, out, chunk: int = 128, keep: dict | None = None) -> None:
    """n snippets starting at ``src`` (f32), snippet i at element offset i * snippet_stride, each [H][W] row-major (unpadded).  Writes
    probabilities into out[n][steps][labels].  The trunk runs in chunks (bounds activation memory); the head runs once over all n.

    Snippets that overlap by half (predict_spectrogram) share the trunk: two levels where both geometries exist -- only the final conv and the
    head run per snippet --, one where only the first does.  Every other layout, and the keep hook, runs the trunk per snippet:
      * in chunks of `chunk` snippets, or
      * engine.two_phase_unshared and n > chunk: in two phases -- the blocks before tail_from_block in chunks of `chunk` (their planes are large),
        the later blocks (planes of a few thousand pixels) over up to tail_chunk snippets per launch to fill the chip.
    The same bits on every route."""
    from orcai_amd.architectures import FINAL_FILTERS

    m = engine.model
    steps, wd, _ = m.stage_shapes()[-1]
    feat = torch.empty((n, steps, wd * FINAL_FILTERS), dtype=torch.float32, device=src.device)
    nb, split = len(m.filters), m.tail_from_block
    geo = shared_geometry(engine, snippet_stride) if keep is None and 2 <= split <= nb else None  # decided before anything is launched
    geo2 = tail_geometry(engine, snippet_stride) if geo is not None else None
    two_phase = geo is None and engine.two_phase_unshared and keep is None and split <= nb and n > chunk
    if geo is None and not two_phase:
        for s in range(0, n, chunk):
            B = min(chunk, n - s)
            engine.trunk_device(src[s * snippet_stride :], snippet_stride, B, feat[s:], keep=keep if s == 0 else None)
    else:
        first = nb + 1 if geo2 is not None else split  # the first stage that runs over a whole tail chunk of snippets
        big = min(n, m.tail_chunk)
        tail = engine._buffers(big, first, nb, need_input=True)
        carry = tail[f"prev{first - 1}"]  # the stages before `first` store every snippet's rows straight into the tail's input planes
        for t0 in range(0, n, big):  # tail chunks stay independent: each computes its own first and last stride
            nt = min(big, n - t0)
            if geo2 is not None:
                _two_level(engine, src[t0 * snippet_stride :], nt, carry, geo, geo2, chunk)
            elif geo is not None:
                _one_level(engine, src[t0 * snippet_stride :], nt, carry, geo, chunk)
            else:
                for s in range(t0, t0 + nt, chunk):
                    B = min(chunk, t0 + nt - s)
                    head = dict(engine._buffers(B, 1, split - 1))
                    head[f"prev{split - 1}"] = carry[s - t0 :]  # the last early block writes straight into the tail's input planes
                    engine.trunk_device(src[s * snippet_stride :], snippet_stride, B, None, first=0, last=split - 1, ws=head)
            engine.trunk_device(None, snippet_stride, nt, feat[t0:], first=first, last=nb + 1, ws=tail)
    engine.head_device(feat, out, keep=keep)
