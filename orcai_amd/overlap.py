"""Geometry of the trunk stage that 50 %-overlapping predict snippets share ("Shared rows of overlapping snippets").

Snippet i of a recording is spectrogram rows [i*H/2, i*H/2 + H) (predict.py, ``predict_spectrogram``): every row is in two snippets.
A convolution with "same" padding, the (3, 2)-window max pooling and the strided residual convolution make a row of a tensor depend
only on nearby rows, so a snippet's activations equal those of any taller image that contains it -- except in a cone of rows at
each snippet edge, where the snippet's zero padding (or the pooling's -inf padding) stands in for rows the taller image has.
Blocks 1 .. S can therefore be computed once per recording row on tall windows ("super-snippets") and the few edge rows of each
snippet ("patches") on short crops of its own first and last rows, whose other edge is wrong by construction but far enough away.

Everything here is exact integer geometry, no device code: ``shared_stage`` says whether a layout qualifies and how, the model
(``ResNetLSTM.forward_device``) plans its launches from the answer.
"""

from __future__ import annotations

from dataclasses import dataclass


def edge_cones(ksize: int, blocks: int) -> list[tuple[str, int, int]]:
    """[(tensor, top, bottom)]: how many rows at the top / bottom edge of each trunk tensor of an image can differ from the same
    rows computed inside a taller image, for "same" k x k convolutions and MaxPooling2D((3, 2), 2, "same") on tensors of even
    height (pooling pads one row at the bottom only).  Tensor names as oracle.model_ref.forward_ref's intermediates."""
    if ksize not in (3, 5, 7) or blocks < 0:
        raise ValueError(f"kernel size {ksize}, {blocks} blocks")
    r = ksize // 2
    t = u = r  # entry conv: its first / last r output rows read the padding
    out = [("conv0", t, u)]
    for b in range(1, blocks + 1):
        t_in, u_in = t, u
        t, u = t + r, u + r
        out.append((f"b{b}/a", t, u))
        t, u = t + r, u + r
        out.append((f"b{b}/b", t, u))
        # pooling window i = rows 2i .. 2i+2 (the last window also covers the -inf pad row); the residual reads row 2i of the block input
        t, u = max(-(-t // 2), -(-t_in // 2)), max(u // 2 + 1, u_in // 2)
        out.append((f"b{b}", t, u))
    return out


@dataclass(frozen=True)
class SharedStage:
    """How blocks 1 .. blocks of a 50 %-overlapping snippet layout are computed once per recording row.  Rows of the stage output
    unless named "input rows"."""

    blocks: int  # S: the shared stage is the entry conv and residual blocks 1 .. S
    rows: int  # stage-output rows of one snippet (H / 2**S)
    period: int  # stage-output rows between consecutive snippets (rows / 2)
    patch_top: int  # rows at the top of every snippet taken from its top crop
    patch_bottom: int  # rows at the bottom of every snippet taken from its bottom crop
    crop: int  # E: input rows of a crop (the first / last E rows of a snippet)
    halo: int  # h: input rows a super-snippet reaches past the rows it keeps, on each side

    @property
    def scale(self) -> int:
        return 2**self.blocks


def shared_stage(H: int, W: int, ksize: int, blocks: int, snippet_stride: int) -> SharedStage | None:
    """The shared-stage geometry for snippets of H x W rows laid out snippet_stride elements apart, or None when sharing does not
    apply: the stride is not half a snippet, H/2 is not a multiple of 2**blocks (a shared row would sit at different pooling phases
    in its two snippets), the kernel size is not 3, 5 or 7, or the crops would not be shorter than half a snippet."""
    if blocks < 1 or ksize not in (3, 5, 7) or H <= 0 or W <= 0 or H % 2 or snippet_stride != (H // 2) * W:
        return None
    scale = 2**blocks
    if (H // 2) % scale:
        return None
    top, bottom = edge_cones(ksize, blocks)[-1][1:]
    rows = H // scale
    if top + bottom >= rows // 2:
        return None
    # a crop keeps its patch rows exact while the cone of its artificial far edge stays clear of them: E / 2**S - far cone >= patch
    crop = (top + bottom) * scale
    halo = max(top, bottom) * scale  # the kept rows of a super-snippet are outside both of its edge cones
    if crop >= H // 2 or halo > H // 2:
        return None
    return SharedStage(blocks=blocks, rows=rows, period=rows // 2, patch_top=top, patch_bottom=bottom, crop=crop, halo=halo)


@dataclass(frozen=True)
class Window:
    """One launch group of the shared stage: `count` images of `height` input rows, image b starting at input row
    start + b * step of the tail chunk; image rows r in [r_lo, r_hi) of the stage output are kept, stored through the row map
    (recording row base + b * img_step + r, see orcai_pool_res_add_scatter) into snippet rows [keep_lo, keep_hi)."""

    start: int
    step: int
    count: int
    height: int
    base: int
    img_step: int
    r_lo: int
    r_hi: int
    keep_lo: int
    keep_hi: int


def plan_windows(geo: SharedStage, H: int, nsnip: int, strides_per_image: int = 8) -> tuple[list[Window], list[Window]]:
    """(super-snippet groups, crop groups) covering every row of nsnip consecutive snippets exactly once.  Input rows are counted
    from the first snippet's first row; nothing outside [0, (nsnip + 1) * H/2) is read.

    Super-snippets are `strides_per_image` snippet strides tall plus a halo on each side, all of one height.  Image j starts at
    input row j * m * H/2 and keeps the rows [h, h + m * H/2) of it (the first image also keeps its top rows: its top edge is the
    first snippet's own).  The rows the uniform images leave at the end are kept by one more image that ends at the last snippet's
    bottom edge.  Fewer rows than one super-snippet: one image of all of them.  Crops: the first / last E rows of every snippet."""
    s = geo.scale
    P = H // 2  # input rows per snippet stride
    total = (nsnip + 1) * P
    keep = (geo.patch_top, geo.rows - geo.patch_bottom)
    m = max(1, strides_per_image)
    hi = m * P + 2 * geo.halo
    supers = []
    if total <= hi:
        supers.append(Window(0, 0, 1, total, 0, 0, 0, total // s, *keep))
    else:
        n_uniform = (total - hi) // (m * P) + 1
        ho = geo.halo // s
        supers.append(Window(0, m * P, n_uniform, hi, 0, m * P // s, ho, ho + m * P // s, *keep))
        done = n_uniform * m * P + geo.halo  # first input row not kept yet
        if done < total:
            start = total - hi
            supers.append(Window(start, 0, 1, hi, start // s, 0, (done - start) // s, hi // s, *keep))
    E = geo.crop
    crops = [Window(0, P, nsnip, E, 0, geo.period, 0, E // s, 0, geo.patch_top),
             Window(H - E, P, nsnip, E, (H - E) // s, geo.period, 0, E // s, geo.rows - geo.patch_bottom, geo.rows)]
    return supers, crops
