"""Geometry of the trunk stage that 50 %-overlapping predict snippets share ("Shared rows of overlapping snippets").

Snippet i of a recording is spectrogram rows [i*H/2, i*H/2 + H) (predict.py, ``predict_spectrogram``): every row is in two snippets.
A convolution with "same" padding, the (3, 2)-window max pooling and the strided residual convolution make a row of a tensor depend
only on nearby rows, so a snippet's activations equal those of any taller image that contains it -- except in a cone of rows at
each snippet edge, where the snippet's zero padding (or the pooling's -inf padding) stands in for rows the taller image has.
Blocks 1 .. S can therefore be computed once per recording row on tall windows ("super-snippets") and the few edge rows of each
snippet ("patches") on short crops of its own first and last rows, whose other edge is wrong by construction but far enough away.

Everything here is exact integer geometry, no device code: ``shared_stage`` says whether a layout qualifies and how, the driver of
both precisions (``orcai_amd/shared_trunk.py``) plans its launches from the answer.
"""

from __future__ import annotations

from dataclasses import dataclass


def edge_cones(ksize: int, blocks: int, first: int | None = None) -> list[tuple[str, int, int]]:
    """[(tensor, top, bottom)]: how many rows at the top / bottom edge of each trunk tensor of an image can differ from the same
    rows computed inside a taller image, for "same" k x k convolutions and MaxPooling2D((3, 2), 2, "same") on tensors of even
    height (pooling pads one row at the bottom only).  Tensor names as oracle.model_ref.forward_ref's intermediates.
    first: the image is the (exact) input of residual block `first` instead of the spectrogram -- no entry conv, cones of blocks
    first .. blocks only."""
    if ksize not in (3, 5, 7) or blocks < 0 or (first is not None and not 1 <= first <= blocks):
        raise ValueError(f"kernel size {ksize}, {blocks} blocks, first {first}")
    r = ksize // 2
    if first is None:
        t = u = r  # entry conv: its first / last r output rows read the padding
        out = [("conv0", t, u)]
    else:
        t = u = 0
        out = []
    for b in range(1 if first is None else first, blocks + 1):
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


def tail_stage(H: int, W: int, ksize: int, first: int, last: int, snippet_stride: int) -> SharedStage | None:
    """Level 2 of the shared trunk: residual blocks first .. last run once per recording row on the output rows of
    the level-1 shared stage (blocks 1 .. first - 1), which are exact per snippet.  The result is a SharedStage whose "input rows"
    are level-1 output rows (SharedStage.blocks = last - first + 1 blocks of this level), or None when level 2 does not apply: level 1
    does not, H/2 is not a multiple of 2**last, or the crops would not be shorter than half a snippet.

    A snippet's own level-1 patch rows differ from the taller image's and spread through blocks first .. last; together with the
    padding cone of a level-2 image's own edges (edge_cones(..., first=first)) that is what edge_cones(ksize, last) bounds from the
    spectrogram on, so the patch rows at block `last` are its cumulative cones."""
    if not 2 <= first <= last:
        return None
    level1 = shared_stage(H, W, ksize, first - 1, snippet_stride)
    if level1 is None or (H // 2) % 2**last:
        return None
    scale = 2 ** (last - first + 1)
    top, bottom = edge_cones(ksize, last)[-1][1:]
    rows_in = level1.rows
    rows = rows_in // scale
    if top + bottom >= rows // 2:
        return None
    crop = (top + bottom) * scale
    halo = max(top, bottom) * scale
    if crop >= rows_in // 2 or halo > rows_in // 2 or crop < max(level1.patch_top, level1.patch_bottom):
        return None
    return SharedStage(blocks=last - first + 1, rows=rows, period=rows // 2, patch_top=top, patch_bottom=bottom, crop=crop, halo=halo)


@dataclass(frozen=True)
class Family:
    """Destination images of orcai_pool_res_add_scatter_families: `count` images of `height` level-1 output rows in the level-2
    planes `planes` ("super" or "crop") from image `image` on; image j holds recording rows [offset + j * period, + height) and takes
    its rows [keep_lo, keep_hi)."""

    planes: str
    image: int
    height: int
    period: int
    offset: int
    count: int
    keep_lo: int
    keep_hi: int


@dataclass(frozen=True)
class TwoLevelPlan:
    """Launch plan of both levels for one tail chunk.  level1: (window, destination families) -- the level-1 windows of
    plan_windows, whose last block's tail stores into the level-2 images instead of the snippets.  supers / crops: (window, first
    image) -- the level-2 windows of plan_windows(level 2), in images of the "super" planes (super_images images of super_height
    rows) and the "crop" planes (top crops of the snippets are images 0 .. nsnip - 1, bottom crops nsnip .. 2 nsnip - 1)."""

    level1: list[tuple[Window, tuple[Family, ...]]]
    supers: list[tuple[Window, int]]
    crops: list[tuple[Window, int]]
    super_images: int
    super_height: int
    crop_height: int


def plan_two_level(geo: SharedStage, geo2: SharedStage, H: int, nsnip: int, strides_per_image: int = 8) -> TwoLevelPlan:
    """Both levels for nsnip consecutive snippets.  Level-2 super-images are laid out as level 1's, in level-1 output rows, with at
    least enough strides per image that a row lies in at most two of them; the crops are every snippet's first / last geo2.crop rows.
    The level-1 super-snippets store every recording row into each super-image that holds it and into the crop rows outside the
    level-1 patches; the level-1 crops store only those patches.  Every row of every level-2 image is written exactly once."""
    P2 = geo.period  # level-1 output rows per snippet stride
    m2 = max(strides_per_image, -(-2 * geo2.halo // P2))
    supers2, crops2 = plan_windows(geo2, geo.rows, nsnip, m2)
    supers1, crops1 = plan_windows(geo, H, nsnip, strides_per_image)
    fams, supers, j = [], [], 0
    for w in supers2:
        fams.append(Family("super", j, w.height, w.step if w.count > 1 else w.height, w.start, w.count, 0, w.height))
        supers.append((w, j))
        j += w.count
    E = geo2.crop
    top, bot = crops2
    crops = [(top, 0), (bot, nsnip)]

    def crop_family(w, image, lo, hi):
        return Family("crop", image, E, w.step, w.start, nsnip, lo, hi)

    level1 = [(w, tuple(fams) + (crop_family(top, 0, geo.patch_top, E), crop_family(bot, nsnip, 0, E - geo.patch_bottom))) for w in supers1]
    level1.append((crops1[0], (crop_family(top, 0, 0, geo.patch_top),)))
    level1.append((crops1[1], (crop_family(bot, nsnip, E - geo.patch_bottom, E),)))
    return TwoLevelPlan(level1, supers, crops, j, supers2[0].height, E)
