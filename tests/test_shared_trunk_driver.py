"""The shared-trunk driver (orcai_amd/shared_trunk.py) against a fake engine, on the CPU: forward_device plans and "launches" a whole prediction,
the engine only writes down what its trunk was asked to do.  From that record alone the row maps are replayed with the launchers' store rules
(tests/row_map_rules.py): every row of every level-2 image and of every snippet's block-4 planes must be written exactly once, from the
recording row that belongs there, and nothing else may be written.  No device: the driver only slices tensors and passes them on."""

from collections import namedtuple

import numpy as np
import pytest
import torch
from row_map_rules import _families_store, _scatter_store

from orcai_amd import shared_trunk
from orcai_amd.architectures import ResNetLSTM
from orcai_amd.overlap import Family

CHUNK = 1  # predict_spectrogram(spec, chunk=1): a row budget of one snippet per launch group
Call = namedtuple("Call", "first last B height src_row src_step input scatter")


class FakeEngine:
    """What shared_trunk.py asks of an engine, with a real (host-side) model for the shapes.  Planes are small CPU tensors, one row of 4 floats per
    image, registered under a name with their image count and the rows an image has; a fresh set on every _buffers call."""

    two_phase_unshared = False

    def __init__(self, k, hw):
        self.model = ResNetLSTM((hw[0], hw[1], 1), 7, [30, 40, 50, 60], k, lstm_units=128, seed=1)
        self.model.tail_chunk, self.model.shared_strides = 8, 3
        self.planes, self.calls = [], []  # [(tensor, name, images, rows)], [Call]

    def fits(self, shapes, blocks):
        return True

    def _buffers(self, B, first=1, last=None, need_input=True, height=None):
        m = self.model
        last = len(m.filters) if last is None else last
        shapes = m.stage_shapes(height)
        ws = {}
        for stage in ([first - 1] if need_input else []) + list(range(first, last + 1)):
            t = torch.zeros((B, 4))
            self.planes.append((t, f"{len(self.planes)}:prev{stage}@{height}", B, shapes[stage][0]))
            ws[f"prev{stage}"] = t
        for b in range(first, last + 1):
            ws[f"a{b}"] = ws[f"b{b}"] = None  # never the driver's business
        return ws

    def locate(self, address):
        """(name, image) of an address inside registered planes."""
        for t, name, B, _ in self.planes:
            off = address - t.data_ptr()
            if 0 <= off < B * 16:
                assert off % 16 == 0
                return name, off // 16
        raise AssertionError(f"address {address:#x} is in no workspace")

    def info(self, name):
        return next((B, rows) for _, nm, B, rows in self.planes if nm == name)

    def trunk_device(self, src, snippet_stride, B, feat, keep=None, first=0, last=None, ws=None, height=None, scatter=None):
        W = self.model.input_hw[1]
        segments = []
        for b0, count, dst in scatter or []:
            if isinstance(dst, shared_trunk.RowMap):
                segments.append((b0, count, dst._replace(planes=self.locate(dst.planes.data_ptr()))))
            else:
                fams = [Family(*self.locate(f.out), f.Hd, f.period, f.offset, f.count, f.keep_lo, f.keep_hi) for f in dst.array]
                segments.append((b0, count, dst._replace(array=fams)))
        self.calls.append(Call(first, last, B, height, None if src is None else src.storage_offset() // W, snippet_stride // W,
                               None if first == 0 else self.locate(ws[f"prev{first - 1}"].data_ptr()), segments))

    def head_device(self, feat, out, keep=None):
        self.calls.append("head")


def _replay(eng, n):
    """Walks the record of one forward_device call over n snippets; returns how many tail chunks it saw."""
    m = eng.model
    (H, W), nb, S = m.input_hw, len(m.filters), m.tail_from_block - 1
    P = H // 2
    geo, geo2 = shared_trunk.shared_geometry(eng, P * W), shared_trunk.tail_geometry(eng, P * W)
    s1, s2 = geo.scale, geo2.scale
    vals, cnt = {}, {}  # per planes name: [image][row] -> the recording row stored there, and how often a row was stored

    def target(name):
        if name not in vals:
            B, rows = eng.info(name)
            vals[name], cnt[name] = [[None] * rows for _ in range(B)], np.zeros((B, rows), int)
        return eng.info(name)

    t0 = chunks = 0
    nsnips = set()
    assert eng.calls[-1] == "head"
    for c in eng.calls[:-1]:
        if c.first == 0:  # level 1: one launch group of B images of c.height spectrogram rows, block S's tail through the families
            assert c.last == S and c.B * c.height <= CHUNK * H + c.height  # the row budget, exceeded by at most one image
            assert 0 <= c.src_row and c.src_row + (c.B - 1) * c.src_step + c.height <= (n + 1) * P  # nothing outside the snippets is read
            ((b0, count, win),) = c.scatter
            assert (b0, count) == (0, c.B) and isinstance(win, shared_trunk.Families) and 1 <= len(win.array) <= 4
            for f in win.array:
                B, rows = target(f.planes)
                assert f.image + f.count <= B and f.height == rows and 0 <= f.keep_lo < f.keep_hi <= rows
            for b in range(c.B):
                top = c.src_row + b * c.src_step - t0 * P  # the image's first spectrogram row, counted from the tail chunk's first
                assert top % s1 == 0 and top // s1 == win.base + b * win.img_step  # the row map speaks of the rows the image was read from
                _families_store(vals, cnt, [top // s1 + r for r in range(c.height // s1)], win, b, top // s1, win.array)
        elif c.last == nb:  # level 2: blocks S + 1 .. nb on all images of one kind, block nb's tail through one row map per window
            assert c.first == S + 1 and c.input[1] == 0
            B, rows = target(c.input[0])
            assert B == c.B and rows * s1 == c.height
            assert np.all(cnt[c.input[0]] == 1)  # every row of every level-2 image written exactly once
            assert [b0 for b0, _, _ in c.scatter] == [0] + list(np.cumsum([k for _, k, _ in c.scatter])[:-1]) and sum(k for _, k, _ in c.scatter) == B
            for b0, count, rm in c.scatter:
                assert isinstance(rm, shared_trunk.RowMap) and rm.planes[1] == 0 and (rm.rows, rm.period) == (geo2.rows, geo2.period)
                nsnips.add(rm.nsnip)
                carry = rm.planes[0]
                assert target(carry)[1] == geo2.rows
                for b in range(count):
                    r0 = rm.base + b * rm.img_step
                    assert vals[c.input[0]][b0 + b] == [r0 * s2 + y for y in range(rows)]  # the image holds the recording rows its window says
                    _scatter_store(vals[carry], cnt[carry], [r0 + r for r in range(rows // s2)], rm, r0, rm.rows, rm.period, rm.nsnip)
        else:  # the final conv over the tail chunk: block nb's planes are complete
            assert c.first == c.last == nb + 1 and c.input == (carry, 0) and nsnips == {c.B}
            nt = c.B
            assert np.all(cnt[carry][:nt] == 1) and not cnt[carry][nt:].any()  # every row of carry[0:nt] exactly once, no other row
            assert vals[carry][:nt] == [[sn * geo2.period + y for y in range(geo2.rows)] for sn in range(nt)]
            for name in cnt:
                assert np.all(cnt[name][: nt if name == carry else None] == 1), name  # no plane was stored into and left incomplete
            vals, cnt, nsnips = {}, {}, set()
            t0, chunks = t0 + nt, chunks + 1
    assert t0 == n and not vals
    return chunks


@pytest.mark.parametrize("n", [1, 2, 3, 17])
@pytest.mark.parametrize("k,hw", [(3, (192, 21)), (5, (320, 21))], ids=["k3", "k5"])  # the smallest planes both stages accept (tests/test_half_share.py)
def test_driver_writes_every_row_exactly_once(k, hw, n):
    eng = FakeEngine(k, hw)
    H, W = hw
    assert shared_trunk.shared_geometry(eng, H // 2 * W) is not None and shared_trunk.tail_geometry(eng, H // 2 * W) is not None
    src = torch.zeros(((n + 1) * (H // 2) + 37) * W)
    out = torch.empty((n, eng.model.out_steps, 7))
    shared_trunk.forward_device(eng, src, H // 2 * W, n, out, chunk=CHUNK)
    assert _replay(eng, n) == -(-n // 8)  # tail chunks of 8, 8 and 1 snippets at n = 17
    level1 = [c for c in eng.calls[:-1] if c.first == 0]
    if n == 17 and k == 3:  # launch groups that do not start at a window's first image, for super-snippets and for crops
        assert {c.scatter[0][2].img_step > 0 and c.scatter[0][2].base > 0 for c in level1} == {True, False}
        assert sum(c.B for c in level1 if c.height == shared_trunk.shared_geometry(eng, H // 2 * W).crop) == 2 * 17

