"""The f16 shared trunk (DESIGN 4.1 on the f16 path) without a device: the two row-map launchers are one contract stated in the header, the
ctypes table and the library, and HalfEngine's geometry is pure integer arithmetic."""

import re
from pathlib import Path

import pytest

from orcai_amd import _native as N
from orcai_amd.architectures import ResNet1DConv, ResNetLSTM
from orcai_amd.half import HalfEngine
from orcai_amd.overlap import shared_stage, tail_stage

ROOT = Path(__file__).resolve().parent.parent

ABI = {
    "orcai_h_pool_res_add_scatter": ["const void* s", "const void* prev", "int B", "int C", "int Cp", "int H", "int W", "int ksize", "const void* wrf", "const float* br",
                                     "void* out", "int Hd", "int nsnip", "int period", "int base", "int img_step", "int r_lo", "int r_hi", "int keep_lo", "int keep_hi",
                                     "void* stream"],
    "orcai_h_pool_res_add_scatter_families": ["const void* s", "const void* prev", "int B", "int C", "int Cp", "int H", "int W", "int ksize", "const void* wrf",
                                              "const float* br", "int base", "int img_step", "int r_lo", "int r_hi", "const orcai_h_row_family* fams", "int n_fams",
                                              "void* stream"],
}


@pytest.mark.parametrize("name", sorted(ABI))
def test_c_entry_point_is_declared_bound_and_exported(name):
    assert name in N.exported_symbols()
    header = re.sub(r"/\*.*?\*/", " ", (ROOT / "include" / "orcai_hip.h").read_text(), flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", header)
    assert m is not None
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert args == ABI[name]
    ret, argtypes = N._SIGNATURES[name]
    assert ret is N.C.c_int and len(argtypes) == len(args)
    for text, ct in zip(args, argtypes):
        assert ct is (N.C.c_void_p if "*" in text else N.C.c_int), (name, text, ct)
    assert getattr(N.lib(), name) is not None  # the library exports it (N.lib() raises on a missing symbol)


def test_row_family_struct_matches_the_header():
    header = (ROOT / "include" / "orcai_hip.h").read_text()
    m = re.search(r"typedef struct \{\s*void\* out;\s*int ([^;]*);\s*\} orcai_h_row_family;", header)
    assert m is not None
    assert [f for f, _ in N.RowFamily._fields_] == ["out"] + [x.strip() for x in m.group(1).split(",")]


def _engine(cls=ResNetLSTM, hw=(736, 171), k=3, **kw):
    m = cls((hw[0], hw[1], 1), 7, [30, 40, 50, 60], k, **kw)
    m.precision = "f16"
    return m, HalfEngine(m)


@pytest.mark.parametrize("cls,kw", [(ResNetLSTM, {"lstm_units": 128}), (ResNet1DConv, {})])
def test_geometry_at_half_overlap(cls, kw):
    m, eng = _engine(cls, **kw)
    H, W = m.input_hw
    assert eng.shared_geometry(H // 2 * W) == shared_stage(H, W, 3, 2, H // 2 * W) != None  # noqa: E711
    assert eng.tail_geometry(H // 2 * W) == tail_stage(H, W, 3, 3, 4, H // 2 * W) != None  # noqa: E711


def test_no_geometry_for_materialised_snippets_or_a_misaligned_height():
    m, eng = _engine()
    assert eng.shared_geometry(736 * 171) is None and eng.tail_geometry(736 * 171) is None  # model.predict: stride H * W
    m, eng = _engine(hw=(740, 171))  # H / 2 = 370 is no multiple of 4: a shared row would sit at two pooling phases
    assert eng.shared_geometry(370 * 171) is None and eng.tail_geometry(370 * 171) is None


def test_share_overlap_and_tail_from_block_mean_what_they_mean_for_f32():
    m, eng = _engine()
    s = 368 * 171
    m.share_overlap = False
    assert eng.shared_geometry(s) is None and eng.tail_geometry(s) is None
    m.share_overlap = True
    m.tail_from_block = 5  # the geometry of blocks 1 .. 4 in one level (forward_device shares only for 2 <= tail_from_block <= 4, as f32)
    assert eng.shared_geometry(s) == shared_stage(736, 171, 3, 4, s)
    m.tail_from_block = 2
    assert eng.shared_geometry(s).blocks == 1 and eng.tail_geometry(s) == tail_stage(736, 171, 3, 2, 4, s)


def test_smallest_plane_that_shares_four_blocks():
    """(192, 21) is the smallest height at k = 3, W = 21 that both stages accept with the default split (blocks 1-2 | 3-4):
    tests/test_half_share_gpu.py runs it end to end."""
    ok = [H for H in range(2, 400, 2) if shared_stage(H, 21, 3, 2, H // 2 * 21) and tail_stage(H, 21, 3, 3, 4, H // 2 * 21)]
    assert ok[0] == 192
    m, eng = _engine(hw=(192, 21))
    assert eng.shared_geometry(96 * 21) is not None and eng.tail_geometry(96 * 21) is not None
