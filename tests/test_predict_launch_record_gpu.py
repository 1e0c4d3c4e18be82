"""predict_spectrogram's launcher calls -- names and every scalar argument, in order -- against the record of the commit before the shared-trunk
driver was lifted out of the two engines (tests/golden/predict_launch_record.json, written by tools/record_predict_launches.py on that commit):
both precisions on five layouts that between them take every route of the driver.  The planning is host-side Python whose only output is these
calls, so an equal record is the same work on the device."""

import importlib.util
import json
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
_spec = importlib.util.spec_from_file_location("record_predict_launches", ROOT / "tools" / "record_predict_launches.py")
tool = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(tool)


@pytest.fixture(scope="module")
def golden():
    doc = json.loads(tool.GOLDEN.read_text())
    assert set(doc["records"]) == {f"{name}/{p}" for name in tool.SCENARIOS for p in tool.PRECISIONS}
    assert doc["about"]["scenarios"] == json.loads(json.dumps({k: dict(input_hw=hw, attributes=at, predict_kwargs=kw) for k, (hw, at, kw) in tool.SCENARIOS.items()}))
    return doc["records"]


@pytest.mark.parametrize("precision", tool.PRECISIONS)
@pytest.mark.parametrize("name", list(tool.SCENARIOS))
def test_launch_record_is_the_parents(golden, name, precision):
    want = golden[f"{name}/{precision}"]
    got = json.loads(json.dumps(tool.record(name, precision)))
    assert len(want) > 30
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"launch {i}"
    assert len(got) == len(want)


def test_the_scenarios_take_every_route(golden):
    """What the committed record itself shows of each route: a re-recorded file cannot quietly stop covering one."""

    def names(key):
        return [fn for fn, _ in golden[key]]

    for p, h in (("f32", ""), ("f16", "h_")):
        fam, one = f"orcai_{h}pool_res_add_scatter_families", f"orcai_{h}pool_res_add_scatter"
        assert fam in names(f"192x21_two_levels/{p}") and fam in names(f"736x171_benchmarked/{p}")
        chunks = golden[f"192x21_three_tail_chunks/{p}"]
        assert [a[-8] for fn, a in chunks if fn == one] == [8] * 8 + [1] * 3  # nsnip: tail chunks of 8, 8 and 1, four / four / three level-2 windows
        assert any(a[-5] > 0 and a[-4] > 0 for fn, a in chunks if fn == fam)  # base, img_step: a launch group that starts inside a window
        assert one in names(f"200x21_one_level/{p}") and fam not in names(f"200x21_one_level/{p}")
        assert not any("scatter" in fn for fn in names(f"196x21_unshared_chunk5/{p}"))
    # 17 snippets in chunks of 5: f32 runs blocks 1-2 per chunk and blocks 3-4 over all 17 (two phases), f16 the whole trunk per chunk
    assert [a[0] for fn, a in golden["196x21_unshared_chunk5/f32"] if fn == "orcai_pool_res_add"] == [5, 5] * 3 + [2, 2] + [17, 17]
    assert [a[0] for fn, a in golden["196x21_unshared_chunk5/f16"] if fn == "orcai_h_pool_res_add"] == [5] * 12 + [2] * 4
