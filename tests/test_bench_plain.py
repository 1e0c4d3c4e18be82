"""bench.py's plain run (the headline line alone) and --dump-outputs: the line carries the headline fields and nothing that needs runs of its
own (those come with --full), --steps sets the timed steps, and the dumped arrays are float32 / float64, within 64 MB, and the same from run
to run with the same arguments."""

import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))


def test_help_lists_full_and_dump_outputs():
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "--full" in r.stdout and "--dump-outputs" in r.stdout


def test_dump_outputs_dtypes_and_limit(tmp_path):
    import bench

    bench.dump_outputs({"f16": np.ones(3, np.float16), "f64": np.arange(3.0), "i64": np.arange(3)}, str(tmp_path / "a"))
    assert np.load(tmp_path / "a" / "f16.npy").dtype == np.float32
    assert np.load(tmp_path / "a" / "f64.npy").dtype == np.float64
    i64 = np.load(tmp_path / "a" / "i64.npy")
    assert i64.dtype == np.float64 and i64.tolist() == [0.0, 1.0, 2.0]
    with pytest.raises(SystemExit):
        bench.dump_outputs({"big": np.zeros((bench.OUTPUT_BYTES_MAX // 4) + 1, np.float32)}, str(tmp_path / "b"))
    assert not (tmp_path / "b").exists()


@pytest.mark.gpu
def test_plain_line_and_outputs_repeat(tmp_path):
    lines, dirs = [], [tmp_path / "run0", tmp_path / "run1"]
    for d in dirs:
        r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--dump-outputs", str(d)],
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        out = [ln for ln in r.stdout.strip().splitlines() if ln.startswith("{")]
        assert len(out) == 1, r.stdout[-2000:]
        lines.append(json.loads(out[0]))
    d = lines[0]
    assert d["metric"] == "audio_seconds_per_s" and d["unit"] == "audio-s/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
    assert d["steps"] == 2 and d["warmup"] == 1 and d["ms_per_step"] > 0 and d["value"] > 0
    assert not {"roofline", "secondary", "secondary2", "cpu_baseline"} & set(d)  # --full only
    names = {"aggregated_predictions", "overlap_count", "label_start", "label_stop", "label_call"}
    for run in dirs:
        files = {f.stem: np.load(f) for f in run.glob("*.npy")}
        assert set(files) == names
        assert all(a.dtype in (np.float32, np.float64) for a in files.values())
        assert sum(f.stat().st_size for f in run.glob("*.npy")) <= 64 << 20
    a, b = (np.load(run / "aggregated_predictions.npy") for run in dirs)
    assert a.shape == (675001 // 16, 7) and np.isfinite(a).all()
    np.testing.assert_allclose(a, b, rtol=0, atol=1e-6)
    np.testing.assert_array_equal(np.load(dirs[0] / "overlap_count.npy"), np.load(dirs[1] / "overlap_count.npy"))
