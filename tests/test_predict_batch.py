"""Several recordings in one detector pass, without a GPU: the layout planner (orcai_amd/batch.py) -- its properties over hand-picked and seeded random
lists of lengths at H = 736 --, the C-ABI tie of the two new symbols, and the CLI's channel option."""

import random

import pytest

from orcai_amd import batch as B

H, SHIFT, TPO = 736, 368, 16
EDGE = [735, 736, 737, 1103, 1104, 1471, 1472, 11251]
NEW_SYMBOLS = {"orcai_overlap_average_ragged": 10, "orcai_pcm_decode_planar": 7}


def _lists():
    rng = random.Random(7)
    out = [EDGE, EDGE[::-1], [736], [737, 736], [11251, 11251, 11251], [100, 735, 5], [736] * 40]
    for _ in range(30):
        out.append([rng.choice(EDGE + [rng.randrange(1, 30000)]) for _ in range(rng.randrange(1, 25))])
    return out


def check_batch(b: B.Batch, frames, max_frames):
    T = [frames[i] for i in b.items]
    assert list(b.frames) == T and len(b.items) == len(b.offsets) == len(b.snippets) == len(b.table) >= 1
    assert all(t >= H for t in T)
    assert b.offsets[0] == 0 and all(o % SHIFT == 0 for o in b.offsets)
    out_row = 0
    taken = set()
    for r, (o, t) in enumerate(zip(b.offsets, T)):
        n = (t - H) // SHIFT + 1  # predict.py:253
        assert b.snippets[r] == (o // SHIFT, n) and n >= 1
        for i in range(o // SHIFT, o // SHIFT + n):  # no real snippet's rows leave its recording, and no two recordings share a snippet
            assert o <= i * SHIFT and i * SHIFT + H <= o + t
            assert i not in taken
            taken.add(i)
        assert b.table[r] == (o // SHIFT, n, t // TPO, out_row)
        out_row += t // TPO
        if r + 1 < len(T):
            assert b.offsets[r + 1] == B.roundup(o + t, SHIFT) >= o + t
            between = b.snippets[r + 1][0] - (o // SHIFT + n)  # the snippets that straddle this boundary
            assert between in (1, 2), (t, between)
    assert b.out_rows == out_row
    assert b.rows == b.offsets[-1] + T[-1]
    assert b.n_total == (b.rows - H) // SHIFT + 1 == b.snippets[-1][0] + b.snippets[-1][1]  # none after the last recording
    assert b.junk == b.n_total - len(taken) and len(T) - 1 <= b.junk <= 2 * (len(T) - 1)
    assert all(0 < rows < SHIFT and row + rows in b.offsets for row, rows in b.gaps())
    assert b.rows <= max_frames or len(T) == 1


@pytest.mark.parametrize("max_frames", [1, 736, 3000, 20000, B.DEFAULT_MAX_FRAMES])
def test_planner_properties(max_frames):
    for frames in _lists():
        batches = B.plan_batches(frames, H, max_frames)
        for b in batches:
            check_batch(b, frames, max_frames)
        planned = [i for b in batches for i in b.items]
        short = B.short_recordings(frames, H)
        assert short == [i for i, t in enumerate(frames) if t < H]
        assert planned == [i for i in range(len(frames)) if i not in short]  # in order, each once, the short ones in no plan
        for b, nxt in zip(batches, batches[1:]):  # a batch closes only before the recording that would take it past max_frames
            assert B.roundup(b.rows, SHIFT) + frames[nxt.items[0]] > max_frames


def test_planner_by_hand():
    b, = B.plan_batches([736, 737, 1104, 1471, 2949], H, 10**6)
    assert b.offsets == (0, 736, 1840, 2944, 4416) and b.rows == 7365
    assert b.snippets == ((0, 1), (2, 1), (5, 2), (8, 2), (12, 7)) and b.n_total == 19 and b.junk == 6
    assert b.table == ((0, 1, 46, 0), (2, 1, 46, 46), (5, 2, 69, 92), (8, 2, 91, 161), (12, 7, 184, 252)) and b.out_rows == 436
    assert b.gaps() == [(1473, 367), (4415, 1)]
    # an over-long recording is a batch of its own, and so closes the one before it
    batches = B.plan_batches([736, 5000, 736, 736], H, 2000)
    assert [x.items for x in batches] == [(0,), (1,), (2, 3)]
    assert B.plan_batches([735, 10], H, 2000) == [] and B.short_recordings([735, 736, 10], H) == [0, 2]
    with pytest.raises(ValueError):
        B.layout([736, 735], H)
    with pytest.raises(ValueError):
        B.layout([], H)


def test_grouper_is_the_planner_one_recording_at_a_time():
    frames = [1104, 736, 2000, 736, 9000, 736]
    g, groups, cur = B.Grouper(H, 4000), [], []
    for i, t in enumerate(frames):
        if not g.fits(t):
            groups.append(tuple(cur))
            cur = []
            g.close()
        g.add(t)
        cur.append(i)
    groups.append(tuple(cur))
    assert groups == [b.items for b in B.plan_batches(frames, H, 4000)] == [(0, 1, 2), (3,), (4,), (5,)]


def test_new_symbols_in_header_table_and_library():
    import test_capi_symbols as S
    from orcai_amd import _native as N

    proto = S.header_prototypes()
    lib = N.lib()
    for name, nargs in NEW_SYMBOLS.items():
        assert name in proto and name in N._SIGNATURES, name
        assert len(proto[name][1]) == len(N._SIGNATURES[name][1]) == nargs, name
        assert getattr(lib, name) is not None


def test_cli_channel_is_a_number_or_all(monkeypatch, tmp_path):
    from click.testing import CliRunner

    import orcai_amd.predict as P
    from orcai_amd.cli import cli

    seen = []
    monkeypatch.setattr(P, "predict", lambda **kw: seen.append((kw["channel"], kw["batch_frames"])))
    wav = tmp_path / "a.wav"
    wav.write_bytes(b"")
    for args in (["-c", "all"], ["-c", "2"], [], ["--batch-frames", "675000"]):
        res = CliRunner().invoke(cli, ["predict", str(wav), *args])
        assert res.exit_code == 0, res.output
    assert seen == [("all", 0), (2, 0), (1, 0), (1, 675000)]
    assert CliRunner().invoke(cli, ["predict", str(wav), "-c", "both"]).exit_code != 0
    assert CliRunner().invoke(cli, ["predict", str(wav), "--batch-frames", "-1"]).exit_code != 0
