"""Layout of several recordings in one detector pass.  Exact integer geometry: no torch, no device.

``forward_device`` reads its input as one tall image with snippet i at row i * H/2, and a snippet's probabilities depend on its own rows only.  So
recordings laid end to end in one buffer, each starting at a row that is a multiple of H/2, go through the detector in one pass: recording r's
snippets are batch snippets o_r / (H/2) .. + n_r - 1, computed from its own rows.  The snippets that straddle the boundary between two recordings
(one or two per boundary) are computed and never read.

``layout`` places the recordings of one batch, ``Grouper`` decides where a batch closes, ``plan_batches`` is both over a list of lengths.
"""

from __future__ import annotations

from dataclasses import dataclass

DEFAULT_MAX_FRAMES = 675_000  # one hour of orcai-V1 spectrogram frames (48 kHz, hop 256): a 0.46 GB buffer of 171 bins


def roundup(x: int, m: int) -> int:
    return -(-x // m) * m


def num_snippets(T: int, H: int) -> int:
    """50 %-overlapping snippets of H rows in T rows (predict.py:253); <= 0: the recording is shorter than one snippet."""
    return (T - H) // (H // 2) + 1


def short_recordings(frames, H: int) -> list[int]:
    """Indices of the recordings too short for one snippet: they enter no plan (compute_aggregated_predictions' ValueError is theirs)."""
    return [i for i, T in enumerate(frames) if T < H]


@dataclass(frozen=True)
class Batch:
    """One detector pass.  Per recording, in buffer order: `items` (index into the planner's list), `frames` (T_r), `offsets` (o_r, first buffer
    row), `snippets` ((first batch snippet, n_r)) and `table` -- the rows of orcai_overlap_average_ragged: (first batch snippet, n_r, S_r output
    steps, first output row).  `rows`: rows of the buffer; `n_total`: snippets forward_device runs over it; `junk`: those that belong to no
    recording; `out_rows`: the sum of S_r."""

    items: tuple
    frames: tuple
    offsets: tuple
    snippets: tuple
    table: tuple
    rows: int
    n_total: int
    junk: int
    out_rows: int

    def gaps(self) -> list[tuple[int, int]]:
        """[(first row, rows)] between the end of one recording and the start of the next: what the caller zero-fills."""
        ends = [o + T for o, T in zip(self.offsets, self.frames)]
        return [(e, o - e) for e, o in zip(ends[:-1], self.offsets[1:]) if o > e]


def layout(frames, H: int, time_reduction: int = 16, items=None) -> Batch:
    """The recordings of ONE batch laid end to end: o_0 = 0, o_{r+1} = roundup(o_r + T_r, H/2).  Every T_r >= H."""
    frames = tuple(int(T) for T in frames)
    if not frames or H < 2 or H % 2 or time_reduction < 1:
        raise ValueError(f"layout of {len(frames)} recordings, H {H}, time reduction {time_reduction}")
    if min(frames) < H:
        raise ValueError(f"a recording of {min(frames)} frames is shorter than one snippet ({H}) and cannot be laid out")
    shift = H // 2
    offsets, snippets, table = [], [], []
    o = out_row = 0
    for T in frames:
        n, S = num_snippets(T, H), T // time_reduction
        offsets.append(o)
        snippets.append((o // shift, n))
        table.append((o // shift, n, S, out_row))
        out_row += S
        end = o + T
        o = roundup(end, shift)
    n_total = num_snippets(end, H)
    return Batch(tuple(items) if items is not None else tuple(range(len(frames))), frames, tuple(offsets), tuple(snippets), tuple(table), end, n_total,
                 n_total - sum(n for _, n in snippets), out_row)


class Grouper:
    """Where a batch closes: before the recording that would take the buffer past max_frames rows.  A recording longer than max_frames is a
    batch of its own.  Incremental, so that a caller can group recordings whose lengths it learns one by one."""

    def __init__(self, H: int, max_frames: int):
        if H < 2 or H % 2 or max_frames < 1:
            raise ValueError(f"H {H}, max_frames {max_frames}")
        self.shift, self.max_frames = H // 2, int(max_frames)
        self.next_offset = 0  # first row of the next recording; 0: the batch is empty

    def fits(self, T: int) -> bool:
        return self.next_offset == 0 or self.next_offset + T <= self.max_frames

    def add(self, T: int) -> None:
        self.next_offset = roundup(self.next_offset + T, self.shift)

    def close(self) -> None:
        self.next_offset = 0


def plan_batches(frames, H: int, max_frames: int = DEFAULT_MAX_FRAMES, time_reduction: int = 16) -> list[Batch]:
    """Consecutive recordings of `frames` (spectrogram rows each) grouped into batches of at most max_frames buffer rows.  Recordings with
    T < H are left out (short_recordings names them); Batch.items says which recordings a batch holds."""
    grouper = Grouper(H, max_frames)
    batches, members = [], []

    def close():
        if members:
            batches.append(layout([frames[i] for i in members], H, time_reduction, items=members))
            members.clear()
        grouper.close()

    for i, T in enumerate(frames):
        if T < H:
            continue
        if not grouper.fits(T):
            close()
        grouper.add(T)
        members.append(i)
    close()
    return batches
