"""Training augmentation on the GPU: SpecAugment-style time / frequency masks, a random level shift and mixing of two snippets of a
batch (``orcai_parameter["model"]["augment"]``).  The reference has none; absent or ``null`` means off and the training
dataset is used exactly as it is.

This module is the specification.  ``plan_ref`` / ``apply_ref`` state the semantics in numpy (uint64 / float32 arithmetic only);
``orcai_augment_plan`` / ``orcai_augment_apply`` (csrc/augment.hip) reproduce them bit for bit.

Draws.  Draw ``j`` of snippet ``b`` of a batch with 64-bit key ``k`` is ``z = finalise(k + 0x9E3779B97F4A7C15 * (b * DRAWS + j + 1))`` mod 2**64
with the splitmix64 finaliser of the Dropout masks (``dropout_mask_kernel``, train_head.hip).  An integer in [0, n) is
``((z >> 32) * n) >> 32``, a uniform f32 in [0, 1) is ``float32(z >> 40) * 2**-24``.  Every draw has a fixed slot (``DRAW_*``), so a
snippet's masks do not move when another option is switched on.

Batch key.  ``batch_key(seed, rank, epoch, batch)`` in Python integers mod 2**64: the seed (an int or a sequence of ints, as
``numpy.random.SeedSequence`` takes them; train() passes ``[SEED_ID_AUGMENT, orcai_parameter["seed"]]``) is reduced to one 64-bit word
``w`` by ``SeedSequence(seed).generate_state(1, uint64)``, then the three counters are absorbed one after the other:

    k = w;  for v in (rank, epoch, batch):  k = finalise(k + 0x9E3779B97F4A7C15 * (v + 1))

``finalise`` is a bijection of the 64-bit words and the multiplier is odd, so two keys that differ in exactly one of rank, epoch and
batch (each below 2**64) are different; keys that differ in more than one collide with probability 2**-64.  The same inputs give the same key.

Plan per snippet (``int32 plan[B][PLAN_WORDS]``, layout in include/orcai_hip.h and ``PLAN_*`` below), then per element of ``x[b][r][c]``:
mix (``fmaxf`` with the partner: the louder of the two in the dB domain), level shift (``fminf(fmaxf(v + shift, 0), 1)``, skipped entirely at
``level_shift == 0``), masks (``mask_value``).  Labels of a mixed snippet: 1 if either has 1, else -1 if either has -1, else 0; with
``mask_labels`` a label step whose rows all lie in the union of the time masks becomes -1 (MASK_VALUE: the loss skips it).
"""

from __future__ import annotations

import math
import numbers

import numpy as np

MAX_MASKS = 8  # ORCAI_AUGMENT_MAX_MASKS
DRAWS = 40  # ORCAI_AUGMENT_DRAWS: draw slots per snippet (35 in use)
PLAN_WORDS = 36  # ORCAI_AUGMENT_PLAN_WORDS
MAX_H, MAX_W = 4096, 1024  # ORCAI_AUGMENT_MAX_H / _MAX_W: the LDS mask images of orcai_augment_apply
FLAG_LEVEL_SHIFT, FLAG_MASK_LABELS = 1, 2  # ORCAI_AUGMENT_LEVEL_SHIFT / _MASK_LABELS
# plan words
PLAN_PARTNER, PLAN_SHIFT, PLAN_N_TIME, PLAN_N_FREQ, PLAN_TIME0, PLAN_FREQ0 = 0, 1, 2, 3, 4, 4 + 2 * MAX_MASKS  # (start, height) pairs from TIME0 / FREQ0
# draw slots
DRAW_MIX, DRAW_PARTNER, DRAW_SHIFT, DRAW_TIME0, DRAW_FREQ0 = 0, 1, 2, 3, 3 + 2 * MAX_MASKS  # (height, start) pairs from TIME0 / FREQ0

DEFAULTS = {"time_masks": 0, "time_mask_rows": 0, "freq_masks": 0, "freq_mask_bins": 0, "level_shift": 0.0, "mix_probability": 0.0, "mask_value": 0.0,
            "mask_labels": False}

_M64 = (1 << 64) - 1
_GOLDEN = 0x9E3779B97F4A7C15


def validate(spec, H: int, W: int) -> dict | None:
    """The checked spec with every key present, or None when augmentation is off.  Every error is a ValueError that names the key."""
    if spec is None:
        return None
    if not isinstance(spec, dict):
        raise ValueError(f"augment: expected a dict or null, got {type(spec).__name__}")
    for k in spec:
        if k not in DEFAULTS:
            raise ValueError(f"augment: unknown key {k!r} (known: {', '.join(DEFAULTS)})")
    out = {**DEFAULTS, **spec}
    for k, hi in (("time_masks", MAX_MASKS), ("time_mask_rows", int(H)), ("freq_masks", MAX_MASKS), ("freq_mask_bins", int(W))):
        v = out[k]
        if isinstance(v, bool) or not isinstance(v, numbers.Integral):
            raise ValueError(f"augment: {k} must be an integer, got {v!r}")
        if not 0 <= v <= hi:
            raise ValueError(f"augment: {k} = {v} is outside 0...{hi}")
        out[k] = int(v)
    for k in ("level_shift", "mix_probability", "mask_value"):
        v = out[k]
        if isinstance(v, bool) or not isinstance(v, numbers.Real) or not math.isfinite(v):
            raise ValueError(f"augment: {k} must be a finite number, got {v!r}")
        if k != "mask_value" and not 0.0 <= v <= 1.0:
            raise ValueError(f"augment: {k} = {v} is outside 0...1")
        out[k] = float(v)
    if not math.isfinite(float(np.float32(out["mask_value"]))):
        raise ValueError(f"augment: mask_value = {out['mask_value']} is not a finite float32")
    if not isinstance(out["mask_labels"], (bool, np.bool_)):
        raise ValueError(f"augment: mask_labels must be true or false, got {out['mask_labels']!r}")
    out["mask_labels"] = bool(out["mask_labels"])
    if out["time_masks"] > 0 and out["time_mask_rows"] == 0:
        raise ValueError("augment: time_masks > 0 needs time_mask_rows > 0")
    if out["freq_masks"] > 0 and out["freq_mask_bins"] == 0:
        raise ValueError("augment: freq_masks > 0 needs freq_mask_bins > 0")
    return out


def _finalise(z: int) -> int:
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def seed_word(seed) -> int:
    """The 64-bit word a seed (int or sequence of ints) stands for."""
    return int(np.random.SeedSequence(seed).generate_state(1, dtype=np.uint64)[0])


def _key(word: int, rank: int, epoch: int, batch: int) -> int:
    k = word & _M64
    for v in (rank, epoch, batch):
        k = _finalise((k + _GOLDEN * (int(v) + 1)) & _M64)
    return k


def batch_key(seed, rank: int, epoch: int, batch: int) -> int:
    """The key of batch `batch` of epoch `epoch` on rank `rank` (formula and guarantees: module docstring)."""
    return _key(seed_word(seed), rank, epoch, batch)


def _draws(key: int, B: int) -> np.ndarray:
    """uint64 [B][DRAWS]: every draw of a batch."""
    with np.errstate(over="ignore"):
        idx = np.arange(B * DRAWS, dtype=np.uint64).reshape(B, DRAWS) + np.uint64(1)
        z = np.uint64(key) + np.uint64(_GOLDEN) * idx
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def _int_below(z: np.ndarray, n) -> np.ndarray:
    return (((z >> np.uint64(32)) * np.asarray(n).astype(np.uint64)) >> np.uint64(32)).astype(np.int64)


def _uniform(z: np.ndarray) -> np.ndarray:
    return (z >> np.uint64(40)).astype(np.float32) * np.float32(2.0**-24)


def plan_ref(key: int, B: int, H: int, W: int, spec: dict) -> np.ndarray:
    """int32 [B][PLAN_WORDS]: what orcai_augment_plan writes."""
    s = validate(spec, H, W) or dict(DEFAULTS)
    z = _draws(key, B)
    b = np.arange(B, dtype=np.int64)
    plan = np.zeros((B, PLAN_WORDS), dtype=np.int32)
    plan[:, PLAN_PARTNER] = -1
    if B > 1:
        mixed = _uniform(z[:, DRAW_MIX]) < np.float32(s["mix_probability"])
        partner = (b + 1 + _int_below(z[:, DRAW_PARTNER], B - 1)) % B
        plan[:, PLAN_PARTNER] = np.where(mixed, partner, -1)
    u = _uniform(z[:, DRAW_SHIFT])
    plan[:, PLAN_SHIFT] = ((u + u - np.float32(1.0)) * np.float32(s["level_shift"])).astype(np.float32).view(np.int32)
    plan[:, PLAN_N_TIME], plan[:, PLAN_N_FREQ] = s["time_masks"], s["freq_masks"]
    for count, largest, extent, draw0, word0 in ((s["time_masks"], s["time_mask_rows"], H, DRAW_TIME0, PLAN_TIME0),
                                                 (s["freq_masks"], s["freq_mask_bins"], W, DRAW_FREQ0, PLAN_FREQ0)):
        for k in range(count):
            height = _int_below(z[:, draw0 + 2 * k], largest + 1)
            plan[:, word0 + 2 * k] = _int_below(z[:, draw0 + 2 * k + 1], extent - height + 1)
            plan[:, word0 + 2 * k + 1] = height
    return plan


def mask_images(plan_row: np.ndarray, H: int, W: int) -> tuple[np.ndarray, np.ndarray]:
    """bool [H], bool [W]: the union of a snippet's time masks and of its frequency masks."""
    rows, cols = np.zeros(H, dtype=bool), np.zeros(W, dtype=bool)
    for image, count, word0 in ((rows, plan_row[PLAN_N_TIME], PLAN_TIME0), (cols, plan_row[PLAN_N_FREQ], PLAN_FREQ0)):
        for k in range(int(count)):
            start, height = int(plan_row[word0 + 2 * k]), int(plan_row[word0 + 2 * k + 1])
            image[start : start + height] = True
    return rows, cols


def apply_ref(x: np.ndarray, y: np.ndarray, plan: np.ndarray, spec: dict) -> tuple[np.ndarray, np.ndarray]:
    """What orcai_augment_apply writes for x f32 [B][H][W], y f32 [B][S][L] under `plan`; float32 arithmetic only, inputs untouched."""
    x, y = np.asarray(x, dtype=np.float32), np.asarray(y, dtype=np.float32)
    B, H, W = x.shape
    S = y.shape[1]
    if H % S:
        raise ValueError(f"{H} spectrogram rows are not a multiple of the {S} label steps")
    s = validate(spec, H, W) or dict(DEFAULTS)
    factor = H // S
    x_out, y_out = np.empty_like(x), np.empty_like(y)
    one, mask = np.float32(1.0), np.float32(-1.0)
    for b in range(B):
        partner = int(plan[b, PLAN_PARTNER])
        v, lab = x[b], y[b]
        if partner >= 0:
            v = np.fmax(v, x[partner])  # fmaxf
            p = y[partner]
            lab = np.where((lab == one) | (p == one), one, np.where((lab == mask) | (p == mask), mask, np.float32(0.0))).astype(np.float32)
        if s["level_shift"] > 0:
            shift = plan[b, PLAN_SHIFT : PLAN_SHIFT + 1].view(np.float32)[0]
            v = np.fmin(np.fmax(v + shift, np.float32(0.0)), np.float32(1.0))
        rows, cols = mask_images(plan[b], H, W)
        x_out[b] = np.where(rows[:, None] | cols[None, :], np.float32(s["mask_value"]), v)
        if s["mask_labels"]:
            lab = np.where(rows.reshape(S, factor).all(axis=1)[:, None], mask, lab)
        y_out[b] = lab
    return x_out, y_out


class Augmenter:
    """``Augmenter(spec, seed, rank)(x, y, epoch, batch) -> (x_aug, y_aug)`` on CUDA tensors x f32 [B][H][W], y f32 [B][S][L]: two launches on the
    current stream (plan, apply), out of place, no host synchronisation.  The entry for a training loop of one's own around OrcaiModule."""

    def __init__(self, spec: dict, seed=None, rank: int = 0):
        if spec is None:
            raise ValueError("augment: Augmenter needs a spec (augmented() passes a dataset through when it is None)")
        self.spec, self.rank = spec, int(rank)
        self.word = seed_word(seed)
        self._checked: dict = {}

    def key(self, epoch: int, batch: int) -> int:
        return _key(self.word, self.rank, epoch, batch)

    def __call__(self, x, y, epoch: int, batch: int):
        import torch

        from orcai_amd import _native as N

        if x.dim() != 3 or y.dim() != 3 or x.shape[0] != y.shape[0] or x.dtype != torch.float32 or y.dtype != torch.float32 or not x.is_cuda or not y.is_cuda:
            raise ValueError(f"augment: expected CUDA float32 x [B][H][W] and y [B][S][L], got {tuple(x.shape)} {x.dtype} and {tuple(y.shape)} {y.dtype}")
        B, H, W = (int(v) for v in x.shape)
        S, L = int(y.shape[1]), int(y.shape[2])
        s = self._checked.get((H, W))
        if s is None:
            s = self._checked[(H, W)] = validate(self.spec, H, W)
        x, y = x.contiguous(), y.contiguous()
        plan = torch.empty((B, PLAN_WORDS), dtype=torch.int32, device=x.device)
        x_out, y_out = torch.empty_like(x), torch.empty_like(y)
        lib, st = N.lib(), N.stream_ptr()
        N.check(lib.orcai_augment_plan(self.key(epoch, batch), B, H, W, s["time_masks"], s["time_mask_rows"], s["freq_masks"], s["freq_mask_bins"],
                                       s["level_shift"], s["mix_probability"], plan.data_ptr(), st), "orcai_augment_plan")
        flags = (FLAG_LEVEL_SHIFT if s["level_shift"] > 0 else 0) | (FLAG_MASK_LABELS if s["mask_labels"] else 0)
        N.check(lib.orcai_augment_apply(x.data_ptr(), y.data_ptr(), plan.data_ptr(), x_out.data_ptr(), y_out.data_ptr(), B, H, W, S, L, s["mask_value"], flags, st),
                "orcai_augment_apply")
        return x_out, y_out


class AugmentedDataset:
    """A training dataset seen through an Augmenter: same ``__len__``, counts its own epochs (one per ``__iter__``) and batches."""

    def __init__(self, dataset, spec: dict, seed=None, rank: int = 0, first_epoch: int = 0):
        self.dataset, self.augmenter, self.epoch = dataset, Augmenter(spec, seed, rank), int(first_epoch)

    def __len__(self) -> int:
        return len(self.dataset)

    def __iter__(self):
        epoch = self.epoch
        self.epoch += 1
        for i, (x, y) in enumerate(self.dataset):
            yield self.augmenter(x, y, epoch, i)


def augmented(dataset, spec, seed=None, rank: int = 0, first_epoch: int = 0):
    """`dataset` itself when `spec` is None; otherwise an iterable of the same length that yields the Augmenter's outputs, batch `i` of its
    epoch `e` (counted from `first_epoch`) under ``batch_key(seed, rank, e, i)``.  For training datasets only: validation and test data are never augmented."""
    if spec is None:
        return dataset
    return AugmentedDataset(dataset, spec, seed, rank, first_epoch)
