"""The tables of ``orcai test`` from integer counts taken on the GPU: the host half of orcai_test_counts.

The kernel (csrc/test_tables.hip) reduces every batch of probabilities and labels to two small integer arrays and adds them to the arrays of the
batches before it:

  conf  int64 [L][4] = {TN, FP, FN, TP} per label over the unmasked elements (compute_confusion_table's four sums);
  mis   int64 [2][L+1][L+1][L]: per direction (0 true_pred, 1 pred_true) how many rows went from source row `src` to column `c` while sharing their
        unit among n2 columns, at index [d][src][c][n2 - 1] (row and column L are NOLABEL).

`counts_from_arrays` is the same arithmetic in numpy -- the written specification and the reference of the tests.  The `*_from_counts` functions turn
counts into the DataFrames of orcai_amd/test.py; `TestCounts` is the device-side accumulator of one dataset.

The ONE place where this route is not the host route's arithmetic: the host sums 1 / n2 row by row (np.add.at), here a cell is the sum over n of
count / n, n ascending, in float64.  Before rounding the two differ by at most about rows * 2^-53 relative, so a written cell can differ only when
m / row_sum lies within that distance of a 3-decimal rounding boundary; they are identical whenever every counted n2 is a power of two (every
share is then exact).  The confusion table is integer arithmetic up to the final divisions and is the same bit for bit.
"""

from __future__ import annotations

import numpy as np
import pandas as pd

from orcai_amd.auxiliary import MASK_VALUE


def counts_from_arrays(y_true, y_pred, mask_value=MASK_VALUE) -> tuple[np.ndarray, np.ndarray]:
    """(conf int64 [L][4], mis int64 [2][L+1][L+1][L]) of labels y_true and probabilities y_pred, [..., L] each, as include/orcai_hip.h states them
    for orcai_test_counts."""
    y = np.asarray(y_true)
    L = y.shape[-1]
    y = y.reshape(-1, L)
    pred = np.asarray(y_pred).reshape(-1, L) >= 0.5  # NaN: not predicted
    unmasked = y != mask_value
    conf = np.empty((L, 4), dtype=np.int64)
    for k, (truth, p) in enumerate(((0, False), (0, True), (1, False), (1, True))):  # TN, FP, FN, TP
        conf[:, k] = (unmasked & (y == truth) & (pred == p)).sum(axis=0)
    yi, pi = y.astype(int), pred.astype(int)  # _stack_batch's truncation
    mis = np.zeros((2, L + 1, L + 1, L), dtype=np.int64)
    rows = np.arange(y.shape[0])
    for d, (m1, m2) in enumerate(((yi, pi), (pi, yi))):
        ones1, ones2 = m1 == 1, m2 == 1
        n1, n2 = ones1.sum(axis=1), ones2.sum(axis=1)
        a = np.argmax(ones1, axis=1)  # the single 1 of the row (valid where n1 == 1)
        src = np.where(n1 == 1, a, L)
        use = ((n1 == 1) & (m2[rows, a] != -1)) | (n1 == 0)  # n1 > 1: the at-most-one-1 mask drops the row
        r, c = np.nonzero(ones2 & (use & (n2 > 0))[:, None])
        np.add.at(mis[d], (src[r], c, n2[r] - 1), 1)
        none = use & (n2 == 0)
        np.add.at(mis[d], (src[none], L, 0), 1)
    return conf, mis


def confusion_table_from_counts(conf: np.ndarray, label_names: list[str]) -> pd.DataFrame:
    """compute_confusion_table's DataFrame from conf int64 [L][4] = {TN, FP, FN, TP}: the same expressions on the same integers."""
    from orcai_amd.test import _confusion_entry

    conf = np.asarray(conf)
    assert conf.shape == (len(label_names), 4), conf.shape
    table = {name: _confusion_entry(*(int(v) for v in conf[idx])) for idx, name in enumerate(label_names)}
    return pd.DataFrame.from_dict(table, orient="index").sort_values(by="Total", ascending=False)


def misclassification_matrix(mis_d: np.ndarray) -> np.ndarray:
    """f64 [L+1][L+1]: m[src][c] = sum over n = 1 .. L (ascending) of mis_d[src][c][n - 1] / n, the un-rounded matrix of one direction."""
    m = np.zeros(mis_d.shape[:2], dtype=np.float64)
    for n in range(1, mis_d.shape[2] + 1):
        m += mis_d[:, :, n - 1].astype(np.float64) / n
    return m


def misclassification_tables_from_counts(mis: np.ndarray, suffix_1: str, suffix_2: str, label_names: list[str]) -> dict:
    """compute_misclassification_tables' dict from mis int64 [2][L+1][L+1][L] (direction 0: suffix_1 -> suffix_2)."""
    from orcai_amd.test import _misclassification_frame

    L = len(label_names)
    mis = np.asarray(mis)
    assert mis.shape == (2, L + 1, L + 1, L), mis.shape
    return {
        "_".join([suffix_1, suffix_2]): _misclassification_frame(misclassification_matrix(mis[0]), suffix_1, suffix_2, label_names),
        "_".join([suffix_2, suffix_1]): _misclassification_frame(misclassification_matrix(mis[1]), suffix_2, suffix_1, label_names),
    }


class TestCounts:
    """conf and mis of one dataset on the device: zeroed once, `add` queues orcai_test_counts for one batch on the current stream (no copy, no
    synchronisation), `result` copies both back in one synchronising transfer."""

    __test__ = False  # not a pytest class

    def __init__(self, num_labels: int, device):
        import torch

        from orcai_amd import _native as N

        if not 1 <= num_labels <= 64:
            raise ValueError(f"orcai_test_counts takes 1..64 labels, got {num_labels}")
        self.L = L = int(num_labels)
        self._buf = torch.empty(4 * L + 2 * (L + 1) * (L + 1) * L, dtype=torch.int64, device=device)  # conf, then mis: one copy back
        N.check(N.lib().orcai_zero_fill(N.ptr(self._buf), 8 * self._buf.numel(), N.stream_ptr()), "orcai_zero_fill")

    def add(self, probs, labels, mask_value: float = MASK_VALUE) -> None:
        """probs, labels: contiguous float32 cuda tensors [..., L] of one shape."""
        import torch

        from orcai_amd import _native as N

        for name, t in (("probs", probs), ("labels", labels)):
            if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
                raise ValueError(f"TestCounts.add: {name} must be a contiguous float32 cuda tensor")
        if probs.shape != labels.shape or probs.shape[-1] != self.L or probs.device != self._buf.device:
            raise ValueError(f"TestCounts.add: probs {tuple(probs.shape)} and labels {tuple(labels.shape)} must be one shape [..., {self.L}] on {self._buf.device}")
        N.check(N.lib().orcai_test_counts(N.ptr(probs), N.ptr(labels), probs.numel() // self.L, self.L, float(mask_value), N.ptr(self._buf),
                                          self._buf.data_ptr() + 8 * 4 * self.L, N.stream_ptr()), "orcai_test_counts")

    def result(self) -> tuple[np.ndarray, np.ndarray]:
        """(conf int64 [L][4], mis int64 [2][L+1][L+1][L]) on the host."""
        L = self.L
        host = self._buf.cpu().numpy()
        return host[: 4 * L].reshape(L, 4), host[4 * L :].reshape(2, L + 1, L + 1, L)
