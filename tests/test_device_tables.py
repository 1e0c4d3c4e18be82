"""orcai_amd/device_tables.py without a GPU: the integer counts behind the tables of `orcai test` (counts_from_arrays, the written specification of
orcai_test_counts) and the tables made from them, against the reference-made golden tables and against the host functions of orcai_amd/test.py."""

import json

import numpy as np
import pytest

from orcai_amd import _native as N
from orcai_amd.device_tables import confusion_table_from_counts, counts_from_arrays, misclassification_matrix, misclassification_tables_from_counts
from orcai_amd.test import _get_mask_for_rows_with_atmost_one_1, _stack_batch, compute_confusion_table, compute_misclassification_tables

CALLS = ["BR", "BUZZ", "HERDING", "PHS", "SS", "TAILSLAP", "WHISTLE"]


@pytest.fixture(scope="module")
def golden(golden_dir):
    with np.load(golden_dir / "test_tables.npz") as z:
        g = {k: z[k] for k in z.files}
    return g, json.loads((golden_dir / "test_tables.json").read_text())


def test_confusion_table_from_counts_is_the_golden_table(golden):
    g, want = golden
    conf, _ = counts_from_arrays(g["y_true"], g["y_pred"])
    table = confusion_table_from_counts(conf, CALLS)
    assert list(table.index) == want["confusion"]["index"] and list(table.columns) == want["confusion"]["columns"]
    assert np.array_equal(table.to_numpy(dtype=np.float64), g["confusion"], equal_nan=True)


def test_misclassification_tables_from_counts_are_the_golden_tables(golden):
    g, want = golden
    _, mis = counts_from_arrays(g["y_true"], g["y_pred"])
    assert mis[:, :, :, 1:].sum() > 0  # the golden batch has rows that share their unit among several columns
    tables = misclassification_tables_from_counts(mis, "true", "pred", CALLS)
    assert sorted(tables) == sorted(want["misclassification"])
    for key, table in tables.items():
        assert list(table.index) == want["misclassification"][key]["index"] and list(table.columns) == want["misclassification"][key]["columns"]
        assert np.array_equal(table.to_numpy(dtype=np.float64), g["mis_" + key], equal_nan=True), key


def random_case(L: int, rows: int = 3000, seed: int = 0, steps: int = 10):
    """(y_true, y_pred) f32 [rows / steps][steps][L]: mostly unlabelled rows, single labels, rows with two or more true labels, rows with many (up to
    all L) predictions, masked elements, one column (the last, for L > 1) that is never unmasked, a NaN and an exact 0.5 among the probabilities."""
    rng = np.random.default_rng(1000 * L + seed)
    y = np.zeros((rows, L), dtype=np.float32)
    p = (rng.random((rows, L)) * 0.45).astype(np.float32)
    kind = rng.random(rows)
    one = rng.integers(0, L, rows)
    single = (kind > 0.5) & (kind <= 0.8)
    y[single, one[single]] = 1
    y[kind > 0.8] = (rng.random((int((kind > 0.8).sum()), L)) < 0.3)  # zero, one or several true labels
    hit = rng.random(rows) < 0.6  # the prediction follows the truth ...
    p[hit] = np.where(y[hit] == 1, 0.9, p[hit])
    many = rng.random(rows) < 0.15  # ... or sets many columns
    p[many] = rng.random((int(many.sum()), L)).astype(np.float32)
    p[rng.random(rows) < 0.02] = 0.75  # every column predicted: n2 = L
    y[rng.random((rows, L)) < 0.1] = -1
    if L > 1:
        y[:, L - 1] = -1  # never unmasked: Total 0, NaN fractions
    p[0, 0], p[1, 0] = 0.5, np.nan
    return y.reshape(-1, steps, L), p.reshape(-1, steps, L)


def host_tables(y, p, names):
    return compute_confusion_table(y, p, names), compute_misclassification_tables(_stack_batch(y), _stack_batch((p >= 0.5).astype(int)), "true", "pred", names)


def sequential_matrices(y, p):
    """The un-rounded matrices of both directions as a sequential float64 sum of the 1 / n2 shares, row by row."""
    L = y.shape[-1]
    yi, pi = _stack_batch(y), _stack_batch((p >= 0.5).astype(int))
    out = []
    for m1, m2 in ((yi, pi), (pi, yi)):
        m = np.zeros((L + 1, L + 1))
        for r1, r2 in zip(m1, m2):
            a = np.flatnonzero(r1 == 1)
            if len(a) > 1 or (len(a) == 1 and r2[a[0]] == -1):
                continue
            src = a[0] if len(a) else L
            c = np.flatnonzero(r2 == 1)
            if len(c):
                m[src, c] += 1.0 / len(c)
            else:
                m[src, L] += 1.0
        out.append(m)
    return out


@pytest.mark.parametrize("L", [1, 3, 7, 33, 64])
def test_tables_from_counts_equal_the_host_functions(L, capsys):
    y, p = random_case(L)
    names = [f"c{i:02d}" for i in range(L)]
    conf, mis = counts_from_arrays(y, p)
    yi, pi = _stack_batch(y), _stack_batch((p >= 0.5).astype(int))
    if L > 2:  # the case holds what it is meant to hold
        assert (~_get_mask_for_rows_with_atmost_one_1(yi)).any() and (pi.sum(axis=1) == L).any() and mis[:, :, :, 2:].sum() > 0
    assert np.array_equal(conf.sum(axis=1), (y.reshape(-1, L) != -1).sum(axis=0))  # the four entries partition the unmasked elements
    want_conf, want_mis = host_tables(y, p, names)
    capsys.readouterr()  # the host route's "more than one 1" warning
    got_conf = confusion_table_from_counts(conf, names)
    assert list(got_conf.index) == list(want_conf.index) and list(got_conf.columns) == list(want_conf.columns)
    assert got_conf.to_numpy(dtype=np.float64).tobytes() == want_conf.to_numpy(dtype=np.float64).tobytes()  # bit for bit, NaN included
    if L > 1:
        assert got_conf.loc[names[-1], "Total"] == 0 and np.isnan(got_conf.loc[names[-1], "TP"])
    got_mis = misclassification_tables_from_counts(mis, "true", "pred", names)
    assert list(got_mis) == list(want_mis)
    for key in want_mis:
        assert list(got_mis[key].index) == list(want_mis[key].index) and list(got_mis[key].columns) == list(want_mis[key].columns)
        assert np.array_equal(got_mis[key].to_numpy(dtype=np.float64), want_mis[key].to_numpy(dtype=np.float64), equal_nan=True), key
    rows = y.shape[0] * y.shape[1]
    for d, seq in enumerate(sequential_matrices(y, p)):
        m = misclassification_matrix(mis[d])
        assert np.all(np.abs(m - seq) <= rows * 2.0**-52 * np.abs(seq)), d


def test_all_zero_input_is_all_nolabel():
    L = 5
    y, p = np.zeros((4, 6, L), dtype=np.float32), np.zeros((4, 6, L), dtype=np.float32)
    conf, mis = counts_from_arrays(y, p)
    assert np.array_equal(conf, np.tile(np.array([24, 0, 0, 0]), (L, 1)))
    want = np.zeros_like(mis)
    want[:, L, L, 0] = 24
    assert np.array_equal(mis, want)
    names = list("abcde")
    want_conf, want_mis = host_tables(y, p, names)
    assert confusion_table_from_counts(conf, names).equals(want_conf)
    got = misclassification_tables_from_counts(mis, "true", "pred", names)
    for key in want_mis:
        assert np.array_equal(got[key].to_numpy(dtype=np.float64), want_mis[key].to_numpy(dtype=np.float64), equal_nan=True)


def test_counts_symbol_is_declared_bound_and_exported():
    sig = N._SIGNATURES["orcai_test_counts"]
    assert sig[0] is N.C.c_int and sig[1] == [N.C.c_void_p, N.C.c_void_p, N.c_i64, N.C.c_int, N.C.c_float, N.C.c_void_p, N.C.c_void_p, N.C.c_void_p]
    assert "int orcai_test_counts(const float* p, const float* y, int64_t M, int L, float mask_value, int64_t* conf, int64_t* mis, void* stream);" in \
        (N.LIB_PATH.parent.parent / "include" / "orcai_hip.h").read_text()
    assert N.lib().orcai_test_counts is not None
