"""
The two written forms of the sublevel-set persistence of a 1-D signal (include/tdaeeg.h) against each other, against the
known answers and against an invariant that uses neither.  numpy only: no GPU, no library.
"""
import itertools

import numpy as np
import pytest

import sublevel_ref as ref

INF = np.inf


def _signals():
    rng = np.random.default_rng(20261020)
    out = []
    for n in list(range(1, 20)) + [63, 64, 65, 127, 250, 257, 513]:
        out.append(rng.standard_normal(n))
        out.append(rng.integers(0, 2, n).astype(np.float64))
        out.append(rng.integers(0, 3, n).astype(np.float64))
        out.append(np.round(np.cumsum(rng.standard_normal(n))))          # a rounded random walk: plateaus and ties
        out.append(np.round(np.cumsum(rng.standard_normal(n)) * 4) / 4)
    return out


SIGNALS = _signals()


def _same(a, b):
    return a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[0].shape == b[0].shape


def test_forms_agree_random_and_ties():
    for x in SIGNALS:
        assert _same(ref.sublevel_union_find(x), ref.sublevel_per_maximum(x)), x


@pytest.mark.parametrize("n", range(1, 8))
def test_forms_agree_exhaustive(n):
    for x in itertools.product((0.0, 1.0, 2.0), repeat=n):
        assert _same(ref.sublevel_union_find(x), ref.sublevel_per_maximum(x)), x


KNOWN = [
    ([3, 1, 4, 1, 5, 9, 2, 6], [(1, 4, 3, 2), (2, 9, 6, 5), (1, INF, 1, -1)]),
    ([1, 0, 1, 0, 1], [(0, 1, 3, 2), (0, INF, 1, -1)]),
    ([2, 2, 2], [(2, INF, 0, -1)]),
    ([5], [(5, INF, 0, -1)]),
]


@pytest.mark.parametrize("x, want", KNOWN)
def test_known_answers(x, want):
    for form in (ref.sublevel_union_find, ref.sublevel_per_maximum):
        rows, idx = form(x)
        got = [(r[0], r[1], int(i[0]), int(i[1])) for r, i in zip(rows, idx)]
        assert got == [tuple(map(float, w[:2])) + w[2:] for w in want]
        assert rows.dtype == np.float64 and idx.dtype == np.int32


def test_betti0_invariant():
    """For every threshold t: #{rows with birth <= t < death} == the number of connected runs of {x <= t}."""
    for x in SIGNALS:
        rows, _ = ref.sublevel_union_find(x)
        for t in np.unique(np.concatenate([x, [x.min() - 1.0, x.max() + 1.0], (x[:-1] + x[1:]) / 2])):
            on = x <= t
            runs = int(on[0]) + int(np.count_nonzero(on[1:] & ~on[:-1]))
            alive = int(np.count_nonzero((rows[:, 0] <= t) & (t < rows[:, 1])))
            assert alive == runs, (x, t)


def test_values_and_indices_are_the_inputs():
    for x in SIGNALS:
        rows, idx = ref.sublevel_union_find(x)
        assert np.array_equal(rows[:, 0], x[idx[:, 0]]) and np.array_equal(rows[:-1, 1], x[idx[:-1, 1]])
        assert (rows[:-1, 0] < rows[:-1, 1]).all()                       # birth == death is dropped
        assert idx[-1, 0] == int(np.argmin(x)) and idx[-1, 1] == -1 and rows[-1, 1] == INF


def test_row_bound():
    assert [ref.rows_bound(n) for n in (1, 2, 3, 4, 250, 4096)] == [1, 1, 2, 2, 125, 2048]
    for x in SIGNALS:
        assert ref.sublevel_union_find(x)[0].shape[0] <= ref.rows_bound(len(x))
    for n in (1, 2, 3, 4, 5, 64, 65, 250):                               # the alternating signal reaches it
        x = (np.arange(n) % 2).astype(np.float64) + 1e-3 * np.arange(n)
        assert ref.sublevel_union_find(x)[0].shape[0] == ref.rows_bound(n)


def test_row_order():
    for x in SIGNALS:
        rows, idx = ref.sublevel_union_find(x)
        keys = [(r[1], r[0], int(i[1])) for r, i in zip(rows[:-1], idx[:-1])]
        assert keys == sorted(keys) and len(set(keys)) == len(keys)


def test_batch_layout_and_flags():
    x = np.array([[3, 1, 4, 1, 5], [1, np.nan, 0, 2, 1], [0, 1, 0, 1, 0]], dtype=np.float64)
    dgm, cnt, idx, status = ref.sublevel_batch(x, cap=4)
    assert cnt.tolist() == [2, 0, 3] and status.tolist() == [0, 64, 0]
    assert np.isnan(dgm[1]).all() and (idx[1] == -1).all() and np.isnan(dgm[0, 2:]).all() and (idx[2, 3:] == -1).all()
