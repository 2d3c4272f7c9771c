"""
The definition of the Euler characteristic curves on the CPU (tests/euler_ref.py): its two statements and the restatement
of the kernel's mask route agree, known answers, the float32 presence rule, NaN and unsorted grids, the relation to the
Betti numbers of the diagrams, and the two forms of the group mean.  No GPU.
"""
from math import comb

import numpy as np
import pytest

import euler_ref as er
from oracle import brute


def _sym(n, rng, values=None):
    d = rng.random((n, n)) * 2 if values is None else rng.choice(values, size=(n, n))
    d = np.tril(d, -1)
    return (d + d.T).astype(np.float32)


def _all_three(keys, grid, thresh=2.0, K=3):
    a = er.counts_comb(keys, grid, thresh, K)
    assert a.dtype == np.int32 and a.shape == (K + 2, len(grid))
    assert np.array_equal(a, er.counts_mat(keys, grid, thresh, K))
    assert np.array_equal(a, er.counts_masks(keys, grid, thresh, K))
    return a


@pytest.mark.parametrize("n", [1, 2, 3, 4, 9, 13])
def test_three_statements_agree_on_random_matrices(n):
    rng = np.random.default_rng(100 + n)
    grid = np.linspace(0.0, 2.0, 7)
    for K in (1, 2, 3):
        out = _all_three(_sym(n, rng), grid, 1.7, K)
        assert (out[0] == n).all()


@pytest.mark.parametrize("values", [[0.5], [0.25, 0.5, 1.0]])
def test_three_statements_agree_on_ties(values):
    rng = np.random.default_rng(7)
    keys = _sym(11, rng, values)
    grid = np.array([0.0, 0.25, 0.3, 0.5, 1.0, 3.0])
    out = _all_three(keys, grid)
    if len(values) == 1:                                   # all keys equal: nothing below 0.5, everything from it on
        assert np.array_equal(out[:4, 2], [11, 0, 0, 0])
        assert np.array_equal(out[:4, 3], [comb(11, j + 1) for j in range(4)])


def test_known_answers():
    n = 10
    full = np.full((n, n), 0.5, np.float32)
    out = _all_three(full, [1.0])
    assert np.array_equal(out[:4, 0], [comb(n, j + 1) for j in range(4)])
    assert out[4, 0] == comb(n, 1) - comb(n, 2) + comb(n, 3) - comb(n, 4)
    # an n-cycle with only its sides present
    cyc = np.full((n, n), 1.5, np.float32)
    for v in range(n):
        cyc[v, (v + 1) % n] = cyc[(v + 1) % n, v] = 0.5
    assert np.array_equal(_all_three(cyc, [1.0])[:, 0], [n, n, 0, 0, 0])
    # the octahedron: every pair but the three antipodal ones
    octa = np.full((6, 6), 0.5, np.float32)
    for v in range(3):
        octa[v, v + 3] = octa[v + 3, v] = 1.5
    assert np.array_equal(_all_three(octa, [1.0])[:, 0], [6, 12, 8, 0, 2])
    # a grid point below every key
    assert np.array_equal(_all_three(full, [0.25])[:, 0], [n, 0, 0, 0, n])


def test_float32_presence_rule():
    d = np.array([[0.0, 1.0 + 2.0 ** -30], [1.0 + 2.0 ** -30, 0.0]])
    keys = er.keys_dm(d)
    assert keys[1, 0] == np.float32(1.0)                   # the key is the float32 value
    assert er.counts_comb(keys, [1.0], K=1)[1, 0] == 1
    k = np.float32(0.7)
    keys = np.array([[0, k], [k, 0]], np.float32)
    grid = [float(k), np.nextafter(np.float64(k), -np.inf)]
    assert list(_all_three(keys, grid, K=1)[1]) == [1, 0]
    # thresh below a key removes the edge at every grid point; (float)thresh is what is compared
    assert list(_all_three(keys, [0.7, 1.0, 5.0], thresh=0.6, K=1)[1]) == [0, 0, 0]
    assert list(_all_three(keys, [1.0], thresh=float(k) + 1e-12, K=1)[1]) == [1]


def test_nan_and_unsorted_grid():
    rng = np.random.default_rng(3)
    keys = _sym(8, rng)
    keys[5, 2] = keys[2, 5] = np.nan
    grid = np.array([1.5, np.nan, 0.2, 2.0, 0.9])
    out = _all_three(keys, grid)
    assert np.array_equal(out[:, 1], [8, 0, 0, 0, 8])      # a NaN grid point holds no edge
    assert out[1, 3] == comb(8, 2) - 1                     # the NaN key is never present
    order = np.argsort(grid[[0, 2, 3, 4]])
    sub = out[:, [0, 2, 3, 4]][:, order]
    assert (np.diff(sub[1]) >= 0).all()                    # each column stands for itself, whatever the order


def test_symmetrise_rules():
    rng = np.random.default_rng(4)
    d = rng.random((5, 5)) * 2 - 0.5
    k1, k0 = er.keys_dm(d, True), er.keys_dm(d, False)
    for a in range(5):
        for b in range(a):
            assert k1[a, b] == np.float32(max((d[a, b] + d[b, a]) / 2, 0.0))
            assert k0[a, b] == np.float32(d[b, a])


def test_betti_inequality_against_the_diagrams():
    from oracle import port
    from tda_eeg_audio_amd import synth
    win = synth.eeg_windows(1, seed=5, windows_per_recording=1)[0][:20]
    _, dist = port.corr_dist(win)
    keys = er.keys_dm(dist)
    grid = np.linspace(0.0, 2.0, 33)
    out = er.counts_mat(keys, grid, 2.0, 2)
    h0, h1 = brute.rips_brute(keys, 2.0)
    equal = 0
    for g, t in enumerate(grid):
        lhs = int(out[0, g]) - int(out[1, g]) + int(out[2, g])
        rhs = er.betti(h0, t) - er.betti(h1, t)
        assert lhs >= rhs, (t, lhs, rhs)
        if out[2, g] == 0:
            assert lhs == rhs, (t, lhs, rhs)
            equal += 1
    assert equal >= 1 and out[2].max() > 0


def test_group_means():
    rng = np.random.default_rng(6)
    blocks = rng.integers(-10_000_000, 10_700_000, size=(9, 5, 4)).astype(np.int32)
    seg = np.array([0, 0, 1, 6, 9], np.int32)              # sizes 0, 1, 5, 3
    status = np.array([0, 0, 4, 0, 16, 0, 0, 4, 4], np.int32)
    for st, mask in ((None, 0), (status, 4 | 16), (status, 4)):
        a, b = er.mean_np(blocks, seg, st, mask), er.mean_exact(blocks, seg, st, mask)
        assert a.tobytes() == b.tobytes()
        assert np.isnan(a[0]).all() and not np.isnan(a[1:3]).any()
    all_skipped = er.mean_np(blocks, np.array([0, 2, 3], np.int32), status, 4)          # the second group is window 2 alone
    assert not np.isnan(all_skipped[0]).any() and np.isnan(all_skipped[1]).all()
    own = er.mean_np(blocks)
    assert own.shape == (9, 5, 4) and np.array_equal(own, blocks.astype(np.float64))
    assert er.mean_np(blocks, seg, status, 4)[3].tobytes() == blocks[6:7].astype(np.float64)[0].tobytes()
