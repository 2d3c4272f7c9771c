"""
The prepared route of the sliced Wasserstein distance, restated on the CPU (tests/sliced_matrix_ref.py; no GPU): the
co-rank merge is the sorted list of the union, value for value, also where a tie rule could matter; and prepare + merge +
the pair kernel's order of additions returns the bytes of sliced_ref.kernel_route.
"""
import numpy as np
import pytest

import sliced_matrix_ref as smr
import sliced_ref as sr
from tda_eeg_audio_amd import utils


def _same_values(X, Y):
    got = smr.corank_merge(X, Y)
    want = np.sort(np.concatenate([X, Y]))
    assert got.shape == want.shape and (got == want).all(), (got, want)              # (== : -0.0 equals 0.0)
    return got


def test_corank_merge_random_sizes():
    rng = np.random.default_rng(41)
    for nx, ny in [(1, 1), (1, 2), (2, 1), (1, 511), (511, 1), (63, 1), (64, 64), (65, 63), (100, 156), (256, 256), (37, 34)]:
        X, Y = np.sort(rng.uniform(-1, 1, nx)), np.sort(rng.uniform(-1, 1, ny))
        _same_values(X, Y)
        _same_values(np.sort(np.round(X * 4) / 4), np.sort(np.round(Y * 4) / 4))      # many ties within and across


def test_corank_merge_adversarial():
    rng = np.random.default_rng(42)
    A, B = sr.random_diagram(rng, 9, ties=True), sr.random_diagram(rng, 14, ties=True)
    # all ties: direction (0, 0) projects every point to 0.0
    PA, PB = smr.prepare(A, [[0.0, 0.0]]), smr.prepare(B, [[0.0, 0.0]])
    assert (_same_values(PA[0, 0], PB[0, 1]) == 0.0).all() and (_same_values(PB[0, 0], PA[0, 1]) == 0.0).all()
    # one list entirely below the other, both ways round: the co-rank is 0 or the whole list
    lo, hi = np.sort(rng.uniform(0, 1, 7)), np.sort(rng.uniform(2, 3, 5))
    assert (_same_values(lo, hi) == np.concatenate([lo, hi])).all()
    assert (_same_values(hi, lo) == np.concatenate([lo, hi])).all()
    _same_values(np.array([1.0]), np.array([1.0]))
    _same_values(np.array([2.0]), np.array([1.0]))
    _same_values(np.array([1.0]), np.array([2.0]))
    # equal values across the two lists: direction (1, 0), a birth of A equal to an h of B
    A2 = np.array([[0.5, 0.75], [0.25, 1.0], [0.5, 0.5]])
    B2 = np.array([[0.25, 0.75], [0.0, 0.5], [0.5, 0.5]])                             # h = 0.5, 0.25, 0.5
    PA, PB = smr.prepare(A2, sr.XY[:1]), smr.prepare(B2, sr.XY[:1])
    assert set(PA[0, 0]) & set(PB[0, 1])
    _same_values(PA[0, 0], PB[0, 1])
    _same_values(PB[0, 0], PA[0, 1])
    # -0.0 against 0.0: equal under ==, whichever of the two the merge returns, and no t_i can tell them apart
    got = _same_values(np.array([-0.0, 0.0, 1.0]), np.array([-0.0, -0.0, 0.0]))
    assert (got[:5] == 0.0).all() and got[5] == 1.0
    assert smr.prepared_route(smr.prepare([[0.0, 1.0]], [[-1.0, 0.0]]), smr.prepare([[0.0, 2.0]], [[-1.0, 0.0]])) == \
        sr.kernel_route([[0.0, 1.0]], [[0.0, 2.0]], [[-1.0, 0.0]])


def test_prepare_is_the_sorted_projections_of_the_header():
    rng = np.random.default_rng(43)
    dirs = utils.default_directions(5)
    for n in (0, 1, 2, 63, 64, 65, 129):
        D = sr.random_diagram(rng, n, ties=n % 2 == 1)
        if n > 2:
            D = np.insert(D, 1, [0.25, np.inf], axis=0)
        P = smr.prepare(D, dirs)
        C = sr.clean(D)
        h = 0.5 * (C[:, 0] + C[:, 1])
        for k, (c, s) in enumerate(dirs):
            assert (P[k, 0] == np.sort((c * C[:, 0]) + (s * C[:, 1]))).all()
            assert (P[k, 1] == np.sort((c * h) + (s * h))).all()


SIZES = [(0, 0), (1, 1), (0, 5), (3, 60), (31, 33), (32, 33), (63, 65), (64, 65), (100, 156), (128, 129), (200, 312), (256, 256)]


@pytest.mark.parametrize("M", [1, 3, 50, 128])
def test_prepared_route_returns_the_pair_kernels_bytes(M):
    rng = np.random.default_rng(44 + M)
    dirs = utils.default_directions(M)
    sizes = SIZES if M == 50 else SIZES[:6]
    for i, (m, n) in enumerate(sizes):
        A, B = sr.random_diagram(rng, m, ties=i % 2 == 0), sr.random_diagram(rng, n, ties=i % 2 == 0)
        PA, PB = smr.prepare(A, dirs), smr.prepare(B, dirs)
        want = sr.kernel_route(A, B, dirs)
        got = smr.prepared_route(PA, PB)
        assert np.float64(got).tobytes() == np.float64(want).tobytes(), (m, n, got, want)
        assert np.float64(smr.prepared_route(PB, PA)).tobytes() == np.float64(want).tobytes()
    assert np.isnan(smr.prepared_route(smr.prepare(sr.random_diagram(rng, 257), dirs), smr.prepare(sr.random_diagram(rng, 256), dirs)))


def test_known_cases_are_exact():
    for A, B, want in sr.KNOWN:
        assert smr.prepared_route(smr.prepare(A, sr.XY), smr.prepare(B, sr.XY)) == want


def test_matrix_entry_rule():
    NP, TL = smr.NO_PAIR, smr.TOO_LARGE
    assert smr.matrix_entry([], []) == (pytest.approx(float("nan"), nan_ok=True), 0, 0)
    assert smr.matrix_entry([1.0, 2.0, np.nan], [0, 0, NP]) == (1.5, 2, 0)
    m, n, f = smr.matrix_entry([1.0, np.nan, 4.0], [0, TL, 0])
    assert (m, n, f) == (2.5, 3, TL)
    m, n, f = smr.matrix_entry([1.0, np.nan, 4.0, 8.0], [0, NP, 0, 0])              # a degenerate partner in the middle: the
    assert (m, n, f) == (2.5, 3, 0)                                                   # first 3 positions are the pairs
    vals = np.random.default_rng(45).uniform(0, 1, 15)
    assert smr.matrix_entry(vals, np.zeros(15, np.int32))[0] == np.mean(vals)
