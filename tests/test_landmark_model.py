"""
The reference of the landmark Rips route (tests/landmark_ref.py) against known answers and theory.  No GPU.

Stability (the reason r_cover is returned): for each of H0 and H1 the landmark diagram lies within bottleneck distance
2 * r_cover of the diagram of the whole cloud.  The bound is exact for the real-valued filtration; the oracle ranks
float32 distances of values up to 2, so every diagram coordinate may be off by a float32 rounding (2^-24 * 2 = 1.2e-7)
of the value the theorem speaks about: the slack 1e-6 is a few of those.
"""
import numpy as np
import pytest

import bottleneck_ref
import landmark_ref as ref


def test_known_answer_on_a_line():
    X = (np.arange(9) / 8.0)[:, None]
    idx, lam, rc = ref.greedy(X, 5)
    assert idx.tolist() == [0, 8, 4, 2, 6]
    assert lam.tolist() == [1.0, 0.5, 0.25, 0.25, 0.125] and rc == 0.125
    # min-max normalisation of this cloud is the identity, bit for bit
    from oracle import port
    assert np.array_equal(port.minmax_normalise(X), X)


@pytest.fixture(scope="module")
def cases():
    out = []
    for name, win, tau, dim, sub, n_perm in ref.stability_cases():
        X = ref.cloud_of(win, tau, dim, sub)
        assert len(X) == ref.n_takens(len(win), dim, tau, sub)
        out.append((name, X, n_perm, ref.landmarks(X, n_perm)))
    return out


def test_case_sizes(cases):
    assert [(len(X), k) for _, X, k, _ in cases] == [(246, 128), (238, 64), (590, 128), (85, 17)]


def test_invariants(cases):
    for name, X, n_perm, (lm, idx, lam, rc, n_lm, n_full) in cases:
        assert n_lm == n_perm and n_full == len(X) and idx[0] == 0, name
        assert (np.diff(lam) <= 0).all(), name                     # insertion radii never grow
        assert rc == lam[-1] and rc > 0, name
        assert len(set(idx.tolist())) == n_perm, name              # distinct points while the radius is positive
        assert np.array_equal(lm, X[idx]), name
        # r_cover is the directed Hausdorff distance cloud -> landmarks, here from coordinate differences: the Gram form
        # -2 x.y + |x|^2 + |y|^2 of the definition carries an absolute error of a few 2^-53 * dim in d^2
        h = ref.directed_hausdorff(X, lm)
        assert abs(h - rc) <= 1e-12 * max(1.0, 1.0 / rc), (name, h, rc)
        # every point is within r_cover of a landmark, and the landmarks are lambda-separated: a greedy permutation
        d = np.sqrt(((lm[:, None] - lm[None]) ** 2).sum(-1))
        for t in range(1, n_perm):
            assert d[t, :t].min() >= lam[t - 1] - 1e-12, (name, t)


def test_identity_case():
    rng = np.random.default_rng(5)
    for P, n_perm in ((3, 3), (17, 17), (40, 64), (128, 128)):
        X = rng.random((P, 3))
        lm, idx, lam, rc, n_lm, n_full = ref.landmarks(X, n_perm)
        assert idx.tolist() == list(range(P)) and n_lm == P == n_full and rc == 0.0 and not lam.any()
        assert np.array_equal(lm, X)
    assert ref.landmarks(rng.random((1025, 2)), 64) is None


def test_ties_and_exhaustion():
    """An integer signal with values 0..4: at most 125 distinct points in 3-D, many equal distances.  The arg-max takes
    the lowest index; once every point is covered at distance 0, index 0 is picked again."""
    s = np.random.default_rng(3).integers(0, 5, 250).astype(np.float64)
    X = ref.cloud_of(s, 1)
    distinct = len(np.unique(X, axis=0))
    assert len(X) == 248 and distinct < 128
    idx, lam, rc = ref.greedy(X, 64)
    assert rc > 0 and len(set(idx.tolist())) == 64
    assert (np.diff(lam) == 0).any()                               # a tie at a positive distance
    idx, lam, rc = ref.greedy(X, 128)
    assert rc == 0.0 and (lam[distinct - 1:] == 0).all() and lam[distinct - 2] > 0
    assert (idx[distinct:] == 0).all()                             # index 0 again: duplicate landmark rows


def test_stability_bound(cases):
    for name, X, n_perm, (lm, *_rest, rc, _n_lm, _n_full) in cases:
        full = ref.diagrams(X)
        land = ref.diagrams(lm)
        for k in (0, 1):
            B = bottleneck_ref.bottleneck_ref(land[k], full[k])
            print(f"{name}: H{k} bottleneck {B:.6f}  2 r_cover {2 * rc:.6f}  ratio {B / (2 * rc):.3f}")
            assert B <= 2 * rc + 1e-6, (name, k, B, rc)


def test_pivot_order_changes_no_float32_distance(cases):
    """Upstream slices its pivot rows; the diagrams here are the cloud path's on the landmark rows.  The two add the
    squared norms in the other order: float64 entries differ, the float32 values Rips ranks do not."""
    for name, X, n_perm, _ in cases:
        n64, n32, n = ref.pivot_order_counts(X, n_perm)
        print(f"{name}: {n64} of {n} float64 entries differ, {n32} float32")
        assert n32 == 0, name
