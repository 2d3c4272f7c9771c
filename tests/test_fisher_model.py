"""
The CPU reference of the persistence Fisher distance (tests/fisher_ref.py) against a 40-digit evaluation of the same float64
arguments, known answers, scikit-learn's Gaussian kernel with the acos form, and the argument checks of the Python layer.
No GPU.
"""
import math

import numpy as np
import pytest

import fisher_ref as pf
from tda_eeg_audio_amd import _lib, engine, pipeline

U = pf.U


def _diagram(rng, n, h0=False, scale=1.0):
    """n float32-valued rows with d > b; h0: every birth 0."""
    b = np.zeros(n, np.float32) if h0 else rng.uniform(0, scale, n).astype(np.float32)
    d = (b + rng.uniform(0.01, scale, n).astype(np.float32)).astype(np.float32)
    return np.stack([b, d], axis=1).astype(np.float64)


def test_args_are_the_engines():
    for sigma in (0.05, 1, 2.5, np.float32(0.5)):
        assert engine.fisher_args(sigma) == pf.args(sigma)
    assert engine.fisher_args(0.5) == -2.0
    for bad in (0, 0.0, -1.0, np.inf, -np.inf, np.nan, True, False, None, "1.0", (1.0,), 1e-170, 1e200):
        with pytest.raises(_lib.TdaError):
            engine.fisher_args(bad)
    assert pf.PF_MAX_POINTS == _lib.PF_MAX_POINTS


MP_CASES = [(0, 1, 0.05, False), (1, 1, 1.0, False), (3, 5, 0.3, False), (17, 9, 0.1, False), (20, 12, 0.05, False),
            (32, 32, 1.0, False), (23, 41, 0.3, True), (40, 24, 0.1, True), (31, 33, 0.05, True), (7, 0, 0.5, True)]


def test_reference_against_forty_digits():
    """exp at 40 digits on the FLOAT64 arguments (dx * dx + dy * dy) * ninv, everything after it at 40 digits:
    |ref - exact| <= 8 * 2^-53 (N <= 64 here; on 15 seeded cases with N up to 168 the worst seen was 2.0)."""
    import mpmath
    mp = mpmath.mp.clone()
    mp.dps = 40
    to_mp = np.frompyfunc(mp.mpf, 1, 1)
    mp_exp, mp_sqrt = np.frompyfunc(mp.exp, 1, 1), np.frompyfunc(mp.sqrt, 1, 1)
    rng = np.random.default_rng(7)
    worst = 0.0
    for m, n, sigma, h0 in MP_CASES:
        A, B = _diagram(rng, m, h0), _diagram(rng, n, h0)
        ninv = pf.args(sigma)
        P, Q = pf.lists(A, B)
        T = np.concatenate([P, Q])
        rp = mp_exp(to_mp(pf.arguments(T, P, ninv))).sum(axis=1)
        rq = mp_exp(to_mp(pf.arguments(T, Q, ninv))).sum(axis=1)
        a, b = mp_sqrt(rp / rp.sum()), mp_sqrt(rq / rq.sum())
        c2 = ((a - b) ** 2).sum()
        exact = 2 * mp.asin(min(mp.sqrt(c2) / 2, mp.mpf(1)))
        for name, fn in (("numpy", pf.distance), ("fsum", pf.distance_fsum)):
            err = float(abs(mp.mpf(fn(A, B, ninv)) - exact)) / U
            worst = max(worst, err)
            assert err <= 8.0, (m, n, sigma, h0, name, err)
    print("worst |ref - exact| / 2^-53:", worst)


def test_known_answers():
    rng = np.random.default_rng(8)
    empty = np.zeros((0, 2))
    assert pf.distance(empty, empty, -0.5) == 0.0 and pf.distance_fsum(empty, empty, -0.5) == 0.0
    junk = np.array([[0.0, np.inf], [np.nan, 0.5], [0.25, np.nan]])
    assert pf.distance(junk, empty, -0.5) == 0.0
    for n in (1, 5, 46, 127):
        A = _diagram(rng, n)
        for sigma in (0.05, 1.0):
            assert pf.distance(A, A.copy(), pf.args(sigma)) == 0.0
            assert pf.distance_fsum(A, A.copy(), pf.args(sigma)) == 0.0
            # non-finite rows never enter, wherever they sit
            assert pf.distance(np.insert(A, [0, n // 2, n], junk, axis=0), np.concatenate([junk, A]), pf.args(sigma)) == 0.0
    for L, sigma in pf.ONE_POINT_CASES:
        want = pf.one_point_closed_form(L, sigma)
        for b in (0.0, 0.375):
            x = np.array([[b, b + L]])
            for fn in (pf.distance, pf.distance_fsum):
                assert abs(fn(x, empty, pf.args(sigma)) - want) <= 8 * U, (L, sigma, b)
                assert abs(fn(empty, x, pf.args(sigma)) - want) <= 8 * U, (L, sigma, b)


def test_range_and_symmetry():
    rng = np.random.default_rng(9)
    for m, n, sigma, h0 in [(0, 3, 0.1, False), (5, 5, 0.01, False), (46, 127, 0.05, True), (46, 127, 1.0, True), (20, 9, 1e-3, False),
                            (33, 64, 0.3, False), (12, 30, 10.0, False)]:
        A, B = _diagram(rng, m, h0), _diagram(rng, n, h0)
        ninv = pf.args(sigma)
        for fn in (pf.distance, pf.distance_fsum):
            d, e = fn(A, B, ninv), fn(B, A, ninv)
            assert 0.0 <= d <= math.pi / 2 and 0.0 <= e <= math.pi / 2
            assert abs(d - e) <= 16 * U, (m, n, sigma, d - e)


def test_independent_route_rbf_kernel_and_acos():
    """Row sums of sklearn's rbf_kernel and the acos form of the paper; on pairs with d >= 0.1 the two forms agree to
    1e-13 (near 0 the acos form loses half its digits, which is why the contract is written through the chord)."""
    from sklearn.metrics.pairwise import rbf_kernel
    rng = np.random.default_rng(10)
    seen = 0
    for m, n, sigma, h0 in [(46, 127, 0.05, True), (46, 127, 0.3, True), (20, 17, 0.1, False), (9, 30, 0.5, False), (64, 1, 0.2, False),
                            (3, 0, 0.1, False)]:
        A, B = _diagram(rng, m, h0), _diagram(rng, n, h0)
        P, Q = pf.lists(A, B)
        T = np.concatenate([P, Q])
        gamma = 1.0 / (2.0 * sigma * sigma)
        rp, rq = rbf_kernel(T, P, gamma=gamma).sum(axis=1), rbf_kernel(T, Q, gamma=gamma).sum(axis=1)
        want = math.acos(min(float(np.sqrt((rp / rp.sum()) * (rq / rq.sum())).sum()), 1.0))
        d = pf.distance(A, B, pf.args(sigma))
        if d >= 0.1:
            seen += 1
            assert abs(d - want) <= 1e-13, (m, n, sigma, d - want)
    assert seen >= 4


def test_step_outputs_fisher():
    assert pipeline.step_outputs() == [] and pipeline.step_outputs(fisher=None) == []
    (o,) = pipeline.step_outputs(fisher=1)
    assert o.name == "pf" and o.shape == (pipeline.PF_COLS,) == (2,) and o.params == 1.0 and isinstance(o.params, float)
    assert pipeline.step_outputs(fisher=o.params)[0].params == o.params
    for bad in (True, 0, 0.0, -0.5, np.nan, np.inf, "1", (1.0,), 1e-170):
        with pytest.raises(ValueError):
            pipeline.step_outputs(fisher=bad)
    everything = pipeline.step_outputs(correlations=True, bottleneck=True, landscapes=(np.linspace(0, 1, 4), 2),
                                       images=(np.linspace(0, 1, 3), np.linspace(0, 1, 4), 0.1, 1), sliced=np.eye(2),
                                       wasserstein_q=(2, "l2"), frechet=(4, 2), kernel_distance=("pss", 0.1), fisher=0.25)
    assert [o.name for o in everything] == ["corr", "bott", "land", "img", "slc", "wq", "fm", "kd", "pf"]
    assert everything[8] == pipeline.Output("pf", (pipeline.PF_COLS,), 0.25)
    assert set(("f0", "f1", "fs0", "fs1")) <= set(pipeline.Workspace.PAIR_BUFFERS)
    assert pipeline.Workspace.pf is None and pipeline.Workspace.f0 is None and pipeline.Workspace.fisher is None
