"""
The sliced Wasserstein distance on the CPU: the reference (tests/sliced_ref.py, the contract of include/tdaeeg.h statement
for statement) against known answers, against scipy's one-dimensional Wasserstein distance direction by direction, and
against its own invariances; the kernel's sorting network and the whole route of csrc/sliced.hip restated in numpy; the
entry points that need no GPU.

The tolerance everywhere is the contract's: two orders of a sum of n non-negative terms differ by at most
2 (n - 1) 2^-53 relative, so (N + 1) 2^-52 for one direction and (N + M + 1) 2^-52 for the whole value.
"""
import ctypes
import os

import numpy as np
import pytest
from scipy.stats import wasserstein_distance

import sliced_ref as sr


def _pairs(n, seed, lo=0, hi=60):
    rng = np.random.default_rng(seed)
    return [(sr.random_diagram(rng, int(rng.integers(lo, hi)), k % 2 == 1), sr.random_diagram(rng, int(rng.integers(lo, hi)), k % 2 == 1))
            for k in range(n)], rng


def test_known_answers_exact():
    for a, b, want in sr.KNOWN:
        for order in ("seq", "fsum"):
            assert sr.sliced_wasserstein(a, b, sr.XY, order) == want
            assert sr.sliced_wasserstein(b, a, sr.XY, order) == want
        assert sr.kernel_route(a, b, sr.XY) == want
    L = [v[0] for v in sr.direction_values([[0, 1]], [[0, 2]], sr.XY)[0]]
    assert L == [0.5, 1.5]
    pairs, _ = _pairs(20, 1)
    from tda_eeg_audio_amd import utils
    dirs = utils.default_directions(7)
    for a, _b in pairs:
        assert sr.sliced_wasserstein(a, a, dirs) == 0.0 and sr.kernel_route(a, a, dirs) == 0.0
        assert sr.sliced_wasserstein(a, np.zeros((0, 2)), dirs) == sr.sliced_wasserstein(a, [[0.0, 0.0]], dirs)


def test_directions_against_scipy():
    """Independent anchor: the mean absolute difference of two sorted lists of equal length is scipy's 1-D Wasserstein
    distance of the two samples, so L_k = N * wasserstein_distance(proj A', proj B')."""
    from tda_eeg_audio_amd import utils
    pairs, _ = _pairs(30, 2, 0, 90)
    dirs = utils.default_directions(9)
    worst = 0.0
    for a, b in pairs:
        vals, N = sr.direction_values(a, b, dirs)
        for L, pu, pv in vals:
            w = N * wasserstein_distance(pu, pv)
            assert abs(L - w) <= (N + 1) * 2.0 ** -52 * L, (L, w, N)
            worst = max(worst, abs(L - w) / max(L, 1e-300))
    print("largest relative difference to scipy:", worst)


def test_reference_invariances():
    from tda_eeg_audio_amd import utils
    pairs, rng = _pairs(40, 3, 0, 80)
    for k, (a, b) in enumerate(pairs):
        dirs = utils.default_directions([1, 3, 16, 50][k % 4])
        M, N = len(dirs), sr.n_points(a, b)
        ref = sr.sliced_wasserstein(a, b, dirs)
        assert ref >= 0.0
        assert sr.sliced_wasserstein(b, a, dirs) == ref                              # |u - v| == |v - u|, same order
        assert abs(sr.sliced_wasserstein(a, b, dirs, "fsum") - ref) <= sr.tolerance(N, M, ref)
        pa, pb = a[rng.permutation(len(a))], b[rng.permutation(len(b))]
        assert abs(sr.sliced_wasserstein(pa, pb, dirs) - ref) <= sr.tolerance(N, M, ref)
        # the same point appended to both: its two projections and its two images pair off at distance 0
        extra = sr.random_diagram(rng, 1)
        more = sr.sliced_wasserstein(np.vstack([a.reshape(-1, 2), extra]), np.vstack([b.reshape(-1, 2), extra]), dirs)
        if len(a) and len(b):                                                        # (an empty side loses its {(0, 0)} instead)
            assert abs(more - ref) <= sr.tolerance(N + 2, M, max(ref, more)), (k, more, ref)


SORT_SIZES = list(range(1, 131)) + [255, 256, 257, 511, 512]


def test_sorting_network_against_numpy():
    rng = np.random.default_rng(4)
    for i, N in enumerate(SORT_SIZES):
        p = rng.standard_normal(N)
        if i % 2:                                                                    # ties, zeros of both signs
            p = np.round(p * 2) / 2
            p[p == 0.0] *= rng.choice([-1.0, 1.0], int((p == 0.0).sum()))
        x = sr.network_sort(p)
        V = sr.values_per_lane(N)
        assert len(x) == 64 * V and (V == 1) == (N <= 64) and 64 * V >= N > (0 if V == 1 else 32 * V)
        assert np.array_equal(x[:N], np.sort(p)) and np.isinf(x[N:]).all() and np.isfinite(x[:N]).all()
        assert sorted(x[:N].tobytes()[8 * q:8 * q + 8] for q in range(N)) == sorted(p.tobytes()[8 * q:8 * q + 8] for q in range(N))
        q = sr.network_sort(rng.permutation(p) + 0.25)
        with np.errstate(invalid="ignore"):
            t = np.abs(x - q)
        assert np.isnan(t[N:]).all() and np.isfinite(np.where(np.arange(len(t)) < N, t, 0.0).sum())


def test_kernel_route_against_reference():
    from tda_eeg_audio_amd import utils
    rng = np.random.default_rng(5)
    sizes = [(0, 0), (1, 1), (1, 2), (3, 60), (31, 33), (32, 33), (46, 122), (63, 65), (64, 65), (100, 156), (128, 129), (256, 256)]
    for k, (m, n) in enumerate(sizes):
        a, b = sr.random_diagram(rng, m, k % 2 == 1), sr.random_diagram(rng, n, k % 2 == 1)
        dirs = utils.default_directions([1, 3, 50, 128, 65][k % 5])
        ref, got = sr.sliced_wasserstein(a, b, dirs), sr.kernel_route(a, b, dirs)
        assert abs(got - ref) <= sr.tolerance(sr.n_points(a, b), len(dirs), ref), (m, n, got, ref)
        assert sr.kernel_route(b, a, dirs) == got
    assert np.isnan(sr.kernel_route(sr.random_diagram(rng, 256), sr.random_diagram(rng, 257), sr.XY))


def test_entry_points():
    from tda_eeg_audio_amd import _lib, engine, pipeline, utils
    for M in (1, 2, 50, 128):
        d = utils.default_directions(M)
        assert d.shape == (M, 2) and d.dtype == np.float64
        assert (np.abs(d[:, 0] ** 2 + d[:, 1] ** 2 - 1.0) <= 2.0 ** -52).all()
        assert d[0].tolist() == [np.cos(-np.pi / 2), np.sin(-np.pi / 2)]
        theta = -np.pi / 2 + np.arange(M) * np.pi / M
        assert np.array_equal(d, np.stack([np.cos(theta), np.sin(theta)], 1))
    with pytest.raises(ValueError):
        utils.default_directions(0)
    assert utils.sliced_wasserstein_kernel(0.0, 1.0) == 1.0
    G = np.array([[0.0, 2.0], [2.0, 0.0]])
    assert np.array_equal(utils.sliced_wasserstein_kernel(G, 0.5), np.exp(-G / (2 * 0.5 ** 2)))
    assert "positive-definite" in utils.sliced_wasserstein_kernel.__doc__
    assert _lib.MAX_DIRECTIONS == sr.MAX_DIRECTIONS == 128 and _lib.SW_MAX_POINTS == sr.SW_MAX_POINTS == 512 and pipeline.SLC_COLS == 2
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("tda_sliced_wasserstein_batch", "tda_sliced_wasserstein_batch_dev"):
        assert name in _lib.SYMBOLS and hasattr(lib, name)
    # the Wasserstein signatures with (dirs, n_dirs) in front of the outputs
    for name, base in (("tda_sliced_wasserstein_batch", "tda_wasserstein_batch"), ("tda_sliced_wasserstein_batch_dev", "tda_wasserstein_batch_dev")):
        res, args = _lib.SYMBOLS[base]
        k = args.index(ctypes.c_int, 8) + 1 if name.endswith("_dev") else len(args) - 2
        assert _lib.SYMBOLS[name] == (res, args[:k] + [ctypes.c_void_p, ctypes.c_int] + args[k:])
    for fn in (engine.sliced_wasserstein_batch, engine.sliced_wasserstein_dev, engine.sliced_wasserstein_gram, utils.safe_sliced_wasserstein):
        assert callable(fn)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "tdaeeg.h")).read()
    assert "tda_sliced_wasserstein_batch_dev(" in header and "tda_sliced_wasserstein_batch(" in header
    assert "#define TDA_MAX_DIRECTIONS 128" in header and "#define TDA_SW_MAX_POINTS  512" in header
    # direction tables are validated on the host, before any launch
    for bad in (np.zeros((0, 2)), np.zeros((129, 2)), np.zeros((3, 3)), np.zeros(4), [[1.0, np.nan]], [[np.inf, 0.0]]):
        with pytest.raises(_lib.TdaError):
            engine._directions(bad)
