"""
The bottleneck distance on the CPU: the block-matrix reference against exhaustive search, the route the kernel takes
(two cover problems per probe, bisection on bit patterns snapped to costs: bottleneck_ref.bottleneck_two_cover) against
the reference, the known answers, and the presence of the entry points.  All comparisons are `==`: every function
returns one of the pair's costs, each a single correctly rounded float64 operation.
"""
import ctypes
import os

import numpy as np

import bottleneck_ref as br


def test_reference_equals_brute_force_and_two_cover():
    pairs = br.small_pairs(400, seed=5)
    assert sum(len(a) + len(b) == 0 for a, b in pairs) > 0          # empty against empty is among them
    for a, b in pairs:
        ref = br.bottleneck_ref(a, b)
        assert ref == br.bottleneck_brute(a, b), (a, b)
        assert ref == br.bottleneck_two_cover(a, b), (a, b)


def test_two_cover_equals_reference_on_large_pairs():
    rng = np.random.default_rng(6)
    probes = []
    for k in range(60):
        M, N = rng.integers(1, 60), rng.integers(1, 130)
        a, b = br.random_diagram(rng, M, k % 3 == 0), br.random_diagram(rng, N, k % 3 == 0)
        if k % 4 == 0:                                              # H0-like: every birth 0
            a[:, 0] = 0.0
            b[:, 0] = 0.0
        assert br.bottleneck_ref(a, b) == br.bottleneck_two_cover(a, b, probes), k
    print("probes per pair: max", max(probes), "mean", np.mean(probes))
    assert max(probes) <= 64


def test_known_answers():
    for a, b, want in br.KNOWN:
        assert br.bottleneck_ref(a, b) == want
        assert br.bottleneck_two_cover(a, b) == want
        assert br.bottleneck_ref(b, a) == want


def test_entry_points_exist():
    from tda_eeg_audio_amd import _lib, engine, utils
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("tda_bottleneck_batch", "tda_bottleneck_batch_dev"):
        assert name in _lib.SYMBOLS
        assert hasattr(lib, name)
    assert _lib.SYMBOLS["tda_bottleneck_batch"] == _lib.SYMBOLS["tda_wasserstein_batch"]
    assert _lib.SYMBOLS["tda_bottleneck_batch_dev"] == _lib.SYMBOLS["tda_wasserstein_batch_dev"]
    assert callable(utils.safe_bottleneck) and callable(engine.bottleneck_batch) and callable(engine.bottleneck_dev)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "tdaeeg.h")).read()
    assert "tda_bottleneck_batch_dev(" in header and "tda_bottleneck_batch(" in header
