"""
Persistence landscapes and Betti curves on the CPU: the numpy reference (landscape_ref) against a brute-force restatement,
the known answers, the properties of the definition, the route the kernel takes (K sorted registers per grid point,
insertion by (max, min) pairs) against the reference, the sequential group sum against np.mean, and the presence of the
entry points.  All comparisons are exact: every value is one correctly rounded float64 operation or a selection.
"""
import os

import numpy as np
import pytest

import landscape_ref as lr

GRID9 = np.linspace(0.0, 2.0, 9)
FOUR = np.array([[0.0, 1.0], [0.0, 2.0], [0.5, 1.5], [0.0, np.inf]])


def _diagrams(seed, n=60):
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        k = int(rng.integers(0, 40))
        out.append(lr.random_diagram(rng, k, kind="f32" if i % 2 else "f64", h0=i % 5 == 0, n_inf=(i % 3 == 0) * min(k, 2)) if k
                   else np.zeros((0, 2)))
    return out


def test_reference_equals_brute_force():
    grids = [np.linspace(0.0, 2.0, 33), np.array([0.3]), np.sort(np.random.default_rng(1).uniform(-0.5, 2.5, 20))[::-1].copy()]
    for i, d in enumerate(_diagrams(2)):
        for K in (1, 3, 8):
            g = grids[i % len(grids)]
            assert np.array_equal(lr.diagram_vector(d, g, K), lr.diagram_vector_brute(d, g, K)), (i, K)


def test_known_answers():
    one = lr.diagram_vector([[0.0, 1.0]], GRID9, 2)
    assert np.array_equal(one[0], [0, .25, .5, .25, 0, 0, 0, 0, 0])
    assert np.array_equal(one[1], np.zeros(9))
    assert np.array_equal(one[2], [1, 1, 1, 1, 0, 0, 0, 0, 0])
    v = lr.diagram_vector(FOUR, GRID9, 3)
    assert np.array_equal(v[0], [0, .25, .5, .75, 1, .75, .5, .25, 0])
    assert np.array_equal(v[1], [0, .25, .5, .25, .5, .25, 0, 0, 0])
    assert np.array_equal(v[2] != 0, GRID9 == 0.75) and v[2][3] == 0.25
    # beta: (0,1) on [0,1), (0,2) on [0,2), (.5,1.5) on [.5,1.5), (0,inf) everywhere from 0
    assert np.array_equal(v[3], [3, 3, 4, 4, 3, 3, 2, 2, 1])
    empty = lr.diagram_vector(np.zeros((0, 2)), GRID9, 5)
    assert empty.shape == (6, 9) and not empty.any()
    inf_only = lr.diagram_vector([[0.5, np.inf]], GRID9, 2)
    assert not inf_only[:2].any() and np.array_equal(inf_only[2], (GRID9 >= 0.5).astype(float))


def test_properties():
    grid = np.linspace(0.0, 2.0, 41)
    rng = np.random.default_rng(3)
    for i, d in enumerate(_diagrams(4)):
        v = lr.diagram_vector(d, grid, 6)
        lam = v[:6]
        assert (lam[:-1] >= lam[1:]).all() and (lam >= 0).all()
        perm = rng.permutation(len(d))
        assert lr.diagram_vector(d[perm], grid, 6).tobytes() == v.tobytes(), i
        fin = d[np.isfinite(d).all(axis=1)]
        half = ((fin[:, 1] - fin[:, 0]) / 2).max() if len(fin) else 0.0
        assert (lam[0] <= half).all()
    # a grid point equal to a birth counts the row, one equal to its death does not
    v = lr.diagram_vector([[0.25, 0.75]], np.array([0.25, 0.5, 0.75]), 1)
    assert np.array_equal(v[1], [1, 1, 0]) and np.array_equal(v[0], [0, 0.25, 0])


def test_insertion_route_equals_reference():
    grids = [np.linspace(0.0, 2.0, 64), np.linspace(2.0, 0.0, 17), np.array([0.0, 0.5, 0.75, 1.0, 1.5, 2.0])]
    for i, d in enumerate(_diagrams(5) + [FOUR, np.repeat(FOUR, 3, axis=0), np.array([[0.4, 0.4], [0.4, 0.4]])]):
        for K in (1, 5, 8):
            g = grids[i % len(grids)]
            assert lr.diagram_vector_insertion(d, g, K).tobytes() == lr.diagram_vector(d, g, K).tobytes(), (i, K)


@pytest.mark.parametrize("n", [1, 2, 15, 89, 300])
def test_sequential_sum_is_np_mean(n):
    rng = np.random.default_rng(100 + n)
    grid = np.linspace(0.0, 2.0, 64)
    vs = [lr.diagram_vector(lr.random_diagram(rng, int(rng.integers(1, 30))), grid, 5) for _ in range(n)]
    assert lr.group_mean(vs).tobytes() == lr.sequential_mean(vs).tobytes()
    if n == 1:
        assert lr.group_mean(vs).tobytes() == vs[0].tobytes()


def test_landscape_mean_groups_and_mask():
    rng = np.random.default_rng(7)
    dg = [lr.random_diagram(rng, 5) for _ in range(6)]
    rows = np.zeros((6, 8, 2)); cnt = np.full(6, 5, np.int32)
    for i, d in enumerate(dg):
        rows[i, :5] = d
    cnt[5] = 11                                                     # truncated: the 8 rows of the buffer
    grid = np.linspace(0, 2, 7)
    out = lr.landscape_mean(rows, cnt, grid, 2, seg_off=[0, 2, 2, 6], status=[0, 4, 0, 0, 16, 0], skip_mask=4 | 16)
    assert np.array_equal(out[0], lr.diagram_vector(dg[0], grid, 2))
    assert np.isnan(out[1]).all()
    want = lr.sequential_mean([lr.diagram_vector(dg[2], grid, 2), lr.diagram_vector(dg[3], grid, 2),
                               lr.diagram_vector(rows[5], grid, 2)])
    assert np.array_equal(out[2], want)


def test_entry_points_exist():
    from tda_eeg_audio_amd import _lib, drivers, engine, utils
    lib = _lib.load()                                               # torch's HIP runtime first, as the package loads it
    for name in ("tda_landscape_mean_dev", "tda_landscape_batch"):
        assert name in _lib.SYMBOLS
        assert hasattr(lib, name)
    assert len(_lib.SYMBOLS["tda_landscape_mean_dev"][1]) == 14 and len(_lib.SYMBOLS["tda_landscape_batch"][1]) == 9
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "tdaeeg.h")).read()
    assert "tda_landscape_mean_dev(" in header and "tda_landscape_batch(" in header
    assert "#define TDA_MAX_LANDSCAPES 8" in header and _lib.MAX_LANDSCAPES == 8 and _lib.MAX_GRID == 256
    for f in (engine.landscape_batch, engine.landscape_mean_dev, utils.persistence_landscape, utils.betti_curve,
              utils.default_landscape_grid, drivers.landscapes_from_distances, drivers.landscape_names):
        assert callable(f)
    assert np.array_equal(utils.default_landscape_grid(), np.linspace(0.0, 2.0, 64))
    names = drivers.landscape_names(["alpha", "beta"], 2, np.linspace(0, 2, 3))
    assert len(names) == 2 * 2 * 3 * 3 and names[0] == "alpha_h0_landscape1_t0" and names[-1] == "beta_h1_betti_t2"


def test_no_cpu_fallback():
    """Without a GPU the landscape of a diagram is an error, never a host computation; a malformed diagram is a ValueError
    before anything is launched."""
    from tda_eeg_audio_amd import utils
    from tda_eeg_audio_amd._lib import TdaError
    with pytest.raises(ValueError):
        utils.persistence_landscape(np.zeros((3, 3)))
    with pytest.raises(ValueError):
        utils.betti_curve([1.0, 2.0])
    from tda_eeg_audio_amd import _lib
    try:
        got = utils.persistence_landscape(FOUR, GRID9, 3)
        beta = utils.betti_curve(FOUR, GRID9)
    except TdaError:
        return                                                      # no GPU: an error, not a host computation
    assert _lib._ctx, "a value without a HIP context: something computed it on the host"
    want = lr.diagram_vector(FOUR, GRID9, 3)
    assert np.array_equal(got, want[:3]) and np.array_equal(beta, want[3])
