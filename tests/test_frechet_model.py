"""
CPU tests of tests/frechet_ref.py, the evaluation of the Frechet mean the GPU tests compare against: known answers with
dyadic coordinates (every sum exact), the invariants of the algorithm, the certificate that the seeded groups of the GPU
tests have unique matchings, and the argument checks of step_outputs(frechet=...).
"""
import numpy as np
import pytest

import frechet_ref as fr
import wasserstein_q_ref as wq

D = lambda *rows: np.array(rows, dtype=np.float64).reshape(-1, 2)
DYADIC = D((0, 2), (0.5, 1.25), (1, 4), (3, 3.5))


def _rows(r):
    return r.mean[:r.cnt]


@pytest.mark.parametrize("m", [1, 2, 3, 7])
def test_copies_give_the_diagram(m):
    r = fr.frechet_mean([DYADIC] * m)
    assert np.array_equal(_rows(r), DYADIC) and r.var == 0.0 and r.iters == 1 and r.status == 0


def test_two_points_meet_halfway():
    r = fr.frechet_mean([D((0, 2)), D((0, 4))])
    assert np.array_equal(_rows(r), D((0, 3))) and r.var == 1.0 and r.status == 0


def test_point_and_empty_diagram():
    # (0, 4) is pulled halfway to its projection (2, 2): (1, 3); W2^2 to (0, 4) is 2, to the empty diagram 0.5 * 2^2 = 2
    r = fr.frechet_mean([D((0, 4)), np.zeros((0, 2))])
    assert np.array_equal(_rows(r), D((1, 3))) and r.var == 2.0
    r = fr.frechet_mean([np.zeros((0, 2)), D((0, 4))])                  # the start is empty: the row is spawned
    assert np.array_equal(_rows(r), D((1, 3))) and r.var == 2.0


def test_far_points_move_halfway_to_the_diagonal():
    r = fr.frechet_mean([D((0, 4)), D((10, 14))])
    assert np.array_equal(_rows(r), D((1, 3), (11, 13))) and r.cnt == 2
    assert r.var == 4.0                                                 # each diagram: 2 to its own point + 0.5 * 2^2


def test_empty_group_and_empty_diagrams():
    r = fr.frechet_mean([])
    assert r.cnt == 0 and np.isnan(r.var) and r.status == 0
    r = fr.frechet_mean([np.zeros((0, 2))] * 3)
    assert r.cnt == 0 and r.var == 0.0 and r.iters == 1 and r.status == 0
    r = fr.frechet_mean([D((0, np.inf), (1, 2)), D((1, 2), (np.nan, 1))])        # non-finite rows do not count
    assert np.array_equal(_rows(r), D((1, 2))) and r.var == 0.0


@pytest.mark.parametrize("shift", [0.5, -3.0, 1024.0])
def test_dyadic_shift(shift):
    g = [np.round(d * 64) / 64 for d in fr.random_group(3, 4, 2, 6)]
    a, b = fr.frechet_mean(g), fr.frechet_mean([d + shift for d in g])
    assert a.cnt == b.cnt and a.iters == b.iters
    assert np.allclose(_rows(b), _rows(a) + shift, rtol=0, atol=1e-12 * max(1.0, abs(shift)))
    assert a.var == pytest.approx(b.var, rel=1e-9)


def test_limits_and_status():
    g = fr.GROUPS["m15_s0"]
    full = fr.frechet_mean(g)
    one = fr.frechet_mean(g, max_iter=1)
    assert full.iters > 1 and one.status == fr.NOT_CONVERGED and one.iters == 1
    assert np.array_equal(_rows(one), fr.finite_rows(g[0]))             # the last iterate that was matched: Y^0
    cut = fr.frechet_mean(g, cap_out=5)
    assert cut.status == fr.TRUNCATED and cut.cnt == full.cnt and cut.var == full.var
    assert np.array_equal(cut.mean, full.mean[:5])
    assert fr.frechet_mean([DYADIC] * 65).status == fr.TOO_LARGE
    big = fr.frechet_mean(fr.far_group(9, 60))
    assert big.status == fr.TOO_LARGE and big.cnt == 0 and np.isnan(big.var)
    ok = fr.frechet_mean(fr.far_group(8, 60))
    assert ok.status == 0 and ok.cnt == 480 and ok.iters == 2


@pytest.mark.parametrize("name", list(fr.GROUPS))
def test_seeded_groups(name):
    """Every seeded group of the GPU tests: the reversed solve gives the same bytes (the matchings met are unique), the
    energy never increases, the run converges well inside the bounds, and the variance is the energy of the output."""
    g = fr.GROUPS[name]
    a, b = fr.frechet_mean(g, 32, 192), fr.frechet_mean(g, 32, 192, reverse=True)
    assert a.status == 0 and a.iters <= 16 and max(a.sizes) <= 192
    assert a.mean.tobytes() == b.mean.tobytes() and (a.cnt, a.var, a.iters, a.sizes, a.energies) == (b.cnt, b.var, b.iters, b.sizes, b.energies)
    assert all(e1 <= e0 for e0, e1 in zip(a.energies, a.energies[1:]))
    Y = _rows(a)
    total = sum(wq.value_ref(Y if len(Y) else np.zeros((0, 2)), d, 2, "l2") for d in g)
    assert total == pytest.approx(len(g) * a.var, rel=1e-12, abs=1e-300)


def test_other_gpu_groups_have_unique_matchings():
    """The remaining groups of the GPU tests, the same certificate: the far points of the size limits, the group without
    its first diagram, the 525 one-diagram groups."""
    for name, g in fr.other_groups().items():
        a, b = fr.frechet_mean(g), fr.frechet_mean(g, reverse=True)
        assert a.mean.tobytes() == b.mean.tobytes() and (a.cnt, a.iters, a.status) == (b.cnt, b.iters, b.status), name
        assert a.var == b.var or (np.isnan(a.var) and np.isnan(b.var)), name
    for d in fr.singles(525):
        a, b = fr.frechet_mean([d], cap_out=16), fr.frechet_mean([d], cap_out=16, reverse=True)
        assert a.mean.tobytes() == b.mean.tobytes() and a.iters == b.iters == 1 and a.var == b.var == 0.0
        assert np.array_equal(a.mean[:a.cnt], fr.finite_rows(d))


def test_batch_clamps_and_masks():
    g = fr.GROUPS["m3_s1"]
    rows = np.zeros((3, 12, 2)); cnt = np.zeros(3, np.int32)
    for i, d in enumerate(g):
        rows[i, :len(d)] = d; cnt[i] = len(d)
    mean, c, var, it, st = fr.batch(rows, cnt, np.array([-2, 3, 9]), cap_out=16)
    want = fr.frechet_mean(g, cap_out=16)
    assert np.array_equal(mean[0], want.mean, equal_nan=True) and c[0] == want.cnt and var[0] == want.var
    assert c[1] == 0 and np.isnan(var[1])
    status = np.array([4, 0, 0], np.int32)
    m2 = fr.batch(rows, cnt, np.array([0, 3]), status=status, skip_mask=4, cap_out=16)
    assert m2[1][0] == fr.frechet_mean(g[1:], cap_out=16).cnt


def test_step_outputs_arguments():
    from tda_eeg_audio_amd import pipeline
    assert [o.name for o in pipeline.step_outputs()] == []
    out = pipeline.step_outputs(wasserstein_q=(2, "l2"), frechet=(32, 8))
    assert [o.name for o in out] == ["wq", "fm"]
    assert out[-1].shape == (3, 34, 2) and out[-1].params == (32, 8)
    names = [o.name for o in pipeline.step_outputs(True, True, (np.linspace(0, 1, 4), 2), None, None, None, (4, 1))]
    assert names == ["corr", "bott", "land", "fm"]
    for bad in ((0, 8), (513, 8), (32, 0), (32, 65), (32,), (32.5, 8), (32, True), "ab", 5):
        with pytest.raises(ValueError):
            pipeline.step_outputs(frechet=bad)
