"""
The CPU statement of the recurrence curves against itself (tests/recurrence_ref.py): the two evaluations of the integers
agree as bytes, the identities of a recurrence plot hold, the plots with answers worked out by hand give them, and the
error of the numpy statement of the two entropies against the 40-digit evaluation is measured again.  No GPU.
"""
import numpy as np
import pytest

import euler_ref as er
import network_ref as nr
import recurrence_cases as rc
import recurrence_ref as rr


def _same(a, b, what=""):
    for x, y, k in zip(a, b, ("counts", "measures", "hist")):
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), (what, k)


SIZES = [1, 2, 3, 4, 5, 8, 31, 33, 47, 63, 64, 65, 96, 127, 128]


@pytest.mark.parametrize("ties", [False, True])
def test_two_evaluations_agree(ties):
    rng = np.random.default_rng(5 + ties)
    for n in SIZES:
        theiler, l_min, v_min = int(rng.integers(1, 4)), int(rng.integers(1, 6)), int(rng.integers(1, 6))
        d = rc.trajectory_dm(1, n, 30 + n, ties)[0]
        grid = np.array([0.3, 0.7, np.nan]) if n > 8 else rc.grid_of(3, n)
        _same(rr.block_dm(d, grid, theiler, l_min, v_min), rr.block_dm(d, grid, theiler, l_min, v_min, route=rr.block_masks_one),
              (n, theiler, l_min, v_min))
    # random matrices (short lines), and a band of every kind around one size
    d = rng.random((70, 70)) * 2.2
    for theiler in (1, 2, 63, 64, 65, 69, 70, 128):
        _same(rr.block_dm(d, [0.9, 1.6], theiler, 1, 2), rr.block_dm(d, [0.9, 1.6], theiler, 1, 2, route=rr.block_masks_one), theiler)


def test_identities():
    for case in [c for c in rc.DM_CASES if c[0] in (47, 65, 128) and c[1] <= 9]:
        n, _, _, theiler, l_min, v_min, _ = case
        dms, grid = rc.dm_case(case)
        cnt, mea, his = rr.block_dm(dms[0], grid, theiler, l_min, v_min)
        ls = np.arange(1, n + 1)
        # every recurrence lies on exactly one diagonal and one vertical line
        assert ((his[0] * ls).sum(-1) == cnt[0]).all() and ((his[1] * ls).sum(-1) == cnt[0]).all(), case
        # the plot is symmetric: every diagonal line has its mirror
        assert not (his[0] % 2).any() and not (cnt[1] % 2).any() and not (cnt[2] % 2).any()
        assert (cnt[3] <= max(n - theiler, 0)).all() and (cnt[6] <= n - 1).all()
        assert ((mea[[0, 1, 4]] >= 0) & (mea[[0, 1, 4]] <= 1)).all()
        if theiler == 1:
            edges = nr.block_dm(dms[0], grid)[0][0]
            assert (cnt[0] == 2 * edges).all(), case


def test_the_inputs_have_lines_of_many_lengths():
    """The trajectories exercise what the plots of random matrices do not: long lines and broad histograms."""
    dms, grid = rc.dm_case((128, 5, 1, 1, 2, 2, False))
    cnt, mea, his = rr.block_dm(dms[0], grid)
    assert cnt[3].max() >= 20 and cnt[6].max() >= 5 and (his[0] > 0).sum(-1).max() >= 10
    assert mea[3].max() > 1.0 and mea[6].max() > 0.5


@pytest.mark.parametrize("name", sorted(rc.known()))
def test_known_answers(name):
    d, (theiler, l_min, v_min), cnt, mea = rc.known()[name]
    for route in (rr.plot_loops, rr.block_masks_one):
        c, m, _ = rr.block_dm(d, [rc.SCALE, 0.0 - 1.0, 2.0], theiler, l_min, v_min, route=route)
        assert c[:, 0].tolist() == cnt, name
        assert m[:, 0].tobytes() == np.array(mea, np.float64).tobytes(), (name, m[:, 0], mea)
        assert not c[:, 1].any() and not m[:, 1].any()
    if name.startswith("periodic"):
        assert mea[1] == 1.0 and mea[4] == 0.0
    if name.startswith("checkerboard"):
        assert mea[2] == mea[3] == mea[5] == mea[6] == 0.0


def test_single_bin_entropy_is_zero():
    H = np.zeros(9, np.int64)
    H[4] = 6
    assert np.float64(rr.entropy(H, 6, 2)).tobytes() == np.float64(0.0).tobytes()
    assert rr.entropy(H, 6, 6) == 0.0 and rr.entropy(np.zeros(9, np.int64), 0, 1) == 0.0


def test_input_forms_and_status_words():
    rng = np.random.default_rng(3)
    pc = rng.random((10, 3))
    grid = [0.3, 0.8]
    (c, m, h), st = rr.block_cloud(pc, 10, grid)
    assert st == 0 and h.shape == (2, 2, 10) and c[0].max() > 0
    for n_pts, want in ((2, er.TDA_WIN_DEGENERATE), (11, er.TDA_WIN_TOO_LARGE)):
        (c, m, h), st = rr.block_cloud(pc, n_pts, grid)
        assert st == want and not c.any() and not m.any() and not h.any()
    sig = np.sin(np.arange(250) * 0.21)
    (c, m, h), st = rr.block_takens(sig, 7, grid)
    assert st == 0 and h.shape == (2, 2, 128) and c[3].max() > 5
    assert rr.block_takens(sig, 0, grid)[1] == er.TDA_WIN_TOO_LARGE and rr.block_takens(sig, 124, grid)[1] == er.TDA_WIN_DEGENERATE


def test_entropy_error_of_the_numpy_statement():
    """The bar of the GPU tests is 8 times the error measured here: measured against the 40-digit evaluation, on the inputs
    of the GPU tests, never against the kernel."""
    worst = 0.0
    for case in [c for c in rc.DM_CASES if c[1] <= 9]:
        n, _, _, theiler, l_min, v_min, _ = case
        dms, grid = rc.dm_case(case)
        for d in dms:
            cnt, _, his = rr.block_dm(d, grid, theiler, l_min, v_min)
            worst = max([worst] + rr.entropy_errors(his, cnt, l_min, v_min))
    for name, (d, (theiler, l_min, v_min), _, _) in rc.known().items():
        cnt, _, his = rr.block_dm(d, [rc.SCALE], theiler, l_min, v_min)
        worst = max([worst] + rr.entropy_errors(his, cnt, l_min, v_min))
    print(f"entropy: largest |numpy statement - 40 digits| = {worst:.3e} = 2^{np.log2(worst):.2f}; "
          f"written {rr.ENTROPY_REF_ERR:.3e}, bar {rr.ENTROPY_BAR:.3e}")
    assert 0.0 < worst <= rr.ENTROPY_REF_ERR
    assert rr.ENTROPY_BAR == 8 * rr.ENTROPY_REF_ERR
