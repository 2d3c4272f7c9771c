"""The CPU oracle on the cases of tests/eeg_shape_cases.py.  tests/test_gpu_eeg_shapes.py holds the EEG window kernels to
the oracle bit for bit at shapes the reference never runs (1..64 channels, 2..1000 samples), so the oracle is held first:
against the definition evaluated in extended precision, against the brute-force reduction at the short windows, and on the
48-channel windows that need more than 512 class bits.  The input conditions the GPU tests rely on are asserted here too,
where the oracle alone decides them.  No GPU."""
import numpy as np
import pytest

import eeg_shape_cases as sc
from oracle import brute, port


def _same_multiset(a, b):
    return np.array_equal(brute.sort_rows(a), brute.sort_rows(b))


# ------------------------------------------------------------------ corr / dist against the definition
def _deviations(n_ch):
    """(corr, dist where the definition's distance exceeds 1e-3, dist below that): the largest absolute deviation of the
    oracle from the definition in np.longdouble over every length of the grid."""
    dev = np.zeros(3)
    off = ~np.eye(n_ch, dtype=bool)
    for n_t in sc.RES_LENGTHS + sc.STREAM_LENGTHS:
        W = sc.windows(n_ch, n_t)
        oc, od = sc.oracle_corr_dist(n_ch, n_t)
        r, d = sc.definition_longdouble(W)
        assert np.isfinite(oc).all() and np.isfinite(od).all()
        assert np.all(od[:, ~off] == 0.0) and np.all(od >= 0.0) and np.all(np.abs(oc) <= 1.0)
        dc = np.abs(oc - r)
        dd = np.abs(od - d)[:, off]
        far = (d[:, off] > 1e-3)
        dev = np.maximum(dev, [float(dc.max()), float(dd[far].max()) if far.any() else 0.0,
                               float(dd[~far].max()) if (~far).any() else 0.0])
    return dev


@pytest.mark.parametrize("n_ch", sc.CORR_CH)
def test_oracle_corr_dist_against_the_definition_in_extended_precision(n_ch):
    """port.corr_dist_batch on the full grid against np.corrcoef + NaN -> 0 + clip + sqrt(2 (1 - r)) + zero diagonal in
    np.longdouble, at the bars of test_gpu_parity.py::test_corr_dist_vs_reference_golden: corr 1e-12, dist 1e-12 where the
    distance exceeds 1e-3 and 1e-7 below that (sqrt near r = 1 turns 1e-16 into 1e-8).  Measured over all 13 channel counts
    with these seeds: 2.9e-15, 1.7e-13 and 3.0e-8 (the last where r is within a rounding or two
    of 1: two-sample windows and duplicated channels)."""
    assert np.finfo(np.longdouble).eps < np.finfo(np.float64).eps, "np.longdouble must be wider than float64 here"
    dev = _deviations(n_ch)
    print(f"n_ch {n_ch}: corr {dev[0]:.2e}  dist (> 1e-3) {dev[1]:.2e}  dist (<= 1e-3) {dev[2]:.2e}")
    assert dev[0] <= 1e-12 and dev[1] <= 1e-12 and dev[2] <= 1e-7, dev


def test_degenerate_windows_have_their_known_matrices():
    """Zero-variance channel: r = NaN -> 0, d = sqrt(2) to every other channel.  Duplicated channel: r = (c / s) / s with
    s = sqrt(c) rounded, i.e. 1 or one or two roundings below it, d = 0 up to sqrt(2 * 2^-51) = 3e-8.  The all-constant
    window: every off-diagonal distance sqrt(2)."""
    for n_ch, n_t in [(2, 2), (17, 9), (33, 33), (48, 256), (64, 289)]:
        oc, od = sc.oracle_corr_dist(n_ch, n_t)
        z = (2 * n_ch) // 3
        other = np.arange(n_ch) != z
        assert np.all(od[2, z, other] == np.sqrt(2.0)) and np.all(oc[2, z, :] == 0.0)
        assert od[3, n_ch - 1, n_ch // 4] <= 3e-8 and 1.0 - oc[3, n_ch - 1, n_ch // 4] <= 2.0 ** -51
        off = ~np.eye(n_ch, dtype=bool)
        assert np.all(od[5][off] == np.sqrt(2.0)) and np.all(oc[5] == 0.0)


# ------------------------------------------------------------------ persistence at the short windows
SHORT_CH = (5, 9, 14, 19)


@pytest.mark.parametrize("n_t", (2, 3, 4, 5, 8))
def test_oracle_persistence_at_short_windows_against_brute_force(n_t):
    """n_t < n_ch: rank-deficient correlations, many equal or nearly equal distances.  port.rips_dm against the textbook
    reduction of oracle/brute.py on every window of a few small stacks."""
    for n_ch in SHORT_CH:
        _, od = sc.oracle_corr_dist(n_ch, n_t)
        for w in range(sc.N_WIN):
            o = sc.oracle_diagrams(n_ch, n_t, w)
            b0, b1 = brute.rips_brute(brute.eeg_prepare(od[w]))
            assert _same_multiset(o[0], b0) and _same_multiset(o[1], b1), (n_ch, n_t, w)


def test_two_sample_windows_have_no_h1_and_deaths_at_0_or_2():
    """n_t = 2: the centred channels are (a, -a), every correlation is +1 or -1 up to one rounding of r (d = 0 or up to
    sqrt(2 * 2^-52) = 2.1e-8 instead; d = 2 is exact in float32), or NaN -> 0 (d = sqrt(2)) beside a zero-variance channel.
    Two clusters at distance 2: no H1 row, finite H0 deaths at 0 (within 3e-8: r one or two roundings from 1) or at 2."""
    for n_ch in SHORT_CH + sc.FUSED_CH:
        _, od = sc.oracle_corr_dist(n_ch, 2)
        vals = np.unique(od.astype(np.float32))
        assert np.all((vals <= 3e-8) | (vals == np.float32(np.sqrt(2.0))) | (vals == 2.0)), vals
        for w in (0, 1, 3, 4):                                  # the windows without a zero-variance channel
            h0, h1 = sc.oracle_diagrams(n_ch, 2, w)
            assert len(h1) == 0, (n_ch, w, h1)
            fin = h0[np.isfinite(h0[:, 1]), 1]
            assert np.all((fin <= 3e-8) | (fin == 2.0)), (n_ch, w, fin)
            assert np.isinf(h0[:, 1]).sum() == 1


def test_three_sample_windows_lie_on_a_circle():
    """n_t = 3: the centred, normalised channels are unit vectors of a plane, d = sqrt(2 (1 - cos angle)) is monotone in the
    angle, and the Rips complex of points of a circle has at most one H1 class (Adamaszek & Adams 2017); the seeded latent
    and white windows of 19 and more channels have exactly one."""
    for n_ch in SHORT_CH + sc.FUSED_CH:
        for w in (0, 1):
            h1 = sc.oracle_diagrams(n_ch, 3, w)[1]
            assert len(h1) <= 1, (n_ch, w, h1)
            if n_ch >= 19:
                assert len(h1) == 1, (n_ch, w)


# ------------------------------------------------------------------ 48 channels: more than 512 classes alive at once
@pytest.mark.parametrize("n_ch,m,n_t,alive", [(48, 24, 250, 529), (48, 23, 250, 528), (48, 24, 64, 529), (48, 23, 64, 528),
                                              (47, 23, 250, 506)])
def test_bipartite_windows_reach_the_bound_of_classes_alive_at_once(n_ch, m, n_t, alive):
    """(m - 1)(n_ch - m - 1) H1 classes alive at once on K(m, n_ch - m): 506 at 47 channels, the most 47 points admit and
    inside the 512 class bits of the widest LDS pass; 529 and 528 at 48, beyond them."""
    W = sc.bipartite_windows(n_ch, m, n_t, 1, seed=3)
    _, d = port.corr_dist(W[0])
    h0, h1 = port.rips_dm(d)
    assert sc.max_alive(h1) == alive == (m - 1) * (n_ch - m - 1)
    assert (alive > 512) == (n_ch == 48)
    assert len(h0) == n_ch and len(h1) <= 1024                 # h1_cap of the GPU test


def test_bipartite_windows_reproduce_the_47_channel_recipe():
    """bipartite_windows(47, 23, 250, ...) is test_gpu_parity.py::_bipartite_windows draw for draw (restated here: that
    module needs a GPU to import its fixtures' targets)."""
    rng = np.random.default_rng(3)
    G = np.full((47, 47), 0.20)
    G[:23, 23:] = 0.23; G[23:, :23] = 0.23
    np.fill_diagonal(G, 1.0)
    ev, U = np.linalg.eigh(G)
    L = (U * np.sqrt(ev)) @ U.T
    ref = []
    for _ in range(2):
        Z = rng.standard_normal((250, 47)); Z -= Z.mean(axis=0)
        Q, _ = np.linalg.qr(Z)
        ref.append((L @ Q.T) * rng.uniform(0.5, 2.0, size=(47, 1)))
    assert np.array_equal(sc.bipartite_windows(47, 23, 250, 2, seed=3), np.stack(ref))


def test_the_48_channel_batch():
    W, bip = sc.batch_48()
    assert W.shape == (sc.N_WIN, 48, 250) and bip == (1, 4)
    _, od = port.corr_dist_batch(W)
    alive = [sc.max_alive(port.rips_dm(od[w])[1]) for w in range(sc.N_WIN)]
    assert alive[1] == 529 and alive[4] == 528 and max(alive[w] for w in (0, 2, 3, 5)) <= 512


# ------------------------------------------------------------------ input conditions of the GPU tests
def test_fused_grid_input_conditions():
    """What tests/test_gpu_eeg_shapes.py relies on, decided by the oracle alone: every window of the fused grid fits the
    default 256 H1 rows, and some need more than 32 and some more than 64 class bits at once (rows of the diagram alive at
    once; the sweep also holds the zero-persistence classes, so it needs no fewer), so that the narrow first passes of
    the fused kernel overflow on their own."""
    rows = alive = 0
    over32 = over64 = 0
    for n_ch in sc.FUSED_CH:
        for n_t in sc.RES_LENGTHS:
            for w in range(sc.N_WIN):
                h1 = sc.oracle_diagrams(n_ch, n_t, w)[1]
                a = sc.max_alive(h1)
                rows, alive = max(rows, len(h1)), max(alive, a)
                over32 += a > 32; over64 += a > 64
    print(f"fused grid: at most {rows} H1 rows, at most {alive} alive at once; {over32} windows above 32, {over64} above 64")
    assert rows <= 256
    assert over32 > 0 and over64 > 0 and over32 > over64
