"""
The analytic-signal connectivity contract on the CPU (include/tdaeeg.h, "Analytic-signal connectivity"): the two
evaluations of tests/connectivity_ref.py against each other, the condition that makes the bars meaningful, known answers,
invariants and the argument checks of the Python layer.  No GPU.
"""
import numpy as np
import pytest

import connectivity_ref as ref
import plv_ref
from tda_eeg_audio_amd import _lib, engine, utils


def _every_window():
    for name, wins in plv_ref.cases().items():
        ex = ref.exact(name)
        for w, x in enumerate(wins):
            yield name, x, {k: v[w] for k, v in ex.items()}


def test_numpy_against_exact():
    """E_REF[m] = max |conn_numpy - conn_exact| over every pair of every window, measured again; the recorded constants
    are held to it within a factor of 2 upwards and 4 downwards (the order of the sums inside numpy's reductions and
    scipy's FFT is the library build's), and the bars are 8 times the constants.  No pair is left out."""
    worst = {m: 0.0 for m in ref.MEASURES}
    pairs = 0
    for name, x, ex in _every_window():
        nu = ref.conn_numpy(x)
        for m in ref.MEASURES:
            assert nu[m].shape == ex[m].shape == (x.shape[0], x.shape[0])
            assert np.isfinite(nu[m]).all() and np.isfinite(ex[m]).all(), (name, m)
            worst[m] = max(worst[m], float(np.abs(nu[m] - ex[m]).max()))
            assert np.array_equal(ex[m], ex[m].T) and (np.diagonal(ex[m]) == 1.0).all()
        pairs += x.shape[0] * (x.shape[0] - 1) // 2
    print("E_ref measured", worst, "recorded", ref.E_REF, "pairs", pairs)
    assert pairs == sum(n_win * n_ch * (n_ch - 1) // 2 for n_ch, _, n_win in plv_ref.SHAPES) + 28
    for m in ref.MEASURES:
        assert ref.E_REF[m] / 4 <= worst[m] <= 2 * ref.E_REF[m], m
        assert ref.BAR[m] == 8 * ref.E_REF[m]
        # a dropped term moves a value by about 1 / n_t = 4e-3: ten orders and more above the bar
        assert ref.BAR[m] * 1e10 < 1 / 250


def test_no_pair_near_a_threshold():
    """The condition that makes the bars meaningful: every off-diagonal pair has A / sqrt(P_i P_j) >= 1e-3 (generic) or
    <= 2^-46 (in phase to rounding; TAU is 2^-40), and every envelope a coefficient of variation >= 1e-3 or is flat by the
    rule -- in both evaluations alike, so that no value is a 0 in one and a quotient in the other."""
    r_gen, r_deg, cv_min, flat_names = np.inf, 0.0, np.inf, []
    for name, x, ex in _every_window():
        nu = ref.conn_numpy(x, diag=True)
        off = ~np.eye(x.shape[0], dtype=bool)
        zero_p = np.isnan(ex["ratio"]) & off                      # P_i P_j == 0: a zero channel
        assert np.array_equal(np.isnan(nu["ratio"]) & off, zero_p)
        for r in (nu["ratio"], ex["ratio"]):
            v = r[off & ~zero_p]
            gen = v > 2.0 ** -46
            assert (v[gen] >= 1e-3).all(), name
            r_gen = min(r_gen, v[gen].min()) if gen.any() else r_gen
            r_deg = max(r_deg, v[~gen].max()) if (~gen).any() else r_deg
        assert np.array_equal((nu["ratio"] > 2.0 ** -46) & off, (ex["ratio"] > 2.0 ** -46) & off)
        assert np.array_equal(nu["flat"], ex["flat"]), name
        for cv in (nu["cv"], ex["cv"]):
            v = cv[~ex["flat"]]
            assert (v >= 1e-3).all(), name
            cv_min = min(cv_min, v.min()) if v.size else cv_min
        flat_names += [(name, int(c)) for c in np.flatnonzero(ex["flat"])]
    print("generic ratio min", r_gen, "degenerate ratio max", r_deg, "smallest coefficient of variation", cv_min)
    assert r_gen >= 0.010 and r_deg <= 1.5e-16 and cv_min >= 0.004
    assert flat_names == [("special_8x250", 4), ("special_8x250", 5)]      # the zero and the constant channel


def test_known_answers():
    bar = ref.BAR
    # a duplicated channel: wpli 0, imcoh 0, coh 1, aec 1; a rescaled one: wpli 0 by the rule
    x = plv_ref.cases()["special_8x250"][0]
    for f in (ref.conn_numpy, ref.conn_exact):
        v = f(x)
        assert v["wpli"][1, 3] == 0.0 and v["imcoh"][1, 3] == 0.0
        assert abs(v["coh"][1, 3] - 1.0) <= bar["coh"] and abs(v["aec"][1, 3] - 1.0) <= bar["aec"]
        assert v["wpli"][2, 6] == 0.0 and v["imcoh"][2, 6] <= bar["imcoh"] and abs(v["coh"][2, 6] - 1.0) <= bar["coh"]
        assert abs(v["aec"][2, 6] - 1.0) <= bar["aec"]
        for k in range(8):                                          # the zero and the constant channel
            if k != 4:
                assert v["wpli"][4, k] == v["imcoh"][4, k] == v["coh"][4, k] == v["aec"][4, k] == 0.0
            if k != 5:
                assert v["aec"][5, k] == 0.0
    # two sinusoids a quarter period apart over whole periods: wpli 1, imcoh = coh (= 1: the real part vanishes)
    t = np.arange(250)
    for k in (5, 10, 31):
        x = np.stack([np.sin(2 * np.pi * k * t / 250), 2.0 * np.cos(2 * np.pi * k * t / 250)])
        for f in (ref.conn_numpy, ref.conn_exact):
            v = f(x)
            assert abs(v["wpli"][0, 1] - 1.0) <= bar["wpli"], (k, f.__name__)
            assert abs(v["imcoh"][0, 1] - v["coh"][0, 1]) <= bar["imcoh"] + bar["coh"]
            assert abs(v["coh"][0, 1] - 1.0) <= bar["coh"]
    # n_t = 2: the table is zero, h = 0, s = 0: wpli and imcoh exactly 0
    for a in ([[1.0, 2.0], [3.0, 1.0]], [[1.0, 2.0], [3.0, -1.0]], [[1.0, -2.0], [0.5, 0.25]]):
        for f in (ref.conn_numpy, ref.conn_exact):
            v = f(np.array(a))
            assert v["wpli"][0, 1] == 0.0 and v["imcoh"][0, 1] == 0.0, a


def test_invariants():
    """Every value in its range, symmetric as bytes, diagonal 1; positive rescaling of a channel changes nothing."""
    for name in ("rand_16x63", "rand_3x65", "special_8x250"):
        x = plv_ref.cases()[name][0]
        v = ref.conn_numpy(x)
        y = x.copy()
        y[1] *= 3.7
        y[0] *= 2.0 ** -20
        vy = ref.conn_numpy(y)
        for m in ref.MEASURES:
            lo = -1.0 if m == "aec" else 0.0
            assert (v[m] >= lo - ref.BAR[m]).all() and (v[m] <= 1 + ref.BAR[m]).all(), (name, m)
            assert v[m].tobytes() == v[m].T.copy().tobytes() and (np.diagonal(v[m]) == 1.0).all()
            assert np.abs(vy[m] - v[m]).max() <= ref.BAR[m], (name, m)
        assert (v["imcoh"] <= v["coh"] + ref.BAR["coh"]).all()
    for m in ref.MEASURES:
        assert plv_ref.dist_bar(0, ref.BAR[m]) == np.sqrt(2 * ref.BAR[m]) and plv_ref.dist_bar(1, ref.BAR[m]) == ref.BAR[m]


def test_argument_checks():
    assert engine.CONNECTIVITY_MEASURES == {"wpli": 0, "imcoh": 1, "coh": 2, "aec": 3}
    assert [engine.connectivity_measure(m) for m in ref.MEASURES] == [0, 1, 2, 3]
    assert ref.TAU == _lib.CONN_TAU == 2.0 ** -40
    for bad in ("plv", "WPLI", "pli", 0, 3, None, True, ("wpli",), b"coh", ""):
        with pytest.raises(ValueError):
            engine.connectivity_measure(bad)
    x = plv_ref.cases()["rand_3x65"][0]
    for f in (utils.compute_connectivity_matrix, utils.compute_connectivity_persistence):
        with pytest.raises(ValueError):
            f(x, "plv")                                             # an unknown measure, before anything is launched
        with pytest.raises(ValueError):
            f(np.zeros(250), "wpli")                                # not a window
        with pytest.raises(ValueError):
            f(np.zeros((1, 250)), "wpli")
        with pytest.raises(ValueError):
            f(np.zeros((3, 1)), "wpli")
    with pytest.raises(ValueError):
        utils.compute_connectivity_persistence(x, "wpli", method="pearson")
    with pytest.raises(NotImplementedError):
        utils.compute_connectivity_persistence(x, "wpli", max_dim=2)
    for bad in ("pearson", 0, None, True):
        with pytest.raises(ValueError):
            engine.connectivity_dist_batch(x, measure="coh", method=bad)
