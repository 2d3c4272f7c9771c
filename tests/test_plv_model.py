"""
The phase-locking value contract on the CPU (include/tdaeeg.h, "Phase-locking value"): the two evaluations of
tests/plv_ref.py against each other, the Hilbert step against the circulant of the host table, known answers, invariants,
and the place of the step output.  No GPU.
"""
import numpy as np
import pytest

import plv_ref as ref
from tda_eeg_audio_amd import pipeline

EPS = 2.0 ** -52


def test_numpy_against_exact():
    """E_ref = max |plv_numpy - plv_exact| over the test inputs, measured again; the recorded constant is held to it within
    a factor of 2 upwards and 4 downwards (the order of the sums inside numpy's matrix products and scipy's FFT is the
    library build's), and the bar is 8 times the constant."""
    worst = {}
    for name, wins in ref.cases().items():
        ex = ref.exact(name)
        worst[name] = max(float(np.abs(ref.plv_numpy(x) - ex[i]).max()) for i, x in enumerate(wins))
        assert np.array_equal(ex[0], ex[0].T) and (np.diagonal(ex[0]) == 1.0).all()
    e = max(worst.values())
    print("E_ref measured", e, "recorded", ref.PLV_E_REF, "bar", ref.PLV_BAR, worst)
    assert ref.PLV_E_REF / 4 <= e <= 2 * ref.PLV_E_REF
    assert ref.PLV_BAR == 8 * ref.PLV_E_REF
    # a dropped term moves a value by about 1 / n_t = 4e-3: eleven to twelve orders above the bar
    assert ref.PLV_BAR * 1e11 < 1 / 250
    # the circulant form of step 1, which the kernel evaluates, is inside the bar too
    for name, wins in ref.cases().items():
        ex = ref.exact(name)
        assert max(float(np.abs(ref.plv_circulant(x) - ex[i]).max()) for i, x in enumerate(wins)) <= ref.PLV_BAR, name


@pytest.mark.parametrize("n_t", [2, 3, 8, 63, 64, 249, 250, 256])
def test_hilbert_is_the_circulant_of_the_host_table(n_t):
    """Step 1: imag(scipy.signal.hilbert(x)) = x @ G.T, G[t][m] = g[(t - m) mod n_t], to the forward error bound of a dot
    product of n_t terms, n_t * eps * (|x| @ |G|.T)."""
    from scipy.signal import hilbert
    rng = np.random.default_rng(n_t)
    x = rng.standard_normal((5, n_t))
    g = ref.hilbert_g(n_t)
    assert g.shape == (n_t,) and g.dtype == np.float64
    G = g[(np.arange(n_t)[:, None] - np.arange(n_t)[None, :]) % n_t]
    h = np.imag(hilbert(x, axis=-1))
    assert (np.abs(h - x @ G.T) <= n_t * EPS * (np.abs(x) @ np.abs(G).T) + 1e-300).all()


def test_known_answers():
    bar = ref.PLV_BAR
    t = np.arange(250)
    for k, (p1, p2) in ((5, (0.3, 2.1)), (10, (0.0, np.pi)), (31, (1.0, -0.4))):     # whole periods, any phase offset
        x = np.stack([np.sin(2 * np.pi * k * t / 250 + p1), 2.0 * np.sin(2 * np.pi * k * t / 250 + p2)])
        for f in (ref.plv_numpy, ref.plv_circulant, ref.plv_exact):
            assert abs(f(x)[0, 1] - 1.0) <= bar, (k, f.__name__)
    rng = np.random.default_rng(1)
    x = rng.standard_normal((2, 250))
    x[1] = 3.0 * x[0]                                               # a channel and its positive multiple
    for f in (ref.plv_numpy, ref.plv_circulant, ref.plv_exact):
        assert abs(f(x)[0, 1] - 1.0) <= bar
    for a in ([[1.0, 2.0], [3.0, 1.0]], [[1.0, 2.0], [3.0, -1.0]], [[1.0, -2.0], [0.5, 0.25]], [[1.0, 1.0], [-2.0, 5.0]]):
        for f in (ref.plv_numpy, ref.plv_circulant, ref.plv_exact):     # n_t = 2: g = 0, every phase is 0 or pi
            p = f(np.array(a))[0, 1]
            assert min(abs(p), abs(p - 1.0)) <= bar, (a, p)
    x = np.zeros((2, 250))
    x[1] = 2.5                                                      # a zero channel (phase 0) against a constant one
    for f in (ref.plv_numpy, ref.plv_circulant, ref.plv_exact):
        assert abs(f(x)[0, 1] - 1.0) <= bar
    x[1] = -2.5                                                     # ... and a negative constant: the phase is pi throughout
    assert abs(ref.plv_exact(x)[0, 1] - 1.0) <= bar


def test_invariants():
    bar = ref.PLV_BAR
    for name in ("rand_16x63", "rand_3x65", "special_8x250"):
        x = ref.cases()[name][0]
        p = ref.plv_numpy(x)
        assert (p >= 0).all() and (p <= 1 + bar).all() and np.array_equal(p, p.T) and (np.diagonal(p) == 1.0).all()
        y = x.copy()
        y[1] *= 3.7                                                 # a positive rescaling of a channel
        y[0] *= 2.0 ** -20
        assert np.abs(ref.plv_numpy(y) - p).max() <= bar
        y = x.copy()
        y[[0, 2]] *= -1.0                                           # both channels of a pair negated
        assert abs(ref.plv_numpy(y)[0, 2] - p[0, 2]) <= bar
    # the distance: zero diagonal, symmetric, and the derived bars in their order
    for m in range(4):
        d = ref.dist_of(p, m)
        assert np.array_equal(d, d.T) and (np.diagonal(d) == 0.0).all() and (d >= 0).all()
    assert ref.dist_bar(0) == ref.dist_bar(3) == np.sqrt(2 * bar) and ref.dist_bar(1) == ref.dist_bar(2) == bar
    assert ref.dist_of(np.array([[1.0, 1.0], [1.0, 1.0]]), 0)[0, 1] == 0.0
    assert abs(ref.dist_of(np.array([[1.0, 1.0 - 1e-16], [1.0 - 1e-16, 1.0]]), 0)[0, 1]) <= 1.5e-8


def test_step_outputs_pl():
    only = pipeline.step_outputs(phase_locking="abs")
    assert [o.name for o in only] == ["pl"] and only[0].shape == (24,) and pipeline.PL_COLS == 24 and only[0].params == 1
    assert pipeline.step_outputs(phase_locking=True)[0].params == 0
    assert [pipeline.step_outputs(phase_locking=m)[0].params for m in ref.METHODS] == [0, 1, 2, 3]
    assert pipeline.step_outputs() == [] and pipeline.step_outputs(phase_locking=None) == []
    every = pipeline.step_outputs(correlations=True, bottleneck=True, landscapes=(np.linspace(0, 1, 4), 2),
                                  images=(np.linspace(0, 1, 3), np.linspace(0, 1, 3), 0.1, 1), sliced=np.eye(2),
                                  wasserstein_q=(2, "l2"), frechet=(8, 4), kernel_distance=("pss", 0.5), fisher=0.5,
                                  sublevel=True, phase_locking=True)
    assert [o.name for o in every] == ["corr", "bott", "land", "img", "slc", "wq", "fm", "kd", "pf", "sl", "pl"]
    import inspect
    assert list(inspect.signature(pipeline.step_outputs).parameters)[-1] == "phase_locking"
    for bad in ("plv", "Euclidean", 0, 1, 2.0, ("euclidean",), b"abs", ""):
        with pytest.raises(ValueError):
            pipeline.step_outputs(phase_locking=bad)
