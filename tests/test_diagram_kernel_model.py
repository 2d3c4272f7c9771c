"""
The CPU reference of the kernels on diagrams (tests/diagram_kernel_ref.py) against known answers, against scikit-learn's
Gaussian kernel, and against a 40-digit evaluation of the same float64 arguments.  No GPU.
"""
import math

import numpy as np
import pytest

import diagram_kernel_ref as dk
from tda_eeg_audio_amd import engine

PSS = dk.named(("pss", 0.1))
PWG = dk.named(("pwg", 0.1, 2.0))


def _diagram(rng, n, scale=1.0):
    """n float32-valued rows with d > b."""
    b = rng.uniform(0, scale, n).astype(np.float32)
    d = b + rng.uniform(0, scale, n).astype(np.float32)
    return np.stack([b, d.astype(np.float32)], axis=1).astype(np.float64)


def test_named_kernels_are_the_engines():
    for kernel in (("pss", 0.1), ("pss", 3), ("pwg", 0.25, 2.0), ("pwg", 1, 1)):
        assert engine.diagram_kernel_args(kernel) == dk.named(kernel)
    assert (dk.KW_ONE, dk.KW_PERS, dk.KW_ATAN) == (engine._lib.TDA_KW_ONE, engine._lib.TDA_KW_PERS, engine._lib.TDA_KW_ATAN)


def test_two_points_closed_form():
    A, B = np.array([[0.0, 1.0]]), np.array([[0.5, 1.5]])
    for sigma in (0.05, 0.5, 2.0):
        k, a, nt = dk.kernel_value(A, B, dk.named(("pss", sigma)))
        want = (math.exp(-0.5 / (8 * sigma)) - math.exp(-2.5 / (8 * sigma))) / (8 * math.pi * sigma)
        assert nt == 1 and abs(k - want) <= 4e-16 * a
        k, a, nt = dk.kernel_value(A, B, dk.named(("pwg", sigma, 3.0)))
        want = math.atan(3.0) ** 2 * math.exp(-0.5 / (2 * sigma * sigma))
        assert nt == 1 and abs(k - want) <= 4e-16 * max(a, 1e-300)
    # non-finite rows never enter; an empty diagram is the zero measure, not {(0, 0)}
    H0 = np.array([[0.0, 1.0], [0.0, np.inf], [np.nan, 0.3]])
    assert dk.kernel_value(H0, B, PSS) == dk.kernel_value(A, B, PSS)
    assert dk.kernel_value(np.zeros((0, 2)), B, PWG) == (0.0, 0.0, 0)
    kv, _, _ = dk.pair(np.zeros((0, 2)), B, PWG)
    assert kv[0] == 0.0 and kv[1] == 0.0 and dk.distance(kv) == np.sqrt(kv[2])


def test_point_on_the_diagonal_adds_exactly_zero_to_pss():
    rng = np.random.default_rng(2)
    B = _diagram(rng, 40)
    diag = np.array([[0.37, 0.37], [1.25, 1.25]])
    a1, a2 = dk.arguments(diag, B, PSS[0], 1)
    assert a1.tobytes() == a2.tobytes()
    assert dk.kernel_value(diag, B, PSS)[0] == 0.0
    A = _diagram(rng, 17)
    assert dk.kernel_value(np.concatenate([A, diag]), B, PSS)[0] == dk.kernel_value(A, B, PSS)[0]


def test_weight_one_without_mirror_is_the_rbf_kernel():
    from sklearn.metrics.pairwise import rbf_kernel
    rng = np.random.default_rng(3)
    A, B = _diagram(rng, 46), _diagram(rng, 122)
    for ninv in (-0.5, -12.5, -50.0):
        k, _, nt = dk.kernel_value(A, B, (ninv, 0, 1.0, dk.KW_ONE, 0.0))
        want = rbf_kernel(A, B, gamma=-ninv).sum()
        assert nt == 46 * 122 and abs(k - want) <= 1e-12 * want


def test_gram_symmetric_and_positive_semidefinite():
    rng = np.random.default_rng(4)
    dgms = [_diagram(rng, int(n)) for n in rng.integers(1, 40, 12)]
    for par in (PSS, PWG, (-3.0, 0, 1.0, dk.KW_PERS, 0.0)):
        G, _, _ = dk.gram([[d] for d in dgms], [[d] for d in dgms], par)
        assert np.abs(G - G.T).max() <= 1e-13 * np.abs(G).max()
        G = 0.5 * (G + G.T)
        assert np.linalg.eigvalsh(G).min() >= -1e-12 * np.trace(G)


def test_group_gram_is_the_average_of_the_diagram_blocks():
    rng = np.random.default_rng(5)
    dgms = [_diagram(rng, int(n)) for n in rng.integers(1, 30, 9)]
    groups = [dgms[0:1], dgms[1:6], [], dgms[6:9]]
    for par in (PSS, PWG):
        G1, _, _ = dk.gram([[d] for d in dgms], [[d] for d in dgms], par)
        G, A, N = dk.gram(groups, groups, par)
        off = [0, 1, 6, 6, 9]
        for g in range(4):
            for h in range(4):
                if g == 2 or h == 2:
                    assert np.isnan(G[g, h]) and N[g, h] == 0
                else:
                    want = G1[off[g]:off[g + 1], off[h]:off[h + 1]].mean()
                    assert abs(G[g, h] - want) <= 1e-12 * A[g, h]


SHAPES = [(1, 1), (3, 65), (46, 46), (64, 63), (46, 122), (130, 17)]


@pytest.mark.parametrize("sigma", [0.01, 0.1, 1.0])
def test_reference_against_forty_digits(sigma):
    """exp and atan at 40 digits on the FLOAT64 arguments a1, a2 and wc * p, everything else in exact arithmetic:
    |ref - exact| <= 1.0 * (A + N_t |ref|) * 2^-53.  (With exp at the exact-arithmetic arguments instead the bound breaks,
    32 at a1 near -596: the arguments are part of the contract.)"""
    import mpmath
    mp = mpmath.mp.clone()
    mp.dps = 40
    to_mp = np.frompyfunc(mp.mpf, 1, 1)
    mp_exp, mp_atan = np.frompyfunc(mp.exp, 1, 1), np.frompyfunc(mp.atan, 1, 1)
    rng = np.random.default_rng(7)
    worst = 0.0
    wc = 1.5
    for (m, n) in SHAPES:
        A, B = _diagram(rng, m), _diagram(rng, n)
        for mirror in (1, 0):
            ninv = -1.0 / (8.0 * sigma) if mirror else -1.0 / (2.0 * sigma * sigma)
            a1, a2 = dk.arguments(A, B, ninv, mirror)
            E = mp_exp(to_mp(a1))
            if mirror:
                E = E - mp_exp(to_mp(a2))
            for weight in (dk.KW_ONE, dk.KW_PERS, dk.KW_ATAN):
                scale = 1.0 / (8.0 * np.pi * sigma) if mirror else 1.0
                par = (ninv, mirror, scale, weight, wc)
                ref, mag, nt = dk.kernel_value(A, B, par)
                w = []
                for F in (A, B):
                    p = F[:, 1] - F[:, 0]
                    w.append(to_mp(np.ones(len(F))) if weight == dk.KW_ONE else to_mp(p) if weight == dk.KW_PERS
                             else mp_atan(to_mp(wc * p)))
                exact = mp.mpf(scale) * (w[0][:, None] * w[1][None, :] * E).sum()
                bound = (mag + nt * abs(ref)) * dk.U
                err = float(abs(mp.mpf(ref) - exact))
                if bound > 0:
                    worst = max(worst, err / bound)
                assert err <= 1.0 * bound, (m, n, mirror, weight, err, bound)
    print("sigma", sigma, "worst |ref - exact| / bound:", worst)
