"""
The persistence Fisher distance of include/tdaeeg.h in numpy: the CPU side of every comparison in tests/test_fisher_model.py,
tests/test_gpu_fisher.py and tests/test_gpu_fisher_pass.py.

    P = F_A, images of F_B;  Q = F_B, images of F_A;  Theta = P, Q
    g = exp((dx * dx + dy * dy) * ninv);  r_P(x), r_Q(x) row sums over P, Q;  Z_P, Z_Q their sums over Theta
    a = sqrt(r_P / Z_P), b = sqrt(r_Q / Z_Q);  c2 = sum (a - b)^2;  out = 2 asin(min(0.5 sqrt(c2), 1))

`distance` adds with numpy's sums, `distance_fsum` adds every sum with math.fsum (the same terms, added exactly, rounded
once), so that the order of a reference's additions is not in a comparison against it.

The tolerance of a GPU value against either is (C + 8 N) * 2^-53 absolute.  8 N bounds two summation
orders: N non-negative terms per r, 2N per Z and per c2; a and b are unit vectors, so the chord moves by at most twice the
relative error of its entries; asin has slope at most sqrt 2 on [0, pi / 2].  C stands for the rounding of exp, sqrt, the
division and asin, and is measured: C = 4 q rounded up to a power of two, at least 4, at most 64, where q is the largest
|gpu - distance_fsum| / 2^-53 over every comparison of tests/test_gpu_fisher.py on an MI355X.
"""
import math

import numpy as np

U = 2.0 ** -53
PF_MAX_POINTS = 512
# Measured on an MI355X (tests/test_gpu_fisher.py, every comparison, the test committed with C = 64): q = 2.000, reached
# three times -- the pair grid's 127 finite rows against the empty diagram (N = 127, sigma 0.1), the one-point closed form at
# L = 1, sigma = 0.1, and the Gram test's 0 against 64 finite rows (N = 64).  All three have one side empty, where out is
# large; for an out in [1, pi / 2] a q of 2.000 is ONE unit in the last place (2^-52).  The largest N, 512, gave 0.195
# (sigma 1.0); the step's own H0 pairs (N up to 168) 1.5.  C = 4 q = 8.
Q_MEASURED = (2.0, "pair grid, 127 finite rows against the empty diagram, sigma 0.1")
C = 8


def args(sigma):
    """ninv of the entry points."""
    return -1.0 / (2.0 * float(sigma) * float(sigma))


def finite_rows(dgm, cap=None, cnt=None):
    """F of a diagram: the rows i < min(max(cnt, 0), cap) with both values finite, in stored order."""
    d = np.asarray(dgm, dtype=np.float64).reshape(-1, 2)
    k = len(d) if cnt is None else max(int(cnt), 0)
    if cap is not None:
        k = min(k, int(cap))
    d = d[:k]
    return d[np.isfinite(d).all(axis=1)]


def lists(A, B):
    """(P, Q) of two diagrams, (N, 2) each."""
    FA, FB = finite_rows(A), finite_rows(B)
    ha, hb = 0.5 * (FA[:, 0] + FA[:, 1]), 0.5 * (FB[:, 0] + FB[:, 1])
    P = np.concatenate([FA, np.stack([hb, hb], axis=1)])
    Q = np.concatenate([FB, np.stack([ha, ha], axis=1)])
    return P, Q


def arguments(X, L, ninv):
    """The float64 arguments of exp for the points X against the list L, operation for operation: (|X|, |L|)."""
    dx = X[:, None, 0] - L[None, :, 0]
    dy = X[:, None, 1] - L[None, :, 1]
    return (dx * dx + dy * dy) * ninv


def _finish(rp, rq, zp, zq, add):
    a = np.sqrt(rp / zp)
    b = np.sqrt(rq / zq)
    d = a - b
    c2 = add(d * d)
    return 2.0 * math.asin(min(0.5 * math.sqrt(c2), 1.0))


def distance(A, B, ninv):
    """The definition with numpy's sums."""
    P, Q = lists(A, B)
    if len(P) == 0:
        return 0.0
    T = np.concatenate([P, Q])
    rp = np.exp(arguments(T, P, ninv)).sum(axis=1)
    rq = np.exp(arguments(T, Q, ninv)).sum(axis=1)
    return _finish(rp, rq, rp.sum(), rq.sum(), lambda v: float(v.sum()))


def distance_fsum(A, B, ninv):
    """The definition with every sum added by math.fsum."""
    P, Q = lists(A, B)
    if len(P) == 0:
        return 0.0
    T = np.concatenate([P, Q])
    rp = np.array([math.fsum(row) for row in np.exp(arguments(T, P, ninv))])
    rq = np.array([math.fsum(row) for row in np.exp(arguments(T, Q, ninv))])
    return _finish(rp, rq, math.fsum(rp), math.fsum(rq), lambda v: math.fsum(v))


def n_points(A, B):
    return len(finite_rows(A)) + len(finite_rows(B))


def tolerance(N, c=None):
    c = C if c is None else c
    return (c + 8.0 * np.asarray(N, dtype=np.float64)) * U


def one_point_closed_form(L, sigma):
    """One point (b, b + L) against the empty diagram: P = {x}, Q = {image of x}, at distance L / sqrt 2; the
    Bhattacharyya coefficient is sech(L^2 / (8 sigma^2)) and the angle 2 atan(tanh(L^2 / (16 sigma^2)))."""
    return 2.0 * math.atan(math.tanh(L * L / (16.0 * sigma * sigma)))


ONE_POINT_CASES = [(2.0, 10.0), (1.0, 2.0), (1.0, 1.0), (0.5, 0.25), (1.0, 0.25), (1.0, 0.1)]      # (L, sigma)
