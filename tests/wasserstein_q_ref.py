"""
CPU references for the Wasserstein distances of order 1 and 2 with the L2 or the L-infinity ground metric (helper module,
no tests in it).

The written contract (include/tdaeeg.h, tda_wasserstein_q_batch): diagrams cleaned as safe_wasserstein cleans them, then,
every line one correctly rounded float64 operation (numpy has no multiply-add),
    dx = fabs(a_b - b_b), dy = fabs(a_d - b_d), p = d - b
    L2:    e = (dx * dx) + (dy * dy);  order 1: C = sqrt(e), diagonal p * 0.7071067811865476
                                       order 2: C = e,       diagonal 0.5 * (p * p)
    L-inf: m = fmax(dx, dy), h = 0.5 * p;  order 1: C = m, diagonal h;  order 2: C = m * m, diagonal h * h
V = the minimum over partial matchings of the matched C plus the diagonal costs of every unmatched point; the result is V
for order 1 and sqrt(V) for order 2.

  value_ref     V by scipy.optimize.linear_sum_assignment on the gains min(0, C - s - t), the original costs re-summed
  value_brute   V as the minimum over ALL partial matchings (M + N <= 8)
  value_line    V by the recurrence of the kernel's equal-birth path, with or without its live-range rule
  distance      V -> the distance
"""
import itertools
import math

import numpy as np
from scipy.optimize import linear_sum_assignment

from bottleneck_ref import clean, random_diagram, small_pairs            # noqa: F401  (the diagrams of the tests)

CP = 0.7071067811865476
VARIANTS = [(1, "l2"), (2, "l2"), (1, "linf"), (2, "linf")]
# the ratio of the larger to the smaller persistence of an equal-birth cell below which its gain is < 0
CUTS = {(1, "l2"): 3.0 + 2.0 * math.sqrt(2.0), (2, "l2"): 2.0 + math.sqrt(3.0), (1, "linf"): 3.0,
        (2, "linf"): (4.0 + math.sqrt(7.0)) / 3.0}


def point_cost(dx, dy, order, ground):
    if ground == "l2":
        e = (dx * dx) + (dy * dy)
        return np.sqrt(e) if order == 1 else e
    m = np.fmax(dx, dy)
    return m if order == 1 else m * m


def diag_cost(D, order, ground):
    p = D[:, 1] - D[:, 0]
    if ground == "l2":
        return p * CP if order == 1 else 0.5 * (p * p)
    h = 0.5 * p
    return h if order == 1 else h * h


def costs(A, B, order, ground):
    """C (M, N), s (M,), t (N,) of two cleaned diagrams."""
    dx = np.abs(A[:, None, 0] - B[None, :, 0])
    dy = np.abs(A[:, None, 1] - B[None, :, 1])
    return point_cost(dx, dy, order, ground), diag_cost(A, order, ground), diag_cost(B, order, ground)


def gains(C, s, t):
    g = (C - s[:, None]) - t[None, :]
    return np.where(g < 0.0, g, 0.0)


def diag_sum(A, B, order, ground):
    """S of the bar: the sum of all diagonal costs of the pair."""
    _, s, t = costs(clean(A), clean(B), order, ground)
    return math.fsum(s) + math.fsum(t)


def value_ref(A, B, order, ground):
    C, s, t = costs(clean(A), clean(B), order, ground)
    g = gains(C, s, t)
    ri, ci = linear_sum_assignment(g)
    real = g[ri, ci] < 0.0
    ri, ci = ri[real], ci[real]
    free_r = np.setdiff1d(np.arange(len(s)), ri)
    free_c = np.setdiff1d(np.arange(len(t)), ci)
    return math.fsum(C[ri, ci]) + math.fsum(s[free_r]) + math.fsum(t[free_c])


def value_brute(A, B, order, ground):
    C, s, t = costs(clean(A), clean(B), order, ground)
    M, N = C.shape
    assert M + N <= 8
    best = math.inf
    for k in range(min(M, N) + 1):
        for rows in itertools.combinations(range(M), k):
            rest_r = math.fsum(s[i] for i in range(M) if i not in rows)
            for cols in itertools.permutations(range(N), k):
                v = math.fsum(C[i, j] for i, j in zip(rows, cols)) + rest_r + math.fsum(t[j] for j in range(N) if j not in cols)
                best = min(best, v)
    return best


def distance(V, order):
    return V if order == 1 else math.sqrt(V)


def distance_ref(A, B, order, ground):
    return distance(value_ref(A, B, order, ground), order)


# ---- the kernel's equal-birth path ------------------------------------------------------------------------------------
LINE_REL, LINE_ABS, LINE_MAX = 1e-9, 1e-150, 1e150
LINE_CUT = {(1, "l2"): 5.828427124746190 * (1.0 + LINE_REL), (2, "l2"): 3.7320508075688772 * (1.0 + LINE_REL),
            (1, "linf"): 3.0 * (1.0 + LINE_REL), (2, "linf"): 2.2152504370215302 * (1.0 + LINE_REL)}


def line_eligible(A, B):
    """rows (the smaller diagram), columns and b0 if the kernel takes its equal-birth path, else None."""
    A, B = clean(A), clean(B)
    R, Cn = (A, B) if len(A) <= len(B) else (B, A)
    b0 = R[0, 0]
    ok = len(R) <= 64 and (R[:, 0] == b0).all() and (Cn[:, 0] == b0).all()
    ok = ok and (np.diff(R[:, 1]) >= 0).all() and (np.diff(Cn[:, 1]) >= 0).all()
    return (R, Cn, b0) if ok else None


def line_gains(R, Cn, order, ground):
    """(rows, columns) computed gains of the equal-birth path: dx is +0.0, the cost a function of dy alone."""
    dy = np.abs(R[:, None, 1] - Cn[None, :, 1])
    if ground == "l2":
        e = dy * dy
        C = np.sqrt(e) if order == 1 else e
    else:
        C = dy if order == 1 else dy * dy
    return gains(C, diag_cost(R, order, ground), diag_cost(Cn, order, ground))


def recurrence(g):
    """F[R-1][C-1] of F[i][j] = min(F[i-1][j], F[i][j-1], F[i-1][j-1] + g_ij) with zero boundaries; 0.0 for an empty
    range.  Row by row: min is exact, so the running minimum along a row has the bits of the cell-by-cell order."""
    R, C = g.shape
    if R == 0 or C == 0:
        return 0.0
    prev = np.zeros(C)
    for i in range(R):
        diag = np.concatenate([[0.0], prev[:-1]]) + g[i]
        prev = np.minimum.accumulate(np.minimum(prev, diag))
    return float(prev[-1])


def live_ranges(b0, dr, dc, order, ground):
    """(ilo, ihi, jlo, jhi) by the kernel's rule; deaths sorted ascending."""
    R, C = len(dr), len(dc)
    cut = LINE_CUT[order, ground]
    mx = max(abs(b0), abs(dr[0]), abs(dr[-1]), abs(dc[0]), abs(dc[-1]))
    if not mx < LINE_MAX:
        return 0, R, 0, C
    p, q = dr - b0, dc - b0
    jlo = int(np.count_nonzero(q * cut + LINE_ABS <= p[0]))
    jhi = max(C - int(np.count_nonzero(q >= p[-1] * cut + LINE_ABS)), jlo)
    if jhi == jlo:
        return 0, 0, jlo, jhi
    ilo = int(np.count_nonzero(p * cut + LINE_ABS <= q[jlo]))
    ihi = max(R - int(np.count_nonzero(p >= q[jhi - 1] * cut + LINE_ABS)), ilo)
    return ilo, ihi, jlo, jhi


def value_line(A, B, order, ground, prune=True):
    """V as the kernel's equal-birth path sums it (all diagonal costs + F, not below 0); None where it is not taken."""
    el = line_eligible(A, B)
    if el is None:
        return None
    R, Cn, b0 = el
    g = line_gains(R, Cn, order, ground)
    if prune:
        ilo, ihi, jlo, jhi = live_ranges(b0, R[:, 1], Cn[:, 1], order, ground)
        g = g[ilo:ihi, jlo:jhi]
    S = math.fsum(diag_cost(R, order, ground)) + math.fsum(diag_cost(Cn, order, ground))
    return max(S + recurrence(g), 0.0)


def h0_diagram(b0, pers, sort=True):
    p = np.asarray(pers, float)
    p = np.sort(p) if sort else p
    return np.stack([np.full(len(p), b0), b0 + p], 1)


_NONE = np.zeros((0, 2))
_A5 = [[0.0, 1.0], [0.25, 0.75], [0.5, 2.0], [1.0, 1.5], [0.125, 0.375]]
# (A, B, {(order, ground): distance}), exact
KNOWN = [
    ([[0, 1]], [[0, 2]], {(1, "l2"): 1.0, (2, "l2"): 1.0, (1, "linf"): 1.0, (2, "linf"): 1.0}),
    ([[0, 1]], _NONE, {(1, "l2"): CP, (2, "l2"): CP, (1, "linf"): 0.5, (2, "linf"): 0.5}),
    (_NONE, _NONE, {v: 0.0 for v in VARIANTS}),
    (_A5, _A5, {v: 0.0 for v in VARIANTS}),                                      # W(A, A), different births
    # both points to the diagonal: order 1 sums 2 + 2 (L-infinity) or 4 c + 4 c (L2); order 2 sqrt(4 + 4) / sqrt(8 + 8)
    ([[0, 4]], [[10, 14]], {(1, "l2"): 4 * CP + 4 * CP, (2, "l2"): 4.0, (1, "linf"): 4.0, (2, "linf"): math.sqrt(8.0)}),
    # (0, 3) to (4, 6): dx = 4, dy = 3 -- L2 5 / 25, L-infinity 4 / 16, against diagonal costs 1.5 + 1 (L-infinity order 1:
    # 2.5 < 4, the diagonal wins), 2.25 + 1 (order 2: 3.25 < 16), L2 order 1 5 c < 5, L2 order 2 4.5 + 2 < 25
    ([[0, 3]], [[4, 6]], {(1, "l2"): 3 * CP + 2 * CP, (2, "l2"): math.sqrt(6.5), (1, "linf"): 2.5, (2, "linf"): math.sqrt(3.25)}),
    # an infinite row is ignored
    ([[0, 1], [0, np.inf]], [[0, 1]], {v: 0.0 for v in VARIANTS}),
    # two points against one, equal births: (0, 10) pairs with (0, 10), the other goes to the diagonal.  (Order 1 with L2
    # is left out: 3 s - 2 s with s = 10 c is not s in every order of the additions.)
    ([[0, 10], [0, 10]], [[0, 10]], {(2, "l2"): math.sqrt(50.0), (1, "linf"): 5.0, (2, "linf"): 5.0}),
]
