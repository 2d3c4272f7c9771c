"""
CPU references for the sliced Wasserstein distance between persistence diagrams (helper module, no tests in it).

The written contract (include/tdaeeg.h), statement for statement: diagrams cleaned as safe_wasserstein cleans them (rows
with a non-finite entry dropped; a non-2-D or empty diagram becomes {(0, 0)}); the image of a row is (h, h) with
h = 0.5 * (b + d); A' = rows of A then images of B, B' = rows of B then images of A; every point is projected as
(c * x) + (s * y) (numpy never fuses the two); both lists sorted; L_k = sum |u_i - v_i|; SW = (sum L_k) / M.

  sliced_wasserstein    the definition with plain sequential sums (order="seq") or math.fsum (order="fsum")
  direction_values      the L_k and the two projected lists of every direction (for the independent anchor)
  network_sort          the sorting network of csrc/sliced.hip restated: same padding, same compare-exchange schedule
  kernel_route          the whole kernel restated, additions in the kernel's order: the bits the GPU gives
  tolerance             the bound of the contract, (N + M + 1) * 2^-52 * value
"""
import math

import numpy as np

from bottleneck_ref import clean, random_diagram            # noqa: F401  (random_diagram: float32-exact points, optional ties)

MAX_DIRECTIONS = 128
SW_MAX_POINTS = 512
XY = np.array([[1.0, 0.0], [0.0, 1.0]])                      # the two-direction table of the exact cases


def augmented(A, B):
    """A', B' (N, 2) and N of two raw diagrams."""
    A, B = clean(A), clean(B)
    ha, hb = 0.5 * (A[:, 0] + A[:, 1]), 0.5 * (B[:, 0] + B[:, 1])
    Ap = np.concatenate([A, np.stack([hb, hb], 1)])
    Bp = np.concatenate([B, np.stack([ha, ha], 1)])
    return Ap, Bp, len(Ap)


def project(P, c, s):
    return (c * P[:, 0]) + (s * P[:, 1])


def direction_values(A, B, dirs):
    """[(L_k by a sequential sum, projections of A', projections of B')] per direction, and N."""
    Ap, Bp, N = augmented(A, B)
    out = []
    for c, s in np.asarray(dirs, dtype=np.float64):
        pu, pv = project(Ap, c, s), project(Bp, c, s)
        t = np.abs(np.sort(pu) - np.sort(pv))
        L = 0.0
        for x in t:
            L += float(x)
        out.append((L, pu, pv))
    return out, N


def sliced_wasserstein(A, B, dirs, order="seq"):
    dirs = np.asarray(dirs, dtype=np.float64)
    Ap, Bp, N = augmented(A, B)
    Ls = []
    for c, s in dirs:
        t = np.abs(np.sort(project(Ap, c, s)) - np.sort(project(Bp, c, s)))
        if order == "fsum":
            Ls.append(math.fsum(t.tolist()))
        else:
            L = 0.0
            for x in t:
                L += float(x)
            Ls.append(L)
    if order == "fsum":
        return math.fsum(Ls) / len(dirs)
    tot = 0.0
    for L in Ls:
        tot += L
    return tot / len(dirs)


def n_points(A, B):
    return len(clean(A)) + len(clean(B))


def tolerance(N, M, value):
    return (N + M + 1) * 2.0 ** -52 * value


# ---- the kernel's route ---------------------------------------------------------------------------------------------
def values_per_lane(N):
    """V of the instantiation a pair of N points takes: 64 V elements per list."""
    return 1 if N <= 64 else 2 if N <= 128 else 4 if N <= 256 else 8


def network_sort(p):
    """The N projections padded with +inf to 64 V elements and sorted by the kernel's bitonic network: for k = 2, 4, ..,
    64 V and j = k/2, .., 1 element e meets e ^ j, ascending where (e & k) == 0; an exchange moves values, it never
    computes one (a strict comparison decides, ties stay).  Returns all 64 V elements."""
    p = np.asarray(p, dtype=np.float64)
    P = 64 * values_per_lane(len(p))
    x = np.concatenate([p, np.full(P - len(p), np.inf)])
    e = np.arange(P)
    k = 2
    while k <= P:
        j = k // 2
        while j >= 1:
            o = x[e ^ j]
            keep_min = ((e & j) != 0) == ((e & k) != 0)
            take = np.where(keep_min, o < x, o > x)
            x = np.where(take, o, x)
            j //= 2
        k *= 2
    return x


def _wave_sum(v):
    """The butterfly over the 64 lanes: partner lane ^ 1, 2, .., 32."""
    lane = np.arange(64)
    for j in (1, 2, 4, 8, 16, 32):
        v = v + v[lane ^ j]
    assert (v == v[0]).all()
    return v[0]


def kernel_route(A, B, dirs):
    """csrc/sliced.hip step by step; element e = 64 r + lane sits in register r of its lane."""
    dirs = np.asarray(dirs, dtype=np.float64)
    Ap, Bp, N = augmented(A, B)
    if N > SW_MAX_POINTS:
        return float("nan")
    V = values_per_lane(N)
    Ls = np.zeros(MAX_DIRECTIONS)
    for k, (c, s) in enumerate(dirs):
        u, v = network_sort(project(Ap, c, s)), network_sort(project(Bp, c, s))
        with np.errstate(invalid="ignore"):
            t = np.abs(u - v)                                       # inf - inf behind N: masked by the rank below
        acc = np.zeros(64)
        for r in range(V):
            e = 64 * r + np.arange(64)
            acc = acc + np.where(e < N, t[e], 0.0)
        Ls[k] = _wave_sum(acc)
    acc = np.zeros(64)
    for k0 in range(0, len(dirs), 64):
        k = k0 + np.arange(64)
        acc = acc + np.where(k < len(dirs), Ls[np.minimum(k, MAX_DIRECTIONS - 1)], 0.0)
    return float(_wave_sum(acc) / len(dirs))


# ---- exact cases on the table XY = [(1, 0), (0, 1)] -----------------------------------------------------------------
KNOWN = [
    ([[0, 1]], [[0, 2]], 1.0),                                      # L = 0.5 and 1.5
    ([[0, 1]], np.zeros((0, 2)), 0.5),                              # against the empty diagram = against {(0, 0)}
    ([[0, 1]], [[0, 0]], 0.5),
    ([[0, 1], [0, np.inf]], [[0, 1]], 0.0),                         # the essential class is ignored
    ([[0, 2], [1, 3]], [[0, 2], [1, 3]], 0.0),
    (np.zeros((0, 2)), np.zeros((0, 2)), 0.0),
]
