"""
CPU restatement of the prepared route of the sliced Wasserstein distance (csrc/sliced_matrix.hip; helper module, no tests
in it): every diagram sorted once per direction, two merges and a sum per pair.

  prepare          the two ascending lists of every direction of one diagram (kind 0: its rows, kind 1: its images)
  corank_merge     the merge of two ascending lists as the kernel makes it: the lane of rank e finds its element by a
                   binary search over how many of the first e + 1 elements come from the first list, SEARCH trips always
  prepared_route   prepare + merge + the pair kernel's order of additions: the bits the GPU gives
  matrix_entry     (mean, pairs, flags) of one entry of the matrix from the values and status words of its positions
"""
import numpy as np

import sliced_ref
from sliced_ref import clean

SEARCH = 10                     # ceil(log2(TDA_SW_MAX_POINTS + 1))
assert 2 ** (SEARCH - 1) < sliced_ref.SW_MAX_POINTS + 1 <= 2 ** SEARCH
TOO_LARGE, NO_PAIR, DEGENERATE = 16, 32, 4


def prepare(D, dirs):
    """(M, 2, m) ascending projections of a raw diagram: [k, 0] of its rows, [k, 1] of its images, by the formula of the
    header ((c * x) + (s * y), also for the images) and the network of the pair kernel."""
    D = clean(D)
    h = 0.5 * (D[:, 0] + D[:, 1])
    m = len(D)
    out = np.empty((len(dirs), 2, m))
    for k, (c, s) in enumerate(np.asarray(dirs, dtype=np.float64)):
        out[k, 0] = sliced_ref.network_sort((c * D[:, 0]) + (s * D[:, 1]))[:m]
        out[k, 1] = sliced_ref.network_sort((c * h) + (s * h))[:m]
    return out


def corank_merge(X, Y):
    """The nx + ny elements of the merge of the ascending lists X and Y, each found on its own: for rank e, K = e + 1,
    the smallest i in [max(0, K - ny), min(K, nx)] with i at the upper end or X[i] > Y[K - i - 1] is the number of
    elements of X among the first K, and the element is max(X[i - 1], Y[K - i - 1])."""
    X, Y = np.asarray(X, dtype=np.float64), np.asarray(Y, dtype=np.float64)
    nx, ny = len(X), len(Y)
    assert nx >= 1 and ny >= 1
    K = np.arange(nx + ny) + 1
    lo, hi = np.maximum(K - ny, 0), np.minimum(K, nx)
    assert (lo <= hi).all()
    for _ in range(SEARCH):
        active = lo < hi
        mid = (lo + hi) >> 1
        assert (~active | ((mid < nx) & (K - mid - 1 >= 0) & (K - mid - 1 < ny))).all()     # no read outside a list
        above = X[np.minimum(mid, nx - 1)] > Y[np.clip(K - mid - 1, 0, ny - 1)]
        hi = np.where(active & above, mid, hi)
        lo = np.where(active & ~above, mid + 1, lo)
    assert (lo == hi).all()
    i, j = lo, K - lo
    assert (i >= 0).all() and (i <= nx).all() and (j >= 0).all() and (j <= ny).all()
    a = np.where(i > 0, X[np.maximum(i - 1, 0)], -np.inf)
    b = np.where(j > 0, Y[np.maximum(j - 1, 0)], -np.inf)
    return np.where(a > b, a, b)


def prepared_route(PA, PB):
    """The distance of a pair from prepare(A, dirs) and prepare(B, dirs), additions in the pair kernel's order."""
    M, m, n = PA.shape[0], PA.shape[2], PB.shape[2]
    N = m + n
    if N > sliced_ref.SW_MAX_POINTS:
        return float("nan")
    lane = np.arange(64)
    Ls = np.zeros(sliced_ref.MAX_DIRECTIONS)
    for k in range(M):
        u = corank_merge(PA[k, 0], PB[k, 1])
        v = corank_merge(PB[k, 0], PA[k, 1])
        t = np.abs(u - v)
        acc = np.zeros(64)
        for e0 in range(0, N, 64):
            e = e0 + lane
            acc = acc + np.where(e < N, t[np.minimum(e, N - 1)], 0.0)
        Ls[k] = sliced_ref._wave_sum(acc)
    acc = np.zeros(64)
    for k0 in range(0, M, 64):
        k = k0 + lane
        acc = acc + np.where(k < M, Ls[np.minimum(k, sliced_ref.MAX_DIRECTIONS - 1)], 0.0)
    return float(sliced_ref._wave_sum(acc) / M)


def matrix_entry(vals, status):
    """One entry of tda_wasserstein_matrix_dev / tda_sliced_matrix_dev from the per-position values and status words of
    its A group (NO_PAIR where a position has no partner): the pairs are the first n positions, n the number of positions
    without NO_PAIR; the mean is np.nanmean over those n values with a pair that has a status counted as NaN."""
    vals, status = np.asarray(vals, dtype=np.float64), np.asarray(status, dtype=np.int32)
    n = int(np.sum((status & NO_PAIR) == 0))
    v = np.where(status[:n] == 0, vals[:n], np.nan)
    # np.nanmean: NaN -> 0.0 in place, numpy's pairwise sum over the n values, / the number of values that are not NaN
    # (without a NaN among them this is np.mean of the n values)
    mean = float(np.nanmean(v)) if (~np.isnan(v)).any() else float("nan")
    flags = int(np.bitwise_or.reduce(status[:n])) & ~(NO_PAIR | DEGENERATE) if n else 0
    return mean, n, flags
