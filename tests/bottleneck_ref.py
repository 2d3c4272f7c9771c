"""
CPU references for the bottleneck distance between persistence diagrams (helper module, no tests in it).

The written contract (include/tdaeeg.h): diagrams cleaned as safe_wasserstein cleans them (rows with a non-finite entry
dropped; a non-2-D or empty diagram becomes {(0, 0)}), L-infinity ground cost, 0.5 * (d - b) to the diagonal, diagonal
to diagonal free, the minimum over matchings of the largest matched cost.  Every cost is one correctly rounded float64
operation, the answer is one of the costs: the three functions below return the same bits.

  bottleneck_ref        the (M+N)^2 block matrix, binary search over its sorted entries, scipy's bipartite matching
  bottleneck_brute      the minimum over all permutations of the block matrix (M + N <= 8)
  bottleneck_two_cover  what csrc/bottleneck.hip solves, step by step: bounds, bisection on the bit patterns with every
                        probe snapped to a cost, two augmenting-path cover problems per probe
"""
import itertools

import numpy as np
from scipy.sparse import csr_matrix
from scipy.sparse.csgraph import maximum_bipartite_matching


def clean(d):
    d = np.asarray(d, dtype=np.float64)
    if d.ndim != 2 or d.size == 0:
        return np.zeros((1, 2))
    d = d[np.isfinite(d).all(axis=1)]
    return d if len(d) else np.zeros((1, 2))


def costs(A, B):
    """C (M, N), s (M,), t (N,) of two cleaned diagrams."""
    C = np.maximum(np.abs(A[:, None, 0] - B[None, :, 0]), np.abs(A[:, None, 1] - B[None, :, 1]))
    return C, 0.5 * (A[:, 1] - A[:, 0]), 0.5 * (B[:, 1] - B[:, 0])


def block_matrix(A, B):
    C, s, t = costs(A, B)
    M, N = len(A), len(B)
    D = np.full((M + N, M + N), np.inf)
    D[:M, :N] = C
    D[np.arange(M), N + np.arange(M)] = s
    D[M + np.arange(N), np.arange(N)] = t
    D[M:, N:] = 0.0
    return D


def bottleneck_ref(A, B):
    D = block_matrix(clean(A), clean(B))
    vals = np.unique(D[np.isfinite(D)])

    def perfect(v):
        m = maximum_bipartite_matching(csr_matrix(D <= v), perm_type="column")
        return bool((m >= 0).all())

    lo, hi = 0, len(vals) - 1
    while lo < hi:
        mid = (lo + hi) // 2
        if perfect(vals[mid]):
            hi = mid
        else:
            lo = mid + 1
    return float(vals[lo])


def bottleneck_brute(A, B):
    D = block_matrix(clean(A), clean(B))
    n = len(D)
    assert n <= 8
    return float(min(max(D[i, p[i]] for i in range(n)) for p in itertools.permutations(range(n))))


# ---- the kernel's route ---------------------------------------------------------------------------------------------
def _cover(E, must):
    """Is there a matching in the bipartite graph E (rows x columns, bool) that covers every row in `must`?  Breadth-first
    augmenting paths, one row per step, as bn_cover runs them."""
    n_col = E.shape[1]
    match = np.full(n_col, -1)              # row of every column
    mu = np.full(E.shape[0], -1)            # column of every row
    for u0 in np.flatnonzero(must):
        reached = np.zeros(n_col, bool)
        par = np.full(n_col, -1)
        queue, head, vend = [u0], 0, -1
        while head < len(queue) and vend < 0:
            u = queue[head]
            head += 1
            new = E[u] & ~reached
            reached |= new
            par[new] = u
            free = np.flatnonzero(new & (match < 0))
            if len(free):
                vend = free[0]
            else:
                queue += match[new].tolist()
        if vend < 0:
            return False
        v = vend
        while True:
            u = par[v]
            vprev = mu[u]
            match[v], mu[u] = u, v
            if u == u0:
                break
            v = vprev
    return True


def bottleneck_two_cover(A, B, stats=None):
    A, B = clean(A), clean(B)
    C, s, t = costs(A, B)
    cand = np.concatenate([C.ravel(), s, t])

    def feasible(v):
        E = C <= v
        return _cover(E, s > v) and _cover(E.T, t > v)

    lo = max(np.minimum(s, C.min(axis=1)).max(), np.minimum(t, C.min(axis=0)).max())
    hi = max(s.max(), t.max())
    probes = 0
    if not lo < hi:
        return float(hi)
    probes += 1
    if feasible(lo):
        return float(lo)
    for _ in range(64):
        lb, hb = np.float64(lo).view(np.uint64), np.float64(hi).view(np.uint64)
        mid = (lb + ((hb - lb) >> np.uint64(1))).view(np.float64)
        below, above = cand[cand <= mid], cand[cand > mid]
        dn = below.max() if len(below) else -1.0
        up = above.min() if len(above) else np.inf
        if dn > lo:
            probes += 1
            if feasible(dn):
                hi = dn
            else:
                lo = mid
        elif not up < hi:
            break
        else:
            probes += 1
            if feasible(up):
                hi = up
                break
            lo = up
    else:
        return float("nan")
    if stats is not None:
        stats.append(probes)
    return float(hi)


# ---- diagrams for the tests -----------------------------------------------------------------------------------------
def random_diagram(rng, n, ties=False):
    """n points with float32-exact coordinates (differences and halves are then exact in float64 as well, but nothing
    relies on that); ties: births in quarters, persistences in fifths."""
    b = rng.uniform(0, 1, n)
    p = rng.uniform(0, 0.6, n)
    if ties:
        b = np.round(b * 4) / 4
        p = np.round(p * 5) / 5
    return np.float32(np.stack([b, b + p], 1)).astype(np.float64).reshape(-1, 2)


def small_pairs(n, seed):
    """n pairs with M, N in [0, 4]; every other one with many ties."""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        M, N = rng.integers(0, 5), rng.integers(0, 5)
        out.append((random_diagram(rng, M, k % 2 == 0), random_diagram(rng, N, k % 2 == 0)))
    return out


KNOWN = [
    ([[0, 1]], [[0, 2]], 1.0),
    ([[0, 1]], np.zeros((0, 2)), 0.5),
    ([[0, 10], [0, 10]], [[0, 10]], 5.0),
    ([[0, 1], [0, np.inf]], [[0, 1]], 0.0),
]
