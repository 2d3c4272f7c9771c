"""
CPU evaluation of the Frechet mean of a group of persistence diagrams (helper module, no tests in it).

The written contract is include/tdaeeg.h, tda_frechet_mean_dev: the algorithm of Turner, Mileyko, Mukherjee and Harer
(2014) with the order-2 L2 costs of tda_wasserstein_q_batch.  The costs and gains come from wasserstein_q_ref, every
matching from scipy's linear_sum_assignment on the gains with the smaller diagram in the row role (Y on a tie), and the
sums run in the orders the header states (V_i: 64 partial sums by index mod 64, folded at distances 32 .. 1).

  frechet_mean   one group -> Result(mean, cnt, var, iters, status, sizes, energies)
  GROUPS         the seeded groups the GPU tests use; tests/test_frechet_model.py certifies on the CPU that every one of
                 them gives the same bytes when each matching is solved on the row- and column-reversed problem, so the
                 matchings met along the way are unique and the GPU has to reproduce the bits
  singles, other_groups   the remaining groups of the GPU tests, certified the same way
"""
import collections

import numpy as np
from scipy.optimize import linear_sum_assignment

import wasserstein_q_ref as wq

MAX_ITER, MAX_POINTS, MAX_GROUP = 64, 512, 64
TRUNCATED, NOT_CONVERGED, TOO_LARGE = 1, 8, 16

Result = collections.namedtuple("Result", "mean cnt var iters status sizes energies")


def finite_rows(d):
    d = np.asarray(d, dtype=np.float64).reshape(-1, 2)
    return d[np.isfinite(d).all(axis=1)]


def lane_sum(y_terms, x_terms):
    """The header's order: 64 partial sums by index mod 64, Y terms then X terms, folded at distances 32 .. 1."""
    a = np.zeros(64)
    for terms in (y_terms, x_terms):
        for q, v in terms:
            a[q % 64] = a[q % 64] + v
    idx = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        a = a + a[idx ^ off]
    return float(a[0])


def match(Y, X, reverse=False):
    """mate (len(Y),): the row of X really matched to each row of Y, or -1; V, the value of the matching."""
    n, ni = len(Y), len(X)
    mate = np.full(n, -1)
    y_row = n <= ni
    R, Cc = (Y, X) if y_row else (X, Y)
    if n and ni:
        C, s, t = wq.costs(R, Cc, 2, "l2")
        g = wq.gains(C, s, t)
        if reverse:
            ri, ci = linear_sum_assignment(g[::-1, ::-1])
            ri, ci = len(R) - 1 - ri, len(Cc) - 1 - ci
        else:
            ri, ci = linear_sum_assignment(g)
        real = g[ri, ci] < 0.0
        ri, ci = ri[real], ci[real]
        if y_row:
            mate[ri] = ci
        else:
            mate[ci] = ri
    cost = lambda j, x: wq.point_cost(np.abs(Y[j, 0] - X[x, 0]), np.abs(Y[j, 1] - X[x, 1]), 2, "l2")
    sy, sx = wq.diag_cost(Y, 2, "l2"), wq.diag_cost(X, 2, "l2")
    taken = set(int(x) for x in mate if x >= 0)
    V = lane_sum([(j, cost(j, mate[j]) if mate[j] >= 0 else sy[j]) for j in range(n)],
                 [(r, sx[r]) for r in range(ni) if r not in taken])
    return mate, V


def pull(k, m, wb, wd):
    """The new row of a point with k matches out of m: the mean of the matches, pulled to the diagonal m - k times."""
    if k == m:
        return wb, wd
    k, m = np.float64(k), np.float64(m)
    h = 0.5 * (wb + wd)
    return ((k * wb) + ((m - k) * h)) / m, ((k * wd) + ((m - k) * h)) / m


def frechet_mean(dgms, max_iter=32, cap_out=MAX_POINTS, reverse=False):
    """dgms: the KEPT diagrams of a group, in buffer order.  As the header: mean (cap_out, 2) NaN beyond the count."""
    assert 1 <= max_iter <= MAX_ITER and cap_out >= 1
    X = [finite_rows(d) for d in dgms]
    m = len(X)
    nan_mean = np.full((cap_out, 2), np.nan)
    fail = lambda st, it, sizes, en: Result(nan_mean, 0, np.nan, it, st, sizes, en)
    if m == 0:
        return fail(0, 0, [], [])
    if m > MAX_GROUP or max(len(x) for x in X) > MAX_POINTS:
        return fail(TOO_LARGE, 0, [], [])
    Y = X[0].copy()
    sizes, energies, status = [], [], 0
    for t in range(max_iter):
        n = len(Y)
        sizes.append(n)
        sb, sd, k = np.zeros(n), np.zeros(n), np.zeros(n, int)
        spawn, F = [], np.float64(0.0)
        for Xi in X:
            mate, V = match(Y, Xi, reverse)
            F = F + V
            hit = mate >= 0
            sb[hit] = sb[hit] + Xi[mate[hit], 0]
            sd[hit] = sd[hit] + Xi[mate[hit], 1]
            k[hit] += 1
            taken = set(int(x) for x in mate[hit])
            spawn += [pull(1, m, Xi[r, 0], Xi[r, 1]) for r in range(len(Xi)) if r not in taken]
        energies.append(float(F))
        rows = [pull(k[j], m, sb[j] / np.float64(k[j]), sd[j] / np.float64(k[j])) for j in range(n) if k[j] > 0] + spawn
        Y1 = np.array(rows, dtype=np.float64).reshape(-1, 2)
        iters = t + 1
        if Y1.shape == Y.shape and Y1.tobytes() == Y.tobytes():
            break
        if len(Y1) > MAX_POINTS:
            return fail(TOO_LARGE, iters, sizes, energies)
        if t + 1 == max_iter:
            status = NOT_CONVERGED
            break
        Y = Y1
    mean = nan_mean.copy()
    mean[:min(len(Y), cap_out)] = Y[:cap_out]
    if len(Y) > cap_out:
        status |= TRUNCATED
    return Result(mean, len(Y), float(F / np.float64(m)), iters, status, sizes, energies)


def batch(rows, cnt, seg_off=None, status=None, skip_mask=0, max_iter=32, cap_out=MAX_POINTS, reverse=False):
    """frechet_mean over diagram buffers, as tda_frechet_mean_batch takes them: (mean, cnt, var, iters, status) arrays."""
    n, cap, _ = rows.shape
    off = np.arange(n + 1) if seg_off is None else np.clip(np.asarray(seg_off), 0, n)
    out = []
    for g in range(len(off) - 1):
        ws = [w for w in range(off[g], off[g + 1]) if status is None or not (int(status[w]) & skip_mask)]
        out.append(frechet_mean([rows[w, :max(0, min(int(cnt[w]), cap))] for w in ws], max_iter, cap_out, reverse))
    return (np.stack([r.mean for r in out]), np.array([r.cnt for r in out], np.int32), np.array([r.var for r in out]),
            np.array([r.iters for r in out], np.int32), np.array([r.status for r in out], np.int32))


# ---- the seeded groups of the GPU tests --------------------------------------------------------------------------------
def random_group(seed, m, lo, hi, spread=1.0):
    """m diagrams of lo..hi points of continuous random float64: births in [0, spread), persistences in (0.05, 0.6)."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(m):
        k = int(rng.integers(lo, hi + 1))
        b = rng.random(k) * spread
        out.append(np.stack([b, b + 0.05 + 0.55 * rng.random(k)], 1))
    return out


def h0_group(seed, m=15, k=46):
    """H0-like: birth 0, float32 deaths, ascending."""
    rng = np.random.default_rng(seed)
    return [np.stack([np.zeros(k), np.sort((0.1 + 1.4 * rng.random(k)).astype(np.float32)).astype(np.float64)], 1) for _ in range(m)]


def far_group(m, k):
    """m diagrams of k points each, every point far from every other: nothing is ever matched across diagrams."""
    return [np.stack([100.0 * (i * k + np.arange(k)), 100.0 * (i * k + np.arange(k)) + 1.0 + i / 64.0], 1) for i in range(m)]


def with_inf(d):
    """d with an essential row (b, +inf) after every third row."""
    out = []
    for i, r in enumerate(d):
        out.append(r)
        if i % 3 == 0:
            out.append([r[0], np.inf])
    return np.array(out, dtype=np.float64).reshape(-1, 2)


def singles(n=525):
    """n one-diagram groups of 0..9 points, essential rows among them."""
    return [with_inf(random_group(1000 + i, 1, 0, 9)[0]) for i in range(n)]


def other_groups():
    """The groups of the GPU tests that are not in GROUPS: the far points of the size limits, the group whose first
    diagram a status word removes."""
    return {"far_8x60": far_group(8, 60), "far_9x60": far_group(9, 60), "m5_s0_without_first": GROUPS["m5_s0"][1:]}


def _groups():
    g = {}
    for m in (1, 2, 3, 5, 15):
        for s in range(2):
            g[f"m{m}_s{s}"] = random_group(100 * m + s, m, 0, 12)
    g["mean_over_64"] = random_group(7, 4, 24, 30, spread=40.0)          # sparse: the mean collects most points of all four
    g["inputs_over_128"] = random_group(8, 2, 130, 140, spread=3.0)
    g["h0_like"] = h0_group(9)
    g["with_empty"] = [np.zeros((0, 2))] + random_group(10, 3, 1, 8) + [np.zeros((0, 2))]
    g["first_empty_only_then_points"] = [np.zeros((0, 2)), np.zeros((0, 2))] + random_group(11, 1, 3, 3)
    g["all_empty"] = [np.zeros((0, 2))] * 3
    g["with_inf"] = [with_inf(d) for d in random_group(12, 4, 3, 10)]
    return g


GROUPS = _groups()
