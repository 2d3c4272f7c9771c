"""
Inputs of the recurrence tests, shared by tests/test_recurrence_model.py (CPU) and tests/test_gpu_recurrence.py: distance
matrices with recurrence curves worked out by hand, and the trajectories whose plots have lines of many lengths (the
inputs on which the entropy bar of recurrence_ref is measured).  Test infrastructure only.
"""
import numpy as np

IN, OUT, SCALE = 0.0, 1.0, 0.5            # a recurrence has distance IN, anything else OUT; the plot is read at SCALE


# ---------------------------------------------------------------- trajectories
def trajectory_dm(n_win, n, seed, ties=False):
    """Distance matrices of noisy closed curves sampled in time order: the plots have diagonal lines (the curve comes
    back), vertical lines (it slows down) and isolated points (the noise).  ties=True rounds the distances to a grid of
    0.05, so that many keys are equal and grid points fall on them."""
    rng = np.random.default_rng(seed)
    out = np.zeros((n_win, n, n))
    for w in range(n_win):
        i = np.arange(n)
        f = rng.uniform(0.02, 0.11)
        ph = 2 * np.pi * f * i + 0.6 * np.sin(2 * np.pi * rng.uniform(0.01, 0.04) * i)
        x = np.stack([np.cos(ph), np.sin(ph), 0.3 * np.sin(2.3 * ph)], axis=1) + rng.normal(0, 0.04, (n, 3))
        d = np.sqrt(((x[:, None, :] - x[None, :, :]) ** 2).sum(-1))
        out[w] = np.round(d / 0.05) * 0.05 if ties else d
    return out


def grid_of(n_grid, seed):
    """[0.45] and then unsorted scales in [0.05, 1.2]."""
    rng = np.random.default_rng(seed)
    return np.concatenate([[0.45], rng.random(max(n_grid - 1, 0)) * 1.15 + 0.05])[:n_grid]


# (n, n_grid, windows, theiler, l_min, v_min, ties): the mask word boundary and the last bit of each word, fewer and more
# grid points than waves, every theiler that meets a word boundary or the window's own size, l_min and v_min in {1, 2, 5}
DM_CASES = [
    (1, 3, 2, 1, 2, 2, False), (2, 4, 2, 1, 1, 1, False), (3, 5, 2, 2, 2, 1, False), (47, 9, 2, 1, 2, 2, True),
    (63, 3, 2, 1, 2, 2, False), (64, 4, 2, 2, 1, 5, False), (65, 5, 2, 1, 5, 1, True), (127, 9, 1, 2, 2, 2, False),
    (128, 5, 1, 1, 2, 2, False), (128, 4, 1, 2, 5, 5, True),
    (128, 3, 1, 63, 2, 2, False), (128, 3, 1, 64, 1, 2, False), (128, 3, 1, 65, 2, 1, False), (128, 3, 1, 127, 1, 1, False),
    (128, 3, 1, 128, 2, 2, False), (65, 3, 1, 63, 2, 2, False), (65, 3, 1, 64, 1, 1, False), (65, 3, 1, 65, 2, 2, False),
    (65, 3, 1, 128, 2, 2, False), (64, 3, 1, 63, 1, 1, False), (64, 3, 1, 64, 2, 2, False), (9, 256, 1, 1, 2, 2, True),
]


def dm_case(case):
    """(dms, grid) of an entry of DM_CASES."""
    n, n_grid, n_win, theiler, l_min, v_min, ties = case
    return trajectory_dm(n_win, n, 1000 + 7 * n + theiler, ties), grid_of(n_grid, 200 + n_grid + n)


# ---------------------------------------------------------------- plots with known answers
def dm_of_plot(R):
    """A symmetric distance matrix whose plot at SCALE (theiler = 1) is R."""
    d = np.where(R, IN, OUT).astype(np.float64)
    np.fill_diagonal(d, 0.0)
    return d


def periodic(n, p):
    """D[i][j] = 0 if (i - j) % p == 0, else 1."""
    i = np.arange(n)
    return np.where((i[:, None] - i[None, :]) % p == 0, IN, OUT).astype(np.float64)


def complete(n):
    return dm_of_plot(~np.eye(n, dtype=bool))


def laminar(n, s, b):
    """b identical consecutive points s .. s + b - 1; every other pair is far."""
    i = np.arange(n)
    blk = (i >= s) & (i < s + b)
    return dm_of_plot(blk[:, None] & blk[None, :] & ~np.eye(n, dtype=bool))


def checkerboard(n):
    """The board on which every line has length 1: R[i][j] = 1 iff i != j and i and j are both even, so that no two
    recurrences touch along a column or along a diagonal.  (The board R = [(i + j) odd] would not do: its odd diagonals are
    full lines.)"""
    i = np.arange(n)
    ev = i % 2 == 0
    return dm_of_plot(ev[:, None] & ev[None, :] & ~np.eye(n, dtype=bool))


def _entropy(H, lines, lo):
    """The header's sum from a dict length -> count."""
    S = np.float64(0.0)
    for l in sorted(H):
        if l >= lo and H[l] > 0:
            p = np.float64(H[l]) / np.float64(lines)
            S = S - p * np.log(p)
    return float(S)


def answer(n, theiler, l_min, v_min, HD, HV):
    """(counts, measures) from the line-length histograms worked out by hand (dicts length -> count)."""
    rec = sum(l * c for l, c in HD.items())
    assert rec == sum(l * c for l, c in HV.items())
    cnt = [rec]
    for H, lo in ((HD, l_min), (HV, v_min)):
        cnt += [sum(c for l, c in H.items() if l >= lo), sum(l * c for l, c in H.items() if l >= lo),
                max([l for l, c in H.items() if c > 0], default=0)]
    N = (n - theiler) * (n - theiler + 1) if theiler <= n else 0
    div = lambda a, b: float(a) / float(b) if b else 0.0          # noqa: E731
    mea = [div(rec, N), div(cnt[2], rec), div(cnt[2], cnt[1]), _entropy(HD, cnt[1], l_min),
           div(cnt[5], rec), div(cnt[5], cnt[4]), _entropy(HV, cnt[4], v_min)]
    return cnt, mea


def _add(H, l, c=1):
    if l >= 1:
        H[l] = H.get(l, 0) + c


def _complete_hists(m, theiler):
    """K_m in time order: diagonal k (theiler <= k < m) is one line of m - k in each triangle; column j has the run of the
    rows 0 .. j - theiler and the run of the rows j + theiler .. m - 1, split by the band."""
    HD, HV = {}, {}
    for k in range(theiler, m):
        _add(HD, m - k, 2)
    for j in range(m):
        _add(HV, j - theiler + 1)
        _add(HV, m - j - theiler)
    return HD, HV


# name -> (distance matrix, (theiler, l_min, v_min), the seven counts in row order, the seven measures)
def known():
    out = {}
    for n in (65, 128):
        # periodic, p = 7: the diagonals 7, 14, ... are full lines n - 7 m (the shortest has 2 points: 65 - 63, 128 - 126);
        # a column holds isolated points.  determinism 1.0, laminarity 0.0
        HD, HV = {}, {}
        for k in range(7, n, 7):
            _add(HD, n - k, 2)
            _add(HV, 1, 2 * (n - k))
        cnt, mea = answer(n, 1, 2, 2, HD, HV)
        assert mea[1] == 1.0 and mea[4] == 0.0 and cnt[3] == n - 7 and cnt[6] == 1
        out[f"periodic_{n}"] = (periodic(n, 7), (1, 2, 2), cnt, mea)
        # complete graph, theiler 1 and across the word boundary
        for theiler, l_min, v_min in ((1, 2, 2), (2, 5, 1), (64, 1, 2)):
            HD, HV = _complete_hists(n, theiler)
            cnt, mea = answer(n, theiler, l_min, v_min, HD, HV)
            assert mea[0] == 1.0 and cnt[3] == n - theiler == cnt[6]
            out[f"complete_{n}_theiler{theiler}"] = (complete(n), (theiler, l_min, v_min), cnt, mea)
        # laminar block of 9 points over the word boundary (60 .. 68) or at the end of the window
        s = 60 if n == 128 else n - 9
        HD, HV = _complete_hists(9, 1)
        cnt, mea = answer(n, 1, 2, 2, HD, HV)
        assert cnt[0] == 72 and cnt[3] == 8 == cnt[6]
        out[f"laminar_{n}"] = (laminar(n, s, 9), (1, 2, 2), cnt, mea)
        # checkerboard: lines of length 1 only
        e = (n + 1) // 2
        cnt, mea = answer(n, 1, 2, 2, {1: e * (e - 1)}, {1: e * (e - 1)})
        assert cnt == [e * (e - 1), 0, 0, 1, 0, 0, 1] and mea[1:] == [0.0] * 6
        out[f"checkerboard_{n}"] = (checkerboard(n), (1, 2, 2), cnt, mea)
        # wide band: nothing is left
        for theiler in (n, 128):
            out[f"wide_band_{n}_theiler{theiler}"] = (complete(n), (theiler, 1, 1), [0] * 7, [0.0] * 7)
    # small n
    out["n1"] = (np.zeros((1, 1)), (1, 1, 1), [0] * 7, [0.0] * 7)
    out["n2_lmin2"] = (complete(2), (1, 2, 2), [2, 0, 0, 1, 0, 0, 1], [1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0])
    out["n2_lmin1"] = (complete(2), (1, 1, 1), [2, 2, 2, 1, 2, 2, 1], [1.0, 1.0, 1.0, 0.0, 1.0, 1.0, 0.0])
    out["n2_theiler2"] = (complete(2), (2, 1, 1), [0] * 7, [0.0] * 7)
    return out
