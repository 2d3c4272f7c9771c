"""
CPU statement of the recurrence curves (include/tdaeeg.h, "Recurrence curves"): recurrence quantification of a window in
time order at every scale of a grid.  The keys and the presence rule are euler_ref's.  The integers are evaluated twice,
independently: plain loops over the boolean matrix (hist_loops, plot_loops), and the erosion / popcount route of the
kernel restated with Python ints (c_masks, block_masks_one).  The float64 measures are the written functions of those
integers, one IEEE operation at a time, with numpy's log.  entropy_mp evaluates the two entropies from the integer
histograms with 40 digits.  The group means are network_ref's.  Test infrastructure only.

The entropy bar.  Rows 3 and 6 of measures are not bytes: they hold the rounding of log.  ENTROPY_REF_ERR is the largest
|written sum with numpy's log - 40-digit value| over the inputs of the tests (recurrence_cases.DM_CASES and the known
answers); tests/test_recurrence_model.py measures it again and fails when it is larger than written here.  The kernel is
allowed ENTROPY_BAR = 8 * ENTROPY_REF_ERR against the numpy statement: the margin DESIGN.md 3.19 and 3.23 give a device
transcendental (a device log a couple of ulp off where numpy's is within one).  A histogram with a single non-zero bin
has p = 1.0, log(1.0) = 0.0 and the entropy 0.0 as bytes.
"""
import numpy as np

import euler_ref as er
import network_ref as nr

ROWS, MEASURES = 7, 7
COUNT_NAMES = ("recurrences", "diag_lines", "diag_points", "diag_longest", "vert_lines", "vert_points", "vert_longest")
MEASURE_NAMES = ("recurrence_rate", "determinism", "diag_mean", "diag_entropy", "laminarity", "trapping_time",
                 "vert_entropy")
RATIO_ROWS = (0, 1, 2, 4, 5)                 # bytes
ENTROPY_ROWS = (3, 6)                        # to ENTROPY_BAR

ENTROPY_REF_ERR = 9.962952019166134e-15      # measured (2^-46.5, on complete_128_theiler2: over a hundred equal bins)
ENTROPY_BAR = 8 * ENTROPY_REF_ERR            # 7.97e-14


# ---------------------------------------------------------------- the plot
def plot(keys, t, thresh, theiler):
    """R[i][j] = 1 iff i != j, |i - j| >= theiler and the edge {i, j} is present."""
    A = er.adjacency(keys, t, thresh)
    i = np.arange(A.shape[0])
    return A & (np.abs(i[:, None] - i[None, :]) >= theiler)


# ---------------------------------------------------------------- first evaluation: plain loops
def _runs(bits):
    """The lengths of the maximal runs of True in a 1-D boolean sequence."""
    out, run = [], 0
    for b in bits:
        if b:
            run += 1
        elif run:
            out.append(run)
            run = 0
    if run:
        out.append(run)
    return out


def hist_loops(R):
    """(HD, HV): int64 arrays of n entries, entry l - 1 = the number of diagonal / vertical lines of length l, over the
    whole matrix."""
    n = R.shape[0]
    HD, HV = np.zeros(n, np.int64), np.zeros(n, np.int64)
    for k in range(-(n - 1), n):
        for ln in _runs([bool(R[i, i + k]) for i in range(max(0, -k), min(n, n - k))]):
            HD[ln - 1] += 1
    for j in range(n):
        for ln in _runs([bool(R[i, j]) for i in range(n)]):
            HV[ln - 1] += 1
    return HD, HV


def counts_of_hist(R, HD, HV, l_min, v_min):
    n = len(HD)
    ls = np.arange(1, n + 1)
    out = [int(R.sum())]
    for H, lo in ((HD, l_min), (HV, v_min)):
        keep = ls >= lo
        out += [int(H[keep].sum()), int((ls * H)[keep].sum()), int(ls[H > 0].max(initial=0))]
    return out


# ---------------------------------------------------------------- second evaluation: erosion and popcounts
def _popc(m):
    return bin(m).count("1")


def c_masks(masks, l_max):
    """C_l, l = 1 .. l_max + 2 (entry l - 1): E_1 = m, E_{l+1} = E_l & (E_l >> 1), C_l = sum over the masks of popc(E_l)."""
    C = []
    E = list(masks)
    for _ in range(l_max + 2):
        C.append(sum(_popc(e) for e in E))
        E = [e & (e >> 1) for e in E]
    return C


def block_masks_one(R, theiler, l_min, v_min):
    """One plot by the kernel's route: columns as Python ints, the diagonals k >= theiler of the upper triangle as ints over
    the row index, every diagonal count doubled."""
    n = R.shape[0]
    cols = [sum(1 << i for i in range(n) if R[i, j]) for j in range(n)]
    diags = [sum(1 << i for i in range(n - k) if (cols[i + k] >> i) & 1) for k in range(theiler, n)]
    CV, CD = c_masks(cols, n), [2 * c for c in c_masks(diags, n)]
    out = [CV[0]]
    hists = []
    for C, lo in ((CD, l_min), (CV, v_min)):
        H = [C[l - 1] - 2 * C[l] + C[l + 1] for l in range(1, n + 1)]
        lines = C[lo - 1] - C[lo] if lo <= n else 0
        points = C[lo - 1] + (lo - 1) * lines if lo <= n else 0
        longest = max([l for l in range(1, n + 1) if C[l - 1] > 0], default=0)
        out += [lines, points, longest]
        hists.append(np.array(H, np.int64))
    return out, hists[0], hists[1]


# ---------------------------------------------------------------- the measures
def entropy(H, lines, lo):
    """S = 0.0; for l = lo, lo + 1, ... with H(l) > 0: p = (double)H(l) / (double)lines; S = S - p * log(p)."""
    S = np.float64(0.0)
    for l in range(lo, len(H) + 1):
        if H[l - 1] > 0:
            p = np.float64(int(H[l - 1])) / np.float64(int(lines))
            S = S - p * np.log(p)
    return float(S)


def entropy_mp(H, lines, lo):
    """The same value with 40 digits (mpmath), from the integers."""
    import mpmath
    with mpmath.workdps(40):
        S = mpmath.mpf(0)
        for l in range(lo, len(H) + 1):
            if H[l - 1] > 0:
                p = mpmath.mpf(int(H[l - 1])) / mpmath.mpf(int(lines))
                S -= p * mpmath.log(p)
        return S


def _ratio(a, b):
    return float(int(a)) / float(int(b)) if b else 0.0


def measures_of(n, theiler, cnt, HD, HV, l_min, v_min):
    rec, dl, dp, _, vl, vp, _ = cnt
    N = (n - theiler) * (n - theiler + 1) if theiler <= n else 0
    return [_ratio(rec, N), _ratio(dp, rec), _ratio(dp, dl), entropy(HD, dl, l_min),
            _ratio(vp, rec), _ratio(vp, vl), entropy(HV, vl, v_min)]


# ---------------------------------------------------------------- curves
def plot_loops(R, theiler, l_min, v_min):
    HD, HV = hist_loops(R)
    return counts_of_hist(R, HD, HV, l_min, v_min), HD, HV


def curves(keys, grid, theiler=1, l_min=2, v_min=2, thresh=2.0, route=plot_loops, n_hist=None):
    """(counts (ROWS, n_grid) int32, measures (MEASURES, n_grid) float64, hist (2, n_grid, n_hist) int32) of the keys of
    one window; the hist columns at and above n are 0."""
    n = np.asarray(keys).shape[0]
    n_hist = n if n_hist is None else n_hist
    grid = np.asarray(grid, dtype=np.float64)
    cnt = np.zeros((ROWS, len(grid)), np.int64)
    mea = np.zeros((MEASURES, len(grid)), np.float64)
    his = np.zeros((2, len(grid), n_hist), np.int64)
    for g, t in enumerate(grid):
        c, HD, HV = route(plot(keys, t, thresh, theiler), theiler, l_min, v_min)
        cnt[:, g], his[0, g, :n], his[1, g, :n] = c, HD, HV
        mea[:, g] = measures_of(n, theiler, c, HD, HV, l_min, v_min)
    return cnt.astype(np.int32), mea, his.astype(np.int32)


def curves_masks(keys, grid, theiler=1, l_min=2, v_min=2, thresh=2.0, n_hist=None):
    return curves(keys, grid, theiler, l_min, v_min, thresh, block_masks_one, n_hist)


def stack(blocks):
    """A list of (counts, measures, hist) per window -> the three batch arrays."""
    return tuple(np.stack([b[k] for b in blocks]) for k in range(3))


def zeros(n_grid, n_hist):
    return np.zeros((ROWS, n_grid), np.int32), np.zeros((MEASURES, n_grid)), np.zeros((2, n_grid, n_hist), np.int32)


# ---------------------------------------------------------------- blocks of the input forms, with their status words
def block_dm(dist, grid, theiler=1, l_min=2, v_min=2, thresh=2.0, symmetrise=True, route=plot_loops):
    return curves(er.keys_dm(dist, symmetrise), grid, theiler, l_min, v_min, thresh, route)


def block_cloud(pc, n_pts, grid, theiler=1, l_min=2, v_min=2, thresh=2.0, normalise=True):
    """((counts, measures, hist with p_cap columns), status) of one window of the cloud form."""
    p_cap = pc.shape[0]
    if n_pts > min(p_cap, er.MAX_POINTS):
        return zeros(len(grid), p_cap), er.TDA_WIN_TOO_LARGE
    if n_pts < 3:
        return zeros(len(grid), p_cap), er.TDA_WIN_DEGENERATE
    return curves(er.keys_cloud(pc[:n_pts], normalise), grid, theiler, l_min, v_min, thresh, n_hist=p_cap), 0


def block_takens(sig, tau, grid, theiler=1, l_min=2, v_min=2, thresh=2.0, dim=3, subsample=2):
    """The same of one Takens window; hist has MAX_POINTS columns."""
    P = er.takens_points(len(sig), tau, dim, subsample)
    if tau < 1 or P > er.MAX_POINTS:
        return zeros(len(grid), er.MAX_POINTS), er.TDA_WIN_TOO_LARGE
    if P < 3:
        return zeros(len(grid), er.MAX_POINTS), er.TDA_WIN_DEGENERATE
    return curves(er.keys_takens(sig, tau, dim, subsample), grid, theiler, l_min, v_min, thresh, n_hist=er.MAX_POINTS), 0


def entropy_errors(hist, cnt, l_min, v_min):
    """The |numpy statement - 40-digit value| of the two entropies at every grid point of one window's blocks."""
    import mpmath
    out = []
    with mpmath.workdps(40):
        for g in range(cnt.shape[1]):
            for q, lines, lo in ((0, cnt[1, g], l_min), (1, cnt[4, g], v_min)):
                H = hist[q, g]
                out.append(float(abs(entropy_mp(H, lines, lo) - mpmath.mpf(entropy(H, lines, lo)))))
    return out


# ---------------------------------------------------------------- group means
mean_exact = nr.mean_exact                                          # the integer blocks
mean_seq = nr.mean_seq                                              # the measures
