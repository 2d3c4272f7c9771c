"""
CPU statement of the Euler characteristic curves (include/tdaeeg.h, "Euler characteristic curves"): the key preparation of
the three input forms through the oracle, the definition of the simplex counts twice (exhaustive subsets; adjacency-matrix
algebra), a restatement of the kernel's mask route with Python ints, and the group mean twice.  Test infrastructure only.

Keys are handed round as a symmetric (n, n) float32 matrix; only k[a][b], a > b, is the contract.
"""
import itertools

import numpy as np

from oracle import brute, port

TDA_WIN_DEGENERATE = 4
TDA_WIN_TOO_LARGE = 16
MAX_POINTS = 128


# ---------------------------------------------------------------- keys
def keys_dm(dist, symmetrise=True):
    """Distance-matrix input: scripts/utils.py:137-139 and the float32 cast, or the entries (i, j), i < j."""
    return brute.eeg_prepare(dist, symmetrise)


def keys_cloud(pc, normalise=True):
    """Point-cloud input: per-column min-max, sklearn's distance, float32.  The kernel's key of a > b adds |x_a|^2 before
    |x_b|^2: the LOWER triangle of oracle.port.cloud_dm."""
    pc = np.asarray(pc, dtype=np.float64)
    d = port.cloud_dm(port.minmax_normalise(pc) if normalise else pc).astype(np.float32)
    low = np.tril(d, -1)
    return low + low.T


def keys_takens(sig, tau, dim=3, subsample=2):
    return keys_cloud(port.takens(sig, dim, int(tau), subsample), True)


def takens_points(n_t, tau, dim, subsample):
    nn = n_t - (dim - 1) * tau
    return (nn + subsample - 1) // subsample if nn > 0 else 0


# ---------------------------------------------------------------- the definition
def adjacency(keys, t, thresh):
    """Edge {a, b} is present iff k <= (float)thresh and (double)k <= t: plain IEEE comparisons (NaN: absent)."""
    k = np.asarray(keys, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        A = (k <= np.float32(thresh)) & (k.astype(np.float64) <= np.float64(t))
    A = np.tril(A, -1)
    return A | A.T


def _finish(rows, n, K):
    rows = np.array(rows, dtype=np.int64).T                      # (K + 1, n_grid)
    chi = sum((-1) ** j * rows[j] for j in range(K + 1))
    out = np.vstack([rows, chi[None]])
    assert np.abs(out).max(initial=0) < 2 ** 31
    return out.astype(np.int32)


def counts_comb(keys, grid, thresh=2.0, K=3):
    """f_j = the number of (j + 1)-subsets whose pairs are all present: itertools.combinations, exhaustive."""
    n = np.asarray(keys).shape[0]
    rows = []
    for t in np.asarray(grid, dtype=np.float64):
        A = adjacency(keys, t, thresh)
        f = [n]
        for j in range(1, K + 1):
            f.append(sum(1 for s in itertools.combinations(range(n), j + 1)
                         if all(A[a, b] for a, b in itertools.combinations(s, 2))))
        rows.append(f)
    return _finish(rows, n, K)


def counts_mat(keys, grid, thresh=2.0, K=3):
    """f_1 = A.sum() / 2, f_2 = trace(A^3) / 6, f_3 = (sum over edges of the edges inside the common neighbourhood) / 6."""
    n = np.asarray(keys).shape[0]
    rows = []
    for t in np.asarray(grid, dtype=np.float64):
        A = adjacency(keys, t, thresh)
        Ai = A.astype(np.int64)
        f = [n, int(Ai.sum()) // 2]
        if K >= 2:
            f.append(int(np.trace(Ai @ Ai @ Ai)) // 6)
        if K >= 3:
            s = 0
            for a, b in zip(*np.nonzero(np.tril(A, -1))):
                N = np.nonzero(A[a] & A[b])[0]
                s += int(Ai[np.ix_(N, N)].sum()) // 2
            assert s % 6 == 0
            f.append(s // 6)
        rows.append(f)
    return _finish(rows, n, K)


def counts_masks(keys, grid, thresh=2.0, K=3):
    """The kernel's route with Python ints: L[v] = the present neighbours below v; per present edge a > b,
    C = L[a] & L[b]; f_2 += popc(C); for c in C from the top, C loses c and f_3 += popc(C & L[c])."""
    k = np.asarray(keys, dtype=np.float32)
    n = k.shape[0]
    th = np.float32(thresh)
    rows = []
    for t in np.asarray(grid, dtype=np.float64):
        L = [0] * n
        for v in range(n):
            for u in range(v):
                if k[v, u] <= th and np.float64(k[v, u]) <= t:
                    L[v] |= 1 << u
        f1 = sum(bin(m).count("1") for m in L)
        f2 = f3 = 0
        for a in range(n):
            for b in range(a):
                if not (L[a] >> b) & 1:
                    continue
                C = L[a] & L[b]
                f2 += bin(C).count("1")
                while C:
                    c = C.bit_length() - 1
                    C &= ~(1 << c)
                    f3 += bin(C & L[c]).count("1")
        rows.append([n, f1, f2, f3][:K + 1])
    return _finish(rows, n, K)


# ---------------------------------------------------------------- blocks of the input forms, with their status words
def block_cloud(pc, n_pts, grid, thresh=2.0, K=3, normalise=True, counts=counts_mat):
    """(block, status) of one window of the cloud form: pc (p_cap, dim), the first n_pts rows count."""
    p_cap = pc.shape[0]
    if n_pts > min(p_cap, MAX_POINTS):
        return np.zeros((K + 2, len(grid)), np.int32), TDA_WIN_TOO_LARGE
    if n_pts < 3:
        return np.zeros((K + 2, len(grid)), np.int32), TDA_WIN_DEGENERATE
    return counts(keys_cloud(pc[:n_pts], normalise), grid, thresh, K), 0


def block_takens(sig, tau, grid, thresh=2.0, K=3, dim=3, subsample=2, counts=counts_mat):
    P = takens_points(len(sig), tau, dim, subsample)
    if tau < 1 or P > MAX_POINTS:
        return np.zeros((K + 2, len(grid)), np.int32), TDA_WIN_TOO_LARGE
    if P < 3:
        return np.zeros((K + 2, len(grid)), np.int32), TDA_WIN_DEGENERATE
    return counts(keys_takens(sig, tau, dim, subsample), grid, thresh, K), 0


# ---------------------------------------------------------------- group means
def _groups(n_win, seg_off):
    if seg_off is None:
        return [(w, w + 1) for w in range(n_win)]
    return [(max(int(seg_off[g]), 0), min(int(seg_off[g + 1]), n_win)) for g in range(len(seg_off) - 1)]


def _kept(w0, w1, status_in, skip_mask):
    return [w for w in range(w0, w1) if status_in is None or not (int(status_in[w]) & skip_mask)]


def mean_np(blocks, seg_off=None, status_in=None, skip_mask=0):
    """np.mean(stack, axis=0) on the integer rows; NaN for an empty group."""
    blocks = np.asarray(blocks)
    out = np.full((len(_groups(len(blocks), seg_off)),) + blocks.shape[1:], np.nan)
    for g, (w0, w1) in enumerate(_groups(len(blocks), seg_off)):
        kept = _kept(w0, w1, status_in, skip_mask)
        if kept:
            out[g] = np.mean(np.stack([blocks[w] for w in kept]), axis=0)
    return out


def mean_exact(blocks, seg_off=None, status_in=None, skip_mask=0):
    """(double)S / (double)m with S the exact integer sum."""
    blocks = np.asarray(blocks)
    out = np.full((len(_groups(len(blocks), seg_off)),) + blocks.shape[1:], np.nan)
    for g, (w0, w1) in enumerate(_groups(len(blocks), seg_off)):
        kept = _kept(w0, w1, status_in, skip_mask)
        if kept:
            S = np.zeros(blocks.shape[1:], dtype=object)
            for w in kept:
                S = S + blocks[w].astype(object)
            out[g] = np.array([float(int(s)) / float(len(kept)) for s in S.ravel()]).reshape(S.shape)
    return out


# ---------------------------------------------------------------- Betti numbers off diagrams
def betti(rows, t):
    """The number of rows with b <= t < d."""
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, 2)
    return int(((rows[:, 0] <= t) & (t < rows[:, 1])).sum())
