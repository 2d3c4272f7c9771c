"""
The two-sample permutation sums of include/tdaeeg.h ("Two-sample permutation sums") evaluated literally in numpy, an
exactly rounded variant of the same index sets, the statistics and p-values made of them, and an enumerator of all
labellings of a small set.  Shared by the CPU model tests and the GPU tests; nothing here touches the library.
"""
import itertools
import math

import numpy as np

ROW_BLOCK = 64            # TDA_PT_ROW_BLOCK (tests/test_permutation_abi.py holds it against the header)


def perm_sums(D, labels, row_block=ROW_BLOCK):
    """The written order.  D (n_mat, n, ld >= n) float64, labels (P, n) of 0 / 1.  Returns (sums (n_mat, 3, P) = S00, S11,
    S01; n1 (P,) int32).  Vectorised over the relabellings only: every one of them sees the same sequence of additions."""
    D = np.asarray(D, dtype=np.float64)
    lab = np.asarray(labels).astype(bool)
    P, n = lab.shape
    out = np.empty((D.shape[0], 3, P))
    with np.errstate(invalid="ignore", over="ignore"):
        for m in range(D.shape[0]):
            S00, S11, S01 = np.zeros(P), np.zeros(P), np.zeros(P)
            for i0 in range(0, n, row_block):
                p00, p11, p01 = np.zeros(P), np.zeros(P), np.zeros(P)
                for i in range(i0, min(i0 + row_block, n)):
                    same, diff = np.zeros(P), np.zeros(P)
                    for j in range(i + 1, n):
                        d = D[m, i, j]
                        eq = lab[:, j] == lab[:, i]
                        same = np.where(eq, same + d, same)
                        diff = np.where(eq, diff, diff + d)
                    p00 = np.where(lab[:, i], p00, p00 + same)
                    p11 = np.where(lab[:, i], p11 + same, p11)
                    p01 = p01 + diff
                S00, S11, S01 = S00 + p00, S11 + p11, S01 + p01
            out[m] = S00, S11, S01
    return out, lab.sum(axis=1).astype(np.int32)


def perm_sums_fsum(D, labels):
    """The same three index sets, each summed with math.fsum (exactly rounded).  Returns (sums (n_mat, 3, P), terms
    (3, P) = the number of entries of each sum, mass (n_mat, 3, P) = the fsum of their absolute values)."""
    D = np.asarray(D, dtype=np.float64)
    lab = np.asarray(labels).astype(np.int64)
    P, n = lab.shape
    iu, ju = np.triu_indices(n, 1)
    sums, mass = np.empty((D.shape[0], 3, P)), np.empty((D.shape[0], 3, P))
    terms = np.empty((3, P), np.int64)
    for p in range(P):
        li, lj = lab[p, iu], lab[p, ju]
        cls = [(li == 0) & (lj == 0), (li == 1) & (lj == 1), li != lj]
        for k in range(3):
            terms[k, p] = int(cls[k].sum())
            for m in range(D.shape[0]):
                v = D[m, iu[cls[k]], ju[cls[k]]]
                sums[m, k, p] = math.fsum(v.tolist())
                mass[m, k, p] = math.fsum(np.abs(v).tolist())
    return sums, terms, mass


SIGN = {"joint_loss": -1, "energy": 1, "mmd": 1}


def statistic(sums, n1, n, name):
    """utils.two_sample_statistic, restated: the same divisions and additions in the same order."""
    s = np.asarray(sums, dtype=np.float64)
    n1 = np.asarray(n1).astype(np.int64)
    n0 = n - n1
    out = np.full(s.shape[:-2] + s.shape[-1:], np.nan)
    for p in range(s.shape[-1]):
        if n0[p] < 2 or n1[p] < 2:
            continue
        a = s[..., 0, p] / float(n0[p] * (n0[p] - 1))
        b = s[..., 1, p] / float(n1[p] * (n1[p] - 1))
        c = s[..., 2, p] / float(n0[p] * n1[p])
        with np.errstate(invalid="ignore"):
            if name == "joint_loss":
                out[..., p] = a + b
            elif name == "mmd":
                out[..., p] = (2.0 * a + 2.0 * b) - 2.0 * c
            elif name == "energy":
                out[..., p] = 2.0 * c - (2.0 * a + 2.0 * b)
            else:
                raise ValueError(name)
    return out


def p_values(stat, finite, name):
    """p and p_family as the docstring of utils.two_sample_permutation_test defines them, matrix by matrix."""
    n_mat, cols = stat.shape
    e = SIGN[name] * stat
    p, z, use = np.full(n_mat, np.nan), np.full(stat.shape, np.nan), np.zeros(n_mat, bool)
    with np.errstate(invalid="ignore", divide="ignore"):
        for m in range(n_mat):
            if finite[m] and not np.isnan(e[m, 0]):
                p[m] = (1 + int(np.sum(e[m, 1:] >= e[m, 0]))) / cols
            if cols > 1:
                mu, sd = e[m, 1:].mean(), e[m, 1:].std()
                z[m] = (e[m] - mu) / sd
                use[m] = bool(finite[m] and np.isfinite(mu) and sd > 0 and not np.isnan(z[m, 0]))
    pf = np.full(n_mat, np.nan)
    if use.any():
        zmax = np.fmax.reduce(z[use], axis=0)
        for m in np.flatnonzero(use):
            pf[m] = (1 + int(np.sum(zmax[1:] >= z[m, 0]))) / cols
    return p, pf


def permutation_test(D, labels, name):
    """utils.two_sample_permutation_test(D, y, labels=labels, statistic=name) from the definitions above."""
    D = np.asarray(D, dtype=np.float64)
    D = D[None] if D.ndim == 2 else D
    labels = np.asarray(labels)
    sums, n1 = perm_sums(D, labels)
    stat = statistic(sums, n1, labels.shape[1], name)
    finite = np.isfinite(sums[:, :, 0]).all(axis=1)
    p, pf = p_values(stat, finite, name)
    return {"observed": stat[:, 0], "null": stat[:, 1:], "p": p, "p_family": pf}


def all_labellings(n, n1):
    """Every labelling of n items with n1 ones, (C(n, n1), n) uint8, in itertools.combinations order."""
    rows = []
    for ones in itertools.combinations(range(n), n1):
        r = np.zeros(n, np.uint8)
        r[list(ones)] = 1
        rows.append(r)
    return np.array(rows)


def two_clusters(n0, n1, seed=0, gap=10.0, dim=3):
    """Euclidean distance matrix of n0 + n1 points in two clusters `gap` apart, and their labels."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n0 + n1, dim))
    x[n0:, 0] += gap
    d = np.sqrt(((x[:, None, :] - x[None, :, :]) ** 2).sum(-1))
    return d, np.r_[np.zeros(n0, np.uint8), np.ones(n1, np.uint8)]
