"""
The kernels on diagrams of include/tdaeeg.h ("Kernels on diagrams") in numpy: np.exp, np.arctan, sequential sums -- for
pairs and for group Gram matrices.  Beside each value the functions return
  A    = |scale| * sum |w_i w_j| (E1 + mirror * E2), divided by n_g n_h for a Gram entry: the size of what was added up
  N_t  the number of terms
which the tolerance is made of.

Tolerance of a GPU value against this reference (the issue's formula):
  |gpu - ref| <= (C * A + 2 N_t |ref|) * 2^-53 + N_t * |scale| * wmax^2 * 2^-1022
The first term is the rounding of exp / atan (C units in the last place of every term, summed in absolute value), the
second two summation orders of N_t terms, the last a subnormal E that the device flushes to zero.

C, by the procedure of DESIGN.md 3.10 / 3.15: q = max |gpu - ref| / (2^-53 * A) over every comparison of
tests/test_gpu_diagram_kernel.py on an MI355X, C = 4 q rounded up to a power of two, at least 4, never above 64.

Measured on an MI355X (DESIGN.md 3.15 has the table):
  * against this reference as it is, q = 474.6 ("gram pwg", the 513 x 513-row tile, N_t = 263,169).  That figure is the
    order of the additions, not exp or atan: rows_sum adds the 263,169 terms one after the other, and the same GPU
    value is q = 0.31 (pss) .. 3.4 (pers) away from the SAME terms added exactly (math.fsum).  The comparisons with
    N_t = 1, where nothing is added, give q <= 3.70.  The order of the additions is what the 2 N_t |ref| term of the
    tolerance is for, so it does not belong in C.
  * against the reference's terms added exactly, q = 7.264 ("gram cross route pers", the 1 x 513-row tile: one GPU thread
    adds its 513 terms in turn).  C = 4 * 7.264 = 29.1 -> 32.
"""
import numpy as np

KW_ONE, KW_PERS, KW_ATAN = 0, 1, 2
U = 2.0 ** -53
# q, the case that gave it, and the C that follows
Q_SEQUENTIAL = 474.621      # against rows_sum as it is: "gram pwg", tile (4, 4), N_t = 263,169 -- summation order
Q_MEASURED = 7.264          # against the same terms added exactly: "gram cross route pers", tile (6, 4), N_t = 513
Q_CASE = "gram cross route, TDA_KW_PERS, a group of 1 finite row against one of 513"
C = 32


def named(kernel):
    """(ninv, mirror, scale, weight, wc) of ("pss", sigma) / ("pwg", sigma, c), written out here on its own."""
    if kernel[0] == "pss":
        sigma = float(kernel[1])
        return (-1.0 / (8.0 * sigma), 1, 1.0 / (8.0 * np.pi * sigma), KW_ONE, 0.0)
    sigma, c = float(kernel[1]), float(kernel[2])
    return (-1.0 / (2.0 * sigma * sigma), 0, 1.0, KW_ATAN, c)


def finite_rows(d):
    d = np.asarray(d, dtype=np.float64).reshape(-1, 2)
    return d[np.isfinite(d).all(axis=1)]


def weights(F, weight, wc):
    p = F[:, 1] - F[:, 0]
    if weight == KW_ONE:
        return np.ones(len(F))
    if weight == KW_PERS:
        return p
    return np.arctan(wc * p)


def arguments(FA, FB, ninv, mirror):
    """The float64 arguments a1 (and a2) of every (i, j), operation for operation."""
    dx = FA[:, None, 0] - FB[None, :, 0]
    dy = FA[:, None, 1] - FB[None, :, 1]
    a1 = (dx * dx + dy * dy) * ninv
    if not mirror:
        return a1, None
    ex = FA[:, None, 0] - FB[None, :, 1]
    ey = FA[:, None, 1] - FB[None, :, 0]
    return a1, (ex * ex + ey * ey) * ninv


def rows_sum(FA, FB, par):
    """(S, sum |w w| (E1 + mirror E2), N_t) of two tables of finite rows; the sum runs term after term, row-major."""
    ninv, mirror, scale, weight, wc = par
    if len(FA) == 0 or len(FB) == 0:
        return 0.0, 0.0, 0
    wa, wb = weights(FA, weight, wc), weights(FB, weight, wc)
    a1, a2 = arguments(FA, FB, ninv, mirror)
    E1 = np.exp(a1)
    ww = wa[:, None] * wb[None, :]
    if mirror:
        E2 = np.exp(a2)
        t = ww * (E1 - E2)
        mag = np.abs(ww) * (E1 + E2)
    else:
        t = ww * E1
        mag = np.abs(ww) * E1
    return float(np.cumsum(t.ravel())[-1]), float(mag.sum()), t.size


def kernel_value(A, B, par):
    """(K, A_abs, N_t) of two diagrams."""
    s, mag, nt = rows_sum(finite_rows(A), finite_rows(B), par)
    return par[2] * s, abs(par[2]) * mag, nt


def pair(A, B, par):
    """([k_ab, k_aa, k_bb], their A, their N_t) of a pair of diagrams."""
    r = [kernel_value(A, B, par), kernel_value(A, A, par), kernel_value(B, B, par)]
    return np.array([x[0] for x in r]), np.array([x[1] for x in r]), np.array([x[2] for x in r])


def distance(kvals):
    """The pair distance from (.., 3) values [k_ab, k_aa, k_bb], operation for operation."""
    kvals = np.asarray(kvals, dtype=np.float64)
    k_ab, k_aa, k_bb = kvals[..., 0], kvals[..., 1], kvals[..., 2]
    return np.sqrt(np.maximum((k_aa + k_bb) - (k_ab + k_ab), 0))


def gram(groups_a, groups_b, par):
    """groups: a list of lists of KEPT diagrams.  (G, A, N_t), each (len(groups_a), len(groups_b)); NaN for a group
    without a diagram."""
    rows_a = [np.concatenate([finite_rows(d) for d in g] + [np.zeros((0, 2))]) for g in groups_a]
    rows_b = [np.concatenate([finite_rows(d) for d in g] + [np.zeros((0, 2))]) for g in groups_b]
    G = np.full((len(groups_a), len(groups_b)), np.nan)
    A = np.zeros(G.shape)
    N = np.zeros(G.shape, np.int64)
    for g, ga in enumerate(groups_a):
        for h, gb in enumerate(groups_b):
            if len(ga) and len(gb):
                s, mag, nt = rows_sum(rows_a[g], rows_b[h], par)
                n = float(len(ga) * len(gb))
                G[g, h], A[g, h], N[g, h] = (par[2] * s) / n, abs(par[2]) * mag / n, nt
    return G, A, N


def wmax(diagrams, par):
    """The largest |w| over the finite rows of the diagrams."""
    m = 0.0
    for d in diagrams:
        F = finite_rows(d)
        if len(F):
            m = max(m, float(np.abs(weights(F, par[3], par[4])).max()))
    return m


def tolerance(A, n_t, ref, scale, w_max, c=None):
    c = C if c is None else c
    return (c * np.asarray(A) + 2.0 * np.asarray(n_t) * np.abs(ref)) * U + np.asarray(n_t) * abs(scale) * w_max * w_max * 2.0 ** -1022
