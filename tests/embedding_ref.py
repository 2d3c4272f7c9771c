"""
CPU statement of the delay and dimension selection (include/tdaeeg.h, "Delay and dimension selection"): the average mutual
information of a window with its own past on a histogram, its first minimum, and the false nearest neighbours of the delay
embeddings of growing dimension.  Everything is stated twice, independently: plain loops over Python floats and ints
(ami_loops, fnn_loops), and vectorised numpy (ami_np, fnn_np).  ami_mp evaluates the mutual information from the integer
counts with 50 digits.  Test infrastructure only.

What is bytes and what is not.  The bins, the joint counts, every output of the false nearest neighbours (nn, counts, frac,
dim) are bytes of the header's text: each float64 operation is written there and the two statements agree bit for bit.
The mutual information holds the rounding of log and of a sum whose order the header leaves to the kernel, so it is compared
to a bar.  AMI_REF_ERR is the largest |numpy statement - 50-digit value| over the inputs of the tests
(embedding_cases.AMI_CASES and the four named signals); tests/test_embedding_model.py measures it again and fails when it
is larger than written here.  The kernel is allowed AMI_BAR = 8 * AMI_REF_ERR against the numpy statement: the margin
DESIGN.md 3.19, 3.23 and 3.25 give a device transcendental.  tau is a function of the stored row (first_minimum), so it is
compared as bytes against the rule applied to the row the kernel returned.
"""
import math

import numpy as np

TDA_WIN_DEGENERATE, TDA_WIN_TOO_LARGE, TDA_WIN_NOT_FINITE = 4, 16, 64
FNN_MAX_DIM = 8
FNN_COUNT_NAMES = ("valid", "false_distance", "false_size", "false_either")

AMI_REF_ERR = 7.636903870884479e-16          # measured (3.44 * 2^-52, on the white noise at 16 bins: some 200 terms of either sign)
AMI_BAR = 8 * AMI_REF_ERR                    # 6.11e-15


# ---------------------------------------------------------------- shared rules
def resolve_max_lag(n_t, max_lag=None):
    """A negative max_lag (None) means n_t / 4; then it is cut to n_t - 2."""
    if max_lag is None or max_lag < 0:
        max_lag = n_t // 4
    return min(int(max_lag), n_t - 2)


def first_minimum(row):
    """The smallest L in [1, len - 2] with row[L] < row[L - 1] and row[L] <= row[L + 1]; 0 without one (also for NaN)."""
    for L in range(1, len(row) - 1):
        if row[L] < row[L - 1] and row[L] <= row[L + 1]:
            return L
    return 0


def fallback_tau(tau, n_t, max_lag=None):
    """What the segments form and compute_tau_ami write when there is no minimum: compute_tau's max(max_lag / 10, 1)."""
    return tau if tau else max(resolve_max_lag(n_t, max_lag) // 10, 1)


def _refused(x):
    return not np.isfinite(np.asarray(x, np.float64)).all()


# ---------------------------------------------------------------- AMI, first statement: plain loops
def bins_loops(x, n_bins):
    x = [float(v) for v in x]
    lo, hi = min(x), max(x)
    w = hi - lo
    return [min(n_bins - 1, int(((v - lo) / w) * float(n_bins))) for v in x]


def ami_loops(x, max_lag=None, n_bins=16):
    """dict(ami (max_lag + 1,) float64, tau int, joint (max_lag + 1, n_bins, n_bins) int32, status int)."""
    x = np.asarray(x, np.float64)
    n_t = x.shape[0]
    ml = resolve_max_lag(n_t, max_lag)
    ami = np.zeros(ml + 1)
    joint = np.zeros((ml + 1, n_bins, n_bins), np.int32)
    if _refused(x):
        return dict(ami=ami + np.nan, tau=0, joint=joint, status=TDA_WIN_NOT_FINITE)
    if x.max() == x.min():
        return dict(ami=ami, tau=0, joint=joint, status=TDA_WIN_DEGENERATE)
    b = bins_loops(x, n_bins)
    for L in range(ml + 1):
        N = n_t - L
        J = [[0] * n_bins for _ in range(n_bins)]
        for i in range(N):
            J[b[i]][b[i + L]] += 1
        r = [sum(J[p]) for p in range(n_bins)]
        s = [sum(J[p][q] for p in range(n_bins)) for q in range(n_bins)]
        S = 0.0
        for p in range(n_bins):
            for q in range(n_bins):
                if J[p][q] > 0:
                    S = S + (float(J[p][q]) / float(N)) * math.log(float(J[p][q] * N) / float(r[p] * s[q]))
        ami[L] = S
        joint[L] = J
    return dict(ami=ami, tau=first_minimum(ami), joint=joint, status=0)


# ---------------------------------------------------------------- AMI, second statement: numpy
def bins_np(x, n_bins):
    x = np.asarray(x, np.float64)
    lo, hi = x.min(), x.max()
    return np.minimum(n_bins - 1, (((x - lo) / (hi - lo)) * np.float64(n_bins)).astype(np.int64))


def joint_np(b, L, n_bins):
    N = b.shape[0] - L
    return np.bincount(b[:N] * n_bins + b[L:], minlength=n_bins * n_bins).reshape(n_bins, n_bins)


def ami_of_joint(J):
    """I of one table of joint counts, the written terms with numpy's log and numpy's sum."""
    J = np.asarray(J, np.int64)
    N = int(J.sum())
    rs = J.sum(1)[:, None] * J.sum(0)[None, :]
    m = J > 0
    return float(((J[m].astype(np.float64) / np.float64(N)) * np.log((J[m] * N).astype(np.float64) / rs[m].astype(np.float64))).sum())


def ami_np(x, max_lag=None, n_bins=16):
    x = np.asarray(x, np.float64)
    n_t = x.shape[0]
    ml = resolve_max_lag(n_t, max_lag)
    ami = np.zeros(ml + 1)
    joint = np.zeros((ml + 1, n_bins, n_bins), np.int32)
    if _refused(x):
        return dict(ami=ami + np.nan, tau=0, joint=joint, status=TDA_WIN_NOT_FINITE)
    if x.max() == x.min():
        return dict(ami=ami, tau=0, joint=joint, status=TDA_WIN_DEGENERATE)
    b = bins_np(x, n_bins)
    for L in range(ml + 1):
        joint[L] = joint_np(b, L, n_bins)
        ami[L] = ami_of_joint(joint[L])
    return dict(ami=ami, tau=first_minimum(ami), joint=joint, status=0)


def ami_mp(J):
    """I of one table of joint counts with 50 digits (mpmath), as an mpf."""
    import mpmath
    J = np.asarray(J, np.int64)
    N = int(J.sum())
    r, s = J.sum(1), J.sum(0)
    with mpmath.workdps(50):
        S = mpmath.mpf(0)
        for p, q in zip(*np.nonzero(J)):
            j = int(J[p, q])
            S += mpmath.mpf(j) / N * mpmath.log(mpmath.mpf(j * N) / (int(r[p]) * int(s[q])))
        return S


def ami_errors(joint, ami):
    """|numpy statement - 50 digits| of every lag of a window."""
    import mpmath
    with mpmath.workdps(50):
        return [float(abs(ami_mp(J) - mpmath.mpf(float(a)))) for J, a in zip(joint, ami)]


def ami_batch(wins, max_lag=None, n_bins=16, route=ami_np):
    """The blocks of a batch as the kernel writes them: ami, tau, joint, status."""
    res = [route(w, max_lag, n_bins) for w in wins]
    return dict(ami=np.array([r["ami"] for r in res]), tau=np.array([r["tau"] for r in res], np.int32),
                joint=np.array([r["joint"] for r in res], np.int32), status=np.array([r["status"] for r in res], np.int32))


# ---------------------------------------------------------------- FNN
def _fnn_empty(n_t, d_max):
    return dict(counts=np.zeros((d_max, 4), np.int32), frac=np.zeros(d_max), dim=0, nn=np.full((d_max, n_t), -1, np.int32),
                status=0)


def _fnn_status(x, tau):
    if _refused(x):
        return TDA_WIN_NOT_FINITE
    if tau < 1:
        return TDA_WIN_TOO_LARGE
    return TDA_WIN_DEGENERATE if len(x) - tau < 2 else 0


def _fnn_finish(out, frac_tol):
    for d in range(out["counts"].shape[0]):
        valid, either = int(out["counts"][d, 0]), int(out["counts"][d, 3])
        out["frac"][d] = float(either) / float(valid) if valid else 0.0
    for d in range(out["counts"].shape[0]):
        valid, either = int(out["counts"][d, 0]), int(out["counts"][d, 3])
        if valid > 0 and float(either) <= frac_tol * float(valid):
            out["dim"] = d + 1
            break
    return out


def size_bound(x, a_tol):
    """R2 = (a_tol * a_tol) * var, mean and variance by sequential sums divided by n_t."""
    n_t = len(x)
    S = 0.0
    for v in x:
        S = S + float(v)
    m = S / float(n_t)
    S = 0.0
    for v in x:
        S = S + (float(v) - m) * (float(v) - m)
    return (a_tol * a_tol) * (S / float(n_t))


def fnn_loops(x, tau, d_max=5, theiler=None, r_tol=10.0, a_tol=2.0, frac_tol=0.05):
    """dict(counts (d_max, 4) int32, frac (d_max,) float64, dim int, nn (d_max, n_t) int32, status int).  The distances of
    all dimensions in one pass over k: D2_d is s after its first d terms, the written order."""
    x = [float(v) for v in np.asarray(x, np.float64)]
    n_t, tau = len(x), int(tau)
    theiler = tau if theiler is None else int(theiler)
    out = _fnn_empty(n_t, d_max)
    out["status"] = _fnn_status(x, tau)
    if out["status"]:
        return out
    R2, rr = size_bound(x, float(a_tol)), float(r_tol) * float(r_tol)
    M = [n_t - d * tau for d in range(d_max + 1)]                  # M[d], d = 1..d_max
    for i in range(max(M[1], 0)):
        best, bj = [0.0] * (d_max + 1), [-1] * (d_max + 1)
        for j in range(M[1]):
            if abs(i - j) < theiler:
                continue
            s = 0.0
            for d in range(1, d_max + 1):
                if i >= M[d] or j >= M[d]:
                    break
                e = x[i + (d - 1) * tau] - x[j + (d - 1) * tau]
                s = s + e * e
                if bj[d] < 0 or s < best[d]:
                    best[d], bj[d] = s, j
        for d in range(1, d_max + 1):
            if i >= M[d] or bj[d] < 0:
                continue
            out["nn"][d - 1, i] = bj[d]
            e = x[i + d * tau] - x[bj[d] + d * tau]
            e2, D2 = e * e, best[d]
            c1 = e2 > rr * D2 if D2 > 0 else e2 > 0.0
            c2 = (D2 + e2) > R2
            out["counts"][d - 1] += (1, c1, c2, c1 or c2)
    return _fnn_finish(out, float(frac_tol))


def fnn_np(x, tau, d_max=5, theiler=None, r_tol=10.0, a_tol=2.0, frac_tol=0.05):
    """The same blocks, a dimension at a time on (M_d, M_d) matrices."""
    x = np.asarray(x, np.float64)
    n_t, tau = x.shape[0], int(tau)
    theiler = tau if theiler is None else int(theiler)
    out = _fnn_empty(n_t, d_max)
    out["status"] = _fnn_status(x, tau)
    if out["status"]:
        return out
    m = np.cumsum(x)[-1] / np.float64(n_t)                         # cumsum adds in order
    R2 = (np.float64(a_tol) * np.float64(a_tol)) * (np.cumsum((x - m) * (x - m))[-1] / np.float64(n_t))
    rr = np.float64(r_tol) * np.float64(r_tol)
    for d in range(1, d_max + 1):
        M = n_t - d * tau
        if M < 2:
            break
        idx = np.arange(M)
        D2 = np.zeros((M, M))
        for k in range(d):
            E = x[idx + k * tau][:, None] - x[idx + k * tau][None, :]
            D2 = D2 + E * E
        ok = np.abs(idx[:, None] - idx[None, :]) >= theiler
        has = ok.any(1)
        j = np.where(ok, D2, np.inf).argmin(1)                     # the first of the smallest: ties to the smallest j
        lost = has & ~ok[idx, j]                                   # every candidate at +inf: the first candidate
        j[lost] = ok[lost].argmax(1)
        i = idx[has]
        j = j[has]
        out["nn"][d - 1, i] = j
        E = x[i + d * tau] - x[j + d * tau]
        e2, Dn = E * E, D2[i, j]
        c1 = np.where(Dn > 0, e2 > rr * Dn, e2 > 0.0)
        c2 = (Dn + e2) > R2
        out["counts"][d - 1] = (has.sum(), c1.sum(), c2.sum(), (c1 | c2).sum())
    return _fnn_finish(out, float(frac_tol))


def fnn_batch(wins, taus, d_max=5, theiler=1, r_tol=10.0, a_tol=2.0, frac_tol=0.05, route=fnn_np):
    """The blocks of a batch as the kernel writes them: counts, frac, dim, nn, status."""
    res = [route(w, t, d_max, theiler, r_tol, a_tol, frac_tol) for w, t in zip(wins, np.broadcast_to(taus, (len(wins),)))]
    return dict(counts=np.array([r["counts"] for r in res], np.int32), frac=np.array([r["frac"] for r in res]),
                dim=np.array([r["dim"] for r in res], np.int32), nn=np.array([r["nn"] for r in res], np.int32),
                status=np.array([r["status"] for r in res], np.int32))
