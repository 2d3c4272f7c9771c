"""
CPU statement of the analytic-signal connectivity contract (include/tdaeeg.h, "Analytic-signal connectivity"), two
evaluations of the same float64 inputs:
  conn_numpy   the definition in numpy, scipy.signal.hilbert for the analytic signal
  conn_exact   the same definition at 40+ digits in the manner of plv_ref.plv_exact: the float64 samples and the float64
               table g are taken as exact numbers (every float64 is an integer times a power of two), the circulant sums
               h = x (*) g, the products s and r and the sums S, A, R, P are exact integers; the envelopes are integer
               square roots at a fixed point of 2^-160 below the samples' unit, their means and centred products again
               exact integers (n_t a - sum a); the final roots and quotients are mpmath at 50 digits.  The threshold tests
               are decided on the integers: A <= TAU sqrt(P_i P_j) as A^2 2^80 <= P_i P_j, and an envelope is flat where
               C 2^80 <= n_t (sum a)^2, C = sum (n_t a - sum a)^2
and the bars that follow from their difference.  No GPU, no project kernels (preprocess._hilbert_g is the host table the
contract names).  The inputs are plv_ref.cases(), not modified.

Tolerance, as measured:
  E_REF[m] = max |conn_numpy - conn_exact| over every pair of every window of plv_ref.cases(), measured on the CPU with
             numpy 2.2.6, scipy 1.15.3, mpmath 1.3.0 (tests/test_connectivity_model.py::test_numpy_against_exact measures it
             again and holds the constants to it)
  BAR[m]   = 8 * E_REF[m]: the kernel's bar, |value_kernel - value_exact| <= BAR[m] (the margin of the PLV: kernel and
             definition sum n_t terms in different orders; a dropped or doubled term moves a value by 1 / n_t = 4e-3)
  dist bars: plv_ref.dist_bar(method, BAR[m])
The bars mean something only where no pair sits near a threshold of the definition: test_connectivity_model asserts that
every pair's A / sqrt(P_i P_j) is >= 1e-3 or <= 2^-46 and every envelope's coefficient of variation >= 1e-3 or flat.
"""
import functools

import numpy as np

import plv_ref

MEASURES = ("wpli", "imcoh", "coh", "aec")
TAU = 2.0 ** -40
# measured (above): the maxima are at rand_61x3 (wpli, imcoh), rand_64x250 (coh) and rand_3x3 (aec)
E_REF = {"wpli": 1.5543122344752192e-15, "imcoh": 3.3306690738754696e-16, "coh": 7.771561172376096e-16,
         "aec": 6.217248937900877e-15}
BAR = {m: 8 * e for m, e in E_REF.items()}
FIX = 160                 # the envelopes' fixed point: 2^-160 of the samples' integer unit


def _sym(v):
    v = np.triu(v, 1)
    v = v + v.T
    np.fill_diagonal(v, 1.0)
    return v


def conn_numpy(x, diag=False):
    """The definition on one window (n_ch, n_t): {measure: (n_ch, n_ch)}.  diag=True: also "ratio" (A / sqrt(P_i P_j), NaN
    where P_i P_j == 0), "cv" (std / mean of every envelope, NaN where the mean is 0) and "flat"."""
    from scipy.signal import hilbert
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[-1]
    h = np.imag(hilbert(x, axis=-1))
    s = h[:, None, :] * x[None, :, :] - x[:, None, :] * h[None, :, :]
    S, A = s.sum(-1), np.abs(s).sum(-1)
    R = x @ x.T + h @ h.T
    P = (x * x + h * h).sum(-1)
    pp = np.outer(P, P)
    den = np.sqrt(pp)
    safe = np.where(pp == 0, 1.0, den)
    out = {}
    deg = A <= TAU * den
    out["wpli"] = _sym(np.where(deg, 0.0, np.abs(S) / np.where(deg, 1.0, A)))
    out["imcoh"] = _sym(np.where(pp == 0, 0.0, np.abs(S) / safe))
    out["coh"] = _sym(np.where(pp == 0, 0.0, np.sqrt(S * S + R * R) / safe))
    a = np.sqrt(x * x + h * h)
    mean = a.mean(-1)
    d = a - mean[:, None]
    C = d @ d.T
    var = (d * d).sum(-1)
    flat = var <= n * (TAU * mean) ** 2
    either = flat[:, None] | flat[None, :]
    out["aec"] = _sym(np.where(either, 0.0, C / np.sqrt(np.where(either, 1.0, np.outer(var, var)))))
    if diag:
        with np.errstate(invalid="ignore", divide="ignore"):
            out["ratio"] = np.where(pp == 0, np.nan, A / safe)
            out["cv"] = np.where(mean == 0, np.nan, np.sqrt(var / n) / np.where(mean == 0, 1.0, mean))
        out["flat"] = flat
    return out


def conn_exact(x):
    """The definition on one window at 40+ digits (module docstring), rounded to float64 at the very end: the four measures
    and the diagnostics of conn_numpy(diag=True)."""
    import math
    import mpmath
    x = np.asarray(x, dtype=np.float64)
    n_ch, n = x.shape
    xi, _ = plv_ref._as_ints(x)
    gi, eg = plv_ref._as_ints(plv_ref.hilbert_g(n))
    Gi = gi[(np.arange(n)[:, None] - np.arange(n)[None, :]) % n]
    H = xi.dot(Gi.T)                                           # exact: h = H * 2^(ex + eg)
    X = xi
    if eg <= 0:                                                # x and h on one integer unit
        X = np.array([[int(v) << (-eg) for v in row] for row in xi], dtype=object).reshape(n_ch, n)
    else:
        H = np.array([[int(v) << eg for v in row] for row in H], dtype=object).reshape(n_ch, n)
    P = [sum(int(X[c, t]) ** 2 + int(H[c, t]) ** 2 for t in range(n)) for c in range(n_ch)]
    R = X.dot(X.T) + H.dot(H.T)
    # the envelopes at the fixed point, their exact centred products (times n^2)
    a = np.array([[math.isqrt((int(X[c, t]) ** 2 + int(H[c, t]) ** 2) << (2 * FIX)) for t in range(n)] for c in range(n_ch)],
                 dtype=object).reshape(n_ch, n)
    asum = [sum(int(v) for v in a[c]) for c in range(n_ch)]
    D = np.array([[n * int(a[c, t]) - asum[c] for t in range(n)] for c in range(n_ch)], dtype=object).reshape(n_ch, n)
    C = D.dot(D.T)
    flat = np.array([int(C[c, c]) << 80 <= n * asum[c] ** 2 for c in range(n_ch)])
    out = {m: np.ones((n_ch, n_ch)) for m in MEASURES}
    out["ratio"] = np.full((n_ch, n_ch), np.nan)
    out["cv"] = np.full(n_ch, np.nan)
    out["flat"] = flat
    with mpmath.workdps(50):
        for c in range(n_ch):
            if asum[c]:
                out["cv"][c] = float(mpmath.sqrt(mpmath.mpf(int(C[c, c])) / n) / asum[c])     # sqrt(C / n^3) / (asum / n)
        for i in range(n_ch):
            for j in range(i + 1, n_ch):
                s = [int(H[i, t]) * int(X[j, t]) - int(X[i, t]) * int(H[j, t]) for t in range(n)]
                S, A, pp = sum(s), sum(abs(v) for v in s), P[i] * P[j]
                den = mpmath.sqrt(mpmath.mpf(pp)) if pp else None
                w = 0.0 if (A * A) << 80 <= pp else float(mpmath.mpf(abs(S)) / A)
                ic = 0.0 if pp == 0 else float(abs(S) / den)
                co = 0.0 if pp == 0 else float(mpmath.sqrt(mpmath.mpf(S * S + int(R[i, j]) ** 2)) / den)
                ae = 0.0 if flat[i] or flat[j] else float(mpmath.mpf(int(C[i, j])) / mpmath.sqrt(mpmath.mpf(int(C[i, i]) * int(C[j, j]))))
                for m, v in zip(MEASURES, (w, ic, co, ae)):
                    out[m][i, j] = out[m][j, i] = v
                if pp:
                    out["ratio"][i, j] = out["ratio"][j, i] = float(A / den)
    return out


@functools.lru_cache(maxsize=None)
def exact(name):
    """conn_exact of every window of plv_ref.cases()[name] as {key: (n_win, ...)}; computed once, shared by the tests."""
    per = [conn_exact(w) for w in plv_ref.cases()[name]]
    out = {k: np.stack([p[k] for p in per]) for k in per[0]}
    for v in out.values():
        v.setflags(write=False)
    return out
