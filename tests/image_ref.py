"""
The persistence image and its group mean in float64 numpy with scipy.special.erfc: the definition of include/tdaeeg.h,
written with the operations it names.  The kernel (csrc/image.hip) evaluates erfc with the device library, so it agrees
with this file to rounding, not bit for bit; beside every mean the functions here return the two figures the tolerance is
made of, per group:
  W_g = (sum of the weights w_i over the finite rows of the kept diagrams) / n_kept
  N_g = the number of those rows
"""
import numpy as np
from scipy.special import erfc

from landscape_ref import cut, random_diagram          # noqa: F401  (random_diagram: the generator the image tests share)

SQRT2 = 1.4142135623730951
EPS = 2.0 ** -53
# C of the tolerance (C * W_g + N_g * |ref|) * 2^-53: 4 x the largest q = |gpu - ref| / (2^-53 * W_g) measured over every
# case of tests/test_gpu_image.py on an MI355X, rounded up to a power of two, at least 4 and never above 128 (a 16-ulp erfc
# gives about 70; more is a kernel error).  Measured q = 3.10 (sides (32, 1), power 1, sigma 0.05; 41
# comparisons) -> 4 x 3.10 = 12.4 -> C = 16.
C = 16


def _finite(rows):
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, 2)
    return rows[np.isfinite(rows).all(axis=1)]


def weights(rows, power):
    """(b, p, w) of the rows of F: p = d - b, w = 1.0, p or p * p."""
    f = _finite(rows)
    b, p = f[:, 0], f[:, 1] - f[:, 0]
    w = np.ones_like(p) if power == 0 else p if power == 1 else p * p
    return b, p, w


def phi(e, c, s):
    """Phi(e, c) = 0.5 * erfc(-((e - c) / s)) for every (centre, edge): (len(c), len(e))."""
    return 0.5 * erfc(-((np.asarray(e, dtype=np.float64)[None, :] - c[:, None]) / s))


def diagram_image(rows, xe, ye, sigma, power):
    """(I, W, N): the image (n_y, n_x) of one diagram (rows already cut to min(cnt, cap)), the sum of its weights and the
    number of its finite rows."""
    xe, ye = np.asarray(xe, dtype=np.float64), np.asarray(ye, dtype=np.float64)
    assert power in (0, 1, 2)
    b, p, w = weights(rows, power)
    s = np.float64(sigma) * SQRT2
    cx, cy = phi(xe, b, s), phi(ye, p, s)
    fx, fy = cx[:, 1:] - cx[:, :-1], cy[:, 1:] - cy[:, :-1]
    img = np.zeros((len(ye) - 1, len(xe) - 1))
    for i in range(len(b)):                                         # in row order
        img = img + (w[i] * fy[i])[:, None] * fx[i][None, :]
    return img, float(w.sum()), len(b)


def _mean(triples, shape):
    """(mean, W_g, N_g) of the kept diagrams' (I, W, N); NaN, 0, 0 without one."""
    if not triples:
        return np.full(shape, np.nan), 0.0, 0
    s = triples[0][0].copy()
    for t in triples[1:]:
        s = s + t[0]
    n = float(len(triples))
    return s / n, sum(t[1] for t in triples) / n, sum(t[2] for t in triples)


def lists_mean(dgms, xe, ye, sigma, power, seg_off, status=None, skip_mask=0):
    """From a list of (k, 2) diagrams (DeviceDiagrams.to_lists()): (mean (n_seg, n_y, n_x), W (n_seg,), N (n_seg,))."""
    shape = (len(ye) - 1, len(xe) - 1)
    n_seg, n = len(seg_off) - 1, len(dgms)
    out, W, N = np.full((n_seg,) + shape, np.nan), np.zeros(n_seg), np.zeros(n_seg, np.int64)
    for g in range(n_seg):
        w0, w1 = max(int(seg_off[g]), 0), min(int(seg_off[g + 1]), n)           # clamped to [0, n_dgm]
        kept = [diagram_image(dgms[w], xe, ye, sigma, power) for w in range(w0, w1)
                if status is None or not (int(status[w]) & skip_mask)]
        out[g], W[g], N[g] = _mean(kept, shape)
    return out, W, N


def image_mean(rows, cnt, xe, ye, sigma, power, seg_off=None, status=None, skip_mask=0):
    """rows (n, cap, 2), cnt (n,) -> (mean (n_seg, n_y, n_x), W (n_seg,), N (n_seg,)): what tda_image_mean_dev computes,
    and the figures of its tolerance."""
    rows = np.asarray(rows, dtype=np.float64)
    n, cap = rows.shape[0], rows.shape[1]
    seg_off = np.arange(n + 1) if seg_off is None else np.asarray(seg_off)
    return lists_mean([cut(rows[w], cnt[w], cap) for w in range(n)], xe, ye, sigma, power, seg_off, status, skip_mask)


def tolerance(ref, W, N, C):
    """(C * W_g + N_g * |ref|) * 2^-53, elementwise: C covers erfc and the roundings of its argument, the N_g term the sum
    of N_g non-negative terms in any order plus the division."""
    return (C * W[:, None, None] + N[:, None, None] * np.abs(ref)) * EPS
