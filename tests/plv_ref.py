"""
CPU statement of the phase-locking value contract (include/tdaeeg.h, "Phase-locking value"), two evaluations of the same
float64 inputs:
  plv_numpy   the definition in numpy, scipy.signal.hilbert for the analytic signal
  plv_exact   the same definition at 40+ digits: the float64 samples and the float64 table g are taken as exact numbers,
              the circulant sums h = x (*) g and the Gram sums are exact integer dot products (every float64 is an
              integer times a power of two), the square roots and quotients of the phasors and of the final modulus are
              mpmath at 50 digits, the phasors rounded to 2^-160 (48 digits) before the Gram sums
and the bars that follow from their difference.  No GPU, no project kernels (preprocess._hilbert_g is the host table the
contract names).

Tolerance, as measured:
  PLV_E_REF = max |plv_numpy - plv_exact| over every window of `cases()`, measured on the CPU with numpy 2.2.6,
              scipy 1.15.3, mpmath 1.3.0 (tests/test_plv_model.py::test_numpy_against_exact measures it again and holds the
              constant to it)
  PLV_BAR   = 8 * PLV_E_REF: the kernel's bar, |plv_kernel - plv_exact| <= PLV_BAR (both are sums of n_t terms in
              different orders; a dropped or doubled term moves a value by 1 / n_t = 4e-3)
  dist bars: dist_bar(method, e) from the PLV bar e -- method 0 sqrt(2 e) (|sqrt(a) - sqrt(b)| <= sqrt(|a - b|), a = 2 (1 - p)),
             1 and 2: e (1-Lipschitz), 3: sqrt(2 e) (|p^2 - q^2| <= 2 |p - q| on [0, 1])
"""
import functools

import numpy as np

PLV_E_REF = 7.771561172376096e-16        # measured (above); 3.5 ulp of 1
PLV_BAR = 8 * PLV_E_REF
METHODS = ("euclidean", "abs", "standard", "sqrt")


def hilbert_g(n):
    from tda_eeg_audio_amd.preprocess import _hilbert_g
    return _hilbert_g(int(n))


def dist_bar(method, e=None):
    e = PLV_BAR if e is None else e
    return float(np.sqrt(2 * e)) if method in (0, 3) else float(e)


def unit_phasors(x, h):
    """Step 2 of the contract in float64: (ur, ui)."""
    m = np.sqrt(x * x + h * h)
    z = m == 0
    ms = np.where(z, 1.0, m)
    return np.where(z, 1.0, x / ms), np.where(z, 0.0, h / ms)


def plv_from_phasors(ur, ui):
    n_t = ur.shape[-1]
    R = ur @ ur.T + ui @ ui.T
    I = ui @ ur.T - ur @ ui.T
    p = np.sqrt(R * R + I * I) / n_t
    p = np.triu(p, 1)
    p = p + p.T
    np.fill_diagonal(p, 1.0)
    return p


def plv_numpy(x):
    """The definition on one window (n_ch, n_t): scipy.signal.hilbert for step 1."""
    from scipy.signal import hilbert
    x = np.asarray(x, dtype=np.float64)
    h = np.imag(hilbert(x, axis=-1))
    return plv_from_phasors(*unit_phasors(x, h))


def plv_circulant(x):
    """The definition with step 1 as the contract writes it: x @ G.T, G the circulant of the host table."""
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[-1]
    g = hilbert_g(n)
    G = g[(np.arange(n)[:, None] - np.arange(n)[None, :]) % n]
    return plv_from_phasors(*unit_phasors(x, x @ G.T))


def dist_of(plv, method):
    """correlation_to_distance (nb2:100-122): clip, formula, clamp at 0, zero diagonal."""
    r = np.clip(plv, -1.0, 1.0)
    if method == 0:
        d = np.sqrt(2.0 * (1.0 - r))
    elif method == 1:
        d = 1.0 - np.abs(r)
    elif method == 2:
        d = 1.0 - r
    elif method == 3:
        d = np.sqrt(1.0 - r * r)
    else:
        raise ValueError("Unknown method")
    d = np.maximum(d, 0.0)
    np.fill_diagonal(d, 0.0)
    return d


def _as_ints(a):
    """a (float64, finite) = ints * 2^e exactly: (object array of Python ints, e)."""
    a = np.asarray(a, dtype=np.float64)
    mant, ex = np.frexp(a)
    m53 = (mant * 9007199254740992.0).astype(np.int64)        # exact: |mant| < 1, 53 bits
    nz = m53 != 0
    e0 = int(ex[nz].min()) if nz.any() else 0
    out = np.empty(a.shape, dtype=object)
    flat_o, flat_m, flat_e = out.reshape(-1), m53.reshape(-1), ex.reshape(-1)
    for k in range(flat_o.shape[0]):
        flat_o[k] = int(flat_m[k]) << (int(flat_e[k]) - e0) if flat_m[k] else 0
    return out, e0 - 53


FIX = 160                 # the phasors' fixed point: 2^-160


def plv_exact(x):
    """The definition on one window at 40+ digits (module docstring), rounded to float64 at the very end."""
    import mpmath
    x = np.asarray(x, dtype=np.float64)
    n_ch, n = x.shape
    xi, ex = _as_ints(x)
    gi, eg = _as_ints(hilbert_g(n))
    Gi = gi[(np.arange(n)[:, None] - np.arange(n)[None, :]) % n]
    hi = xi.dot(Gi.T)                                          # exact: h = hi * 2^(ex + eg)
    ur = np.empty((n_ch, n), dtype=object)
    ui = np.empty((n_ch, n), dtype=object)
    one = 1 << FIX
    with mpmath.workdps(50):
        for c in range(n_ch):
            for t in range(n):
                a, b = xi[c, t], hi[c, t]
                if a == 0 and b == 0:
                    ur[c, t], ui[c, t] = one, 0
                    continue
                xv = mpmath.ldexp(mpmath.mpf(a), ex)
                hv = mpmath.ldexp(mpmath.mpf(b), ex + eg)
                m = mpmath.sqrt(xv * xv + hv * hv)
                ur[c, t] = int(mpmath.nint(mpmath.ldexp(xv / m, FIX)))
                ui[c, t] = int(mpmath.nint(mpmath.ldexp(hv / m, FIX)))
        R = ur.dot(ur.T) + ui.dot(ui.T)
        I = ui.dot(ur.T) - ur.dot(ui.T)
        p = np.ones((n_ch, n_ch))
        for i in range(n_ch):
            for j in range(i + 1, n_ch):
                v = mpmath.ldexp(mpmath.sqrt(mpmath.mpf(R[i, j] * R[i, j] + I[i, j] * I[i, j])), -2 * FIX) / n
                p[i, j] = p[j, i] = float(v)
    return p


def _rng_windows(n_win, n_ch, n_t, seed):
    """EEG-like windows: a few oscillations shared between the channels with channel-dependent phase and gain, plus noise."""
    rng = np.random.default_rng(seed)
    t = np.arange(n_t) / 250.0
    x = rng.standard_normal((n_win, n_ch, n_t))
    for f in (6.0, 10.0, 21.0):
        ph = rng.uniform(0, 2 * np.pi, (n_win, n_ch, 1))
        amp = rng.uniform(0.0, 3.0, (n_win, n_ch, 1))
        x += amp * np.sin(2 * np.pi * f * t + ph)
    return x


# (n_ch, n_t, n_win): the lane, tile, block and odd / even boundaries of the kernel, not the full product; (47, 250), (56, 250)
# and (64, 250) / (64, 256) are the three time-block sizes (64, 32 and 16 samples); at (58, 213) the 64-sample tile fits the
# 160 KiB of a CU by its dynamic bytes alone (163,824) and not with the kernel's static LDS in front of them
SHAPES = ((2, 2, 3), (3, 3, 3), (16, 63, 2), (17, 64, 2), (3, 65, 3), (48, 249, 1), (47, 250, 2), (64, 250, 1), (64, 256, 1),
          (2, 256, 3), (61, 3, 2), (56, 250, 1), (58, 213, 1))


@functools.lru_cache(maxsize=None)
def cases():
    """{name: windows (n_win, n_ch, n_t)}: the test inputs E_REF is measured on.  Computed once; do not modify."""
    out = {}
    for k, (n_ch, n_t, n_win) in enumerate(SHAPES):
        out[f"rand_{n_ch}x{n_t}"] = _rng_windows(n_win, n_ch, n_t, 100 + k)
    # a duplicated channel (PLV 1, distance near sqrt(2 e)), a zero channel, a constant channel, a positive multiple
    x = _rng_windows(1, 8, 250, 7)
    x[0, 3] = x[0, 1]
    x[0, 4] = 0.0
    x[0, 5] = 2.5
    x[0, 6] = 3.0 * x[0, 2]
    out["special_8x250"] = x
    for v in out.values():
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def exact(name):
    """plv_exact of every window of cases()[name], (n_win, n_ch, n_ch); computed once, shared by the tests."""
    v = np.stack([plv_exact(w) for w in cases()[name]])
    v.setflags(write=False)
    return v
