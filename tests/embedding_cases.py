"""
Inputs of the delay and dimension selection tests, shared by the CPU model tests and the GPU parity tests: the four named
signals with the answers the literature's rules give on them, and the smallest shapes at which the kernels can still go
wrong.  Test infrastructure only.

What the shapes are for.  ami_kernel: four waves take four lags per round, so 9 lags are three rounds with a part-filled
last one and 2 lags (n_t = 4) are not even one; 67 samples are one full trip of a wave and a tail of 3; 250 samples at lag
L leave 250 - L pairs, a different tail for every wave; max_lag at its cut n_t - 2 leaves N = 2 pairs; 2, 16 and 32 bins are
4, 256 and 1024 cells: a part of one trip, four trips, sixteen; the largest sample of every window equals hi and lands in
the last bin through the clamp.  fnn_kernel: 64 lanes to a wave and 256 points to a trip, so M_d straddling 64 (n_t = 70,
tau = 3: 67, 64, 61, ...) moves the last wave's edge through the dimensions and n_t = 300 needs a second trip; n_t = 10 with
tau = 3 runs out of points at d = 3 (M_3 = 1) and has none at d = 4; theiler = n_t leaves no candidate at all.
"""
import numpy as np

import embedding_ref as er


# ---------------------------------------------------------------- the four named signals
def sine():
    """sin(2 pi t / 40) + 0.05 noise, 250 samples, seed 7."""
    return np.sin(2 * np.pi * np.arange(250) / 40) + 0.05 * np.random.default_rng(7).standard_normal(250)


def lorenz(n=500, dt=0.02, skip=2000, every=2):
    """x of the Lorenz system (sigma 10, rho 28, beta 8/3) from (1, 1, 1) by RK4 steps of dt, every `every`-th step after
    `skip` steps of transient."""
    def f(v):
        return np.array([10.0 * (v[1] - v[0]), v[0] * (28.0 - v[2]) - v[1], v[0] * v[1] - 8.0 / 3.0 * v[2]])
    v, out = np.array([1.0, 1.0, 1.0]), []
    for k in range(skip + n * every):
        if k >= skip and (k - skip) % every == 0:
            out.append(v[0])
        k1 = f(v); k2 = f(v + 0.5 * dt * k1); k3 = f(v + 0.5 * dt * k2); k4 = f(v + dt * k3)
        v = v + dt / 6.0 * (k1 + 2 * k2 + 2 * k3 + k4)
    return np.array(out)


def henon(n=250):
    """x of the Henon map (a 1.4, b 0.3) from (0, 0)."""
    x, y, out = 0.0, 0.0, []
    for _ in range(n):
        out.append(x)
        x, y = 1.0 - 1.4 * x * x + y, 0.3 * x
    return np.array(out)


def white_noise():
    return np.random.default_rng(1).standard_normal(250)


# name -> (signal, first AMI minimum at max_lag None and 16 bins, dim at d_max 5, frac_tol 0.05, theiler 1 -- None: not stated)
def named():
    return {"sine": (sine(), 7, 2), "lorenz": (lorenz(), 6, 3), "henon": (henon(), 7, None), "white_noise": (white_noise(), 2, None)}


SINE_EITHER = (214, 5, 0)           # false_either of the sine at tau 7, theiler 1, d = 1, 2, 3 ...
SINE_VALID = (243, 236, 229)        # ... over this many points


# ---------------------------------------------------------------- AMI shapes
def _walk(n_win, n_t, seed):
    """Smooth random signals (a random walk through a short moving average): an AMI curve with structure."""
    rng = np.random.default_rng(seed)
    w = np.cumsum(rng.standard_normal((n_win, n_t + 4)), axis=1)
    return (w[:, 4:] + w[:, 3:-1] + w[:, 2:-2]) / 3.0 + 0.1 * rng.standard_normal((n_win, n_t))


def alternating(n_t):
    return np.where(np.arange(n_t) % 2 == 0, -1.5, 2.0)


def repeated_integers():
    return np.array([0.0, 1.0, 2.0, 3.0] * 8)


# (name, windows, max_lag, n_bins)
def ami_cases():
    nm = named()
    four = np.stack([nm[k][0] for k in ("sine", "henon", "white_noise")])
    mixed = _walk(5, 67, 11)
    mixed[1, 30] = np.nan
    mixed[3] = 0.75
    mixed[4, 5] = np.inf
    return [
        ("n_t4", np.array([[0.0, 1.0, 2.0, 3.0], [1.0, 0.0, 1.0, 0.0], [3.0, -1.0, 0.5, 0.5]]), None, 2),
        ("n_t4_lag2", np.array([[0.0, 1.0, 2.0, 3.0], [2.0, 0.0, 1.0, 0.0]]), 7, 3),
        ("nine_lags", _walk(3, 67, 1), 8, 16),
        ("lag_at_cut", _walk(2, 67, 2), 1000, 32),
        ("lag_zero", _walk(2, 67, 3), 0, 16),
        ("named_16", four, None, 16),
        ("named_2", four, 9, 2),
        ("named_32", four[:2], 13, 32),
        ("lorenz", nm["lorenz"][0][None], None, 16),
        ("alternating", np.stack([alternating(66), alternating(66)[::-1] * 3.0]), 6, 2),
        ("refused_among_good", mixed, 8, 16),
        ("integers", repeated_integers()[None], None, 4),
    ]


# ---------------------------------------------------------------- FNN shapes
# (name, windows, taus, d_max, theiler)
def fnn_cases():
    nm = named()
    w70 = _walk(3, 70, 21)
    w10 = _walk(2, 10, 22)
    bad = _walk(4, 70, 23)
    bad[2, 69] = np.nan
    return [
        ("straddle_64", w70, 3, 5, 1),
        ("straddle_64_theiler3", w70, 3, 5, 3),
        ("runs_out_of_points", w10, 3, 5, 1),
        ("no_candidate", w70[:2], 3, 3, 70),
        ("integers", repeated_integers()[None], 1, 3, 1),
        ("integers_tau4", repeated_integers()[None], 4, 4, 2),
        ("tau_per_window", bad, np.array([3, 0, 3, 69], np.int32), 4, 2),
        ("tau_degenerate", w10, np.array([8, 9], np.int32), 2, 1),
        ("d_max_1", w70, 5, 1, 1),
        ("d_max_8", w70, 2, 8, 2),
        ("second_trip", _walk(1, 300, 24), 2, 3, 2),
        ("constant", np.full((1, 40), 2.5), 2, 3, 1),
        ("sine", nm["sine"][0][None], 7, 5, 1),
        ("sine_theiler_tau", nm["sine"][0][None], 7, 5, 7),
    ]


_CACHE = {}


def reference(kind, name):
    """The numpy statement of a case, computed once: a dict of the blocks of the batch."""
    if (kind, name) not in _CACHE:
        if kind == "ami":
            _, wins, max_lag, n_bins = next(c for c in ami_cases() if c[0] == name)
            _CACHE[kind, name] = er.ami_batch(wins, max_lag, n_bins)
        else:
            _, wins, taus, d_max, theiler = next(c for c in fnn_cases() if c[0] == name)
            _CACHE[kind, name] = er.fnn_batch(wins, taus, d_max, theiler)
    return _CACHE[kind, name]
