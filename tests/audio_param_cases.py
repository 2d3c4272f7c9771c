"""Seeded inputs for the audio branch off the reference's single configuration (n_t = 250, dim = 3, subsample = 2,
max_lag = 125): delays for lengths 2..2048 and every kind of max_lag, Takens windows for dim 1..4 and subsample 1..3,
explicit clouds for dim 1, 2, 4, cloud buffers with per-window point counts whose unused rows are NaN, and correlation
matrices for the four corr -> dist methods.  The same builders feed tests/test_audio_params_model.py (the oracle's
generic branches against plain restatements, no GPU) and tests/test_gpu_audio_params.py (the kernels against the
oracle).  TEST INFRASTRUCTURE."""
import functools

import numpy as np

from oracle import port
from tda_eeg_audio_amd import synth

SEED = 2024

# ---------------------------------------------------------------------------------------------------- tau
TAU_LENGTHS = (2, 3, 4, 5, 9, 63, 64, 65, 66, 127, 128, 129, 130, 250, 257, 513, 1000, 2048)
TAU_SIGNALS = ("white", "walk", "cosine", "constant", "ramp", "slow_cosine")
LAG_CHUNKS = ((1, 64), (65, 128), (129, 192), (193, 256), (257, 1 << 30))       # tau_kernel walks 64 lags per trip


def tau_max_lags(n_t):
    return (None, 1, 2, n_t // 2, n_t - 1, n_t, n_t + 7, 125)


def lag_chunk(tau):
    return next(i for i, (lo, hi) in enumerate(LAG_CHUNKS) if lo <= tau <= hi)


@functools.lru_cache(maxsize=None)
def tau_cases():
    """[(n_t, max_lag, (6, n_t) float64)]: one entry per (length, max_lag) pair, its rows in the order of TAU_SIGNALS.
    18 lengths x 8 max_lag x 6 signals = 864 windows."""
    rng = np.random.default_rng(SEED)
    out = []
    for n_t in TAU_LENGTHS:
        t = np.arange(n_t, dtype=np.float64)
        for max_lag in tau_max_lags(n_t):
            u = rng.uniform(0.3, 3.0)
            sig = np.stack([
                rng.standard_normal(n_t),
                np.cumsum(rng.standard_normal(n_t)),
                np.cos(2.0 * np.pi * t / (n_t * u)) + 0.01 * rng.standard_normal(n_t),
                np.full(n_t, 1.5),
                t.copy(),
                np.cos(2.0 * np.pi * t / max(4.0, 0.9 * n_t)) + 1e-3 * rng.standard_normal(n_t),
            ])
            sig.setflags(write=False)
            out.append((n_t, max_lag, sig))
    return out


def tau_longdouble(s, max_lag=None):
    """The delay rule of the reference (scripts/utils.py:92-104) in extended precision with direct lag sums: the first
    lag in [1, min(max_lag, len)) whose autocorrelation of the centred signal is <= 0, else max(max_lag // 10, 1), with
    max_lag = len // 4 when not given and never above len - 1.  Returns (tau, margin): margin = min |ac[i]| / ac[0] over
    the lags that were examined (inf when there was none, 0 for a signal without variance), i.e. how far the decision
    is from a sign that rounding could turn."""
    x = np.asarray(s, dtype=np.longdouble)
    n = len(x)
    if max_lag is None:
        max_lag = n // 4
    max_lag = min(int(max_lag), n - 1)
    c = x - x.sum() / np.longdouble(n)
    ac0 = (c * c).sum()
    margin = np.longdouble(np.inf)
    for i in range(1, min(max_lag, n)):
        ac = (c[i:] * c[:n - i]).sum()
        margin = min(margin, abs(ac) / ac0) if ac0 > 0 else np.longdouble(0.0)
        if ac / (ac0 + np.longdouble(1e-10)) <= 0:
            return max(i, 1), float(margin)
    return max(max_lag // 10, 1), float(margin)


# ---------------------------------------------------------------------------------------------------- Takens
TAKENS_WINDOWS = ("walk", "band", "white", "constant", "ramp", "repeated")
# (dim, subsample, n_t, tau) -> P
TAKENS_GRID = (
    (1, 2, 250, 3),      # points on a line, P = 125
    (1, 1, 128, 1),      # P = 128
    (2, 2, 250, 5),
    (2, 1, 100, 9),
    (4, 2, 250, 1),      # P = 124: dim = 4 leaves the narrow first-pass layout
    (4, 2, 250, 7),
    (4, 1, 64, 2),
    (3, 1, 130, 1),      # P = 128
    (3, 1, 250, 61),     # P = 128 while p_max (at tau = 1) is clamped from 248
    (3, 3, 250, 4),      # P = 81
    (3, 2, 256, 1),      # P = 127: beyond the narrow layout's 124 points
    (3, 2, 20, 2),       # P = 8
    (4, 1, 15, 2),       # P = 9
    (2, 1, 12, 1),       # P = 11
)
BRUTE_P = 12             # brute.rips_brute is run up to this many points
MIXED_TAU = dict(dim=3, subsample=1, n_t=250, tau=(60, 61, 62, 124, 125, 0))
MIXED_P = (130, 128, 126, 2, 0, 250)
MIXED_STATUS = (16, 0, 0, 4, 4, 16)


def takens_windows(rng, n_t, seed):
    rep = np.repeat(rng.standard_normal((n_t + 1) // 2), 2)[:n_t]
    w = np.stack([
        np.cumsum(rng.standard_normal(n_t)),
        synth.audio_windows(1, "alpha", seed=seed, n_t=n_t)[0],
        rng.standard_normal(n_t),
        np.full(n_t, 0.75),
        np.arange(n_t, dtype=np.float64),
        rep,
    ])
    w.setflags(write=False)
    return w


def takens_points(n_t, dim, tau, subsample):
    n = n_t - (dim - 1) * tau
    return -(-n // subsample) if n > 0 else 0


@functools.lru_cache(maxsize=None)
def takens_cases():
    """[(dim, subsample, n_t, tau, (6, n_t) float64)], the rows in the order of TAKENS_WINDOWS."""
    rng = np.random.default_rng(SEED + 1)
    return [(dim, sub, n_t, tau, takens_windows(rng, n_t, SEED + 10 + i))
            for i, (dim, sub, n_t, tau) in enumerate(TAKENS_GRID)]


@functools.lru_cache(maxsize=None)
def mixed_tau_batch():
    """(windows (6, 250), tau (6,) int32): one batch with oversized, valid and degenerate windows side by side."""
    rng = np.random.default_rng(SEED + 2)
    w = takens_windows(rng, MIXED_TAU["n_t"], SEED + 99)
    w = w[[0, 1, 2, 5, 0, 1]].copy()           # no constant or ramp among the valid ones: general position
    w.setflags(write=False)
    return w, np.array(MIXED_TAU["tau"], np.int32)


def takens_cloud(s, dim, tau, subsample):
    """The reference's index rule written out: rows s[i + k tau], k < dim, for i = 0, subsample, ... < n_t - (dim-1) tau."""
    n = len(s) - (dim - 1) * tau
    rows = [[s[i + k * tau] for k in range(dim)] for i in range(0, max(n, 0), subsample)]
    return np.array(rows, dtype=np.float64).reshape(-1, dim)


# ---------------------------------------------------------------------------------------------------- clouds
CLOUD_DIMS = (1, 2, 4)
CLOUD_P = (3, 4, 12, 40, 64, 65, 124, 128)


@functools.lru_cache(maxsize=None)
def cloud_cases():
    """[(kind, dim, P, (P, dim) float64)]: uniform and random-walk clouds; every fourth has its second half on top of
    its first (zero-length edges)."""
    rng = np.random.default_rng(SEED + 3)
    out = []
    for kind in ("random", "walk"):
        for dim in CLOUD_DIMS:
            for P in CLOUD_P:
                pc = rng.random((P, dim)) if kind == "random" else np.cumsum(rng.standard_normal((P, dim)), axis=0)
                if len(out) % 4 == 3:
                    pc[P // 2:] = pc[:P - P // 2]
                pc.setflags(write=False)
                out.append((kind, dim, P, pc))
    return out


RAGGED = ((40, (0, 1, 2, 3, 17, 39, 40, 41)), (200, (128, 129, 5, 100)))
RAGGED_DIMS = (2, 3, 4)


@functools.lru_cache(maxsize=None)
def ragged_cloud_batches():
    """[(p_cap, dim, buffer (n_win, p_cap, dim), n_pts (n_win,) int32)]: every row at or past n_pts[w] is NaN, so a read
    beyond a window's own points poisons its min-max or one of its keys."""
    rng = np.random.default_rng(SEED + 4)
    out = []
    for p_cap, counts in RAGGED:
        for dim in RAGGED_DIMS:
            buf = rng.random((len(counts), p_cap, dim))
            for w, n in enumerate(counts):
                buf[w, min(n, p_cap):] = np.nan
            buf.setflags(write=False)
            out.append((p_cap, dim, buf, np.array(counts, np.int32)))
    return out


# ---------------------------------------------------------------------------------------------------- corr -> dist
CORR_SIZES = (1, 2, 47, 64, 129)
CORR_STACK = 500              # 500 * 47 * 47 = 1,104,500 > 4096 * 256 elements: a second grid-stride trip


@functools.lru_cache(maxsize=None)
def corr_cases():
    """[(name, (n_win, n, n) float64)]: Pearson matrices of random windows from the oracle, one stack large enough for a
    second trip of the grid-stride loop, and one crafted matrix of edge values."""
    rng = np.random.default_rng(SEED + 5)
    out = []
    for n in CORR_SIZES:
        w = rng.standard_normal((3, n, 40)) + 0.5 * rng.standard_normal((3, 1, 40))
        out.append((f"pearson_n{n}", port.corr_dist_batch(w)[0]))
    w = rng.standard_normal((CORR_STACK, 47, 16)) + 0.5 * rng.standard_normal((CORR_STACK, 1, 16))
    stack = port.corr_dist_batch(w)[0]
    i = np.arange(47)
    # a Pearson diagonal is 1 and gives distance 0 under every method by itself: from the middle of the stack on (the
    # second trip begins at element 4096 * 256, in window 474) the diagonal holds other values, so that only the rule
    # "diagonal = 0" can put the zeros there
    stack[CORR_STACK // 2:, i, i] = rng.uniform(-1.0, 1.0, (CORR_STACK - CORR_STACK // 2, 47))
    stack[-1, 46, 46] = np.nan
    out.append(("pearson_stack", stack))
    e, tiny, nan, inf = 2.0 ** -52, 5e-324, np.nan, np.inf
    vals = [1.0, -1.0, 1.0 + e, -1.0 - e, 2.0, -2.0, 0.0, -0.0, 1e-200, -1e-200, tiny, -tiny, 1.0 - 2.0 ** -53,
            -(1.0 - 2.0 ** -53), nan, inf, -inf, 0.5, -0.5, 0.999, 1.0 - e, -1.0 + e, 0.1, 0.7071067811865476]
    m = np.resize(np.array(vals), (8, 8)).copy()       # 64 cells: every value at least twice, off and on the diagonal
    m[0, 0] = nan
    m[1, 1] = 2.0
    m[2, 2] = -inf
    m[3, 3] = 1.0
    m[7, 0] = nan
    out.append(("crafted", m[None]))
    for _, c in out:
        c.setflags(write=False)
    return out
