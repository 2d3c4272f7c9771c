"""Seeded cases for the EEG window kernels away from the reference's 47 x 250 windows: cd_window_products
(csrc/corr_dist_dev.h) as corr_dist_kernel<NB, RES> and as the fused eeg_window kernels (csrc/rips.hip).  Shared by
tests/test_eeg_shapes_model.py (the oracle held against the definition), tests/test_gpu_eeg_shapes.py and
tests/eeg_resident_child.py.

The kernel pads channels to 16 NB and samples to 32-sample tiles that run in double trips of 2 x 8 samples; it exists as
NB 1..4, resident (n_t <= 256) and streaming; the fused kernel is NB = 3, 33..48 channels, 2..256 samples.  The lengths
stand on both sides of every one of those boundaries."""
import functools

import numpy as np

from oracle import port
from tda_eeg_audio_amd import synth

CORR_CH = (1, 2, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64)
FUSED_CH = (33, 34, 40, 46, 47, 48)
RES_LENGTHS = (2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 24, 25, 31, 32, 33, 63, 64, 65, 224, 225, 249, 255, 256)
STREAM_LENGTHS = (257, 258, 287, 288, 289, 500, 1000)       # corr_dist_kernel only

# the windows of every stack, in order (see windows())
KINDS = ("latent", "white", "zero-variance channel", "duplicated channel", "offset last channel", "constant window",
         "white", "white")
N_WIN = len(KINDS)


def nb_of(n_ch):
    return (n_ch + 15) // 16


def channels_of_nb(nb):
    return tuple(c for c in CORR_CH if nb_of(c) == nb)


def seed_of(n_ch, n_t):
    return 100003 * n_ch + 17 * n_t


@functools.lru_cache(maxsize=None)
def windows(n_ch, n_t):
    """(N_WIN, n_ch, n_t): synth.eeg_windows' "latent" and "white" models, then (on latent and white windows of their own)
    a zero-variance channel, a duplicated channel, the last channel lifted by 1e3 (its mean is taken in the partial last
    16-channel block), one all-constant window, and two more white ones.  Read-only: the tests share it."""
    s = seed_of(n_ch, n_t)
    lat = synth.eeg_windows(3, seed=s, n_ch=n_ch, n_t=n_t, kind="latent")
    whi = synth.eeg_windows(4, seed=s + 7, n_ch=n_ch, n_t=n_t, kind="white")
    W = np.empty((N_WIN, n_ch, n_t))
    W[0] = lat[0]
    W[1] = whi[0]
    W[2] = lat[1]
    W[2, (2 * n_ch) // 3] = 1.25                            # zero-variance channel
    W[3] = whi[1]
    W[3, n_ch - 1] = W[3, n_ch // 4]                        # duplicated channel (itself at n_ch = 1)
    W[4] = lat[2]
    W[4, n_ch - 1] += 1e3                                   # offset in the last channel
    W[5] = -0.75                                            # all-constant window
    W[6:] = whi[2:]                                         # (white noise has the most classes alive at once)
    W.setflags(write=False)
    return W


@functools.lru_cache(maxsize=None)
def oracle_corr_dist(n_ch, n_t):
    """(corr, dist) of windows(n_ch, n_t) by the CPU oracle, computed once."""
    c, d = port.corr_dist_batch(windows(n_ch, n_t))
    c.setflags(write=False); d.setflags(write=False)
    return c, d


@functools.lru_cache(maxsize=None)
def oracle_diagrams(n_ch, n_t, w):
    """[H0, H1] of window w of windows(n_ch, n_t) by the CPU oracle, computed once."""
    return port.rips_dm(oracle_corr_dist(n_ch, n_t)[1][w])


def definition_longdouble(W):
    """The definition the reference runs (np.corrcoef, NaN -> 0, clip, sqrt(2 (1 - r)), zero diagonal;
    notebooks/2_graph_construction.ipynb:86-122), evaluated in np.longdouble on the same float64 samples."""
    W = np.asarray(W, dtype=np.longdouble)
    n_win, n_ch, n_t = W.shape
    X = W - W.mean(axis=2, keepdims=True)
    cov = X @ X.transpose(0, 2, 1) / np.longdouble(n_t - 1)
    sd = np.sqrt(np.einsum("wii->wi", cov))
    with np.errstate(invalid="ignore", divide="ignore"):
        r = cov / sd[:, :, None] / sd[:, None, :]
    r = np.clip(r, -1, 1)                                   # (np.corrcoef clips, nb2:105 again)
    r = np.where(np.isnan(r), np.longdouble(0), r)          # nb2:95
    d = np.sqrt(2 * (1 - r))
    d = np.maximum(d, 0)
    idx = np.arange(n_ch)
    d[:, idx, idx] = 0
    return r, d


def max_alive(h1):
    """Largest number of H1 rows alive at once: births <= x < deaths, over the sorted events."""
    h1 = np.asarray(h1, dtype=np.float64).reshape(-1, 2)
    if len(h1) == 0:
        return 0
    b, d = np.sort(h1[:, 0]), np.sort(h1[:, 1])
    return int((np.searchsorted(b, b, side="right") - np.searchsorted(d, b, side="right")).max())


def bipartite_windows(n_ch, m, n_t, n_rep, seed):
    """Windows whose correlation graph is K(m, n_ch - m): every cross-group correlation 0.23, every within-group one 0.20
    (a positive-definite Gram matrix), so the m (n_ch - m) cross edges (d = 1.241) enter before any within-group edge
    (d = 1.265) and (m - 1)(n_ch - m - 1) H1 classes are alive at once.  tests/test_gpu_parity.py::_bipartite_windows is
    (47, 23, 250), draw for draw."""
    assert n_t > n_ch, "the channels need n_ch orthonormal centred directions"
    rng = np.random.default_rng(seed)
    c, w = 0.23, 0.20
    G = np.full((n_ch, n_ch), w)
    G[:m, m:] = c; G[m:, :m] = c
    np.fill_diagonal(G, 1.0)
    ev, U = np.linalg.eigh(G)
    assert ev.min() > 0
    L = (U * np.sqrt(ev)) @ U.T
    out = np.empty((n_rep, n_ch, n_t))
    for k in range(n_rep):
        Z = rng.standard_normal((n_t, n_ch))
        Z -= Z.mean(axis=0)
        Q, _ = np.linalg.qr(Z)
        out[k] = (L @ Q.T) * rng.uniform(0.5, 2.0, size=(n_ch, 1))      # per-channel scale: correlation unchanged
    return out


@functools.lru_cache(maxsize=None)
def batch_48():
    """The 48-channel batch with more than 512 classes alive at once: K(24,24) at index 1 and K(23,25) at index 4 among
    ordinary 48-channel windows.  Returns (windows, indices of the bipartite ones)."""
    W = np.array(windows(48, 250))
    W[1] = bipartite_windows(48, 24, 250, 1, seed=3)[0]
    W[4] = bipartite_windows(48, 23, 250, 1, seed=4)[0]
    W.setflags(write=False)
    return W, (1, 4)


# ---- sliding form of corr_dist_kernel: (n_ch, win_len, step, n_samples) ----
SLIDING_CH = (5, 33, 64)
SLIDING_WIN = (2, 33, 256, 300)


def sliding_cases():
    out = []
    for n_ch in SLIDING_CH:
        for win_len in SLIDING_WIN:
            for step in (1, 7, win_len + 3):
                n_s = win_len + 3 * step
                n_s += 1 - (n_s & 1)                         # odd row stride
                out += [(n_ch, win_len, step, n_s), (n_ch, win_len, step, win_len), (n_ch, win_len, step, win_len - 1)]
    return out


def n_windows(n_s, win_len, step):
    return (n_s - win_len) // step + 1 if n_s >= win_len else 0


def sliding_signal(n_rec, n_ch, n_s, win_len, step, seed):
    """(n_rec, n_ch, n_s) recordings; with step > win_len the samples in the gaps between the windows (and behind the
    last one) are NaN: a kernel that uses a sample outside its window poisons the matrix."""
    rng = np.random.default_rng(seed)
    sig = rng.standard_normal((n_rec, n_ch, n_s)) + 0.4 * rng.standard_normal((n_rec, 1, n_s))
    if step > win_len:
        used = np.zeros(n_s, bool)
        for k in range(n_windows(n_s, win_len, step)):
            used[k * step:k * step + win_len] = True
        sig[:, :, ~used] = np.nan
    return sig


def stack_of(sig, win_len, step):
    """create_sliding_windows (notebooks/1_preprocesamiento.ipynb:314-381) of every recording, recording-major."""
    n_rec, n_ch, n_s = sig.shape
    n = n_windows(n_s, win_len, step)
    return np.stack([sig[r, :, k * step:k * step + win_len] for r in range(n_rec) for k in range(n)]) if n else \
        np.empty((0, n_ch, win_len))


# ---- cut of the fused grid for the TDA_EEG_RESIDENT=1 child ----
RESIDENT_CH = (33, 47, 48)
RESIDENT_LENGTHS = (2, 9, 33, 250, 256)


def as_recordings(W):
    """A stack of 8 windows as recordings the fused kernel reads in place.  sig: (2, n_ch, 4 n_t), four windows end to end
    per recording (win_len = step = n_t gives the stack back, in order).  packed / start / ld / order: recordings of 3 and
    5 windows, one and three samples longer than that, packed back to back, and a window table in shuffled order
    (table row k is window order[k])."""
    n, n_ch, n_t = W.shape
    assert n == 8
    sig = np.stack([np.concatenate(list(W[4 * r:4 * r + 4]), axis=1) for r in range(2)])
    lens = [3 * n_t + 1, 5 * n_t + 3]
    recs = [np.concatenate(list(W[:3]) + [np.zeros((n_ch, 1))], axis=1), np.concatenate(list(W[3:]) + [np.zeros((n_ch, 3))], axis=1)]
    order = np.array([5, 1, 7, 0, 4, 2, 6, 3])
    start = np.array([(0 if w < 3 else n_ch * lens[0]) + (w if w < 3 else w - 3) * n_t for w in order], np.int64)
    ld = np.array([lens[0] if w < 3 else lens[1] for w in order], np.int64)
    return np.ascontiguousarray(sig), np.concatenate([r.ravel() for r in recs]), start, ld, order


# ---- device tensors and their comparison (torch) ----
def to_device(a, dev):
    """A copy of the array on the device (the shared cases are read-only, which torch.from_numpy warns about)."""
    import torch
    return torch.from_numpy(np.array(a)).to(dev)


def bytes_equal(a, b):
    import torch
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64))


def same_diagrams(a, b):
    """Two DeviceDiagrams: counts and status equal, rows equal up to the counts (bit for bit, in order)."""
    import torch
    if not (torch.equal(a.c0, b.c0) and torch.equal(a.c1, b.c1) and torch.equal(a.status, b.status)):
        return False
    dev = a.c0.device
    m0 = torch.arange(a.h0.shape[1], device=dev)[None, :] < a.c0[:, None].clamp(max=a.h0.shape[1])
    m1 = torch.arange(a.h1.shape[1], device=dev)[None, :] < a.c1[:, None].clamp(max=a.h1.shape[1])
    n0 = torch.arange(b.h0.shape[1], device=dev)[None, :] < b.c0[:, None].clamp(max=b.h0.shape[1])
    n1 = torch.arange(b.h1.shape[1], device=dev)[None, :] < b.c1[:, None].clamp(max=b.h1.shape[1])
    return bytes_equal(a.h0[m0], b.h0[n0]) and bytes_equal(a.h1[m1], b.h1[n1])
