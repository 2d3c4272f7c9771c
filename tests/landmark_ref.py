"""
CPU reference of the landmark Rips route (helper module, no tests in it): the text of include/tdaeeg.h, "Landmark Rips",
in numpy on the oracle's building blocks.

  cloud_of        oracle.port.takens, then oracle.port.minmax_normalise
  greedy          the selection: d(., p) is column p of oracle.port.cloud_dm -- every operation is one the oracle states
                  and the cloud Rips kernel already reproduces bit for bit
  landmarks       the outputs of the kernel for one window: (lm, idx, lambda, r_cover, n_lm, n_full), None when refused
  diagrams        port.rips_f32(float32(cloud_dm(rows))): the oracle's diagrams of any normalised cloud
  directed_hausdorff  max over the cloud of the distance to the nearest landmark, from coordinate differences -- an
                  independent route to r_cover (equal up to the rounding of the Gram form, not bit for bit)
"""
import numpy as np

from oracle import port

LM_MAX_POINTS = 1024
MAX_POINTS = 128


def n_takens(n_t, dim, tau, subsample):
    nn = n_t - (dim - 1) * tau
    return -(-nn // subsample) if nn > 0 else 0


def cloud_of(window, tau, dim=3, subsample=1, normalise=True):
    pc = port.takens(window, dim, int(tau), subsample)
    return port.minmax_normalise(pc) if normalise and len(pc) else pc


def greedy(X, n_perm):
    """(idx, lambda, r_cover) of a cloud X (P, dim) as it stands (normalised or not)."""
    X = np.ascontiguousarray(X, dtype=np.float64)
    P = len(X)
    if P <= n_perm:
        return np.arange(P, dtype=np.int32), np.zeros(P), 0.0
    dm = port.cloud_dm(X)                   # dm[:, p]: ((-2 dot + |x_i|^2) + |x_p|^2), clamped, diagonal 0, sqrt
    idx = np.zeros(n_perm, np.int32)
    lam = np.zeros(n_perm)
    ds = dm[:, 0].copy()
    for t in range(1, n_perm):
        idx[t] = np.argmax(ds)              # the lowest index of the maximum
        lam[t - 1] = ds[idx[t]]
        ds = np.minimum(ds, dm[:, idx[t]])
    lam[n_perm - 1] = ds.max()
    return idx, lam, float(lam[n_perm - 1])


def landmarks(X, n_perm):
    """The kernel's outputs for the (already normalised) cloud X, or None for a cloud it refuses."""
    if len(X) > LM_MAX_POINTS:
        return None
    idx, lam, rc = greedy(X, n_perm)
    return X[idx], idx, lam, rc, len(idx), len(X)


def diagrams(X):
    """[H0, H1] of the oracle for a normalised cloud of >= 3 points."""
    return port.rips_f32(port.cloud_dm(np.ascontiguousarray(X)).astype(np.float32))


def directed_hausdorff(X, L):
    d = np.sqrt(((X[:, None, :] - L[None, :, :]) ** 2).sum(axis=2))
    return float(d.min(axis=1).max())


def band_window(n_t, seed, band="alpha"):
    from tda_eeg_audio_amd import synth
    return synth.audio_windows(1, band, seed=seed, n_t=n_t)[0]


def stability_cases():
    """The seeded inputs of the stability test: (name, window, tau, dim, subsample, n_perm)."""
    rng = np.random.default_rng(20241)
    return [
        ("noise-250", rng.standard_normal(250), 2, 3, 1, 128),          # P = 246
        ("band-250", band_window(250, 7), 6, 3, 1, 64),                 # P = 238
        ("band-600", band_window(600, 11, "theta"), 5, 3, 1, 128),      # P = 590
        ("band-250-sub2", band_window(250, 13, "delta"), 40, 3, 2, 17),  # P = 85
    ]


def pivot_order_counts(X, n_perm):
    """Upstream slices its pivot rows (dperm2all[:, idx_perm]); against the columns d(., p) of the selection that adds the
    two squared norms in the other order, i.e. it is the transpose of the landmark distance matrix.  Returns (entries
    that differ in float64, entries that differ after the cast to float32, entries)."""
    idx, _, _ = greedy(X, n_perm)
    b = port.cloud_dm(X[idx])               # the composition: the cloud path on the landmark rows
    return int((b.T != b).sum()), int((b.T.astype(np.float32) != b.astype(np.float32)).sum()), b.size
