"""
utils.py -- drop-in for the hot-path names of the reference's scripts/utils.py.

Same names, arguments and error behaviour (file:line of the reference in each docstring);
every computation runs in the HIP kernels of libtdaeeg.so through the C ABI.  A driver that
does ``from tda_eeg_audio_amd.utils import *`` instead of ``from utils import *`` keeps working.
Single-call functions launch a batch of one; ``with utils.batch():`` around the reference's per-window loop turns
the same calls into one launch per stage (see class batch); for throughput use tda_eeg_audio_amd.engine / pipeline,
which keep whole batches resident in HBM.

Not provided here (host-side preparation in front of the path):
load_audio, compute_envelope, bandpass_filter, resample_audio (utils.py:47-79).

Beyond the reference: permute_labels_by_subject (utils.py:198-215) feeds subject_permutations and
two_sample_permutation_test, the permutation test of Robinson and Turner on distance / Gram matrices between recordings.
"""
import numpy as np

from . import engine
from ._lib import LM_MAX_POINTS, TdaError

# ── TDA parameters ── (scripts/utils.py:24-27)
MAX_DIM = 1
MAX_EDGE_LENGTH = 2.0
TAKENS_DIM = 3
TAKENS_SUBSAMPLE = 2

# ── Frequency bands ── (scripts/utils.py:30-36)
FREQ_BANDS = {
    "delta": (0.5, 4),
    "theta": (4, 8),
    "alpha": (8, 13),
    "beta": (13, 30),
    "gamma": (30, 50),
}

# ── Sampling rates ── (scripts/utils.py:39-40)
FS_AUDIO = 44100
FS_EEG = 250

FEATURE_KEYS = ["n_features", "n_essential", "mean_birth", "std_birth", "mean_death", "std_death",
                "mean_persistence", "std_persistence", "max_persistence", "total_persistence",
                "persistence_entropy"]


def create_windows(s, win_samples, step_samples):
    """scripts/utils.py:82-89 -- overlapping windows of a 1-D signal (pure slicing, host side)."""
    s = np.asarray(s)
    n = (len(s) - win_samples) // step_samples + 1 if len(s) >= win_samples else 0
    if n <= 0:
        return np.array([]).reshape(0, win_samples)
    idx = np.arange(n)[:, None] * step_samples + np.arange(win_samples)[None, :]
    return s[idx]


def compute_tau(s, max_lag=None):
    """scripts/utils.py:92-104 -- first zero crossing of the autocorrelation (tau_kernel)."""
    s = np.asarray(s, dtype=np.float64).reshape(1, -1)
    return int(engine.tau_batch(s, max_lag)[0])


def _signal(s, name):
    s = np.asarray(s, dtype=np.float64)
    if s.ndim != 1 or s.shape[0] < 1:
        raise ValueError(f"{name}: a 1-D signal")
    return s.reshape(1, -1)


def compute_ami(s, max_lag=None, n_bins=16):
    """Average mutual information, in nats, of a 1-D signal with itself L samples later, L = 0..max_lag, on a histogram of
    n_bins equal bins between the signal's minimum and maximum (include/tdaeeg.h, "Delay and dimension selection"; Fraser
    & Swinney 1986): a (max_lag + 1,) float64 array.  max_lag None is len(s) // 4, as compute_tau; it is cut to len(s) - 2.
    A constant signal gives zeros; ValueError for a bad argument or a sample that is not finite."""
    ami, _, _, st = engine.ami_batch(_signal(s, "compute_ami"), max_lag, n_bins)
    if st[0] & 64:
        raise ValueError("compute_ami: the signal has a sample that is not finite")
    return ami[0]


def compute_tau_ami(s, max_lag=None, n_bins=16):
    """The twin of compute_tau with the nonlinear statistic: the first local minimum of compute_ami(s, max_lag, n_bins),
    the smallest L >= 1 with I(L) < I(L - 1) and I(L) <= I(L + 1).  Without one (a monotone curve, a constant signal)
    compute_tau's fallback max(max_lag // 10, 1)."""
    w = _signal(s, "compute_tau_ami")
    _, tau, _, st = engine.ami_batch(w, max_lag, n_bins)
    if st[0] & 64:
        raise ValueError("compute_tau_ami: the signal has a sample that is not finite")
    return int(tau[0]) if tau[0] else max(engine.ami_args(w.shape[1], max_lag, n_bins)[0] // 10, 1)


def false_nearest_neighbours(s, tau, max_dim=5, theiler=None, r_tol=10.0, a_tol=2.0, frac_tol=0.05):
    """False nearest neighbours of the delay embeddings of s with delay tau in the dimensions 1..max_dim (include/tdaeeg.h,
    "Delay and dimension selection"; Kennel, Brown & Abarbanel 1992): a dict of rows, each (max_dim,) -- the int32 counts
    valid (points with a neighbour), false_distance (the next coordinate moves the neighbour away by more than r_tol times
    their distance), false_size (the pair ends further apart than a_tol standard deviations of s), false_either, and the
    float64 fraction = false_either / valid -- with "dim", the smallest dimension whose fraction is at most frac_tol (0
    without one).  theiler: neighbours closer than theiler samples in time do not count; None means tau.  tau < 1 is a
    TdaError, as in the Takens calls; ValueError for a bad argument or a sample that is not finite."""
    from . import _lib
    w = _signal(s, "false_nearest_neighbours")
    if isinstance(tau, bool) or not isinstance(tau, (int, np.integer)):
        raise ValueError(f"tau must be an integer, not {tau!r}")
    theiler = max(int(tau), 1) if theiler is None else theiler
    cnt, frac, dim, _, st = engine.fnn_batch(w, int(tau), max_dim, theiler, r_tol, a_tol, frac_tol)
    if st[0] & 64:
        raise ValueError("false_nearest_neighbours: the signal has a sample that is not finite")
    if st[0] & 16:
        raise TdaError("tau must be >= 1")
    out = {name: cnt[0, :, k] for k, name in enumerate(_lib.FNN_COUNT_NAMES)}
    out.update(fraction=frac[0], dim=int(dim[0]))
    return out


def estimate_embedding_dimension(s, tau, max_dim=5, theiler=None, r_tol=10.0, a_tol=2.0, frac_tol=0.05):
    """The "dim" of false_nearest_neighbours: the smallest dimension in 1..max_dim at which at most frac_tol of the points
    have a false nearest neighbour; 0 when none has (raise max_dim, or the signal is noise)."""
    return false_nearest_neighbours(s, tau, max_dim, theiler, r_tol, a_tol, frac_tol)["dim"]


def takens_embedding(s, dim, tau, subsample=1):
    """scripts/utils.py:107-116 -- the (P, dim) delay cloud.  A pure gather; the batched path
    (engine.takens_rips_batch) performs it inside the Rips kernel and never materialises it."""
    s = np.asarray(s)
    n = len(s) - (dim - 1) * tau
    if n <= 0:
        return np.array([]).reshape(0, dim)
    indices = np.arange(n)[:, None] + np.arange(dim)[None, :] * tau
    pc = s[indices]
    if subsample > 1:
        pc = pc[::subsample]
    return pc


def _check_dim(max_dim):
    if max_dim != 1:
        raise NotImplementedError("the HIP engine computes H0 and H1 (maxdim=1), as the reference does")


_NO_BATCH_N_PERM = ("n_perm is not recorded by utils.batch (its add_cloud normalises, and the landmark route must not "
                    "normalise twice): call engine.cloud_landmarks_batch / engine.takens_rips_landmarks_dev directly")


def greedy_landmarks(point_cloud, n_perm, normalise=True):
    """ripser's greedy permutation (n_perm) of one (P, dim) cloud of up to 1024 rows: (idx_perm, lambdas, r_cover), the
    furthest-point order from point 0, the insertion radii and the covering radius (include/tdaeeg.h, "Landmark Rips").
    P <= n_perm: every point, in its own order, with radii 0."""
    if _ACTIVE is not None:
        raise NotImplementedError(_NO_BATCH_N_PERM)
    pc = np.asarray(point_cloud, dtype=np.float64)
    if pc.ndim != 2 or pc.shape[0] < 1:
        raise ValueError("greedy_landmarks: a (P, dim) cloud with P >= 1")
    if pc.shape[0] > LM_MAX_POINTS:
        raise TdaError(f"more than {LM_MAX_POINTS} points: not supported by the landmark kernel")
    _, idx, lam, rc, n_lm, _ = engine.cloud_landmarks_batch(pc[None], n_perm, normalise=normalise)
    k = int(n_lm[0])
    return idx[0, :k].copy(), lam[0, :k].copy(), float(rc[0])


def _landmark_persistence(point_cloud, max_edge_length, n_perm):
    if point_cloud.shape[0] > LM_MAX_POINTS:
        raise TdaError(f"more than {LM_MAX_POINTS} points: not supported by the landmark kernel")
    lm, _, _, _, n_lm, _ = engine.cloud_landmarks_batch(point_cloud[None], n_perm)
    # the landmark rows are normalised already: the cloud path takes them as they are
    h0, h1, st = engine.cloud_rips_batch(lm, n_pts=n_lm, normalise=False, thresh=max_edge_length, h1_cap=_h1_cap(int(n_lm[0])))
    _check_status(st[0])
    return [h0[0], h1[0]]


def compute_audio_persistence(point_cloud, max_dim=MAX_DIM, max_edge_length=MAX_EDGE_LENGTH, n_perm=None):
    """scripts/utils.py:123-132 -- [H0, H1] of a point cloud (min-max normalised, Rips).  n_perm (ripser's keyword): Rips
    on n_perm greedy landmarks, for clouds of up to 1024 rows; each diagram then lies within bottleneck distance
    2 * r_cover (greedy_landmarks) of the whole cloud's."""
    _check_dim(max_dim)
    point_cloud = np.asarray(point_cloud, dtype=np.float64)
    if n_perm is not None and _ACTIVE is not None:
        raise NotImplementedError(_NO_BATCH_N_PERM)
    if len(point_cloud) < 3:
        return [np.array([[0, 0]]), np.array([[0, 0]])]
    if n_perm is not None:
        return _landmark_persistence(point_cloud, max_edge_length, n_perm)
    if _ACTIVE is not None:
        return _ACTIVE.add_cloud(point_cloud, max_edge_length)
    h0, h1, st = engine.cloud_rips_batch(point_cloud[None], thresh=max_edge_length, h1_cap=_h1_cap(len(point_cloud)))
    _check_status(st[0])
    return [h0[0], h1[0]]


def compute_eeg_persistence(dist_matrix, max_dim=MAX_DIM, max_edge_length=MAX_EDGE_LENGTH):
    """scripts/utils.py:135-141 -- [H0, H1] of a distance matrix (symmetrised, diag 0, >= 0)."""
    _check_dim(max_dim)
    dm = np.asarray(dist_matrix, dtype=np.float64)
    if dm.ndim != 2 or dm.shape[0] != dm.shape[1]:
        raise ValueError("Distance matrix is not square")      # the only thing ripser rejects
    if _ACTIVE is not None:
        return _ACTIVE.add_dm(dm, max_edge_length)
    h0, h1, st = engine.rips_dm_batch(dm[None], thresh=max_edge_length, symmetrise=True,
                                      h1_cap=_h1_cap(dm.shape[0]))
    _check_status(st[0])
    return [h0[0], h1[0]]


def _generators_result(h0, c0, h1, c1, g, idx=None):
    """One window's diagrams and generator outputs as compute_*_generators return them; idx (optional) maps the vertex
    numbers back to the caller's (the landmark indices of n_perm)."""
    n0, n1 = min(int(c0[0]), h0.shape[1]), min(int(c1[0]), h1.shape[1])
    back = (lambda a: a) if idx is None else (lambda a: np.where(a >= 0, idx[np.maximum(a, 0)], -1))
    gen = back(g["h1_gen"][0, :n1].astype(np.int64))
    part = g["part"][0]
    if idx is not None:
        part = part[:len(idx)]
    return {"dgms": [h0[0, :n0].copy(), h1[0, :n1].copy()],
            "h0_edges": back(g["h0_edge"][0, :n0].astype(np.int64)),
            "h1_birth_edges": gen[:, :2], "h1_death_edges": gen[:, 2:],
            "cycles": [back(g["cyc"][0, r, :min(int(g["cyc_len"][0, r]), g["cyc"].shape[2])].astype(np.int64))
                       for r in range(n1)],
            "flags": g["h1_flag"][0, :n1].copy(), "participation": part.copy()}


def compute_eeg_generators(distance_matrix, thresh=MAX_EDGE_LENGTH):
    """The twin of compute_eeg_persistence that also says where the features live (include/tdaeeg.h, "Generators and
    representative cycles"; ripser's do_cocycles, GUDHI's flag_persistence_generators): a dict of
      dgms [H0, H1]            the diagrams of compute_eeg_persistence
      h0_edges (len(H0), 2)    the forest edge [a, b], a > b, of every finite H0 row; -1 for the essential rows
      h1_birth_edges, h1_death_edges (len(H1), 2)   the edge that closes the loop of every H1 row and the youngest edge of
                               the triangle that kills it; -1, -1 for the death edge of an essential row
      cycles                   per H1 row the vertices of a representative cycle, birth_a ... birth_b
      flags (len(H1),)         TDA_GEN_* bits; 0 on generic input
      participation (n,)       per channel the persistence summed over the unflagged finite rows whose cycle visits it.
    Not recorded by utils.batch(): it launches at once."""
    dm = np.asarray(distance_matrix, dtype=np.float64)
    if dm.ndim != 2 or dm.shape[0] != dm.shape[1]:
        raise ValueError("Distance matrix is not square")
    h0, c0, h1, c1, st = engine.rips_dm_batch(dm[None], thresh=thresh, symmetrise=True, h1_cap=_h1_cap(dm.shape[0]), raw=True)
    _check_status(st[0])
    return _generators_result(h0, c0, h1, c1, engine.generators_dm_batch(dm[None], h0, c0, h1, c1, thresh=thresh))


def compute_audio_generators(point_cloud, thresh=MAX_EDGE_LENGTH, n_perm=None):
    """The twin of compute_audio_persistence: the same dict for a (P, dim) point cloud, min-max normalised; the vertex
    numbers are row numbers of point_cloud.  With n_perm (ripser's keyword) the complex is that of the n_perm greedy
    landmarks and every index is mapped back through the landmark indices, as ripser's idx_perm allows; participation
    then has one entry per landmark, in landmark order, and the dict also holds idx_perm.  Fewer than 3 points: TdaError
    (there is no complex); more than 128 (1024 with n_perm): TdaError."""
    pc = np.asarray(point_cloud, dtype=np.float64)
    if pc.ndim != 2 or pc.shape[0] < 1:
        raise ValueError("compute_audio_generators: a (P, dim) point cloud")
    if pc.shape[0] < 3:
        raise TdaError("fewer than 3 points: no Rips complex to take generators from")
    if n_perm is None:
        h0, c0, h1, c1, st = engine.cloud_rips_batch(pc[None], thresh=thresh, h1_cap=_h1_cap(len(pc)), raw=True)
        _check_status(st[0])
        return _generators_result(h0, c0, h1, c1, engine.generators_cloud_batch(pc[None], h0, c0, h1, c1, thresh=thresh))
    if pc.shape[0] > LM_MAX_POINTS:
        raise TdaError(f"more than {LM_MAX_POINTS} points: not supported by the landmark kernel")
    lm, idx, _, _, n_lm, _ = engine.cloud_landmarks_batch(pc[None], n_perm)
    # the landmark rows are normalised already: the cloud path takes them as they are
    h0, c0, h1, c1, st = engine.cloud_rips_batch(lm, n_pts=n_lm, normalise=False, thresh=thresh, h1_cap=_h1_cap(int(n_lm[0])),
                                                 raw=True)
    _check_status(st[0])
    g = engine.generators_cloud_batch(lm, h0, c0, h1, c1, n_pts=n_lm, normalise=False, thresh=thresh)
    idx_perm = idx[0, :int(n_lm[0])].astype(np.int64)
    out = _generators_result(h0, c0, h1, c1, g, idx_perm)
    out["idx_perm"] = idx_perm
    return out


def compute_eeg_euler_curve(distance_matrix, grid, max_dim=3, thresh=MAX_EDGE_LENGTH):
    """The twin of compute_eeg_persistence for the Euler characteristic curve (include/tdaeeg.h, "Euler characteristic
    curves"): the (max_dim + 2, n_grid) int32 block of the simplex counts f_0 .. f_max_dim and chi of the Rips complex of
    the symmetrised distance matrix at every scale of grid, by the keys compute_eeg_persistence uses.  Not recorded by
    utils.batch(): it launches at once.  ValueError for a bad grid or max_dim."""
    dm = np.asarray(distance_matrix, dtype=np.float64)
    if dm.ndim != 2 or dm.shape[0] != dm.shape[1]:
        raise ValueError("Distance matrix is not square")
    out, _ = engine.euler_dm_batch(dm[None], grid, max_dim=max_dim, thresh=thresh, symmetrise=True)
    return out[0]


def compute_audio_euler_curve(point_cloud, grid, max_dim=3, thresh=MAX_EDGE_LENGTH):
    """The twin of compute_audio_persistence: the same block for a (P, dim) point cloud, min-max normalised, by the keys
    compute_audio_persistence uses.  A cloud of fewer than 3 points gives zeros, as its diagrams are [[0, 0]]; more than
    128 points are a TdaError."""
    pc = np.asarray(point_cloud, dtype=np.float64)
    if pc.ndim != 2 or pc.shape[0] < 1:
        raise ValueError("compute_audio_euler_curve: a (P, dim) point cloud")
    out, st = engine.euler_cloud_batch(pc[None], grid, max_dim=max_dim, thresh=thresh)
    _check_status(st[0])
    return out[0]


def _network_rows(counts, measures, nodal):
    """The blocks of one window as a dict of named rows (_lib.NET_COUNT_NAMES, NET_MEASURE_NAMES; "nodal_" + a name of
    NET_NODAL_NAMES for the per-vertex rows)."""
    from . import _lib
    out = {name: counts[k] for k, name in enumerate(_lib.NET_COUNT_NAMES)}
    out.update({name: measures[k] for k, name in enumerate(_lib.NET_MEASURE_NAMES)})
    if nodal is not None:
        out.update({"nodal_" + name: nodal[k] for k, name in enumerate(_lib.NET_NODAL_NAMES)})
    return out


def compute_eeg_network_curves(distance_matrix, grid, nodal=False, thresh=MAX_EDGE_LENGTH):
    """The twin of compute_eeg_euler_curve for the graph measures (include/tdaeeg.h, "Network curves"): a dict of named
    rows, each (n_grid,) -- the int32 counts edges, isolated, max_degree, wedges, triangles, components, largest, pairs,
    hops, diameter and the float64 measures transitivity, clustering, efficiency, path_length of the graph of the
    symmetrised distance matrix thresholded at every scale of grid, by the keys compute_eeg_persistence uses.  nodal=True
    adds the (n_grid, n) int32 rows nodal_degree, nodal_triangles, nodal_reach, nodal_farness, nodal_eccentricity.  Not
    recorded by utils.batch(): it launches at once.  ValueError for a bad grid."""
    dm = np.asarray(distance_matrix, dtype=np.float64)
    if dm.ndim != 2 or dm.shape[0] != dm.shape[1]:
        raise ValueError("Distance matrix is not square")
    cnt, mea, nod, _ = engine.network_dm_batch(dm[None], grid, nodal=nodal, thresh=thresh, symmetrise=True)
    return _network_rows(cnt[0], mea[0], nod[0] if nodal else None)


def compute_audio_network_curves(point_cloud, grid, nodal=False, thresh=MAX_EDGE_LENGTH):
    """The twin of compute_audio_euler_curve: the same dict for a (P, dim) point cloud, min-max normalised, by the keys
    compute_audio_persistence uses (the nodal rows are (n_grid, P)).  A cloud of fewer than 3 points gives zeros, as its
    diagrams are [[0, 0]]; more than 128 points are a TdaError."""
    pc = np.asarray(point_cloud, dtype=np.float64)
    if pc.ndim != 2 or pc.shape[0] < 1:
        raise ValueError("compute_audio_network_curves: a (P, dim) point cloud")
    cnt, mea, nod, st = engine.network_cloud_batch(pc[None], grid, nodal=nodal, thresh=thresh)
    _check_status(st[0])
    return _network_rows(cnt[0], mea[0], nod[0] if nodal else None)


def _recurrence_rows(counts, measures, hist):
    """The blocks of one window as a dict of named rows (_lib.RQA_COUNT_NAMES, RQA_MEASURE_NAMES; diag_hist and vert_hist
    for the line-length histograms, column l - 1 for the length l)."""
    from . import _lib
    out = {name: counts[k] for k, name in enumerate(_lib.RQA_COUNT_NAMES)}
    out.update({name: measures[k] for k, name in enumerate(_lib.RQA_MEASURE_NAMES)})
    if hist is not None:
        out.update({"diag_hist": hist[0], "vert_hist": hist[1]})
    return out


def compute_recurrence_curves_from_distances(distance_matrix, grid, theiler=1, l_min=2, v_min=2, histograms=False,
                                             thresh=MAX_EDGE_LENGTH):
    """Recurrence quantification of a distance matrix whose rows are in time order, at every scale of grid
    (include/tdaeeg.h, "Recurrence curves"): a dict of named rows, each (n_grid,) -- the int32 counts recurrences,
    diag_lines, diag_points, diag_longest, vert_lines, vert_points, vert_longest and the float64 measures recurrence_rate,
    determinism, diag_mean, diag_entropy, laminarity, trapping_time, vert_entropy of the recurrence plot of the symmetrised
    matrix, by the keys compute_eeg_persistence uses.  theiler: pairs closer than theiler steps are no recurrences;
    l_min, v_min: the shortest diagonal / vertical line that counts.  histograms=True adds the (n_grid, n) int32 rows
    diag_hist and vert_hist.  Not recorded by utils.batch(): it launches at once.  ValueError for a bad argument."""
    dm = np.asarray(distance_matrix, dtype=np.float64)
    if dm.ndim != 2 or dm.shape[0] != dm.shape[1]:
        raise ValueError("Distance matrix is not square")
    cnt, mea, his, _ = engine.recurrence_dm_batch(dm[None], grid, theiler, l_min, v_min, histograms, thresh, True)
    return _recurrence_rows(cnt[0], mea[0], his[0] if histograms else None)


def compute_audio_recurrence_curves(point_cloud, grid, theiler=1, l_min=2, v_min=2, histograms=False,
                                    thresh=MAX_EDGE_LENGTH):
    """The same dict for a (P, dim) point cloud whose rows are in time order (a Takens embedding), min-max normalised, by
    the keys compute_audio_persistence uses (the histogram rows are (n_grid, P)).  A cloud of fewer than 3 points gives
    zeros, as its diagrams are [[0, 0]]; more than 128 points are a TdaError."""
    pc = np.asarray(point_cloud, dtype=np.float64)
    if pc.ndim != 2 or pc.shape[0] < 1:
        raise ValueError("compute_audio_recurrence_curves: a (P, dim) point cloud")
    cnt, mea, his, st = engine.recurrence_cloud_batch(pc[None], grid, theiler, l_min, v_min, histograms, thresh=thresh)
    _check_status(st[0])
    return _recurrence_rows(cnt[0], mea[0], his[0] if histograms else None)


def compute_signal_recurrence_curves(x, tau, grid, dim=TAKENS_DIM, subsample=TAKENS_SUBSAMPLE, theiler=1, l_min=2, v_min=2,
                                     histograms=False, thresh=MAX_EDGE_LENGTH):
    """The same dict for the delay embedding of a 1-D signal x with delay tau (takens_embedding(x, dim, tau, subsample),
    gathered inside the kernel): the curves of compute_audio_recurrence_curves of that cloud.  One step of a line is
    `subsample` samples; the histogram rows are (n_grid, 128).  Fewer than 3 points give zeros; more than 128 points or
    tau < 1 are a TdaError."""
    x = np.asarray(x, dtype=np.float64)
    if x.ndim != 1 or x.shape[0] < 1:
        raise ValueError("compute_signal_recurrence_curves: a 1-D signal")
    cnt, mea, his, _, st = engine.recurrence_takens_batch(x[None], int(tau), grid, theiler, l_min, v_min, histograms, dim,
                                                          subsample, thresh)
    _check_status(st[0])
    return _recurrence_rows(cnt[0], mea[0], his[0] if histograms else None)


def compute_sublevel_persistence(x, return_index=False):
    """H0 of the sublevel-set (lower-star) filtration of a time series (include/tdaeeg.h, "Sublevel-set persistence of time
    series"; ripser's lower_star example on a 1-D signal): an (m, 2) array like dgms[0], every local minimum paired with
    the local maximum at which its basin merges into a deeper one, finite rows in ripser's H0 order, the global minimum's
    (x[g], inf) last.  return_index=True: (diagram, (m, 2) int32 indices of the birth and death samples, -1 for the
    essential death).  A 2-D input (n_signals, n_t) gives a list, one launch for all.  Superlevel sets: pass -x.  Not
    recorded by utils.batch(): it launches at once.  ValueError for samples that are not finite; TdaError for more than
    SL_MAX_SAMPLES samples."""
    a = np.asarray(x, dtype=np.float64)
    if a.ndim not in (1, 2) or a.shape[-1] < 1:
        raise ValueError("compute_sublevel_persistence: a signal of at least one sample, or an (n_signals, n_t) array")
    dgm, cnt, idx, st = engine.sublevel_batch(a.reshape(-1, a.shape[-1]))
    if st.any():
        raise ValueError("compute_sublevel_persistence: the signal has samples that are not finite")
    out = [(dgm[i, :cnt[i]].copy(), idx[i, :cnt[i]].copy()) if return_index else dgm[i, :cnt[i]].copy()
           for i in range(dgm.shape[0])]
    return out[0] if a.ndim == 1 else out


def _plv_window(window):
    a = np.asarray(window, dtype=np.float64)
    if a.ndim != 2 or a.shape[0] < 2 or a.shape[1] < 2:
        raise ValueError("a window (n_ch, n_t) of at least two channels and two samples")
    return a


def compute_plv_matrix(window):
    """The phase-locking value of every pair of channels of a window (n_ch, n_t) (include/tdaeeg.h, "Phase-locking value";
    Lachaux et al. 1999): an (n_ch, n_ch) symmetric matrix in [0, 1] with ones on the diagonal, the phases those of
    scipy.signal.hilbert of the window itself.  Not recorded by utils.batch(): it launches at once.  ValueError for samples
    that are not finite; TdaError for more than PLV_MAX_CHANNELS channels or PLV_MAX_SAMPLES samples."""
    _, plv, st = engine.plv_dist_batch(_plv_window(window)[None])
    if st.any():
        raise ValueError("compute_plv_matrix: the window has samples that are not finite")
    return plv[0]


def compute_plv_persistence(window, method="euclidean", max_dim=MAX_DIM, max_edge_length=MAX_EDGE_LENGTH):
    """[H0, H1] of the Rips complex on the phase-locking distance of a window's channels, in the format of
    compute_eeg_persistence: correlation_to_distance(compute_plv_matrix(window), method) through the Rips call of
    compute_eeg_persistence.  Not recorded by utils.batch(): it launches at once.  ValueError for an unknown method or
    samples that are not finite."""
    _check_dim(max_dim)
    dist, _, st = engine.plv_dist_batch(_plv_window(window)[None], method=method, want_plv=False)
    if st.any():
        raise ValueError("compute_plv_persistence: the window has samples that are not finite")
    h0, h1, rst = engine.rips_dm_batch(dist, thresh=max_edge_length, symmetrise=True, h1_cap=_h1_cap(dist.shape[1]))
    _check_status(rst[0])
    return [h0[0], h1[0]]


def compute_connectivity_matrix(window, measure):
    """An analytic-signal connectivity of every pair of channels of a window (n_ch, n_t) (include/tdaeeg.h, "Analytic-signal
    connectivity"): measure "wpli" (weighted phase-lag index, Vinck et al. 2011), "imcoh" (imaginary part of coherency,
    Nolte et al. 2004), "coh" (coherence) or "aec" (correlation of the amplitude envelopes): an (n_ch, n_ch) symmetric
    matrix with ones on the diagonal, the analytic signal that of scipy.signal.hilbert of the window itself.  Not recorded
    by utils.batch(): it launches at once.  ValueError for an unknown measure or samples that are not finite; TdaError for
    more than PLV_MAX_CHANNELS channels or PLV_MAX_SAMPLES samples."""
    _, value, st = engine.connectivity_dist_batch(_plv_window(window)[None], measure=measure)
    if st.any():
        raise ValueError("compute_connectivity_matrix: the window has samples that are not finite")
    return value[0]


def compute_connectivity_persistence(window, measure, method="euclidean", max_dim=MAX_DIM, max_edge_length=MAX_EDGE_LENGTH):
    """[H0, H1] of the Rips complex on the distance of a window's channels under an analytic-signal connectivity, the twin
    of compute_plv_persistence: correlation_to_distance(compute_connectivity_matrix(window, measure), method) through the
    Rips call of compute_eeg_persistence.  Not recorded by utils.batch(): it launches at once.  ValueError for an unknown
    measure or method or samples that are not finite."""
    _check_dim(max_dim)
    dist, _, st = engine.connectivity_dist_batch(_plv_window(window)[None], measure=measure, method=method, want_value=False)
    if st.any():
        raise ValueError("compute_connectivity_persistence: the window has samples that are not finite")
    h0, h1, rst = engine.rips_dm_batch(dist, thresh=max_edge_length, symmetrise=True, h1_cap=_h1_cap(dist.shape[1]))
    _check_status(rst[0])
    return [h0[0], h1[0]]


def _h1_cap(n):
    return max(256, n * (n - 1) // 2 - (n - 1)) if n <= 64 else 1024


def _check_status(st):
    if st & 2:
        raise TdaError("H1 class overflow left after the full ladder (cannot happen for <= 128 points)")
    if st & 1:
        raise TdaError("H1 diagram truncated; call engine.rips_dm_batch with a larger h1_cap")
    if st & 16:
        raise TdaError("more than 128 points: not supported by the LDS-resident kernels")


def extract_features(diagram):
    """scripts/utils.py:144-177 -- the 11 scalar features of one diagram (features_kernel)."""
    if _ACTIVE is not None:
        return _ACTIVE.add_features(diagram)
    rows, cnt = engine.pack_diagrams([np.asarray(diagram, dtype=np.float64)])
    f = engine.features_batch(rows, cnt)[0]
    out = {k: float(v) for k, v in zip(FEATURE_KEYS, f)}
    out["n_features"] = int(f[0])
    out["n_essential"] = int(f[1])
    return out


def safe_wasserstein(dgm1, dgm2):
    """scripts/utils.py:180-191 -- persim.wasserstein on cleaned diagrams; NaN on any failure."""
    if _ACTIVE is not None:
        return _ACTIVE.add_pair(dgm1, dgm2)
    try:
        d1, d2 = np.asarray(dgm1), np.asarray(dgm2)
        ra, ca = engine.pack_diagrams([d1 if d1.ndim == 2 else np.zeros((0, 2))])
        rb, cb = engine.pack_diagrams([d2 if d2.ndim == 2 else np.zeros((0, 2))])
        out, st = engine.wasserstein_batch(ra, ca, rb, cb, want_status=True)
        return float(out[0]) if st[0] == 0 else np.nan
    except Exception:
        return np.nan


def _clean_pair_diagram(d):
    """What safe_wasserstein hands to the solver: the diagram, or nothing for one that is not 2-D (utils.py:182-187; the
    kernel drops the non-finite rows and substitutes {(0, 0)}).  Raises for anything that is not a (k, 2) table."""
    d = np.asarray(d, dtype=np.float64)
    if d.ndim != 2 or d.size == 0:
        return np.zeros((0, 2))
    if d.shape[1] != 2:
        raise ValueError("a persistence diagram has two columns")
    return d


def safe_bottleneck(dgm1, dgm2):
    """Bottleneck distance of two diagrams cleaned as safe_wasserstein cleans them (include/tdaeeg.h: L-infinity ground
    cost, (d - b) / 2 to the diagonal, the largest matched cost of the best matching); NaN on any failure."""
    if _ACTIVE is not None:
        return _ACTIVE.add_bottleneck(dgm1, dgm2)
    try:
        ra, ca = engine.pack_diagrams([_clean_pair_diagram(dgm1)])
        rb, cb = engine.pack_diagrams([_clean_pair_diagram(dgm2)])
        out, st = engine.bottleneck_batch(ra, ca, rb, cb, want_status=True)
        return float(out[0]) if st[0] == 0 else np.nan
    except Exception:
        return np.nan


def safe_wasserstein_q(dgm1, dgm2, order=2, ground="l2"):
    """Wasserstein distance of order 1 or 2 of two diagrams cleaned as safe_wasserstein cleans them, with the "l2"
    ((d - b) / sqrt 2 to the diagonal) or the "linf" ((d - b) / 2) ground metric (include/tdaeeg.h); NaN on any failure."""
    if _ACTIVE is not None:
        return _ACTIVE.add_wasserstein_q(dgm1, dgm2, order, ground)
    try:
        ra, ca = engine.pack_diagrams([_clean_pair_diagram(dgm1)])
        rb, cb = engine.pack_diagrams([_clean_pair_diagram(dgm2)])
        out, st = engine.wasserstein_q_batch(ra, ca, rb, cb, order=order, ground=ground, want_status=True)
        return float(out[0]) if st[0] == 0 else np.nan
    except Exception:
        return np.nan


def default_landscape_grid(n=64):
    """The grid the landscape functions use when none is given: n points over the filtration, 0 .. MAX_EDGE_LENGTH."""
    return np.linspace(0.0, MAX_EDGE_LENGTH, n)


def _landscape_args(diagram, grid):
    """The diagram as a (k, 2) float64 table (a queued one stays queued) and the grid as a 1-D float64 array."""
    if not isinstance(diagram, _Deferred):
        diagram = np.asarray(diagram, dtype=np.float64)
        if diagram.ndim != 2 or diagram.shape[1] != 2:
            raise ValueError("a persistence diagram is a (k, 2) table")
    grid = default_landscape_grid() if grid is None else np.ascontiguousarray(grid, dtype=np.float64)
    if grid.ndim != 1:
        raise ValueError("the grid is a 1-D array")
    return diagram, grid


def _landscape_one(diagram, grid, levels):
    if diagram.shape[0]:
        rows, cnt = diagram[None], np.array([diagram.shape[0]], np.int32)
    else:
        rows, cnt = np.zeros((1, 1, 2)), np.zeros(1, np.int32)
    return engine.landscape_batch(rows, cnt, grid, levels)[0]


def persistence_landscape(diagram, grid=None, levels=5):
    """The persistence landscape of one diagram on a grid (include/tdaeeg.h): (levels, n_grid) float64, level k the k-th
    largest of the tents min(t - b, d - t) of the finite rows, 0 where there are fewer.  grid: default_landscape_grid().
    Not in the reference; ValueError for a diagram that is not a (k, 2) table."""
    diagram, grid = _landscape_args(diagram, grid)
    if _ACTIVE is not None:
        return _ACTIVE.add_landscape(diagram, grid, int(levels), False)
    return _landscape_one(diagram, grid, levels)[:-1]


def betti_curve(diagram, grid=None):
    """The Betti curve of one diagram on a grid (include/tdaeeg.h): (n_grid,) float64, the number of rows with
    b <= t < d (rows that never die count).  ValueError for a diagram that is not a (k, 2) table."""
    diagram, grid = _landscape_args(diagram, grid)
    if _ACTIVE is not None:
        return _ACTIVE.add_landscape(diagram, grid, 1, True)
    return _landscape_one(diagram, grid, 1)[-1]


def default_image_edges(n_x=20, n_y=20, birth_range=(0.0, MAX_EDGE_LENGTH), pers_range=(0.0, MAX_EDGE_LENGTH)):
    """(xe, ye): n_x + 1 evenly spaced birth edges over birth_range and n_y + 1 persistence edges over pers_range; by
    default both span the filtration, 0 .. MAX_EDGE_LENGTH."""
    return (np.linspace(float(birth_range[0]), float(birth_range[1]), int(n_x) + 1),
            np.linspace(float(pers_range[0]), float(pers_range[1]), int(n_y) + 1))


def persistence_image(dgm, xe, ye, sigma, power=1):
    """The persistence image of one diagram (include/tdaeeg.h): (n_y, n_x) float64, row r the persistence axis; every
    finite row (b, d) is a normal density of width sigma at (b, d - b), weighted by (d - b) ** power and integrated over
    the pixels between the birth edges xe (n_x + 1) and the persistence edges ye (n_y + 1).  Not in the reference.
    ValueError, before any GPU call, for a diagram that is not a (k, 2) table, for edges that are not finite and strictly
    ascending (or more than MAX_IMAGE_SIDE pixels a side), for a sigma that is not finite and > 0 and for a power outside
    {0, 1, 2}."""
    if not isinstance(dgm, _Deferred):
        dgm = np.asarray(dgm, dtype=np.float64)
        if dgm.ndim != 2 or dgm.shape[1] != 2:
            raise ValueError("a persistence diagram is a (k, 2) table")
    xe, ye, sigma, power = engine.image_args(xe, ye, sigma, power)
    if _ACTIVE is not None:
        return _ACTIVE.add_image(dgm, xe, ye, sigma, power)
    if dgm.shape[0]:
        rows, cnt = dgm[None], np.array([dgm.shape[0]], np.int32)
    else:
        rows, cnt = np.zeros((1, 1, 2)), np.zeros(1, np.int32)
    return engine.image_batch(rows, cnt, xe, ye, sigma, power)[0]


def frechet_mean(dgms, max_iter=32):
    """The Frechet mean of a group of diagrams in the order-2 Wasserstein metric with the L2 ground metric
    (include/tdaeeg.h: the algorithm of Turner et al. 2014, started at the first diagram) and the group's Frechet variance
    around it: (mean (k, 2) float64, variance, iterations, converged).  Rows with a non-finite entry do not count.  At
    most 64 diagrams of at most FM_MAX_POINTS finite rows each; converged is False when max_iter (1..FM_MAX_ITER)
    iterations did not reach a fixed point -- the mean is then the last iterate, with its own variance.  An empty group
    gives ((0, 2), NaN, 0, True).  Runs at once, also inside a `batch`.  Not in the reference; ValueError for a diagram that
    is not a (k, 2) table, TdaError for a group the kernel has no room for."""
    tabs = []
    for d in dgms:
        d = np.asarray(d, dtype=np.float64)
        if d.ndim != 2 or d.shape[1] != 2:
            if d.size:
                raise ValueError("a persistence diagram is a (k, 2) table")
            d = np.zeros((0, 2))
        tabs.append(d)
    cap = max([len(d) for d in tabs] + [1])
    rows = np.zeros((max(len(tabs), 1), cap, 2)); cnt = np.zeros(max(len(tabs), 1), np.int32)
    for i, d in enumerate(tabs):
        rows[i, :len(d)] = d
        cnt[i] = len(d)
    mean, mc, var, it, st = engine.frechet_mean_batch(rows, cnt, seg_off=np.array([0, len(tabs)], np.int32), max_iter=max_iter)
    if st[0] & ~engine._lib.TDA_WIN_NOT_CONVERGED:
        raise TdaError(f"frechet_mean: status {int(st[0]):#x} (more than 64 diagrams, more than {engine._lib.FM_MAX_POINTS} points "
                            "in a diagram or in the mean, or a solver bound)")
    return mean[0, :mc[0]].copy(), float(var[0]), int(it[0]), not st[0] & engine._lib.TDA_WIN_NOT_CONVERGED


def default_directions(M=50):
    """(M, 2) float64 table (cos theta_k, sin theta_k), theta_k = -pi/2 + k * pi / M: the directions of
    persim.sliced_wasserstein, computed by numpy on the host (the kernel never evaluates a trigonometric function)."""
    M = int(M)
    if M < 1:
        raise ValueError("M must be >= 1")
    theta = -np.pi / 2 + np.arange(M) * np.pi / M
    return np.stack([np.cos(theta), np.sin(theta)], axis=1)


def sliced_wasserstein_kernel(d, sigma=1.0):
    """exp(-d / (2 * sigma**2)) of a sliced Wasserstein distance or Gram matrix d (engine.sliced_wasserstein_gram): the
    positive-definite kernel on diagrams of Carriere, Cuturi and Oudot (2017), for SVMs and kernel PCA.  Plain numpy."""
    return np.exp(-np.asarray(d, dtype=np.float64) / (2.0 * float(sigma) ** 2))


def safe_sliced_wasserstein(dgm1, dgm2, dirs=None, M=50):
    """Sliced Wasserstein distance of two diagrams cleaned as safe_wasserstein cleans them (include/tdaeeg.h) over the
    (M, 2) direction table dirs; dirs=None means default_directions(M).  NaN on any failure."""
    if _ACTIVE is not None:
        return _ACTIVE.add_sliced(dgm1, dgm2, dirs, M)
    try:
        d = default_directions(M) if dirs is None else dirs
        ra, ca = engine.pack_diagrams([_clean_pair_diagram(dgm1)])
        rb, cb = engine.pack_diagrams([_clean_pair_diagram(dgm2)])
        out, st = engine.sliced_wasserstein_batch(ra, ca, rb, cb, d, want_status=True)
        return float(out[0]) if st[0] == 0 else np.nan
    except Exception:
        return np.nan


def diagram_kernel(dgm1, dgm2, kernel=("pss", 0.1)):
    """The value of a kernel on diagrams for two diagrams (include/tdaeeg.h): kernel = ("pss", sigma), the persistence
    scale-space kernel of Reininghaus et al. (2015), or ("pwg", sigma, c), the persistence weighted Gaussian kernel of
    Kusano et al. (2016) with weight atan(c * persistence).  Rows with a non-finite entry do not count; an empty diagram is
    the zero measure and gives 0.0.  Runs at once, also inside a `batch`.  Not in the reference; TdaError for a bad kernel,
    ValueError for a diagram that is not a (k, 2) table."""
    par = engine.diagram_kernel_args(kernel)
    ra, ca = engine.pack_diagrams([_clean_pair_diagram(dgm1)])
    rb, cb = engine.pack_diagrams([_clean_pair_diagram(dgm2)])
    _, kv = engine.diagram_kernel_batch(ra, ca, rb, cb, par)
    return float(kv[0, 0])


def kernel_distance(dgm1, dgm2, kernel=("pss", 0.1)):
    """The distance a kernel on diagrams induces, sqrt(k(A, A) + k(B, B) - 2 k(A, B)) (include/tdaeeg.h), for the kernels
    of diagram_kernel.  It needs no matching.  NaN on any failure, as safe_wasserstein."""
    if _ACTIVE is not None:
        return _ACTIVE.add_kernel_distance(dgm1, dgm2, kernel)
    try:
        ra, ca = engine.pack_diagrams([_clean_pair_diagram(dgm1)])
        rb, cb = engine.pack_diagrams([_clean_pair_diagram(dgm2)])
        out, _, st = engine.diagram_kernel_batch(ra, ca, rb, cb, engine.diagram_kernel_args(kernel), want_status=True)
        return float(out[0]) if st[0] == 0 else np.nan
    except Exception:
        return np.nan


def diagram_kernel_gram(dgms, kernel=("pss", 0.1)):
    """(n, n) Gram matrix of a kernel on diagrams over a list of diagrams, symmetric as bytes, ready for
    SVC(kernel="precomputed") or kernel PCA.  TdaError for a bad kernel, ValueError for a diagram that is not a (k, 2)
    table."""
    par = engine.diagram_kernel_args(kernel)
    tabs = [_clean_pair_diagram(d) for d in dgms]
    if not tabs:
        return np.zeros((0, 0))
    rows, cnt = engine.pack_diagrams(tabs)
    return engine.diagram_kernel_gram(rows, cnt, par)


def persistence_fisher_distance(dgm1, dgm2, sigma=1.0):
    """The persistence Fisher distance of Le and Yamada (2018) between two diagrams (include/tdaeeg.h): both diagrams,
    each with the other's diagonal images, smoothed by Gaussians of width sigma into two probability vectors on the
    points of both, and the Fisher information metric (the angle between their square roots) between them.  In
    [0, pi / 2], exactly 0.0 for a diagram against itself; rows with a non-finite entry do not count.  It needs no
    matching.  NaN on any failure (a bad sigma, more than PF_MAX_POINTS finite rows in all), as kernel_distance."""
    if _ACTIVE is not None:
        return _ACTIVE.add_fisher_distance(dgm1, dgm2, sigma)
    try:
        ra, ca = engine.pack_diagrams([_clean_pair_diagram(dgm1)])
        rb, cb = engine.pack_diagrams([_clean_pair_diagram(dgm2)])
        out, st = engine.persistence_fisher_batch(ra, ca, rb, cb, sigma, want_status=True)
        return float(out[0]) if st[0] == 0 else np.nan
    except Exception:
        return np.nan


def persistence_fisher_kernel(dgm1, dgm2, sigma=1.0, t=1.0):
    """The persistence Fisher kernel exp(-t * persistence_fisher_distance(dgm1, dgm2, sigma)); NaN where the distance is."""
    return np.exp(-t * float(persistence_fisher_distance(dgm1, dgm2, sigma)))


def persistence_fisher_distances(dgms, sigma=1.0):
    """(n, n) matrix of the persistence Fisher distances over a list of diagrams, symmetric as bytes, its diagonal 0.0;
    NaN where a pair has more than PF_MAX_POINTS finite rows in all.  (0, 0) for an empty list.  TdaError for a bad sigma,
    ValueError for a diagram that is not a (k, 2) table."""
    engine.fisher_args(sigma)
    tabs = [_clean_pair_diagram(d) for d in dgms]
    if not tabs:
        return np.zeros((0, 0))
    rows, cnt = engine.pack_diagrams(tabs)
    return engine.persistence_fisher_gram(rows, cnt, sigma)


def persistence_fisher_gram(dgms, sigma=1.0, t=1.0):
    """(n, n) Gram matrix exp(-t * D) of the persistence Fisher kernel over a list of diagrams, D as
    persistence_fisher_distances gives it: symmetric as bytes, ready for SVC(kernel="precomputed")."""
    return np.exp(-t * persistence_fisher_distances(dgms, sigma))


# --------------------------------------------------------------------------------------------
# two-sample permutation test on distance / Gram matrices between recordings
# --------------------------------------------------------------------------------------------
def permute_labels_by_subject(y, subjects, rng):
    """scripts/utils.py:198-215: one draw of a subject-level relabelling.  Every subject carries the label of its first
    recording; rng.permutation shuffles those labels over the sorted unique subjects, and every recording takes its
    subject's new label.  One call of rng.permutation per draw, on an array of one label per subject in np.unique order, so
    the stream of a Generator is consumed exactly as by the reference's function."""
    y = np.asarray(y)
    _, first, inverse = np.unique(np.asarray(subjects), return_index=True, return_inverse=True)
    return rng.permutation(y[first])[inverse.reshape(-1)].astype(y.dtype, copy=False)


def subject_permutations(y, subjects=None, n_permutations=10000, seed=42):
    """(n_permutations + 1, n) uint8 labellings for two_sample_permutation_test: row 0 is y, row k the k-th draw of
    permute_labels_by_subject(y, subjects, rng) from ONE rng = default_rng(seed) (rng.permutation(y) when subjects is
    None).  y must hold 0 / 1."""
    y = np.asarray(y)
    assert y.ndim == 1 and ((y == 0) | (y == 1)).all(), "y must be a vector of 0 / 1 labels"
    rng = np.random.default_rng(seed)
    out = np.empty((int(n_permutations) + 1, y.shape[0]), np.uint8)
    out[0] = y
    if subjects is None:
        for k in range(1, out.shape[0]):
            out[k] = rng.permutation(y)
        return out
    _, first, inverse = np.unique(np.asarray(subjects), return_index=True, return_inverse=True)
    per_subject, inverse = y[first], inverse.reshape(-1)
    for k in range(1, out.shape[0]):
        out[k] = rng.permutation(per_subject)[inverse]
    return out


TWO_SAMPLE_STATISTICS = {"joint_loss": -1, "energy": 1, "mmd": 1}      # the side of the null that counts as extreme


def two_sample_statistic(sums, n1, n, statistic):
    """The statistic of a two-sample test from the sums of engine.permutation_sums_batch: sums (..., 3, P) = S00, S11, S01,
    n1 (P,) the items labelled 1, n the items in all; returns (..., P).  With n0 = n - n1, a = S00 / (n0 (n0 - 1)),
    b = S11 / (n1 (n1 - 1)), c = S01 / (n0 n1), each one float64 division by an exact integer product:
      "joint_loss"  a + b            the joint loss of Robinson and Turner (2017), half the mean within-group distance of
                                     each group, added; SMALL means separated
      "mmd"         (2a + 2b) - 2c   the unbiased MMD^2 of a Gram matrix; LARGE means separated
      "energy"      2c - (2a + 2b)   the energy distance of a distance matrix, the negative of "mmd" as bytes; LARGE means
                                     separated
    A relabelling with a group of fewer than 2 items gives NaN.  a + b is symmetric in the two groups, so a labelling and
    its complement give the same bytes."""
    if statistic not in TWO_SAMPLE_STATISTICS:
        raise ValueError(f"Unknown statistic: {statistic!r}")
    s = np.asarray(sums, dtype=np.float64)
    n1 = np.asarray(n1).astype(np.int64)
    n0 = int(n) - n1
    ok = (n0 >= 2) & (n1 >= 2)
    d0 = np.where(ok, n0 * (n0 - 1), 1).astype(np.float64)
    d1 = np.where(ok, n1 * (n1 - 1), 1).astype(np.float64)
    d01 = np.where(ok, n0 * n1, 1).astype(np.float64)
    a, b, c = s[..., 0, :] / d0, s[..., 1, :] / d1, s[..., 2, :] / d01
    with np.errstate(invalid="ignore"):
        if statistic == "joint_loss":
            t = a + b
        elif statistic == "mmd":
            t = (2.0 * a + 2.0 * b) - 2.0 * c
        else:
            t = 2.0 * c - (2.0 * a + 2.0 * b)
    return np.where(ok, t, np.nan)


def permutation_p_values(stat, finite, statistic):
    """p and p_family of two_sample_permutation_test from stat (n_mat, P + 1), column 0 the observed labelling, and finite
    (n_mat,) bool (see there)."""
    sign = TWO_SAMPLE_STATISTICS[statistic]
    n_mat, cols = stat.shape
    with np.errstate(invalid="ignore", divide="ignore"):
        e = sign * stat                                                    # large = extreme (exact: a sign flip)
        p = (1 + (e[:, 1:] >= e[:, :1]).sum(axis=1)) / cols
        p = np.where(finite & ~np.isnan(stat[:, 0]), p, np.nan)
        # (row by row: the mean and standard deviation of a matrix are those of its own contiguous vector of null values)
        null = [np.ascontiguousarray(e[m, 1:]) for m in range(n_mat)]
        mu = np.array([v.mean() if cols > 1 else np.nan for v in null]).reshape(n_mat, 1)
        sd = np.array([v.std() if cols > 1 else np.nan for v in null]).reshape(n_mat, 1)
        z = (e - mu) / sd
        use = finite & np.isfinite(mu[:, 0]) & (sd[:, 0] > 0)
        zmax = np.full(cols, -np.inf)
        for m in np.flatnonzero(use):
            zmax = np.fmax(zmax, z[m])
        pf = np.array([(1 + (zmax[1:] >= z[m, 0]).sum()) / cols if use[m] and not np.isnan(z[m, 0]) else np.nan
                       for m in range(n_mat)], dtype=np.float64)
    return p, pf


def two_sample_permutation_test(D, y, subjects=None, n_permutations=10000, statistic="joint_loss", seed=42, labels=None,
                                ctx=None):
    """The two-sample permutation test of Robinson and Turner (2017) on distance matrices between diagrams (statistic
    "joint_loss", or "energy"), and its kernel twin on Gram matrices ("mmd"): is group y == 1 different from group y == 0?
    D: (n_mat, n, n) or one (n, n) matrix, a numpy array or a float64 torch tensor on the GPU (it stays there); only its
    upper triangle is read.  The relabellings are subject_permutations(y, subjects, n_permutations, seed), or `labels`
    ((n_permutations + 1, n) of 0 / 1, row 0 the observed labelling) when given.  The sums of every (matrix, relabelling)
    come from ONE call of the HIP kernel (include/tdaeeg.h, "Two-sample permutation sums"), so every number below is a
    fixed function of the inputs.  Returns a dict:
      observed (n_mat,)            the statistic under y
      null (n_mat, n_permutations) under the relabellings
      p (n_mat,)                   (1 + #{k: null[m, k] at least as extreme as observed[m]}) / (n_permutations + 1); ties count
                                   as extreme, the convention of drivers.comparison_summary; a NaN null value (a relabelling
                                   with a group below 2 items) is never extreme
      p_family (n_mat,)            the max-statistic correction for testing the n_mat matrices at once.  With e = the
                                   statistic signed so that large is extreme, mu_m and sd_m the mean and the (population)
                                   standard deviation of matrix m's null values, z[m, k] = (e[m, k] - mu_m) / sd_m for the
                                   observed labelling (k = 0) and every relabelling, and zmax[k] = max over m of z[m, k]:
                                   p_family[m] = (1 + #{k >= 1: zmax[k] >= z[m, 0]}) / (n_permutations + 1).  Matrices with
                                   p = NaN, a NaN null value or sd_m = 0 take no part and get NaN.  For n_mat = 1 it is p (z is monotone in e).
      n1 (n_permutations + 1,)     items labelled 1 under every relabelling
    A matrix with a non-finite value in its upper triangle has p = p_family = NaN (its observed sums show it: every pair is
    in one of them)."""
    if statistic not in TWO_SAMPLE_STATISTICS:
        raise ValueError(f"Unknown statistic: {statistic!r}")
    lab = subject_permutations(y, subjects, n_permutations, seed) if labels is None else np.asarray(labels)
    assert lab.ndim == 2 and lab.shape[0] >= 1, "labels must be (n_permutations + 1, n)"
    n = lab.shape[1]
    if not getattr(D, "is_cuda", False):
        d = np.asarray(D, dtype=np.float64)
        sums, n1 = engine.permutation_sums_batch(d[None] if d.ndim == 2 else d, lab, ctx=ctx)
    else:
        import torch
        packed = torch.from_numpy(engine.pack_labels(lab).view(np.int64)).to(D.device)
        d = D if D.is_contiguous() else D.contiguous()
        out_t, n1_t = engine.permutation_sums_dev(d, packed, n_perm=lab.shape[0], ctx=ctx)
        sums, n1 = out_t.cpu().numpy(), n1_t.cpu().numpy()
    stat = two_sample_statistic(sums, n1, n, statistic)                   # (n_mat, P + 1)
    finite = np.isfinite(sums[:, :, 0]).all(axis=1)
    p, pf = permutation_p_values(stat, finite, statistic)
    return {"observed": stat[:, 0].copy(), "null": stat[:, 1:].copy(), "p": p, "p_family": pf, "n1": n1,
            "statistic": statistic}


# --------------------------------------------------------------------------------------------
# batch(): the reference's per-window loop, unchanged, at one launch per stage
# --------------------------------------------------------------------------------------------
class _Deferred:
    """A result that exists once its batch has been flushed; every use of the value flushes."""
    __slots__ = ("_batch", "_value")

    def __init__(self, batch):
        self._batch, self._value = batch, None

    def _get(self):
        if self._value is None:
            self._batch.flush()
        return self._value


class DeferredArray(_Deferred):
    """One persistence diagram, (k, 2) float64, of a queued compute_*_persistence call."""
    __slots__ = ()

    def __array__(self, dtype=None, copy=None):
        v = self._get()
        return v if dtype is None else v.astype(dtype)

    def __len__(self):
        return len(self._get())

    def __getitem__(self, i):
        return self._get()[i]

    def __iter__(self):
        return iter(self._get())

    @property
    def shape(self):
        return self._get().shape

    @property
    def ndim(self):
        return 2

    def __repr__(self):
        return repr(self._get())


class DeferredVector(DeferredArray):
    """The Betti curve, (n_grid,) float64, of a queued betti_curve call."""
    __slots__ = ()

    @property
    def ndim(self):
        return 1


class DeferredScalar(_Deferred):
    """The value of a queued safe_wasserstein, safe_bottleneck, safe_wasserstein_q or safe_sliced_wasserstein call."""
    __slots__ = ()

    def __float__(self):
        return float(self._get())

    def __array__(self, dtype=None, copy=None):
        return np.asarray(self._get(), dtype=dtype or np.float64)

    def __repr__(self):
        return repr(float(self))


class DeferredFeatures(_Deferred):
    """The dict of a queued extract_features call."""
    __slots__ = ()

    def __getitem__(self, k):
        return self._get()[k]

    def keys(self):
        return self._get().keys()

    def items(self):
        return self._get().items()

    def values(self):
        return self._get().values()

    def __iter__(self):
        return iter(self._get())

    def __len__(self):
        return len(self._get())

    def __repr__(self):
        return repr(self._get())


_ACTIVE = None


class batch:
    """``with utils.batch():`` around the reference's per-window loop (scripts/tda_eeg_audio_comparison.py:88-99,
    scripts/matched_vs_mismatched.py:57-63,87-95) -- the loop stays as it is; compute_audio_persistence,
    compute_eeg_persistence, safe_wasserstein, safe_bottleneck, safe_wasserstein_q, safe_sliced_wasserstein, kernel_distance, persistence_fisher_distance, extract_features, persistence_landscape, betti_curve and
    persistence_image
    queue their arguments and hand back deferred results,
    and on leaving the block (or at the first use of a value) everything queued runs as ONE launch per stage: the point
    clouds of all windows, the distance matrices of all windows, all Wasserstein pairs, all bottleneck pairs, all feature
    vectors, all landscapes and Betti curves of one grid, all images of one (xe, ye, sigma, power).  Values,
    error behaviour (NaN from safe_wasserstein, [[0, 0]] for degenerate clouds, ValueError for a non-square matrix) and
    result types after the block are those of the immediate calls."""

    def __init__(self):
        self.clouds, self.dms, self.pairs, self.feats, self.bpairs, self.lands = [], [], [], [], [], []
        self.imgs = []
        self.spairs = []              # safe_sliced_wasserstein: (dgm1, dgm2, direction table, deferred value)
        self.qpairs = []              # safe_wasserstein_q: (dgm1, dgm2, (order, ground), deferred value)
        self.kpairs = []              # kernel_distance: (dgm1, dgm2, kernel, deferred value)
        self.fpairs = []              # persistence_fisher_distance: (dgm1, dgm2, sigma, deferred value)

    def __enter__(self):
        global _ACTIVE
        if _ACTIVE is not None:
            raise RuntimeError("utils.batch() blocks do not nest")
        _ACTIVE = self
        return self

    def __exit__(self, et, ev, tb):
        global _ACTIVE
        _ACTIVE = None
        if et is None:
            self.flush()
        return False

    # ---- queueing (called by the module functions while the block is active)
    def add_cloud(self, pc, thresh):
        d = [DeferredArray(self), DeferredArray(self)]
        self.clouds.append((pc, float(thresh), d))
        return d

    def add_dm(self, dm, thresh):
        d = [DeferredArray(self), DeferredArray(self)]
        self.dms.append((dm, float(thresh), d))
        return d

    def add_pair(self, a, b):
        s = DeferredScalar(self)
        self.pairs.append((a, b, s))
        return s

    def add_bottleneck(self, a, b):
        s = DeferredScalar(self)
        self.bpairs.append((a, b, s))
        return s

    def add_wasserstein_q(self, a, b, order, ground):
        s = DeferredScalar(self)
        self.qpairs.append((a, b, (order, ground), s))
        return s

    def add_sliced(self, a, b, dirs, M):
        s = DeferredScalar(self)
        try:
            d = np.ascontiguousarray(default_directions(M) if dirs is None else dirs, dtype=np.float64)
        except Exception:
            d = None                                # a malformed table: NaN for this pair alone
        self.spairs.append((a, b, d, s))
        return s

    def add_kernel_distance(self, a, b, kernel):
        s = DeferredScalar(self)
        try:
            par = engine.diagram_kernel_args(kernel)
        except Exception:
            par = None                              # a bad kernel: NaN for this pair alone
        self.kpairs.append((a, b, par, s))
        return s

    def add_fisher_distance(self, a, b, sigma):
        s = DeferredScalar(self)
        try:
            engine.fisher_args(sigma)
            sigma = float(sigma)
        except Exception:
            sigma = None                            # a bad sigma: NaN for this pair alone
        self.fpairs.append((a, b, sigma, s))
        return s

    def add_features(self, dgm):
        f = DeferredFeatures(self)
        self.feats.append((dgm, f))
        return f

    def add_landscape(self, dgm, grid, levels, betti):
        if not 1 <= levels <= engine._lib.MAX_LANDSCAPES or not 1 <= grid.shape[0] <= engine._lib.MAX_GRID:
            raise TdaError("landscape levels must be 1..8 and the grid 1..256 points")
        d = DeferredVector(self) if betti else DeferredArray(self)
        self.lands.append((dgm, grid, levels, betti, d))
        return d

    def add_image(self, dgm, xe, ye, sigma, power):
        d = DeferredArray(self)
        self.imgs.append((dgm, (xe.tobytes(), ye.tobytes(), sigma, power), (xe, ye), d))
        return d

    @staticmethod
    def _resolve(x):
        return x._value if isinstance(x, _Deferred) else x

    def flush(self):
        clouds, dms, pairs, feats, bpairs, lands = self.clouds, self.dms, self.pairs, self.feats, self.bpairs, self.lands
        self.clouds, self.dms, self.pairs, self.feats, self.bpairs, self.lands = [], [], [], [], [], []
        imgs, self.imgs = self.imgs, []
        spairs, self.spairs = self.spairs, []
        qpairs, self.qpairs = self.qpairs, []
        kpairs, self.kpairs = self.kpairs, []
        fpairs, self.fpairs = self.fpairs, []
        # ---- stage 1: all Rips calls (one launch per kernel flavour, threshold and matrix size)
        for th in sorted({c[1] for c in clouds}):
            grp = [c for c in clouds if c[1] == th]
            p_cap, dim = max(len(c[0]) for c in grp), grp[0][0].shape[1]
            pcs = np.zeros((len(grp), p_cap, dim))
            for i, c in enumerate(grp):
                pcs[i, :len(c[0])] = c[0]
            h0, h1, st = engine.cloud_rips_batch(pcs, n_pts=[len(c[0]) for c in grp], thresh=th, h1_cap=_h1_cap(p_cap))
            for i, c in enumerate(grp):
                _check_status(st[i])
                c[2][0]._value, c[2][1]._value = h0[i], h1[i]
        for key in sorted({(d[0].shape[0], d[1]) for d in dms}):
            grp = [d for d in dms if (d[0].shape[0], d[1]) == key]
            h0, h1, st = engine.rips_dm_batch(np.stack([d[0] for d in grp]), thresh=key[1], symmetrise=True, h1_cap=_h1_cap(key[0]))
            for i, d in enumerate(grp):
                _check_status(st[i])
                d[2][0]._value, d[2][1]._value = h0[i], h1[i]
        # ---- stage 2: all Wasserstein pairs, all feature vectors
        if pairs:
            def clean(x):
                x = np.asarray(self._resolve(x))
                return x if x.ndim == 2 else np.zeros((0, 2))
            try:
                ra, ca = engine.pack_diagrams([clean(p[0]) for p in pairs])
                rb, cb = engine.pack_diagrams([clean(p[1]) for p in pairs])
                out, st = engine.wasserstein_batch(ra, ca, rb, cb, want_status=True)
                for i, p in enumerate(pairs):
                    p[2]._value = float(out[i]) if st[i] == 0 else np.nan
            except Exception:                       # utils.py:190-191: any failure -> NaN
                for p in pairs:
                    p[2]._value = np.nan
        if bpairs:
            # one launch for every well-formed pair; a malformed one is NaN by itself
            good = []
            for p in bpairs:
                p[2]._value = np.nan
                try:
                    good.append((_clean_pair_diagram(self._resolve(p[0])), _clean_pair_diagram(self._resolve(p[1])), p[2]))
                except Exception:
                    pass
            try:
                if good:
                    ra, ca = engine.pack_diagrams([g[0] for g in good])
                    rb, cb = engine.pack_diagrams([g[1] for g in good])
                    out, st = engine.bottleneck_batch(ra, ca, rb, cb, want_status=True)
                    for i, g in enumerate(good):
                        g[2]._value = float(out[i]) if st[i] == 0 else np.nan
            except Exception:
                pass
        if spairs:
            # one launch per direction table; a malformed pair or table is NaN by itself
            groups = {}
            for p in spairs:
                p[3]._value = np.nan
                try:
                    g = (_clean_pair_diagram(self._resolve(p[0])), _clean_pair_diagram(self._resolve(p[1])), p[3])
                    groups.setdefault((p[2].shape, p[2].tobytes()), (p[2], []))[1].append(g)
                except Exception:
                    pass
            for d, good in groups.values():
                try:
                    ra, ca = engine.pack_diagrams([g[0] for g in good])
                    rb, cb = engine.pack_diagrams([g[1] for g in good])
                    out, st = engine.sliced_wasserstein_batch(ra, ca, rb, cb, d, want_status=True)
                    for i, g in enumerate(good):
                        g[2]._value = float(out[i]) if st[i] == 0 else np.nan
                except Exception:
                    pass
        if qpairs:
            # one launch per (order, ground); a malformed pair or a bad (order, ground) is NaN by itself
            groups = {}
            for p in qpairs:
                p[3]._value = np.nan
                try:
                    g = (_clean_pair_diagram(self._resolve(p[0])), _clean_pair_diagram(self._resolve(p[1])), p[3])
                    groups.setdefault(p[2], []).append(g)
                except Exception:
                    pass
            for (order, ground), good in groups.items():
                try:
                    ra, ca = engine.pack_diagrams([g[0] for g in good])
                    rb, cb = engine.pack_diagrams([g[1] for g in good])
                    out, st = engine.wasserstein_q_batch(ra, ca, rb, cb, order=order, ground=ground, want_status=True)
                    for i, g in enumerate(good):
                        g[2]._value = float(out[i]) if st[i] == 0 else np.nan
                except Exception:
                    pass
        if kpairs:
            # one launch per kernel; a malformed pair or a bad kernel is NaN by itself
            groups = {}
            for p in kpairs:
                p[3]._value = np.nan
                try:
                    g = (_clean_pair_diagram(self._resolve(p[0])), _clean_pair_diagram(self._resolve(p[1])), p[3])
                    if p[2] is not None:
                        groups.setdefault(p[2], []).append(g)
                except Exception:
                    pass
            for par, good in groups.items():
                try:
                    ra, ca = engine.pack_diagrams([g[0] for g in good])
                    rb, cb = engine.pack_diagrams([g[1] for g in good])
                    out, _, st = engine.diagram_kernel_batch(ra, ca, rb, cb, par, want_status=True)
                    for i, g in enumerate(good):
                        g[2]._value = float(out[i]) if st[i] == 0 else np.nan
                except Exception:
                    pass
        if fpairs:
            # one launch per sigma; a malformed pair or a bad sigma is NaN by itself
            groups = {}
            for p in fpairs:
                p[3]._value = np.nan
                try:
                    g = (_clean_pair_diagram(self._resolve(p[0])), _clean_pair_diagram(self._resolve(p[1])), p[3])
                    if p[2] is not None:
                        groups.setdefault(p[2], []).append(g)
                except Exception:
                    pass
            for sigma, good in groups.items():
                try:
                    ra, ca = engine.pack_diagrams([g[0] for g in good])
                    rb, cb = engine.pack_diagrams([g[1] for g in good])
                    out, st = engine.persistence_fisher_batch(ra, ca, rb, cb, sigma, want_status=True)
                    for i, g in enumerate(good):
                        g[2]._value = float(out[i]) if st[i] == 0 else np.nan
                except Exception:
                    pass
        if feats:
            rows, cnt = engine.pack_diagrams([np.asarray(self._resolve(f[0]), dtype=np.float64) for f in feats])
            F = engine.features_batch(rows, cnt)
            for i, f in enumerate(feats):
                out = {k: float(v) for k, v in zip(FEATURE_KEYS, F[i])}
                out["n_features"] = int(F[i][0])
                out["n_essential"] = int(F[i][1])
                f[1]._value = out
        # ---- landscapes and Betti curves: one launch per distinct grid, at the most levels asked for on it (level k does
        # not depend on how many levels are computed; the Betti curve is the last row)
        for key in sorted({g[1].tobytes() for g in lands}):
            grp = [g for g in lands if g[1].tobytes() == key]
            dg = []
            for g in grp:
                d = np.asarray(self._resolve(g[0]), dtype=np.float64)
                if d.ndim != 2 or d.shape[1] != 2:
                    raise ValueError("a persistence diagram is a (k, 2) table")
                dg.append(d)
            rows, cnt = engine.pack_diagrams(dg)
            V = engine.landscape_batch(rows, cnt, grp[0][1], max(g[2] for g in grp))
            for i, g in enumerate(grp):
                g[4]._value = V[i, -1].copy() if g[3] else V[i, :g[2]].copy()
        # ---- persistence images: one launch per distinct (xe, ye, sigma, power)
        for key in sorted({g[1] for g in imgs}):
            grp = [g for g in imgs if g[1] == key]
            dg = []
            for g in grp:
                d = np.asarray(self._resolve(g[0]), dtype=np.float64)
                if d.ndim != 2 or d.shape[1] != 2:
                    raise ValueError("a persistence diagram is a (k, 2) table")
                dg.append(d)
            rows, cnt = engine.pack_diagrams(dg)
            V = engine.image_batch(rows, cnt, grp[0][2][0], grp[0][2][1], key[2], key[3])
            for i, g in enumerate(grp):
                g[3]._value = V[i].copy()
