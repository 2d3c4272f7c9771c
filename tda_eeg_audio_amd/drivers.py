"""
drivers.py -- batched counterparts of the reference's per-recording drivers, on the
reference's on-disk formats.

  select_windows_even / select_windows_md5   window selection, reproduced exactly (host side):
        np.linspace(0, n-1, 15, dtype=int)          scripts/tda_eeg_audio_comparison.py:77-80,
                                                    scripts/matched_vs_mismatched.py:52-55,77-80
        default_rng(md5(f"{dir}-{band}-{42}")[:8]).choice(n, size, replace=False)
                                                    scripts/tda_eeg_classification_v2.py:394-398
  process_file_features   scripts/tda_eeg_classification_v2.py:338-442  (220 features / recording)
  landscapes_from_distances / landscape_names
                          (not in the reference) mean persistence landscapes and Betti curves of the same groups
  images_from_distances / image_names
                          (not in the reference) mean persistence images of the same groups
  get_eeg_diagrams        scripts/matched_vs_mismatched.py:66-85
  get_audio_diagrams_from_windows / compute_cross_wasserstein   mvm:43-63, 87-95
  process_recording_arrays  scripts/tda_eeg_audio_comparison.py:63-122 given the band-passed audio windows
  process_recording / process_recording_file / run_analysis / detailed_rows
                            cmp:45-157 from the raw audio track (.mat) and the graphs/ tree to the rows of
                            results/eeg_audio_tda_detailed.csv
  validate_distance_matrix  scripts/tda_eeg_classification_v2.py:110-140 (first window of every band, v2:380-382)
  save_dataset              v2:670-688 incl. features/metadata.csv / metadata.json
  comparison_rows / comparison_summary / run_comparison
                            cmp:145-157 and cmp:161-220 from the rows and correlations of a batched pass
                            (recordings.*RecordingPass(correlations=True)): the detailed table and the per-band statistics
                            of results/eeg_audio_tda_comparison.json
  match_rows_host / match_mismatch_summary
                            the per-band statistics of the match-mismatch matrix (recordings.MatchMismatchPass)
  two_sample_from_diagrams  (not in the reference) the two-sample permutation test of Robinson and Turner between two groups
                            of recordings, on a sliced Wasserstein, persistence Fisher or kernel matrix of their diagrams
"""
import hashlib
from pathlib import Path

import numpy as np

from . import engine
from .utils import FEATURE_KEYS, FREQ_BANDS, MAX_EDGE_LENGTH, TAKENS_DIM, TAKENS_SUBSAMPLE

MAX_WINDOWS = 15            # cmp:39, mvm:32
BANDS = list(FREQ_BANDS)    # v2:63 order: delta, theta, alpha, beta, gamma


def select_windows_even(n_win, max_windows=MAX_WINDOWS):
    if n_win > max_windows:
        return np.linspace(0, n_win - 1, max_windows, dtype=int)
    return np.arange(n_win)


def select_windows_md5(dirname, band, n_windows, max_n, random_state=42):
    max_n = min(int(max_n), n_windows)
    seed = int(hashlib.md5(f"{dirname}-{band}-{random_state}".encode()).hexdigest()[:8], 16)
    return np.random.default_rng(seed).choice(n_windows, size=max_n, replace=False)


def check_status(st, what, allow_degenerate=False):
    """Raises on any window status the drivers cannot publish: class overflow beyond the widest pass (2), H1 rows
    cut at h1_cap (1), a cloud with more than TDA_MAX_POINTS points (16).  The reference has no such limits (ripser
    grows its columns on the heap), so silently passing a cut diagram on would be a different answer."""
    st = np.asarray(st)
    bad = st & (1 | 2 | 16)
    if not allow_degenerate:
        bad = bad | (st & 4)
    if bad.any():
        w = int(np.nonzero(bad)[0][0])
        raise RuntimeError(f"{what}: window {w} reported status {int(st[w])} "
                           "(1: H1 rows cut at h1_cap, 2: class capacity exceeded, 16: cloud too large)")


def validate_distance_matrix(distance_matrix, name=""):
    """scripts/tda_eeg_classification_v2.py:110-140 -- (is_valid, issues) with the reference's checks, order and
    messages: 2-D, square, symmetric (rtol 1e-5, atol 1e-8), no value below -1e-10, zero diagonal (atol 1e-10), no
    NaN, no Inf.  The reference runs it on the FIRST window of every band only (v2:380) and only logs the outcome
    into the recording's metadata (v2:381-382): a host-side check of one 47 x 47 matrix per recording-band.
    This function MIRRORS v2:110-140 by contract -- the same seven checks in the same order with the same tolerances and
    the same (Spanish) message strings, because the messages are an output format (they land in metadata.csv /
    metadata.json, v2:684-688) and are pinned by a fixture generated from the reference (tests/golden)."""
    distance_matrix = np.asarray(distance_matrix)
    issues = []
    if distance_matrix.ndim != 2:
        issues.append(f"No es 2D: forma={distance_matrix.shape}")
        return False, issues
    n, m = distance_matrix.shape
    if n != m:
        issues.append(f"No es cuadrada: forma=({n}, {m})")
        return False, issues
    if not np.allclose(distance_matrix, distance_matrix.T, rtol=1e-5, atol=1e-8):
        max_diff = np.max(np.abs(distance_matrix - distance_matrix.T))
        issues.append(f"No simétrica: asimetría máxima={max_diff:.6f}")
    if np.any(distance_matrix < -1e-10):
        issues.append(f"Valores negativos presentes: min={np.min(distance_matrix):.6f}")
    diag = np.diag(distance_matrix)
    if not np.allclose(diag, 0, atol=1e-10):
        issues.append(f"Diagonal no cero: max={np.max(np.abs(diag)):.6f}")
    if np.any(np.isnan(distance_matrix)):
        issues.append("Contiene valores NaN")
    if np.any(np.isinf(distance_matrix)):
        issues.append("Contiene valores Inf")
    return len(issues) == 0, issues


def feature_names(bands=BANDS):
    """Column order of features/feature_names.txt (v2:429-436)."""
    names = []
    for band in bands:
        for f in FEATURE_KEYS:
            names += [f"{band}_h0_{f}_mean", f"{band}_h0_{f}_std", f"{band}_h1_{f}_mean", f"{band}_h1_{f}_std"]
    return names


def _rips_of_groups(dist_list, thresh, what):
    """The shared opening of the *_from_distances family: the windows of every group through ONE Rips launch -- once more,
    large enough, where a window has more H1 rows than the default capacity -- and the status check.  Returns the raw
    diagrams (h0, c0, h1, c1) and the int32 segment table of the groups."""
    sizes = np.array([len(d) for d in dist_list])
    allw = np.concatenate([np.asarray(d, dtype=np.float64) for d in dist_list if len(d)], axis=0)
    h0, c0, h1, c1, st = engine.rips_dm_batch(allw, thresh=thresh, raw=True)
    if (st & 1).any():                         # more H1 rows than the default capacity: once more, large enough
        h0, c0, h1, c1, st = engine.rips_dm_batch(allw, thresh=thresh, raw=True, h1_cap=int(c1.max()))
    check_status(st, what)
    return h0, c0, h1, c1, np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)


def _upload_sets(h0, c0, h1, c1, seg):
    """(ctx, device, (rows_t, counts_t) of H0 and then of H1, seg_t): the segment table on the device, and the two diagram
    sets, each uploaded when the caller's loop comes to it."""
    import torch
    ctx = engine.get_ctx()
    dev = torch.device("cuda", ctx.device)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)      # noqa: E731
    return ctx, dev, ((up(rows), up(cnt)) for rows, cnt in ((h0, c0), (h1, c1))), up(seg)


def features_from_distances(dist_list, thresh=MAX_EDGE_LENGTH):
    """dist_list: list of (k_i, n, n) arrays, one per (recording, band) group, windows already
    selected.  One Rips launch + two feature launches + one aggregation launch for all groups.
    Returns (len(dist_list), 44) float64."""
    h0, c0, h1, c1, seg = _rips_of_groups(dist_list, thresh, "features_from_distances")
    return engine.aggregate_batch(engine.features_batch(h0, c0), engine.features_batch(h1, c1), seg)


def landscapes_from_distances(dist_list, grid, levels, thresh=MAX_EDGE_LENGTH):
    """dist_list as features_from_distances takes it.  The same Rips launch with the same status checks, then one launch
    per diagram set (H0, H1) that writes only the group means: (len(dist_list), 2, levels + 1, n_grid) float64, per group
    the mean persistence landscape (levels 1..levels) and the mean Betti curve (last row) over its windows on `grid`
    (include/tdaeeg.h; engine.landscape_mean_dev).  A group without a window is NaN."""
    import torch
    ctx, dev, sets, seg_t = _upload_sets(*_rips_of_groups(dist_list, thresh, "landscapes_from_distances"))
    grid_t = torch.from_numpy(np.ascontiguousarray(grid, dtype=np.float64)).to(dev)
    out = torch.empty((2, len(dist_list), int(levels) + 1, grid_t.numel()), dtype=torch.float64, device=dev)
    for s, (rows_t, cnt_t) in enumerate(sets):
        engine.landscape_mean_dev(rows_t, cnt_t, grid_t, levels, seg_off_t=seg_t, out_t=out[s], ctx=ctx)
    return out.permute(1, 0, 2, 3).cpu().numpy().copy()


def frechet_means_from_distances(dist_list, thresh=MAX_EDGE_LENGTH, max_iter=32):
    """dist_list as features_from_distances takes it.  The same Rips launch with the same status checks, then one launch
    per diagram set (H0, H1): per group the Frechet mean of its windows' diagrams in the order-2 Wasserstein metric and
    their Frechet variance around it (include/tdaeeg.h; engine.frechet_mean_dev).  Returns a list over the groups of
    {"h0": (mean (k, 2), variance, iterations, status), "h1": ...}; a group without a window has an empty mean and a NaN
    variance.  status is the group's word: TDA_WIN_NOT_CONVERGED keeps its mean, any other bit has none."""
    ctx, _, sets, seg_t = _upload_sets(*_rips_of_groups(dist_list, thresh, "frechet_means_from_distances"))
    out = [dict() for _ in dist_list]
    for name, (rows_t, cnt_t) in zip(("h0", "h1"), sets):
        res = engine.frechet_mean_dev(rows_t, cnt_t, seg_off_t=seg_t, max_iter=max_iter, ctx=ctx)
        mean, mc, var, it, fst = (t.cpu().numpy() for t in res)
        for g in range(len(dist_list)):
            out[g][name] = (mean[g, :mc[g]].copy(), float(var[g]), int(it[g]), int(fst[g]))
    return out


def diagram_kernel_gram_from_distances(dist_list, kernel=("pss", 0.1), thresh=MAX_EDGE_LENGTH):
    """dist_list as features_from_distances takes it, one group of window distance matrices per recording.  The same Rips
    launch with the same status checks, then one launch per diagram set (H0, H1): the (2, n_rec, n_rec) float64 Gram
    matrices of the kernel on diagrams `kernel` -- ("pss", sigma) or ("pwg", sigma, c), engine.diagram_kernel_args --
    between the recordings' mean embeddings (include/tdaeeg.h; engine.diagram_kernel_gram_dev): entry [g, h] is the average
    of the kernel over all pairs of a window of g and a window of h.  Symmetric as bytes, ready for
    SVC(kernel="precomputed"); the row and column of a recording without a window are NaN.  TdaError for a bad kernel."""
    import torch
    par = engine.diagram_kernel_args(kernel)
    ctx, dev, sets, seg_t = _upload_sets(*_rips_of_groups(dist_list, thresh, "diagram_kernel_gram_from_distances"))
    out = torch.empty((2, len(dist_list), len(dist_list)), dtype=torch.float64, device=dev)
    for s, (rows_t, cnt_t) in enumerate(sets):
        engine.diagram_kernel_gram_dev(rows_t, cnt_t, par, seg_off_a=seg_t, out_t=out[s], ctx=ctx)
    return out.cpu().numpy()


def landscape_names(bands=BANDS, levels=5, grid=None):
    """Column names of landscapes_from_distances(...)[r] of every band, flattened band by band: per band and diagram set
    (h0, h1) the levels 1..levels and then the Betti curve, each at every grid point in order."""
    n_grid = 64 if grid is None else len(grid)
    names = []
    for band in bands:
        for h in ("h0", "h1"):
            for lev in [f"landscape{k}" for k in range(1, int(levels) + 1)] + ["betti"]:
                names += [f"{band}_{h}_{lev}_t{j}" for j in range(n_grid)]
    return names


def euler_curves_from_distances(dist_list, grid, max_dim=3, thresh=MAX_EDGE_LENGTH):
    """dist_list as features_from_distances takes it.  No Rips launch: one launch counts the simplices of every window on
    `grid`, a second one writes the group means: (len(dist_list), max_dim + 2, n_grid) float64, per group the mean simplex
    counts f_0 .. f_max_dim and the mean Euler characteristic over its windows (include/tdaeeg.h; engine.euler_dm_dev).
    A group without a window is NaN.  ValueError for a bad grid or max_dim."""
    import torch
    grid, max_dim = engine.euler_args(grid, max_dim)
    ctx = engine.get_ctx()
    dev = torch.device("cuda", ctx.device)
    sizes = np.array([len(d) for d in dist_list])
    seg_t = torch.from_numpy(np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)).to(dev)
    grid_t = torch.from_numpy(grid).to(dev)
    if sizes.sum() == 0:
        counts_t = torch.empty((0, max_dim + 2, grid.shape[0]), dtype=torch.int32, device=dev)
        mean_t = engine.euler_mean_dev(counts_t, 0, max_dim, grid.shape[0], seg_off_t=seg_t, ctx=ctx)
    else:
        allw = np.concatenate([np.asarray(d, dtype=np.float64) for d in dist_list if len(d)], axis=0)
        _, _, mean_t = engine.euler_dm_dev(torch.from_numpy(np.ascontiguousarray(allw)).to(dev), grid_t, max_dim, thresh,
                                           seg_off_t=seg_t, ctx=ctx)
    return mean_t.cpu().numpy()


def euler_names(bands=BANDS, max_dim=3, grid=None):
    """Column names of euler_curves_from_distances(...)[r] of every band, flattened band by band: per band the counts
    f0 .. f<max_dim> and then chi, each at every grid point in order."""
    n_grid = 64 if grid is None else len(grid)
    return [f"{band}_{row}_t{j}" for band in bands for row in [f"f{k}" for k in range(int(max_dim) + 1)] + ["chi"]
            for j in range(n_grid)]


def _network_group_means(net):
    """(n_seg, NET_ROWS + NET_MEASURES, n_grid) float64 of a DeviceNetworkCurves with its means: counts, then measures."""
    import torch
    return torch.cat([net.mean_counts, net.mean_measures], dim=1).cpu().numpy()


def network_curves_from_distances(dist_list, grid, nodal=False, thresh=MAX_EDGE_LENGTH):
    """dist_list as features_from_distances takes it.  No Rips launch: one launch computes the graph measures of every
    window's thresholded graph on `grid` (include/tdaeeg.h, "Network curves"; engine.network_dm_dev), the next ones write
    the group means: (len(dist_list), NET_ROWS + NET_MEASURES, n_grid) float64, per group the mean over its windows of the
    integer rows (_lib.NET_COUNT_NAMES) and then of the float64 measures (_lib.NET_MEASURE_NAMES), the columns named by
    network_names.  nodal=True: (means, nodal_means), the second (len(dist_list), NET_NODAL, n_grid, n) float64 with the
    rows of _lib.NET_NODAL_NAMES.  A group without a window is NaN.  ValueError for a bad grid."""
    import torch
    from . import _lib
    grid = engine.network_args(grid)
    ctx = engine.get_ctx()
    dev = torch.device("cuda", ctx.device)
    sizes = np.array([len(d) for d in dist_list])
    seg_t = torch.from_numpy(np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)).to(dev)
    grid_t = torch.from_numpy(grid).to(dev)
    if sizes.sum() == 0:
        n = next((np.asarray(d).shape[-1] for d in dist_list if np.asarray(d).ndim == 3), 1)
        means = np.full((len(dist_list), _lib.NET_ROWS + _lib.NET_MEASURES, grid.shape[0]), np.nan)
        return (means, np.full((len(dist_list), _lib.NET_NODAL, grid.shape[0], n), np.nan)) if nodal else means
    allw = np.concatenate([np.asarray(d, dtype=np.float64) for d in dist_list if len(d)], axis=0)
    net = engine.network_dm_dev(torch.from_numpy(np.ascontiguousarray(allw)).to(dev), grid_t, nodal, thresh, seg_off_t=seg_t,
                                ctx=ctx)
    means = _network_group_means(net)
    return (means, net.mean_nodal.cpu().numpy()) if nodal else means


def network_names(bands=BANDS, grid=None):
    """Column names of network_curves_from_distances(...)[r] of every band, flattened band by band: per band the integer
    rows and then the measures, each at every grid point in order."""
    from . import _lib
    n_grid = 64 if grid is None else len(grid)
    return [f"{band}_{row}_t{j}" for band in bands for row in _lib.NET_COUNT_NAMES + _lib.NET_MEASURE_NAMES
            for j in range(n_grid)]


NETWORK_MEASURES = ("pearson", "plv") + tuple(engine.CONNECTIVITY_MEASURES)


def connectivity_network_curves_from_windows(win_list, measure, grid, method="euclidean"):
    """win_list: list of (k_i, n_ch, n_t) arrays of EEG windows, one per (recording, band) group.  Per group the mean over
    its windows of the network curves on `grid` of the graph on the distance of the window's channels under `measure`:
    "pearson" (engine.corr_dist_dev; method must be "euclidean"), "plv" (engine.plv_dist_dev) or one of
    engine.CONNECTIVITY_MEASURES (engine.connectivity_dist_dev).  (len(win_list), NET_ROWS + NET_MEASURES, n_grid) float64,
    counts then measures, as network_curves_from_distances.  All on the device: distances, curves, means.  A window the
    connectivity kernel flags (a sample that is not finite) is left out of its group's mean; a group without a kept window
    is NaN.  ValueError for an unknown measure or method or a bad grid."""
    import torch
    from . import _lib
    grid = engine.network_args(grid)
    if not isinstance(measure, str) or measure not in NETWORK_MEASURES:
        raise ValueError(f"connectivity: one of {sorted(NETWORK_MEASURES)}, not {measure!r}")
    if measure == "pearson":
        if method != "euclidean":
            raise ValueError("connectivity: the Pearson distance is euclidean")
    elif measure == "plv":
        engine.plv_method(method)
    else:
        engine._dist_method(method)
    sizes = np.array([len(w) for w in win_list])
    if sizes.sum() == 0:
        return np.full((len(win_list), _lib.NET_ROWS + _lib.NET_MEASURES, grid.shape[0]), np.nan)
    ctx = engine.get_ctx()
    dev = torch.device("cuda", ctx.device)
    seg_t = torch.from_numpy(np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)).to(dev)
    allw = np.concatenate([np.asarray(w, dtype=np.float64) for w in win_list if len(w)], axis=0)
    win_t = torch.from_numpy(np.ascontiguousarray(allw)).to(dev)
    st = None
    if measure == "pearson":
        dist = engine.corr_dist_dev(win_t, ctx=ctx)
    elif measure == "plv":
        dist, _, st = engine.plv_dist_dev(win_t, method=method, ctx=ctx)
    else:
        dist, _, st = engine.connectivity_dist_dev(win_t, measure=measure, method=method, ctx=ctx)
    net = engine.network_dm_dev(dist, torch.from_numpy(grid).to(dev), seg_off_t=seg_t, status_in=st,
                                skip_mask=0x7fffffff if st is not None else 0, ctx=ctx)
    return _network_group_means(net)


def recurrence_curves_from_windows(win_list, tau_list, grid, theiler=1, l_min=2, v_min=2, histograms=False, dim=TAKENS_DIM,
                                   subsample=TAKENS_SUBSAMPLE, thresh=MAX_EDGE_LENGTH):
    """win_list: list of (k_i, n_t) arrays of signal windows, one per (recording, band) group; tau_list: per group one
    delay (the reference's one tau per recording and band) or k_i delays, one per window.  Per group the mean over its
    windows of the recurrence curves on `grid` of the window's delay embedding (include/tdaeeg.h, "Recurrence curves";
    engine.recurrence_takens_dev): (len(win_list), RQA_ROWS + RQA_MEASURES, n_grid) float64, the integer rows
    (_lib.RQA_COUNT_NAMES) and then the measures (_lib.RQA_MEASURE_NAMES), the columns named by recurrence_names.
    histograms=True: (means, hist_means), the second (len(win_list), 2, n_grid, 128) float64, diagonal then vertical line
    lengths.  All on the device: embedding, keys, curves, means.  A window the kernel refuses (fewer than 3 or more than 128
    points, tau < 1) is left out of its group's mean, as the reference skips a cloud of fewer than 3 points; a group
    without a kept window is NaN.  ValueError for a bad grid, theiler, l_min, v_min or tau_list."""
    import torch
    from . import _lib
    grid, theiler, l_min, v_min = engine.recurrence_args(grid, theiler, l_min, v_min)
    if len(tau_list) != len(win_list):
        raise ValueError("tau_list: one entry per group")
    sizes = np.array([len(w) for w in win_list])
    taus = []
    for k, tau in zip(sizes, tau_list):
        tau = np.asarray(tau)
        if tau.ndim > 1 or (tau.ndim == 1 and tau.shape[0] != k) or not np.issubdtype(tau.dtype, np.integer):
            raise ValueError("tau_list: per group one integer delay or one per window")
        taus.append(np.broadcast_to(tau, (k,)).astype(np.int32))
    n_rows = _lib.RQA_ROWS + _lib.RQA_MEASURES
    if sizes.sum() == 0:
        means = np.full((len(win_list), n_rows, grid.shape[0]), np.nan)
        return (means, np.full((len(win_list), 2, grid.shape[0], _lib.MAX_POINTS), np.nan)) if histograms else means
    ctx = engine.get_ctx()
    dev = torch.device("cuda", ctx.device)
    seg_t = torch.from_numpy(np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)).to(dev)
    allw = np.concatenate([np.asarray(w, dtype=np.float64) for w in win_list if len(w)], axis=0)
    if allw.ndim != 2:
        raise ValueError("win_list: (k_i, n_t) arrays")
    rq = engine.recurrence_takens_dev(torch.from_numpy(np.ascontiguousarray(allw)).to(dev),
                                      torch.from_numpy(np.concatenate(taus)).to(dev), torch.from_numpy(grid).to(dev), theiler,
                                      l_min, v_min, histograms, dim, subsample, thresh, seg_off_t=seg_t, skip_mask=4 | 16,
                                      ctx=ctx)
    means = torch.cat([rq.mean_counts, rq.mean_measures], dim=1).cpu().numpy()
    return (means, rq.mean_hist.cpu().numpy()) if histograms else means


def recurrence_names(bands=BANDS, grid=None):
    """Column names of recurrence_curves_from_windows(...)[r] of every band, flattened band by band: per band the integer
    rows and then the measures, each at every grid point in order."""
    from . import _lib
    n_grid = 64 if grid is None else len(grid)
    return [f"{band}_{row}_t{j}" for band in bands for row in _lib.RQA_COUNT_NAMES + _lib.RQA_MEASURE_NAMES
            for j in range(n_grid)]


def embedding_parameters_from_windows(win_list, max_lag=None, n_bins=16, max_dim=5, theiler=None, r_tol=10.0, a_tol=2.0,
                                      frac_tol=0.05):
    """win_list: list of (k_i, n_t) arrays of signal windows, one per (recording, band) group.  Per group the two
    parameters of its delay embedding, chosen from the signal (include/tdaeeg.h, "Delay and dimension selection"), and the
    curves behind them: (len(win_list), 2 + n_lag + max_dim) float64 with n_lag = the resolved max_lag + 1, the columns
    named by embedding_names --
      tau_ami          the first minimum of the average mutual information of the group's FIRST window, as the reference
                       takes its one tau per recording and band, compute_tau's fallback without a minimum
                       (engine.ami_segments_dev); this delay feeds the false nearest neighbours of every window of the group
      dim_fnn          the smallest dimension d with V > 0 and (double)E <= frac_tol * (double)V, V and E the group's sums
                       of valid and false_either at d; 0 without one
      ami_L0 ...       the mean over the group's windows of their mutual information curves (engine.ami_dev)
      fnn_frac_d1 ...  the mean over the group's windows of their fractions of false neighbours (engine.fnn_dev)
    The means add the kept windows in window order and divide by their number; a window with a status word (a sample that
    is not finite, a constant window, too short for the delay) is left out, a group without a kept window is NaN.  theiler:
    None means every group's own delay.  All on the device: delays, curves, neighbours, sums.  ValueError for a bad
    argument."""
    import torch
    sizes = np.array([len(w) for w in win_list], dtype=np.int64)
    shapes = {np.shape(w)[1:] for w in win_list if len(w)}
    if len(shapes) > 1 or any(len(s) != 1 for s in shapes):
        raise ValueError("win_list: (k_i, n_t) arrays of one n_t")
    if theiler is not None and (isinstance(theiler, bool) or not isinstance(theiler, (int, np.integer))):
        raise ValueError(f"theiler must be an integer or None, not {theiler!r}")
    if not shapes:
        lag, _ = engine.ami_args(4, max_lag, n_bins)
        engine.fnn_args(4, max_dim, 1, r_tol, a_tol, frac_tol)
        if max_lag is None or max_lag < 0:
            raise ValueError("max_lag: without a window there is no length to take a quarter of")
        out = np.full((len(win_list), 2 + int(max_lag) + 1 + max_dim), np.nan)
        out[:, :2] = 0.0
        return out
    n_t = shapes.pop()[0]
    lag, n_bins = engine.ami_args(n_t, max_lag, n_bins)
    d_max = engine.fnn_args(n_t, max_dim, 1 if theiler is None else theiler, r_tol, a_tol, frac_tol)[0]
    ctx = engine.get_ctx()
    dev = torch.device("cuda", ctx.device)
    n, n_seg, k_max = int(sizes.sum()), len(win_list), int(sizes.max())
    seg = np.concatenate([[0], np.cumsum(sizes)])
    seg_t = torch.from_numpy(seg.astype(np.int32)).to(dev)
    W = torch.from_numpy(np.ascontiguousarray(np.concatenate([np.asarray(w, dtype=np.float64) for w in win_list if len(w)]))).to(dev)
    tau_seg = torch.empty(n_seg, dtype=torch.int32, device=dev)
    tau_win = torch.empty(n, dtype=torch.int32, device=dev)
    engine.ami_segments_dev(W, seg_t, lag, n_bins, tau_seg, tau_win, ctx=ctx)
    emb = engine.ami_dev(W, lag, n_bins, ctx=ctx)
    if theiler is not None:
        fnn = engine.fnn_dev(W, tau_win, d_max, theiler, r_tol, a_tol, frac_tol, ctx=ctx)
    else:
        # one launch per delay that occurs: the Theiler window is a parameter of the launch
        fnn = engine.DeviceEmbedding(n, 0, d_max, dev)
        for v in torch.unique(tau_win).tolist():
            idx = (tau_win == v).nonzero().flatten()
            part = engine.fnn_dev(W[idx].contiguous(), tau_win[idx].contiguous(), d_max, min(max(int(v), 1), n_t), r_tol, a_tol,
                                  frac_tol, ctx=ctx)
            for name in ("counts", "frac", "dim", "fnn_status"):
                getattr(fnn, name).index_copy_(0, idx, getattr(part, name))

    # window k of every group side by side, so that the sums run in window order
    pos = seg_t[:-1, None].long() + torch.arange(k_max, device=dev)[None, :]
    there = pos < seg_t[1:, None].long()
    pos = pos.clamp(max=n - 1)

    def group_mean(val, status):
        keep = there & (status[pos] == 0)
        S = torch.zeros((n_seg, val.shape[1]), dtype=torch.float64, device=dev)
        for k in range(k_max):
            S = S + torch.where(keep[:, k, None], val[pos[:, k]], torch.zeros((), dtype=torch.float64, device=dev))
        return S / keep.sum(1, dtype=torch.float64)[:, None]

    keep = (there & (fnn.fnn_status[pos] == 0))[:, :, None, None]
    tot = (fnn.counts[pos].long() * keep).sum(1)                                        # (n_seg, d_max, 4), exact
    V, E = tot[:, :, 0], tot[:, :, 3]
    ok = (V > 0) & (E.double() <= float(frac_tol) * V.double())
    dim = torch.where(ok.any(1), ok.int().argmax(1) + 1, torch.zeros((), dtype=torch.int64, device=dev))
    out = torch.cat([tau_seg.double()[:, None], dim.double()[:, None], group_mean(emb.ami, emb.ami_status),
                     group_mean(fnn.frac, fnn.fnn_status)], dim=1)
    return out.cpu().numpy()


def embedding_names(n_lag, max_dim=5, bands=BANDS):
    """Column names of embedding_parameters_from_windows(...)[r] of every band, flattened band by band."""
    return [f"{band}_{name}" for band in bands for name in
            ["tau_ami", "dim_fnn"] + [f"ami_L{k}" for k in range(n_lag)] + [f"fnn_frac_d{d}" for d in range(1, max_dim + 1)]]


def channel_participation_from_distances(dist_list, thresh=MAX_EDGE_LENGTH):
    """dist_list as features_from_distances takes it.  The same Rips launch with the same status checks, then one launch
    that finds the birth edge and a representative cycle of every H1 row and one that writes the group means
    (include/tdaeeg.h, "Generators and representative cycles"; engine.generators_dm_dev).  Returns (mean, flagged): mean
    (len(dist_list), n) float64, per group and channel the mean over its windows of the persistence carried by the loops
    that visit the channel (a group without a window is NaN), and flagged, the number of H1 rows that were left out because
    a tie or a short cycle buffer flagged them."""
    import torch
    if not sum(len(d) for d in dist_list):
        n = next((np.asarray(d).shape[-1] for d in dist_list if np.asarray(d).ndim == 3), 0)
        return np.full((len(dist_list), n), np.nan), 0
    h0, c0, h1, c1, seg = _rips_of_groups(dist_list, thresh, "channel_participation_from_distances")
    ctx = engine.get_ctx()
    dev = torch.device("cuda", ctx.device)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)      # noqa: E731
    allw = np.concatenate([np.asarray(d, dtype=np.float64) for d in dist_list if len(d)], axis=0)
    gen = engine.generators_dm_dev(up(allw), (None, None, up(h1), up(c1)), thresh, True, seg_off_t=up(seg), ctx=ctx)
    return gen.mean.cpu().numpy(), int((gen.h1_flag != 0).sum().item())


def participation_names(bands=BANDS, n_ch=47):
    """Column names of channel_participation_from_distances(...)[0][r] of every band, flattened band by band."""
    return [f"{band}_part_ch{c}" for band in bands for c in range(int(n_ch))]


def connectivity_features_from_windows(win_list, measure, method="euclidean"):
    """win_list: list of (k_i, n_ch, n_t) arrays of EEG windows, one per (recording, band) group.  Per group the np.nanmean
    over its windows of the 11 extract_features values of H0 and then of H1 of the Rips complex on the distance of the
    window's channels under the analytic-signal connectivity `measure` ("wpli", "imcoh", "coh" or "aec"; include/tdaeeg.h,
    engine.connectivity_dist_dev): (len(win_list), 22) float64, the columns named by connectivity_names.  All on the device,
    the way the phase-locking stage of the step does it: one launch for the distances, rips_dm_dev with the whole retry
    ladder (exact by itself, whatever the context's retry policy, which is put back), the finishing pass, the segment
    means.  A window the connectivity kernel flags (a sample that is not finite) is handed to Rips as points on a line and
    counts as NaN, as does a window with a Rips status; a group without a window is NaN.  ValueError for an unknown measure
    or method."""
    import torch
    from .utils import _h1_cap
    engine.connectivity_measure(measure)
    ctx = engine.get_ctx()
    dev = torch.device("cuda", ctx.device)
    sizes = np.array([len(w) for w in win_list])
    n_win = int(sizes.sum())
    seg_t = torch.from_numpy(np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)).to(dev)
    out = torch.full((len(win_list), 22), float("nan"), dtype=torch.float64, device=dev)
    if n_win == 0:
        engine._dist_method(method)
        return out.cpu().numpy()
    allw = np.concatenate([np.asarray(w, dtype=np.float64) for w in win_list if len(w)], axis=0)
    n_ch = allw.shape[1]
    dist, _, st = engine.connectivity_dist_dev(torch.from_numpy(np.ascontiguousarray(allw)).to(dev), measure=measure,
                                               method=method, ctx=ctx)
    bad = st != 0
    line = torch.from_numpy(np.abs(np.subtract.outer(np.arange(n_ch), np.arange(n_ch))) / n_ch).to(dev)
    dist = torch.where(bad[:, None, None], line, dist).contiguous()
    dgm = engine.DeviceDiagrams(n_win, n_ch, _h1_cap(n_ch), dev)
    policy = ctx.retry_policy
    ctx.set_retry_policy(ctx.RETRY_AUTO)
    try:
        engine.rips_dm_dev(dist, dgm, ctx=ctx)
    finally:
        ctx.set_retry_policy(policy)
    f0 = torch.empty((n_win, 11), dtype=torch.float64, device=dev)
    f1 = torch.empty((n_win, 11), dtype=torch.float64, device=dev)
    engine.diagram_finish_dev([(dgm.h0, dgm.c0, False, f0), (dgm.h1, dgm.c1, True, f1)], ctx=ctx)
    bad = bad | (dgm.status != 0)
    nan = torch.full((), float("nan"), dtype=torch.float64, device=dev)
    cols = torch.where(bad[:, None], nan, torch.cat([f0, f1], dim=1)).t().contiguous()
    for k in range(22):
        out[:, k].copy_(engine.segment_nanmean_dev(cols[k], seg_t, ctx=ctx))
    return out.cpu().numpy()


def connectivity_names(measure):
    """Column names of connectivity_features_from_windows(...)[g]: the features of H0, then of H1."""
    engine.connectivity_measure(measure)
    return [f"{measure}_{h}_{f}_mean" for h in ("h0", "h1") for f in FEATURE_KEYS]


def images_from_distances(dist_list, xe, ye, sigma, power=1, thresh=MAX_EDGE_LENGTH):
    """dist_list as features_from_distances takes it.  The same Rips launch with the same status checks, then one launch
    per diagram set (H0, H1) that writes only the group means: (len(dist_list), 2, n_y, n_x) float64, per group the mean
    persistence image over its windows on the birth edges xe and the persistence edges ye (include/tdaeeg.h;
    engine.image_mean_dev).  A group without a window is NaN.  ValueError for bad edges, sigma or power."""
    import torch
    xe, ye, sigma, power = engine.image_args(xe, ye, sigma, power)
    ctx, dev, sets, seg_t = _upload_sets(*_rips_of_groups(dist_list, thresh, "images_from_distances"))
    xe_t, ye_t = torch.from_numpy(xe).to(dev), torch.from_numpy(ye).to(dev)
    out = torch.empty((2, len(dist_list), ye.shape[0] - 1, xe.shape[0] - 1), dtype=torch.float64, device=dev)
    for s, (rows_t, cnt_t) in enumerate(sets):
        engine.image_mean_dev(rows_t, cnt_t, xe_t, ye_t, sigma, power, seg_off_t=seg_t, out_t=out[s], ctx=ctx)
    return out.permute(1, 0, 2, 3).cpu().numpy().copy()


def image_names(bands=BANDS, n_x=20, n_y=20):
    """Column names of images_from_distances(...)[r] of every band, flattened band by band: per band and diagram set
    (h0, h1) the pixels row by row, r the persistence index and c the birth index."""
    return [f"{band}_{h}_image_r{r}_c{c}" for band in bands for h in ("h0", "h1") for r in range(int(n_y)) for c in range(int(n_x))]


def process_file_features(file_dir, freq_bands=BANDS, max_dim=1, max_edge_length=MAX_EDGE_LENGTH,
                          max_windows_per_band=None, window_sampling="random", random_state=42):
    """v2:338-442 -- returns (features dict in reference key order, metadata)."""
    file_dir = Path(file_dir)
    metadata = {"n_windows": {}, "n_windows_used": {}, "validation_issues": [],
                "window_sampling": window_sampling, "max_windows_per_band": max_windows_per_band}
    groups, bands_present = [], []
    for band in freq_bands:
        dist_file = file_dir / f"{band}_distances.npy"
        if not dist_file.exists():
            metadata["n_windows"][band] = 0
            continue
        try:
            dms = np.load(dist_file)
        except Exception as e:
            metadata["validation_issues"].append(f"{band}: error de carga - {e}")
            continue
        n_windows = dms.shape[0]
        metadata["n_windows"][band] = n_windows
        if n_windows == 0:
            continue
        is_valid, issues = validate_distance_matrix(dms[0], f"{band}[0]")             # v2:380-382
        if not is_valid:
            metadata["validation_issues"].extend([f"{band}: {i}" for i in issues])
        if max_windows_per_band is None:
            use = np.arange(n_windows)
        else:
            max_n = max_windows_per_band.get(band, n_windows) if isinstance(max_windows_per_band, dict) \
                else int(max_windows_per_band)
            max_n = min(max_n, n_windows)
            use = select_windows_md5(file_dir.name, band, n_windows, max_n, random_state) \
                if window_sampling == "random" else np.arange(max_n)
        metadata["n_windows_used"][band] = len(use)
        groups.append(dms[use]); bands_present.append(band)
    file_features = {}
    if groups:
        agg = features_from_distances(groups, max_edge_length)
        for g, band in enumerate(bands_present):
            k = 0
            for f in FEATURE_KEYS:
                for tag in ("h0", "h1"):
                    for stat in ("mean", "std"):
                        file_features[f"{band}_{tag}_{f}_{stat}"] = agg[g, k]
                        k += 1
    metadata["n_windows_total"] = int(sum(metadata["n_windows"].values()))
    metadata["n_windows_used_total"] = int(sum(metadata["n_windows_used"].values()))
    return file_features, metadata


def get_eeg_diagrams(graph_dir, bands=BANDS):
    """mvm:66-85 -- {band: [[H0, H1] per selected window]} from <band>_distances.npy."""
    graph_dir = Path(graph_dir)
    if not graph_dir.exists():
        return None
    result = {}
    for bname in bands:
        dist_file = graph_dir / f"{bname}_distances.npy"
        if not dist_file.exists():
            continue
        dms = np.load(str(dist_file))
        if dms.shape[0] == 0:
            continue
        idx = select_windows_even(dms.shape[0])
        h0, h1, st = engine.rips_dm_batch(dms[idx])
        check_status(st, f"get_eeg_diagrams({bname})")
        result[bname] = [[a, b] for a, b in zip(h0, h1)]
    return result


def get_audio_diagrams_from_windows(audio_wins):
    """mvm:50-62 for one band: selected windows, tau from the first one, Takens + Rips; windows
    whose cloud has < 3 points are skipped (mvm:60)."""
    n_win = len(audio_wins)
    if n_win == 0:
        return []
    idx = select_windows_even(n_win)
    sel = np.asarray(audio_wins, dtype=np.float64)[idx]
    tau = int(engine.tau_batch(sel[:1], max_lag=sel.shape[1] // 2)[0])
    h0, h1, npts, st = engine.takens_rips_batch(sel, tau, TAKENS_DIM, TAKENS_SUBSAMPLE)
    check_status(st, "get_audio_diagrams", allow_degenerate=True)
    return [[a, b] for a, b, p in zip(h0, h1, npts) if p >= 3]


def compute_cross_wasserstein(eeg_dgms_band, audio_dgms_band):
    """mvm:87-95 -- nanmean of W(H1, H1) over windows paired by index."""
    n = min(len(eeg_dgms_band), len(audio_dgms_band))
    if n == 0:
        return np.nan
    ra, ca = engine.pack_diagrams([d[1] for d in eeg_dgms_band[:n]])
    rb, cb = engine.pack_diagrams([d[1] for d in audio_dgms_band[:n]])
    w, st = engine.wasserstein_batch(ra, ca, rb, cb, want_status=True)
    w = np.where(st == 0, w, np.nan)
    return float(engine.segment_nanmean(w, np.array([0, n], np.int32))[0])


def process_recording_arrays(audio_band_windows, eeg_dists_by_band):
    """cmp:63-122 for one recording.  audio_band_windows: {band: (n_a, 250) band-passed audio
    windows}; eeg_dists_by_band: {band: (n_e, 47, 47)}.  Returns {band: {...}} with the keys of
    the reference's per-band result (wasserstein_h0/h1, n_windows, tau) plus the per-window H1
    feature time series used by its Spearman step (cmp:104-115)."""
    out = {}
    for bname in BANDS:
        if bname not in audio_band_windows or bname not in eeg_dists_by_band:
            continue
        aw = np.asarray(audio_band_windows[bname], dtype=np.float64)
        ed = np.asarray(eeg_dists_by_band[bname], dtype=np.float64)
        n_win = min(len(aw), ed.shape[0])
        if n_win == 0:
            continue
        idx = select_windows_even(n_win)
        tau = int(engine.tau_batch(aw[idx[:1]], max_lag=aw.shape[1] // 2)[0])          # cmp:83
        a0, ac0, a1, ac1, npts, ast = engine.takens_rips_batch(aw[idx], tau, TAKENS_DIM, TAKENS_SUBSAMPLE, raw=True)
        check_status(ast, f"process_recording({bname}) audio", allow_degenerate=True)
        keep = npts >= 3                                                               # cmp:90-91
        if not keep.any():
            continue
        e0, ec0, e1, ec1, est = engine.rips_dm_batch(ed[idx], raw=True)
        check_status(est, f"process_recording({bname}) eeg")
        k = np.nonzero(keep)[0].astype(np.int32)
        w0, s0 = engine.wasserstein_batch(e0, ec0, a0, ac0, k, k, want_status=True)
        w1, s1 = engine.wasserstein_batch(e1, ec1, a1, ac1, k, k, want_status=True)
        w0 = np.where(s0 == 0, w0, np.nan); w1 = np.where(s1 == 0, w1, np.nan)
        seg = np.array([0, len(k)], np.int32)
        fa = engine.features_batch(a1[k], ac1[k])
        fe = engine.features_batch(e1[k], ec1[k])
        out[bname] = {
            "wasserstein_h0": float(engine.segment_nanmean(w0, seg)[0]),
            "wasserstein_h1": float(engine.segment_nanmean(w1, seg)[0]),
            "n_windows": int(len(idx)), "tau": tau,
            "audio_h1_features": fa, "eeg_h1_features": fe,
        }
        r, p = engine.spearman_batch(fa, fe, seg)                       # cmp:104-114
        out[bname]["feature_correlations"] = {f: {"r": float(r[0, k]), "p": float(p[0, k])}
                                              for k, f in enumerate(engine.SPEARMAN_FEATURES)}
    return out


# --------------------------------------------------------------------------------------
# whole-corpus feature matrix (scripts/tda_eeg_classification_v2.py:445-606, 670-688)
# --------------------------------------------------------------------------------------
def compute_min_windows_per_band(graphs_dirs, freq_bands=BANDS):
    """v2:445-474 -- global per-band minimum window count (np.load with mmap: headers only)."""
    min_windows = {band: np.inf for band in freq_bands}
    for graphs_dir in graphs_dirs:
        graphs_dir = Path(graphs_dir)
        if not graphs_dir.exists():
            continue
        for file_dir in [d for d in graphs_dir.iterdir() if d.is_dir()]:
            for band in freq_bands:
                dist_file = file_dir / f"{band}_distances.npy"
                if not dist_file.exists():
                    continue
                try:
                    n_windows = np.load(dist_file, mmap_mode="r").shape[0]
                    if n_windows > 0:
                        min_windows[band] = min(min_windows[band], n_windows)
                except Exception:
                    continue
    return {b: (0 if v == np.inf else int(v)) for b, v in min_windows.items()}


def _entries(graphs_dir_slow, graphs_dir_fast, batch_start=0, batch_end=None):
    """v2:532-541 -- sorted slow recordings (label 0) then sorted fast ones (label 1), sliced."""
    slow = sorted([d for d in Path(graphs_dir_slow).iterdir() if d.is_dir()])
    fast = sorted([d for d in Path(graphs_dir_fast).iterdir() if d.is_dir()])
    entries = [(d, 0) for d in slow] + [(d, 1) for d in fast]
    total = len(entries)
    if batch_end is None or batch_end < 0:
        batch_end = total
    return entries[max(0, batch_start):min(batch_end, total)], total


def create_dataset(graphs_dir_slow, graphs_dir_fast, freq_bands=BANDS, max_dim=1, max_edge_length=MAX_EDGE_LENGTH,
                   equalize_windows=True, window_sampling="random", max_windows_per_band="min", random_state=42,
                   batch_start=0, batch_end=None, rank=0, world_size=1, gather=None):
    """v2:499-606.  Returns (X, y, subjects, feature_names, filenames, metadata) with the reference's
    row order.  All recordings of this call go through ONE Rips launch (+ features + aggregation).

    world_size > 1: recordings are dealt to ranks by dist.shard_recordings (descending window
    count), every rank computes its rows and `gather(local_rows, my_recs, shards, n_total)`
    (dist.all_gather_rows) assembles the full X on every rank -- this replaces the reference's
    BATCH_START/BATCH_END partial files and their merge (v2:55-60, 608-638)."""
    if equalize_windows and max_windows_per_band == "min":
        max_windows_per_band = compute_min_windows_per_band([graphs_dir_slow, graphs_dir_fast], freq_bands)
    elif not equalize_windows:
        max_windows_per_band = None
    entries, _ = _entries(graphs_dir_slow, graphs_dir_fast, batch_start, batch_end)
    n_rec = len(entries)
    names = feature_names(freq_bands)
    # window counts decide the sharding (mmap: headers only)
    n_win_rec = np.zeros(n_rec, dtype=np.int64)
    for i, (d, _) in enumerate(entries):
        for band in freq_bands:
            f = d / f"{band}_distances.npy"
            if f.exists():
                n_win_rec[i] += np.load(f, mmap_mode="r").shape[0]
    if world_size > 1:
        from . import dist as tdist
        shards = tdist.shard_recordings(n_win_rec, world_size)
        mine = shards[rank]
    else:
        shards, mine = None, np.arange(n_rec)
    groups, where, metadata = [], [], [None] * n_rec
    for i in mine:
        file_dir, label = entries[i]
        md = {"n_windows": {}, "n_windows_used": {}, "validation_issues": [], "window_sampling": window_sampling,
              "max_windows_per_band": max_windows_per_band}
        for bi, band in enumerate(freq_bands):
            dist_file = file_dir / f"{band}_distances.npy"
            if not dist_file.exists():
                md["n_windows"][band] = 0
                continue
            dms = np.load(dist_file)
            n_windows = dms.shape[0]
            md["n_windows"][band] = n_windows
            if n_windows == 0:
                continue
            is_valid, issues = validate_distance_matrix(dms[0], f"{band}[0]")           # v2:380-382
            if not is_valid:
                md["validation_issues"].extend([f"{band}: {i}" for i in issues])
            if max_windows_per_band is None:
                use = np.arange(n_windows)
            else:
                max_n = max_windows_per_band.get(band, n_windows) if isinstance(max_windows_per_band, dict) \
                    else int(max_windows_per_band)
                max_n = min(max_n, n_windows)
                use = select_windows_md5(file_dir.name, band, n_windows, max_n, random_state) \
                    if window_sampling == "random" else np.arange(max_n)
            md["n_windows_used"][band] = len(use)
            groups.append(dms[use]); where.append((i, bi))
        md["n_windows_total"] = int(sum(md["n_windows"].values()))
        md["n_windows_used_total"] = int(sum(md["n_windows_used"].values()))
        md["filename"] = file_dir.name; md["subject"] = file_dir.name.split("_")[0]; md["label"] = label
        metadata[i] = md
    X = np.full((n_rec, 44 * len(freq_bands)), np.nan)
    if groups:
        agg = features_from_distances(groups, max_edge_length)
        for g, (i, bi) in enumerate(where):
            X[i, 44 * bi:44 * (bi + 1)] = agg[g]
    if world_size > 1:
        import torch
        import torch.distributed as tdist_
        from . import dist as tdist
        gather = gather or tdist.all_gather_rows
        # the rows travel from this rank's GPU (RCCL moves device memory; gloo, in the rehearsals, is staged
        # through the host by all_gather_rows itself) and come back to the host once assembled
        dev = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")
        X = gather(torch.from_numpy(X[mine]).to(dev), mine, shards, n_rec).cpu().numpy()
        if tdist_.is_initialized():              # the per-recording metadata of the other ranks (v2:684-688 saves all)
            parts = [None] * world_size
            tdist_.all_gather_object(parts, [(int(i), metadata[i]) for i in mine])
            for part in parts:
                for i, md in part:
                    metadata[i] = md
    y = np.array([lab for _, lab in entries])
    filenames = [d.name for d, _ in entries]
    subjects = np.array([f.split("_")[0] for f in filenames])
    return X, y, subjects, names, filenames, [m for m in metadata if m is not None]


def save_dataset(features_dir, X, y, subjects, names, filenames, metadata=None):
    """v2:670-688 -- features/X.npy, y.npy, subjects.npy, feature_names.txt, filenames.txt and, when the
    per-recording metadata are given, metadata.csv (pandas.DataFrame(all_metadata).to_csv(index=False)) and
    metadata.json (indent 2, ensure_ascii False)."""
    import json
    features_dir = Path(features_dir)
    features_dir.mkdir(exist_ok=True, parents=True)
    np.save(features_dir / "X.npy", X)
    np.save(features_dir / "y.npy", y)
    np.save(features_dir / "subjects.npy", subjects)
    (features_dir / "feature_names.txt").write_text("".join(f"{n}\n" for n in names))
    (features_dir / "filenames.txt").write_text("".join(f"{n}\n" for n in filenames))
    if metadata:
        import pandas as pd
        pd.DataFrame(metadata).to_csv(features_dir / "metadata.csv", index=False)
        with open(features_dir / "metadata.json", "w") as f:
            json.dump(metadata, f, indent=2, ensure_ascii=False)


DETAILED_COLUMNS = ["filename", "condition", "subject", "band", "wasserstein_h0", "wasserstein_h1", "n_windows", "tau"] + \
    [f"corr_{feat}_{k}" for feat in engine.SPEARMAN_FEATURES for k in ("r", "p")]


def process_recording_file(filename, condition, data_dir, graphs_dir, fs_audio=44100):
    """cmp:45-124 on the reference's directory layout: data/<condition>/<filename>.mat (audio track `y`, averaged
    over its channels as load_audio does, utils.py:47-53) and graphs/<condition>/<stem>/<band>_distances.npy.
    Returns the reference's result dict {"filename", "condition", "subject", "bands": {...}} or None when a path is
    missing or no band survives (cmp:48-49, cmp:124)."""
    mat_path = Path(data_dir) / condition / filename
    graph_dir = Path(graphs_dir) / condition / filename.replace(".mat", "")
    if not mat_path.exists() or not graph_dir.exists():
        return None
    import scipy.io as sio
    y = sio.loadmat(str(mat_path))["y"]
    if y.ndim == 2:
        y = y.mean(axis=1)
    dists = {}
    for bname in BANDS:
        f = graph_dir / f"{bname}_distances.npy"
        if f.exists():                                                   # cmp:67-70
            dists[bname] = np.load(str(f))
    bands = process_recording(y.astype(np.float64), dists, fs_audio)
    for bd in bands.values():                                            # the reference keeps scalars only (cmp:116-122)
        bd.pop("audio_h1_features", None); bd.pop("eeg_h1_features", None)
    if not bands:
        return None
    return {"filename": filename, "condition": condition, "subject": filename.split("_")[0], "bands": bands}


def detailed_rows(all_results):
    """cmp:145-157 -- one row per (recording, band): the columns of results/eeg_audio_tda_detailed.csv."""
    rows = []
    for r in all_results:
        for bname, bd in r["bands"].items():
            row = {"filename": r["filename"], "condition": r["condition"], "subject": r["subject"], "band": bname,
                   "wasserstein_h0": bd["wasserstein_h0"], "wasserstein_h1": bd["wasserstein_h1"],
                   "n_windows": bd["n_windows"], "tau": bd["tau"]}
            for feat, vals in bd["feature_correlations"].items():
                row[f"corr_{feat}_r"] = vals["r"]
                row[f"corr_{feat}_p"] = vals["p"]
            rows.append(row)
    return rows


def run_analysis(data_dir, graphs_dir, out_csv=None, conditions=("slow", "fast")):
    """cmp:126-157, the per-recording half: every data/<condition>/*.mat in sorted order through
    process_recording_file, then the detailed table (written as results/eeg_audio_tda_detailed.csv when out_csv is
    given).  The statistics behind it (cmp:161-220) are comparison_summary on that table; the batched route from raw
    recordings to both is run_comparison.  The plots (cmp:238-304) are outside this engine."""
    import pandas as pd
    all_results = []
    for condition in conditions:
        d = Path(data_dir) / condition
        for fn in sorted(f.name for f in d.glob("*.mat")) if d.exists() else []:
            r = process_recording_file(fn, condition, data_dir, graphs_dir)
            if r:
                all_results.append(r)
    df = pd.DataFrame(detailed_rows(all_results), columns=DETAILED_COLUMNS)
    if out_csv:
        Path(out_csv).parent.mkdir(parents=True, exist_ok=True)
        df.to_csv(out_csv, index=False)
    return all_results, df


def process_recording(audio, eeg_dists_by_band, fs_audio=44100):
    """cmp:45-124 from the raw audio track (44.1 kHz, as load_audio returns it, utils.py:47-53) and the
    recording's EEG distance matrices: resample -> envelope -> per-band filter -> windows
    (preprocess.audio_to_band_windows, all filters on the GPU) -> process_recording_arrays."""
    from . import preprocess
    return process_recording_arrays(preprocess.audio_to_band_windows(audio, fs_audio), eeg_dists_by_band)


def fdr_bh(pvals, alpha=0.05):
    """Benjamini-Hochberg as statsmodels' multipletests(method="fdr_bh") (mvm:213): p * m / rank on the sorted values, running
    minimum from the largest down, clipped at 1.  Returns (reject, p_corrected) in the order given."""
    p = np.asarray(pvals, dtype=np.float64)
    m = len(p)
    order = np.argsort(p, kind="stable")
    adj = p[order] * m / np.arange(1, m + 1)
    adj = np.minimum(np.minimum.accumulate(adj[::-1])[::-1], 1.0)
    out = np.empty(m)
    out[order] = adj
    return out <= alpha, out


def control_summary(rows, subjects, conditions=None, bands=BANDS):
    """mvm:180-221, host only: the per-band statistics of the control experiment from the rows of
    recordings.ControlPass ((n_rec, n_bands, >= 2): w_matched, w_mismatched first), one subject label per recording.
    Per band: rows with a NaN are dropped (mvm:182), the subjects' means taken (mvm:183-186), then n, the two means, the
    direction, Wilcoxon's p of the differences (1.0 when all are zero, mvm:197-200), Cohen's d (mvm:202), how many
    subjects have matched < mismatched; below 5 subjects {"n", "status": "insufficient"} (mvm:189-191).  Benjamini-
    Hochberg over the bands' p-values, a missing one counting as 1.0 (mvm:212-217).  The keys are those of the
    reference's results/matched_vs_mismatched.json.  conditions: accepted for symmetry with mvm's rows; the summary
    pools both (mvm's per-condition figures, mvm:226-247, are printed only and are this function on a subset of rows)."""
    from scipy.stats import wilcoxon
    rows = np.asarray(rows, dtype=np.float64)
    subjects = np.asarray([str(s) for s in subjects])
    bands = list(bands)
    assert rows.ndim == 3 and rows.shape[0] == len(subjects) and rows.shape[1] == len(bands) and rows.shape[2] >= 2
    assert conditions is None or len(conditions) == len(subjects)
    results = {}
    for b, band in enumerate(bands):
        wm, wx = rows[:, b, 0], rows[:, b, 1]
        ok = ~np.isnan(wm) & ~np.isnan(wx)
        subj = sorted(set(subjects[ok]))                                       # groupby sorts its keys
        sm = np.array([[wm[ok & (subjects == s)].mean(), wx[ok & (subjects == s)].mean()] for s in subj]).reshape(-1, 2)
        n = len(sm)
        if n < 5:
            results[band] = {"n": n, "status": "insufficient"}
            continue
        diff = sm[:, 0] - sm[:, 1]
        mean_m, mean_x = sm[:, 0].mean(), sm[:, 1].mean()
        p = wilcoxon(diff)[1] if np.any(diff != 0) else 1.0
        n_lower = int(np.sum(diff < 0))
        results[band] = {"n": n, "w_matched": float(mean_m), "w_mismatched": float(mean_x),
                         "direction": "matched < mismatched" if mean_m < mean_x else "matched > mismatched",
                         "p": float(p), "cohens_d": float(np.mean(diff) / (np.std(diff, ddof=1) + 1e-10)),
                         "n_matched_lower": n_lower, "pct_matched_lower": float(n_lower / n * 100)}
    reject, pfdr = fdr_bh([results[b].get("p", 1.0) for b in bands])
    for i, band in enumerate(bands):
        if "p" in results[band]:
            results[band]["p_fdr"] = float(pfdr[i])
            results[band]["sig_fdr"] = bool(reject[i])
    return results


def match_rows_host(dist, own_col, keep=None):
    """engine.match_rows_dev restated in numpy: dist (n_rec, n_bands, n_col), own_col (n_rec,) -> (n_rec, n_bands, 5)
    [w_own, n_valid, n_less, n_equal, null_mean] (the device's rows without the pair count).  keep: optional bool
    (n_rec, n_col), the columns that may count among the others of a recording (the own column never does)."""
    dist = np.asarray(dist, dtype=np.float64)
    n_rec, nb, n_col = dist.shape
    out = np.full((n_rec, nb, 5), np.nan)
    out[:, :, 1:4] = 0.0
    for r in range(n_rec):
        own = int(own_col[r]) if 0 <= own_col[r] < n_col else -1
        others = np.ones(n_col, bool) if keep is None else np.asarray(keep[r], bool).copy()
        if own >= 0:
            others[own] = False
        for b in range(nb):
            v = dist[r, b, others & np.isfinite(dist[r, b])]
            w = dist[r, b, own] if own >= 0 else np.nan
            out[r, b, 0], out[r, b, 1] = w, len(v)
            if not np.isnan(w):
                out[r, b, 2], out[r, b, 3] = np.sum(v < w), np.sum(v == w)
            if len(v):
                out[r, b, 4] = v.mean()
    return out


def match_mismatch_summary(rows, dist, subjects, conditions=None, bands=BANDS, candidates=None, exclude_same_subject=False):
    """Host only: the per-band statistics of the match-mismatch matrix of recordings.MatchMismatchPass.  rows
    (n_rec, n_bands, 6) [w_own, n_own_pairs, n_valid, n_less, n_equal, null_mean], dist (n_rec, n_bands, n_col), one
    subject label per recording; candidates: the recording of every column (default: all, in order).  The sliced matrix of
    MatchMismatchPass(sliced=dirs) is a valid input as well: rows = slc_rows_h, dist = slc_dist_h.  Per band, over the
    recordings with a finite w_own and at least one other finite column:
      n, top1 (share of recordings whose true audio has midrank 1 + n_less + n_equal / 2 = 1 among n_valid + 1
      candidates), mean_percentile (mean of (n_less + n_equal / 2) / n_valid: 0 = always the closest, 0.5 = chance),
      matched_mean, null_mean, Wilcoxon's p of w_own - null_mean across recordings (1.0 when all differences are zero),
      Cohen's d of that paired difference -- control_summary's conventions (mvm:197-202); below 5 recordings
      {"n", "status": "insufficient"} -- and Benjamini-Hochberg over the bands (fdr_bh, mvm:212-217).
    exclude_same_subject=True: the counts and the null mean are taken again from dist with the columns of the
    recording's own subject left out, the own column excepted (another recording of the same infant is no independent
    mismatch).  conditions: accepted for symmetry with control_summary."""
    from scipy.stats import wilcoxon
    rows, dist = np.asarray(rows, dtype=np.float64), np.asarray(dist, dtype=np.float64)
    subjects = np.asarray([str(s) for s in subjects])
    bands = list(bands)
    n_rec, nb, n_col = dist.shape
    cand = np.arange(n_rec) if candidates is None else np.asarray(candidates, dtype=np.int64).ravel()
    assert rows.shape == (n_rec, nb, 6) and len(subjects) == n_rec and nb == len(bands) and len(cand) == n_col
    assert conditions is None or len(conditions) == n_rec
    if exclude_same_subject:
        own_col = np.full(n_rec, -1, np.int64)
        own_col[cand] = np.arange(n_col)
        m = match_rows_host(dist, own_col, keep=subjects[:, None] != subjects[cand][None, :])
        w_own, n_valid, n_less, n_equal, null = (m[:, :, j] for j in range(5))
    else:
        w_own, n_valid, n_less, n_equal, null = (rows[:, :, j] for j in (0, 2, 3, 4, 5))
    results = {}
    for b, band in enumerate(bands):
        ok = np.isfinite(w_own[:, b]) & (n_valid[:, b] > 0)
        n = int(ok.sum())
        if n < 5:
            results[band] = {"n": n, "status": "insufficient"}
            continue
        below = n_less[ok, b] + 0.5 * n_equal[ok, b]
        diff = w_own[ok, b] - null[ok, b]
        p = wilcoxon(diff)[1] if np.any(diff != 0) else 1.0
        results[band] = {"n": n, "top1": float(np.mean(1.0 + below == 1.0)), "mean_percentile": float(np.mean(below / n_valid[ok, b])),
                         "matched_mean": float(w_own[ok, b].mean()), "null_mean": float(null[ok, b].mean()), "p": float(p),
                         "cohens_d": float(np.mean(diff) / (np.std(diff, ddof=1) + 1e-10))}
    reject, pfdr = fdr_bh([results[b].get("p", 1.0) for b in bands])
    for i, band in enumerate(bands):
        if "p" in results[band]:
            results[band]["p_fdr"] = float(pfdr[i])
            results[band]["sig_fdr"] = bool(reject[i])
    return results


# --------------------------------------------------------------------------------------
# scripts/tda_eeg_audio_comparison.py from a batched pass: the detailed table and the per-band statistics
# --------------------------------------------------------------------------------------
COMPARISON_CONDITIONS = ("slow", "fast")        # cmp:131,171-172
_SUMMARY_MEANS = ("wasserstein_h0", "wasserstein_h1", "corr_mean_persistence_r", "corr_persistence_entropy_r")   # cmp:165-169


def comparison_rows(rows, corr, filenames, conditions, bands=BANDS):
    """cmp:145-157 from the outputs of a pass built with correlations=True: rows (n_rec, n_bands, >= 4) [W_H0, W_H1, tau,
    n_windows, ...], corr (n_rec, n_bands, 10) [r, p] of the five series.  One dict of DETAILED_COLUMNS per (recording,
    band), recordings in the order given, bands in `bands` order; subject = the file name up to its first "_" (cmp:51).
    Left out, as the reference leaves them out: a recording without a window (n_windows == 0, cmp:71-72) and a band none of
    whose windows reached the distances (NaN correlation cells, cmp:101-102)."""
    rows = np.asarray(rows, dtype=np.float64)
    corr = np.asarray(corr, dtype=np.float64)
    bands = list(bands)
    n_rec = len(filenames)
    assert len(conditions) == n_rec and rows.shape[:2] == (n_rec, len(bands)) and rows.shape[2] >= 4
    assert corr.shape == (n_rec, len(bands), len(DETAILED_COLUMNS) - 8)
    out = []
    for r in range(n_rec):
        fn = str(filenames[r])
        for b, band in enumerate(bands):
            if rows[r, b, 3] == 0 or np.isnan(corr[r, b]).any():
                continue
            row = {"filename": fn, "condition": str(conditions[r]), "subject": fn.split("_")[0], "band": band,
                   "wasserstein_h0": float(rows[r, b, 0]), "wasserstein_h1": float(rows[r, b, 1]),
                   "n_windows": int(rows[r, b, 3]), "tau": int(rows[r, b, 2])}
            row.update((c, float(v)) for c, v in zip(DETAILED_COLUMNS[8:], corr[r, b]))
            out.append(row)
    return out


def comparison_summary(table, bands=BANDS, n_permutations=1000, alpha=0.05):
    """cmp:161-220, host only: the `band_results` of results/eeg_audio_tda_comparison.json from the detailed table (the
    dicts of comparison_rows / detailed_rows, or a DataFrame with those columns).  Per band: the means per (subject,
    condition) of the two distances and two correlations (cmp:165-169), the subjects present in both conditions, sorted
    (cmp:173-175); below 5 of them only {"n_subjects", "band"}; otherwise Wilcoxon's p of the slow - fast differences of
    W_H0, W_H1 and corr_mean_persistence_r (1.0 when all are zero, cmp:184-186), the sign-flip permutation p of W_H1
    (default_rng(42) anew per band, n_permutations draws of choice([-1, 1], n), (exceed + 1) / (n_permutations + 1),
    cmp:189-193), Cohen's d with the sample standard deviation (cmp:196), the direction, how many subjects have slow <
    fast and the condition means.  Then Benjamini-Hochberg over the bands' wass_h1_p, a missing one counting as 1.0, written
    into every band (cmp:216-220)."""
    from scipy.stats import wilcoxon
    if hasattr(table, "to_dict"):
        table = table.to_dict("records")
    bands = list(bands)
    slow_c, fast_c = COMPARISON_CONDITIONS
    stats = {}
    for band in bands:
        cells = {}                                                       # (subject, condition) -> rows of the four columns
        for row in table:
            if row["band"] == band:
                cells.setdefault((str(row["subject"]), str(row["condition"])), []).append([row[c] for c in _SUMMARY_MEANS])
        means = {k: np.mean(np.asarray(v, dtype=np.float64), axis=0) for k, v in cells.items()}
        common = sorted({s for s, c in means if c == slow_c} & {s for s, c in means if c == fast_c})
        n = len(common)
        bs = {"n_subjects": n, "band": band}
        if n >= 5:
            slow = np.array([means[s, slow_c] for s in common])
            fast = np.array([means[s, fast_c] for s in common])
            d0, d1, dc = (slow[:, k] - fast[:, k] for k in (0, 1, 2))
            p0, p1, pc = (float(wilcoxon(d)[1]) if np.any(d != 0) else 1.0 for d in (d0, d1, dc))
            rng = np.random.default_rng(42)
            obs = abs(np.mean(d1))
            exceed = sum(1 for _ in range(n_permutations) if abs(np.mean(d1 * rng.choice([-1, 1], n))) >= obs)
            bs.update({
                "wass_h0_slow": float(slow[:, 0].mean()), "wass_h0_fast": float(fast[:, 0].mean()), "wass_h0_p": p0,
                "wass_h1_slow": float(slow[:, 1].mean()), "wass_h1_fast": float(fast[:, 1].mean()), "wass_h1_p": p1,
                "wass_h1_perm_p": float((exceed + 1) / (n_permutations + 1)),
                "wass_h1_cohens_d": float(np.mean(d1) / (np.std(d1, ddof=1) + 1e-10)),
                "wass_h1_direction": "slow < fast" if np.mean(d1) < 0 else "slow > fast",
                "corr_slow": float(slow[:, 2].mean()), "corr_fast": float(fast[:, 2].mean()), "corr_p": pc,
                "n_slow_lower": int(np.sum(d1 < 0)),
            })
        stats[band] = bs
    reject, pfdr = fdr_bh([stats[b].get("wass_h1_p", 1.0) for b in bands], alpha)
    for i, band in enumerate(bands):
        stats[band]["wass_h1_p_fdr"] = float(pfdr[i])
        stats[band]["wass_h1_sig_fdr"] = bool(reject[i])
    return stats


def run_comparison(pass_, raw_h, second_h, filenames, conditions, out_csv=None, out_json=None):
    """cmp:126-220 from raw recordings in one batched pass: pass_ is a recordings.RecordingPass, RaggedRecordingPass or
    RaggedAudioRecordingPass built with correlations=True, raw_h / second_h the two pinned inputs of its `run`.  Returns
    (rows, corr, table, summary): the pass' rows and correlations as numpy arrays, comparison_rows and
    comparison_summary of them.  out_csv: the table as results/eeg_audio_tda_detailed.csv; out_json: the counts and
    `band_results` of results/eeg_audio_tda_comparison.json."""
    if not getattr(pass_, "correlations", False):
        raise ValueError("run_comparison needs a pass built with correlations=True")
    bands = BANDS if len(pass_.bands) == len(BANDS) else [f"band{b}" for b in range(len(pass_.bands))]
    rows = pass_.run(raw_h, second_h).numpy().copy()
    corr = pass_.corr_h.numpy().copy()
    table = comparison_rows(rows, corr, filenames, conditions, bands)
    summary = comparison_summary(table, bands)
    if out_csv:
        import pandas as pd
        Path(out_csv).parent.mkdir(parents=True, exist_ok=True)
        pd.DataFrame(table, columns=DETAILED_COLUMNS).to_csv(out_csv, index=False)
    if out_json:
        import json
        Path(out_json).parent.mkdir(parents=True, exist_ok=True)
        kept = {(t["filename"], t["condition"]) for t in table}
        doc = {"n_recordings": len(kept), "n_subjects": len({t["subject"] for t in table}),
               "n_slow": sum(1 for _, c in kept if c == COMPARISON_CONDITIONS[0]),
               "n_fast": sum(1 for _, c in kept if c == COMPARISON_CONDITIONS[1]), "band_results": summary}
        with open(out_json, "w") as f:
            json.dump(doc, f, indent=2)
    return rows, corr, table, summary


def two_sample_from_diagrams(dgms, y, subjects=None, metric=("sliced", None), ctx=None, **kw):
    """(not in the reference) The two-sample permutation test of utils.two_sample_permutation_test on the recordings'
    diagrams: is the topology of group y == 1 different from that of group y == 0?  The (n_rec, n_rec) matrix is built on
    the device by the existing Gram calls and goes to the permutation kernel without leaving it.
      metric = ("sliced", dirs)     dgms: one diagram per recording; sliced Wasserstein distances over the (M, 2) direction
                                    table dirs (None: utils.default_directions()); statistic "joint_loss"
      metric = ("fisher", sigma)    the same with the persistence Fisher distance; "joint_loss"
      metric = ("kernel", kernel)   dgms: per recording a LIST of diagrams (its windows); the Gram matrix of the recordings'
                                    mean embeddings under a kernel of engine.diagram_kernel_args, e.g. ("pss", 0.1); "mmd"
    statistic=..., n_permutations, seed and labels go on to two_sample_permutation_test, whose dict comes back."""
    import torch
    from . import utils
    from ._lib import get_ctx
    ctx = ctx or get_ctx()
    dev = torch.device("cuda", ctx.device)
    kind, par = metric
    if kind == "kernel":
        flat = [utils._clean_pair_diagram(d) for rec in dgms for d in rec]
        seg_off = np.concatenate([[0], np.cumsum([len(rec) for rec in dgms])]).astype(np.int32)
    elif kind in ("sliced", "fisher"):
        flat = [utils._clean_pair_diagram(d) for d in dgms]
    else:
        raise ValueError(f"Unknown metric: {kind!r}")
    rows, cnt = engine.pack_diagrams(flat)
    rows_t, cnt_t = torch.from_numpy(rows).to(dev), torch.from_numpy(cnt).to(dev)
    if kind == "sliced":
        dirs = engine._directions(utils.default_directions() if par is None else par)
        G = engine.sliced_wasserstein_gram_dev(rows_t, cnt_t, torch.from_numpy(dirs).to(dev), ctx=ctx)
    elif kind == "fisher":
        G = engine.persistence_fisher_gram_dev(rows_t, cnt_t, par, ctx=ctx)
    else:
        G = engine.diagram_kernel_gram_dev(rows_t, cnt_t, par, seg_off_a=torch.from_numpy(seg_off).to(dev), ctx=ctx)
    kw.setdefault("statistic", "mmd" if kind == "kernel" else "joint_loss")
    return utils.two_sample_permutation_test(G, y, subjects=subjects, ctx=ctx, **kw)
