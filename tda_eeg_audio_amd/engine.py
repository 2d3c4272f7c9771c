"""
engine.py -- batched numpy / torch-tensor front end of libtdaeeg.so.

Every function here is a thin marshalling layer over one C-ABI entry point of
include/tdaeeg.h; all arithmetic happens in the HIP kernels.  There is no CPU path.

  host arrays  : corr_dist_batch, rips_dm_batch, takens_rips_batch, cloud_rips_batch,
                 tau_batch, features_batch, aggregate_batch, wasserstein_batch, bottleneck_batch, wasserstein_q_batch,
                 sliced_wasserstein_batch, sliced_wasserstein_gram,
                 landscape_batch, image_batch, frechet_mean_batch, temporal_corr_batch,
                 takens_landmarks_batch, cloud_landmarks_batch (greedy permutation, ripser's n_perm)
                 sublevel_batch (H0 of the sublevel-set filtration of 1-D signals)
                 plv_dist_batch (phase-locking value matrix of a window's channels and its distance matrix)
                 connectivity_dist_batch (wPLI, imaginary coherency, coherence or envelope correlation of a window's
                 channels and its distance matrix; CONNECTIVITY_MEASURES, connectivity_measure)
                 pack_labels / permutation_sums_batch (within- and between-group sums of matrices under relabellings)
                 euler_dm_batch, euler_cloud_batch, euler_takens_batch (simplex counts and Euler characteristic of the Rips
                 complex on a grid of scales, by the keys of the Rips entry points)
                 network_dm_batch, network_cloud_batch, network_takens_batch (the graph measures of the thresholded graphs on
                 a grid of scales, by the same keys and presence rule; network_args)
                 recurrence_dm_batch, recurrence_cloud_batch, recurrence_takens_batch (recurrence quantification of the
                 windows in time order on a grid of scales, by the same keys and presence rule; recurrence_args)
                 generators_dm_batch, generators_cloud_batch, generators_takens_batch (the edges behind the rows of the
                 diagrams, a representative cycle per H1 row and the participation of every vertex; generators_args)
                 ami_batch, fnn_batch (the delay at the first minimum of the average mutual information and the dimension
                 at which the false nearest neighbours vanish; ami_args, fnn_args)
  device tensors (torch, already resident in HBM, launched on torch's current stream):
                 the ``*_dev`` twins -- used by bench.py and the multi-GPU driver.
                 wasserstein_cross_dev / cross_rows_dev: the control experiment's pairs, resolved on the device
                 from group tables (recordings.ControlPass).
                 wasserstein_matrix_dev / match_rows_dev: every group against every candidate column
                 (recordings.MatchMismatchPass).
                 sliced_prepare_dev / sliced_wasserstein_prepared_dev / sliced_wasserstein_gram_dev / sliced_matrix_dev:
                 the sliced Wasserstein distance with every diagram sorted once (MatchMismatchPass(sliced=dirs)).
                 takens_landmarks_dev / cloud_landmarks_dev / takens_rips_landmarks_dev: Rips on greedy landmarks for clouds
                 above 128 points (Workspace(takens=(dim, subsample, n_perm))).
                 sublevel_dev / sublevel_features_dev: sublevel-set diagrams of signals read stacked or in place, and
                 their 11 features through a bounded scratch (Workspace(sublevel=True)).
                 plv_dist_dev: phase-locking value distance matrices of windows read stacked or in place, ready for
                 rips_dm_dev (Workspace(phase_locking=method)).
                 connectivity_dist_dev: the same for wPLI, imaginary coherency, coherence and envelope correlation
                 (drivers.connectivity_features_from_windows).
                 permutation_sums_dev: the sums of a two-sample permutation test on matrices that never leave the device
                 (utils.two_sample_permutation_test, drivers.two_sample_from_diagrams).
                 euler_dm_dev / euler_cloud_dev / euler_takens_dev / euler_mean_dev / euler_eeg_windows_dev: Euler
                 characteristic and simplex-count curves of resident windows and their group means
                 (utils.compute_eeg_euler_curve, drivers.euler_curves_from_distances).
                 network_dm_dev / network_cloud_dev / network_takens_dev / network_mean_dev / network_eeg_windows_dev:
                 the network curves of resident windows and their group means, into a DeviceNetworkCurves
                 (utils.compute_eeg_network_curves, drivers.network_curves_from_distances).
                 recurrence_dm_dev / recurrence_cloud_dev / recurrence_takens_dev / recurrence_mean_dev: the recurrence
                 curves of resident windows and their group means, into a DeviceRecurrenceCurves
                 (utils.compute_signal_recurrence_curves, drivers.recurrence_curves_from_windows).
                 ami_dev / ami_segments_dev / fnn_dev: delay and dimension selection of resident windows, into a
                 DeviceEmbedding; ami_segments_dev writes the per-window delays the Takens forms take
                 (utils.compute_tau_ami, drivers.embedding_parameters_from_windows).
                 generators_dm_dev / generators_cloud_dev / generators_takens_dev / generators_mean_dev /
                 generators_eeg_windows_dev: generators and cycles of resident windows from a DeviceDiagrams or raw row
                 tensors, into a DeviceGenerators (utils.compute_eeg_generators,
                 drivers.channel_participation_from_distances).
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import f64, i32, ptr, get_ctx

MAX_EDGE_LENGTH = 2.0      # scripts/utils.py:25
DEFAULT_H1_CAP = 256


def _diagrams(rows, cnt, cap):
    """(n, cap, 2) rows + counts -> list of (k,2) float64 arrays."""
    return [rows[i, :min(int(cnt[i]), cap)].copy() for i in range(rows.shape[0])]


# ------------------------------------------------------------------ host-array API
def corr_dist_batch(windows, want_corr=True, ctx=None):
    ctx = ctx or get_ctx()
    w = f64(windows)
    n_win, n_ch, n_t = w.shape
    dist = np.empty((n_win, n_ch, n_ch))
    corr = np.empty((n_win, n_ch, n_ch)) if want_corr else None
    ctx.check(ctx.lib.tda_corr_dist_batch(ctx.h, ptr(w), n_win, n_ch, n_t, ptr(dist), ptr(corr)))
    return (corr, dist) if want_corr else dist


def corr_dist_sliding(signal, win_len=250, step=62, want_corr=False, ctx=None):
    """(n_ch, n_samples) band-passed recording -> distance matrices of its sliding windows
    (nb1:314-381 + nb2:198-207 fused)."""
    ctx = ctx or get_ctx()
    s = f64(signal)
    n_ch, n_s = s.shape
    n_win = (n_s - win_len) // step + 1 if n_s >= win_len else 0
    dist = np.empty((n_win, n_ch, n_ch))
    corr = np.empty((n_win, n_ch, n_ch)) if want_corr else None
    ctx.check(ctx.lib.tda_corr_dist_sliding(ctx.h, ptr(s), n_ch, n_s, win_len, step, ptr(dist), ptr(corr), None))
    return (corr, dist) if want_corr else dist


def corr_dist_sliding_dev(sig_t, win_len=250, step=62, dist_t=None, corr_t=None, ctx=None):
    import torch
    ctx = ctx or get_ctx()
    assert sig_t.is_cuda and sig_t.dtype == torch.float64 and sig_t.is_contiguous()
    n_ch, n_s = sig_t.shape
    n_win = (n_s - win_len) // step + 1 if n_s >= win_len else 0
    if dist_t is None:
        dist_t = torch.empty((n_win, n_ch, n_ch), dtype=torch.float64, device=sig_t.device)
    ctx.check(ctx.lib.tda_corr_dist_sliding_dev(ctx.h, _tp(sig_t), n_ch, n_s, win_len, step, _tp(dist_t), _tp(corr_t),
                                                None, _stream()))
    return dist_t


DIST_METHODS = {"euclidean": 0, "abs": 1, "standard": 2, "sqrt": 3}     # nb2:107-116
METHOD_NAMES = ("euclidean", "abs", "standard", "sqrt")                 # the names by number


def corr_to_dist_batch(corr, method="euclidean", ctx=None):
    if method not in DIST_METHODS:
        raise ValueError(f"Unknown method: {method}")                      # nb2:117
    ctx = ctx or get_ctx()
    c = f64(corr)
    n_win, n, _ = c.shape
    dist = np.empty_like(c)
    ctx.check(ctx.lib.tda_corr_to_dist_batch(ctx.h, ptr(c), n_win, n, DIST_METHODS[method], ptr(dist)))
    return dist


def rips_dm_batch(dms, thresh=MAX_EDGE_LENGTH, symmetrise=True, h1_cap=DEFAULT_H1_CAP, ctx=None, raw=False):
    ctx = ctx or get_ctx()
    d = f64(dms)
    n_win, n, n2 = d.shape
    assert n == n2, "distance matrices must be square"   # the only thing ripser itself rejects
    h0 = np.empty((n_win, n, 2)); h1 = np.empty((n_win, h1_cap, 2))
    c0 = np.empty(n_win, np.int32); c1 = np.empty(n_win, np.int32); st = np.empty(n_win, np.int32)
    ctx.check(ctx.lib.tda_rips_dm_batch(ctx.h, ptr(d), n_win, n, float(thresh), int(bool(symmetrise)),
                                        ptr(h0), n, ptr(c0), ptr(h1), h1_cap, ptr(c1), ptr(st)))
    if raw:
        return h0, c0, h1, c1, st
    return _diagrams(h0, c0, n), _diagrams(h1, c1, h1_cap), st


def takens_rips_batch(windows, taus, dim=3, subsample=2, thresh=MAX_EDGE_LENGTH, h1_cap=DEFAULT_H1_CAP,
                      ctx=None, raw=False):
    ctx = ctx or get_ctx()
    w = f64(windows)
    n_win, n_t = w.shape
    tau = i32(np.broadcast_to(np.asarray(taus), (n_win,)))
    h0_cap = _lib.MAX_POINTS
    h0 = np.empty((n_win, h0_cap, 2)); h1 = np.empty((n_win, h1_cap, 2))
    c0 = np.empty(n_win, np.int32); c1 = np.empty(n_win, np.int32)
    npts = np.empty(n_win, np.int32); st = np.empty(n_win, np.int32)
    ctx.check(ctx.lib.tda_takens_rips_batch(ctx.h, ptr(w), ptr(tau), n_win, n_t, dim, subsample, float(thresh),
                                            ptr(h0), h0_cap, ptr(c0), ptr(h1), h1_cap, ptr(c1), ptr(npts), ptr(st)))
    if raw:
        return h0, c0, h1, c1, npts, st
    return _diagrams(h0, c0, h0_cap), _diagrams(h1, c1, h1_cap), npts, st


def cloud_rips_batch(clouds, n_pts=None, normalise=True, thresh=MAX_EDGE_LENGTH, h1_cap=DEFAULT_H1_CAP,
                     ctx=None, raw=False):
    ctx = ctx or get_ctx()
    pc = f64(clouds)
    n_win, p_cap, dim = pc.shape
    n_pts = i32(np.full(n_win, p_cap) if n_pts is None else n_pts)
    h0_cap = max(p_cap, 3)
    h0 = np.empty((n_win, h0_cap, 2)); h1 = np.empty((n_win, h1_cap, 2))
    c0 = np.empty(n_win, np.int32); c1 = np.empty(n_win, np.int32); st = np.empty(n_win, np.int32)
    ctx.check(ctx.lib.tda_cloud_rips_batch(ctx.h, ptr(pc), ptr(n_pts), n_win, p_cap, dim, int(bool(normalise)),
                                           float(thresh), ptr(h0), h0_cap, ptr(c0), ptr(h1), h1_cap, ptr(c1),
                                           ptr(st)))
    if raw:
        return h0, c0, h1, c1, st
    return _diagrams(h0, c0, h0_cap), _diagrams(h1, c1, h1_cap), st


def landmark_args(n_perm, dim, subsample=1):
    """The parameters of the greedy permutation as the kernel takes them (include/tdaeeg.h, "Landmark Rips"): ints, with
    3 <= n_perm <= MAX_POINTS, 1 <= dim <= 4, subsample >= 1.  TdaError, before any GPU call, for anything else."""
    for name, v, lo, hi in (("n_perm", n_perm, 3, _lib.MAX_POINTS), ("dim", dim, 1, 4), ("subsample", subsample, 1, None)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < lo or (hi is not None and v > hi):
            raise _lib.TdaError(f"landmarks: {name} must be an integer in [{lo}, {'...' if hi is None else hi}], not {v!r}")
    return int(n_perm), int(dim), int(subsample)


def _landmark_out(n_win, n_perm, dim):
    """Host output buffers of a landmark call; rows and entries from n_lm on keep these zeros."""
    return (np.zeros((n_win, n_perm, dim)), np.zeros((n_win, n_perm), np.int32), np.zeros((n_win, n_perm)),
            np.zeros(n_win), np.zeros(n_win, np.int32), np.zeros(n_win, np.int32))


def takens_landmarks_batch(windows, taus, n_perm, dim=3, subsample=1, ctx=None):
    """Greedy permutation (ripser's n_perm) of the normalised Takens cloud of every window: (lm (n_win, n_perm, dim),
    lm_idx, lm_lambda, r_cover, n_lm, n_full), include/tdaeeg.h "Landmark Rips".  A refused window (tau < 1, more than
    LM_MAX_POINTS points) has n_lm = MAX_POINTS + 1 and r_cover NaN."""
    n_perm, dim, subsample = landmark_args(n_perm, dim, subsample)
    ctx = ctx or get_ctx()
    w = f64(windows)
    n_win, n_t = w.shape
    tau = i32(np.broadcast_to(np.asarray(taus), (n_win,)))
    lm, idx, lam, rc, n_lm, n_full = _landmark_out(n_win, n_perm, dim)
    ctx.check(ctx.lib.tda_takens_landmarks(ctx.h, ptr(w), ptr(tau), n_win, n_t, dim, subsample, n_perm, ptr(lm), ptr(idx),
                                           ptr(lam), ptr(rc), ptr(n_lm), ptr(n_full)))
    return lm, idx, lam, rc, n_lm, n_full


def cloud_landmarks_batch(clouds, n_perm, n_pts=None, normalise=True, ctx=None):
    """The same from explicit clouds (n_win, p_cap, dim) with n_pts rows each, p_cap <= LM_MAX_POINTS."""
    ctx = ctx or get_ctx()
    pc = f64(clouds)
    n_win, p_cap, dim = pc.shape
    n_perm, dim, _ = landmark_args(n_perm, dim)
    n_pts = i32(np.full(n_win, p_cap) if n_pts is None else n_pts)
    lm, idx, lam, rc, n_lm, n_full = _landmark_out(n_win, n_perm, dim)
    ctx.check(ctx.lib.tda_cloud_landmarks(ctx.h, ptr(pc), ptr(n_pts), n_win, p_cap, dim, int(bool(normalise)), n_perm,
                                          ptr(lm), ptr(idx), ptr(lam), ptr(rc), ptr(n_lm), ptr(n_full)))
    return lm, idx, lam, rc, n_lm, n_full


def sublevel_rows(n_t):
    """TDA_SL_ROWS(n_t): the most rows the sublevel-set diagram of n_t samples can have, the essential one included."""
    return (int(n_t) + 1) // 2


def sublevel_batch(sig, n_t=None, win_start=None, win_ld=None, n_ch=None, cap=None, dgm=None, idx=None, ctx=None):
    """H0 of the sublevel-set filtration of 1-D signals (include/tdaeeg.h, "Sublevel-set persistence of time series"):
    (dgm (n_sig, cap, 2), cnt (n_sig), idx (n_sig, cap, 2) int32, status (n_sig)).  sig (n_sig, n_t), or (n_win, n_ch, n_t)
    with signal w * n_ch + c; or, with the int64 tables win_start / win_ld (n_win each) and n_ch, n_t, a flat array whose
    signal w * n_ch + c starts at element win_start[w] + c * win_ld[w].  Only rows [0, cnt) are written: the rest of dgm /
    idx keeps what the caller's buffers hold (NaN / -1 in the ones made here).  A signal with a sample that is not finite has
    cnt 0 and status TDA_WIN_NOT_FINITE.  TdaError for n_t outside [1, SL_MAX_SAMPLES], n_ch < 1 or cap < sublevel_rows(n_t)."""
    ctx = ctx or get_ctx()
    s = f64(sig)
    if win_start is None and win_ld is None:
        if s.ndim == 2:
            s = s[:, None, :]
        n_win, n_ch, n_t = s.shape
        ws = wl = None
    else:
        ws, wl = (np.ascontiguousarray(t, dtype=np.int64) for t in (win_start, win_ld))
        assert ws.shape == wl.shape and ws.ndim == 1 and n_ch is not None and n_t is not None
        n_win, n_ch, n_t = ws.shape[0], int(n_ch), int(n_t)
        if n_win and n_ch >= 1 and n_t >= 1:
            assert ws.min() >= 0 and wl.min() >= 0 and int((ws + (n_ch - 1) * wl).max()) + n_t <= s.size, "table past the end of sig"
    cap = sublevel_rows(n_t) if cap is None else int(cap)
    n_sig = n_win * max(n_ch, 0)
    rows = max(cap, 0)
    dgm = np.full((n_sig, rows, 2), np.nan) if dgm is None else dgm
    idx = np.full((n_sig, rows, 2), -1, np.int32) if idx is None else idx
    assert dgm.dtype == np.float64 and dgm.flags.c_contiguous and dgm.shape == (n_sig, rows, 2)
    assert idx.dtype == np.int32 and idx.flags.c_contiguous and idx.shape == (n_sig, rows, 2)
    cnt = np.zeros(n_sig, np.int32)
    status = np.zeros(n_sig, np.int32)
    ctx.check(ctx.lib.tda_sublevel_batch(ctx.h, ptr(s), ptr(ws), ptr(wl), n_win, n_ch, n_t, ptr(dgm), cap, ptr(cnt), ptr(idx),
                                         ptr(status)))
    return dgm, cnt, idx, status


def _host_windows(sig, n_t, win_start, win_ld, n_ch):
    """The window arguments of plv_dist_batch / connectivity_dist_batch: (sig as float64, the int64 tables or None twice,
    n_win, n_ch, n_t) of stacked windows (n_win, n_ch, n_t), one window (n_ch, n_t), or a flat array with tables."""
    s = f64(sig)
    if win_start is None and win_ld is None:
        if s.ndim == 2:
            s = s[None]
        n_win, n_ch, n_t = s.shape
        ws = wl = None
    else:
        ws, wl = (np.ascontiguousarray(t, dtype=np.int64) for t in (win_start, win_ld))
        assert ws.shape == wl.shape and ws.ndim == 1 and n_ch is not None and n_t is not None
        n_win, n_ch, n_t = ws.shape[0], int(n_ch), int(n_t)
        if n_win and n_ch >= 1 and n_t >= 1:
            assert ws.min() >= 0 and wl.min() >= 0 and int((ws + (n_ch - 1) * wl).max()) + n_t <= s.size, "table past the end of sig"
    return s, ws, wl, n_win, n_ch, n_t


def plv_method(method):
    """The method number of a phase-locking distance: one of DIST_METHODS' names, or True for "euclidean".  ValueError for
    anything else."""
    if method is True:
        return 0
    if not isinstance(method, str) or method not in DIST_METHODS:
        raise ValueError(f"phase_locking: one of {sorted(DIST_METHODS)} or True, not {method!r}")
    return DIST_METHODS[method]


def plv_dist_batch(sig, n_t=None, win_start=None, win_ld=None, n_ch=None, method="euclidean", want_plv=True, ctx=None):
    """Phase-locking value of the channels of every window (include/tdaeeg.h, "Phase-locking value") and its distance
    matrix: (dist (n_win, n_ch, n_ch), plv the same or None, status (n_win)).  sig (n_win, n_ch, n_t) or one window
    (n_ch, n_t); or, with the int64 tables win_start / win_ld (n_win each) and n_ch, n_t, a flat array whose row c of window w
    starts at element win_start[w] + c * win_ld[w].  The Hilbert transform is the window's own (scipy.signal.hilbert of the
    window).  A window with a sample that is not finite has NaN blocks and status TDA_WIN_NOT_FINITE.  ValueError for an
    unknown method, TdaError for n_ch outside [2, PLV_MAX_CHANNELS] or n_t outside [2, PLV_MAX_SAMPLES]."""
    from .preprocess import _hilbert_g
    m = plv_method(method)
    ctx = ctx or get_ctx()
    s, ws, wl, n_win, n_ch, n_t = _host_windows(sig, n_t, win_start, win_ld, n_ch)
    nc = max(n_ch, 0)
    dist = np.empty((n_win, nc, nc))
    plv = np.empty((n_win, nc, nc)) if want_plv else None
    status = np.zeros(n_win, np.int32)
    g = _hilbert_g(n_t) if n_t >= 1 else np.zeros(1)
    ctx.check(ctx.lib.tda_plv_dist_batch(ctx.h, ptr(s), ptr(ws), ptr(wl), n_win, n_ch, n_t, ptr(g), m, ptr(dist), ptr(plv),
                                         ptr(status)))
    return dist, plv, status


# the measures of tda_connectivity_dist_batch by name (include/tdaeeg.h, "Analytic-signal connectivity")
CONNECTIVITY_MEASURES = {"wpli": _lib.TDA_CONN_WPLI, "imcoh": _lib.TDA_CONN_IMCOH, "coh": _lib.TDA_CONN_COH,
                         "aec": _lib.TDA_CONN_AEC}


def connectivity_measure(name):
    """The measure number of an analytic-signal connectivity: one of CONNECTIVITY_MEASURES' names.  ValueError for anything
    else."""
    if not isinstance(name, str) or name not in CONNECTIVITY_MEASURES:
        raise ValueError(f"connectivity: one of {sorted(CONNECTIVITY_MEASURES)}, not {name!r}")
    return CONNECTIVITY_MEASURES[name]


def _dist_method(method):
    if not isinstance(method, str) or method not in DIST_METHODS:
        raise ValueError(f"connectivity: method one of {sorted(DIST_METHODS)}, not {method!r}")
    return DIST_METHODS[method]


def connectivity_dist_batch(sig, n_t=None, win_start=None, win_ld=None, n_ch=None, measure=None, method="euclidean",
                            want_value=True, ctx=None):
    """wPLI, imaginary coherency, coherence or envelope correlation of the channels of every window (include/tdaeeg.h,
    "Analytic-signal connectivity") and its distance matrix: (dist (n_win, n_ch, n_ch), value the same or None, status
    (n_win)).  measure: one of CONNECTIVITY_MEASURES' names.  sig and the tables as plv_dist_batch takes them; the analytic
    signal is the window's own.  A window with a sample that is not finite has NaN blocks and status TDA_WIN_NOT_FINITE.
    ValueError for an unknown measure or method, TdaError for n_ch outside [2, PLV_MAX_CHANNELS] or n_t outside
    [2, PLV_MAX_SAMPLES]."""
    from .preprocess import _hilbert_g
    k, m = connectivity_measure(measure), _dist_method(method)
    ctx = ctx or get_ctx()
    s, ws, wl, n_win, n_ch, n_t = _host_windows(sig, n_t, win_start, win_ld, n_ch)
    nc = max(n_ch, 0)
    dist = np.empty((n_win, nc, nc))
    value = np.empty((n_win, nc, nc)) if want_value else None
    status = np.zeros(n_win, np.int32)
    g = _hilbert_g(n_t) if n_t >= 1 else np.zeros(1)
    ctx.check(ctx.lib.tda_connectivity_dist_batch(ctx.h, ptr(s), ptr(ws), ptr(wl), n_win, n_ch, n_t, ptr(g), k, m, ptr(dist),
                                                  ptr(value), ptr(status)))
    return dist, value, status


def pack_labels(labels):
    """(n_perm, n) labels in {0, 1} -> the (TDA_PT_WORDS(n_perm), n) uint64 layout of tda_perm_sums_batch: bit p % 64 of
    word [p // 64][j] is labels[p][j]; the bits past n_perm are 0."""
    lab = np.asarray(labels)
    assert lab.ndim == 2, "labels must be (n_perm, n)"
    assert ((lab == 0) | (lab == 1)).all(), "labels must be 0 or 1"
    n_perm, n = lab.shape
    nw = _lib.pt_words(n_perm)
    bits = np.zeros((nw * 64, n), np.uint8)
    bits[:n_perm] = lab
    by = np.packbits(bits.reshape(nw, 8, 8, n), axis=2, bitorder="little")[:, :, 0, :]     # (nw, 8, n): byte k = bits 8k..8k+7
    return np.ascontiguousarray(by.transpose(0, 2, 1)).view("<u8").reshape(nw, n)


def _perm_shape(shape, n):
    assert len(shape) in (2, 3), "D must be (n_mat, n, ld) or (n, ld)"
    n_mat, rows, ld = (1,) + tuple(shape) if len(shape) == 2 else tuple(shape)
    assert rows == n, "D has another number of rows than the labels have items"
    return int(n_mat), int(ld)


def permutation_sums_batch(D, labels, ctx=None):
    """The sums of include/tdaeeg.h, "Two-sample permutation sums": D (n_mat, n, ld) float64 with ld >= n (or one matrix,
    (n, ld)), of which only the entries i < j < n are read; labels (n_perm, n) in {0, 1}.  Returns
    (sums (n_mat, 3, n_perm): S00, S11, S01 as the bytes of the written order; n1 (n_perm) int32).  TdaError for n outside
    [2, PT_MAX_ITEMS], no relabelling or more than PT_MAX_PERM."""
    ctx = ctx or get_ctx()
    lab = np.asarray(labels)
    assert lab.ndim == 2, "labels must be (n_perm, n)"
    n_perm, n = lab.shape
    d = f64(D)
    n_mat, ld = _perm_shape(d.shape, n)
    packed = pack_labels(lab) if n_perm else np.zeros((1, n), np.uint64)
    out = np.empty((n_mat, 3, n_perm))
    n1 = np.empty(n_perm, np.int32)
    ctx.check(ctx.lib.tda_perm_sums_batch(ctx.h, ptr(d), n_mat, n, ld, ptr(packed), n_perm, ptr(out), ptr(n1)))
    return out, n1


def tau_batch(windows, max_lag=None, ctx=None):
    ctx = ctx or get_ctx()
    w = f64(windows)
    n_win, n_t = w.shape
    tau = np.empty(n_win, np.int32)
    ctx.check(ctx.lib.tda_tau_batch(ctx.h, ptr(w), n_win, n_t, -1 if max_lag is None else int(max_lag), ptr(tau)))
    return tau


def _int_in(name, v, lo, hi):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= v <= hi:
        raise ValueError(f"{name} must be an integer in {lo}..{hi}, not {v!r}")
    return int(v)


def ami_args(n_t, max_lag=None, n_bins=16):
    """The parameters of the average mutual information as the kernel takes them (include/tdaeeg.h, "Delay and dimension
    selection"): (max_lag, n_bins) with max_lag resolved -- None or a negative value is n_t // 4, then the cut to n_t - 2 --
    so that a row of ami has max_lag + 1 entries.  ValueError, before any GPU call, for n_t outside 4..AMI_MAX_SAMPLES,
    n_bins outside 2..AMI_MAX_BINS or a max_lag that is no integer."""
    n_t = _int_in("n_t", n_t, 4, _lib.AMI_MAX_SAMPLES)
    n_bins = _int_in("n_bins", n_bins, 2, _lib.AMI_MAX_BINS)
    if max_lag is None:
        max_lag = -1
    if isinstance(max_lag, bool) or not isinstance(max_lag, (int, np.integer)):
        raise ValueError(f"max_lag must be an integer or None, not {max_lag!r}")
    max_lag = n_t // 4 if max_lag < 0 else int(max_lag)
    return min(max_lag, n_t - 2), n_bins


def fnn_args(n_t, d_max=5, theiler=1, r_tol=10.0, a_tol=2.0, frac_tol=0.05):
    """The parameters of the false nearest neighbours as the kernel takes them: (d_max, theiler, r_tol, a_tol, frac_tol).
    ValueError, before any GPU call, for n_t outside 4..FNN_MAX_SAMPLES, d_max outside 1..FNN_MAX_DIM, theiler outside
    1..n_t, r_tol or a_tol not > 0, frac_tol outside [0, 1]."""
    n_t = _int_in("n_t", n_t, 4, _lib.FNN_MAX_SAMPLES)
    d_max = _int_in("d_max", d_max, 1, _lib.FNN_MAX_DIM)
    theiler = _int_in("theiler", theiler, 1, n_t)
    tol = []
    for name, v in (("r_tol", r_tol), ("a_tol", a_tol), ("frac_tol", frac_tol)):
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)):
            raise ValueError(f"{name} must be a number, not {v!r}")
        tol.append(float(v))
    if not tol[0] > 0.0 or not tol[1] > 0.0:
        raise ValueError("r_tol and a_tol must be > 0")
    if not 0.0 <= tol[2] <= 1.0:
        raise ValueError("frac_tol must be in [0, 1]")
    return (d_max, theiler) + tuple(tol)


def ami_batch(windows, max_lag=None, n_bins=16, joint=False, ctx=None):
    """Average mutual information of every window with its own past and its first minimum (include/tdaeeg.h, "Delay and
    dimension selection"): windows (n_win, n_t) float64 -> (ami (n_win, max_lag + 1) float64 in nats, tau (n_win,) int32,
    joint (n_win, max_lag + 1, n_bins, n_bins) int32 or None, status) with max_lag as ami_args resolves it.  tau is 0
    without a minimum.  A window with a sample that is not finite has TDA_WIN_NOT_FINITE and NaN, a constant one
    TDA_WIN_DEGENERATE and 0.0."""
    w = f64(windows)
    if w.ndim != 2:
        raise ValueError("windows: (n_win, n_t)")
    n_win, n_t = w.shape
    lag, n_bins = ami_args(n_t, max_lag, n_bins)
    ctx = ctx or get_ctx()
    ami = np.zeros((n_win, lag + 1))
    tau, st = np.zeros(n_win, np.int32), np.zeros(n_win, np.int32)
    jnt = np.zeros((n_win, lag + 1, n_bins, n_bins), np.int32) if joint else None
    ctx.check(ctx.lib.tda_ami_batch(ctx.h, ptr(w), n_win, n_t, lag, n_bins, ptr(ami), ptr(tau), ptr(jnt), ptr(st)))
    return ami, tau, jnt, st


def fnn_batch(windows, taus, d_max=5, theiler=1, r_tol=10.0, a_tol=2.0, frac_tol=0.05, nn=False, ctx=None):
    """False nearest neighbours of the delay embeddings of dimension 1..d_max of every window (include/tdaeeg.h, "Delay and
    dimension selection"): windows (n_win, n_t) float64, taus one delay or one per window -> (counts (n_win, d_max, 4) int32
    with the columns _lib.FNN_COUNT_NAMES, frac (n_win, d_max) float64, dim (n_win,) int32, nn (n_win, d_max, n_t) int32 or
    None, status).  dim is 0 where no dimension has a fraction of at most frac_tol.  A window with tau < 1 has
    TDA_WIN_TOO_LARGE, one with n_t - tau < 2 TDA_WIN_DEGENERATE, and zeros."""
    w = f64(windows)
    if w.ndim != 2:
        raise ValueError("windows: (n_win, n_t)")
    n_win, n_t = w.shape
    par = fnn_args(n_t, d_max, theiler, r_tol, a_tol, frac_tol)
    ctx = ctx or get_ctx()
    tau = i32(np.broadcast_to(np.asarray(taus), (n_win,)))
    cnt = np.zeros((n_win, par[0], _lib.FNN_COLS), np.int32)
    frac = np.zeros((n_win, par[0]))
    dim, st = np.zeros(n_win, np.int32), np.zeros(n_win, np.int32)
    nbr = np.zeros((n_win, par[0], n_t), np.int32) if nn else None
    ctx.check(ctx.lib.tda_fnn_batch(ctx.h, ptr(w), ptr(tau), n_win, n_t, *par, ptr(cnt), ptr(frac), ptr(dim), ptr(nbr), ptr(st)))
    return cnt, frac, dim, nbr, st


def pack_diagrams(dgms, cap=None):
    """list of (k,2) arrays -> (n, cap, 2) float64 + counts."""
    arrs = [np.asarray(d, dtype=np.float64).reshape(-1, 2) if np.asarray(d).ndim == 2 and np.asarray(d).size
            else np.zeros((0, 2)) for d in dgms]
    cap = cap or max(1, max((a.shape[0] for a in arrs), default=1))
    rows = np.zeros((len(arrs), cap, 2))
    cnt = np.zeros(len(arrs), np.int32)
    for i, a in enumerate(arrs):
        assert a.shape[0] <= cap
        rows[i, :a.shape[0]] = a
        cnt[i] = a.shape[0]
    return rows, cnt


def features_batch(rows, cnt, ctx=None):
    ctx = ctx or get_ctx()
    rows = f64(rows); cnt = i32(cnt)
    n, cap, _ = rows.shape
    feat = np.empty((n, _lib.N_FEATURES))
    ctx.check(ctx.lib.tda_features_batch(ctx.h, ptr(rows), ptr(cnt), n, cap, ptr(feat)))
    return feat


def aggregate_batch(feat_h0, feat_h1, seg_off, ctx=None):
    ctx = ctx or get_ctx()
    f0 = f64(feat_h0); f1 = f64(feat_h1); off = i32(seg_off)
    n_seg = len(off) - 1
    out = np.empty((n_seg, 4 * _lib.N_FEATURES))
    ctx.check(ctx.lib.tda_aggregate_batch(ctx.h, ptr(f0), ptr(f1), ptr(off), n_seg, f0.shape[0], ptr(out)))
    return out


def segment_nanmean(x, seg_off, ctx=None):
    ctx = ctx or get_ctx()
    x = f64(x); off = i32(seg_off)
    out = np.empty(len(off) - 1)
    ctx.check(ctx.lib.tda_segment_nanmean(ctx.h, ptr(x), ptr(off), len(off) - 1, x.shape[0], ptr(out)))
    return out


SPEARMAN_FEATURES = ["mean_persistence", "total_persistence", "persistence_entropy", "max_persistence", "n_features"]
SPEARMAN_COLS = [6, 9, 10, 8, 0]          # their columns in the 11-feature vector (cmp:106-107)


def spearman_batch(feat_a, feat_b, seg_off, cols=SPEARMAN_COLS, ctx=None):
    """r (n_seg, len(cols)) and the two-sided p-value (scipy's Student-t formula on the host)."""
    ctx = ctx or get_ctx()
    fa = f64(feat_a); fb = f64(feat_b); off = i32(seg_off); cc = i32(cols)
    n_seg = len(off) - 1
    r = np.empty((n_seg, len(cc)))
    ctx.check(ctx.lib.tda_spearman_batch(ctx.h, ptr(fa), ptr(fb), fa.shape[0], fa.shape[1], ptr(cc), len(cc), ptr(off),
                                         n_seg, ptr(r)))
    from scipy import stats
    n = np.diff(off).astype(float)[:, None]
    dof = n - 2
    with np.errstate(divide="ignore", invalid="ignore"):
        t = r * np.sqrt((dof / ((r + 1.0) * (1.0 - r))).clip(0))
        p = 2 * stats.t.sf(np.abs(t), dof)
    # the reference reports r = 0, p = 1 for short or constant series (cmp:113-114)
    short = (n < 5) | (r == 0.0) & _degenerate(fa, fb, off, cc)
    p = np.where(short, 1.0, p)
    return r, p


def _degenerate(fa, fb, off, cols):
    out = np.zeros((len(off) - 1, len(cols)), bool)
    for s in range(len(off) - 1):
        a, b = off[s], off[s + 1]
        for k, c in enumerate(cols):
            out[s, k] = (b - a) < 5 or np.std(fa[a:b, c]) <= 1e-10 or np.std(fb[a:b, c]) <= 1e-10
    return out


def _check_cols(cols, ld):
    cc = i32(cols).ravel()
    if len(cc) == 0 or cc.min() < 0 or cc.max() >= ld:
        raise ValueError(f"feature columns {cc.tolist()} outside [0, {ld})")
    return cc


def temporal_corr_batch(feat_a, feat_b, seg_off, status_b=None, cols=SPEARMAN_COLS, ctx=None):
    """cmp:90-91,104-114 on the per-window H1 feature matrices of a step, (n_win, 11) each: per group (n_seg, 2 *
    len(cols)) = [r, p] per column over the windows whose audio status has neither TDA_WIN_DEGENERATE nor
    TDA_WIN_TOO_LARGE; NaN where none is left, (0, 1) under the reference's guard.  r and p both come from the device."""
    ctx = ctx or get_ctx()
    fa = f64(feat_a); fb = f64(feat_b); off = i32(seg_off)
    assert fa.ndim == 2 and fa.shape == fb.shape
    cc = _check_cols(cols, fa.shape[1])
    st = None if status_b is None else i32(status_b)
    assert st is None or st.shape == (fa.shape[0],)
    n_seg = len(off) - 1
    out = np.empty((n_seg, 2 * len(cc)))
    if fa.shape[0] == 0:                           # groups without a window: nothing to stage
        out.fill(np.nan)
        return out
    ctx.check(ctx.lib.tda_temporal_corr_batch(ctx.h, ptr(fa), ptr(fb), fa.shape[0], fa.shape[1], ptr(cc), len(cc), ptr(off),
                                              n_seg, ptr(st), ptr(out)))
    return out


def _pair_batch(entry, rows_a, cnt_a, rows_b, cnt_b, idx_a, idx_b, ctx, want_status, *extra):
    """The marshalling of the host-array pair distances: the entry point `entry` with `extra` arguments before out / status."""
    ra = f64(rows_a); rb = f64(rows_b); ca = i32(cnt_a); cb = i32(cnt_b)
    n_a, cap_a, _ = ra.shape
    n_b, cap_b, _ = rb.shape
    if idx_a is None and idx_b is None:
        assert n_a == n_b
        n_pairs = n_a
    else:
        n_pairs = len(idx_a if idx_a is not None else idx_b)
    ia = None if idx_a is None else i32(idx_a)
    ib = None if idx_b is None else i32(idx_b)
    out = np.empty(n_pairs); st = np.empty(n_pairs, np.int32)
    ctx.check(entry(ctx.h, ptr(ra), ptr(ca), n_a, cap_a, ptr(rb), ptr(cb), n_b, cap_b, ptr(ia), ptr(ib), n_pairs, *extra, ptr(out),
                    ptr(st)))
    return (out, st) if want_status else out


def wasserstein_batch(rows_a, cnt_a, rows_b, cnt_b, idx_a=None, idx_b=None, ctx=None, want_status=False):
    ctx = ctx or get_ctx()
    return _pair_batch(ctx.lib.tda_wasserstein_batch, rows_a, cnt_a, rows_b, cnt_b, idx_a, idx_b, ctx, want_status)


def bottleneck_batch(rows_a, cnt_a, rows_b, cnt_b, idx_a=None, idx_b=None, ctx=None, want_status=False):
    """Bottleneck distance of diagram pairs (include/tdaeeg.h: L-infinity ground cost, (d - b) / 2 to the diagonal, the
    largest matched cost under the best matching); arguments and results as wasserstein_batch."""
    ctx = ctx or get_ctx()
    return _pair_batch(ctx.lib.tda_bottleneck_batch, rows_a, cnt_a, rows_b, cnt_b, idx_a, idx_b, ctx, want_status)


GROUNDS = {"l2": _lib.TDA_GROUND_L2, "linf": _lib.TDA_GROUND_LINF}


def wasserstein_q_args(order, ground):
    """(order, ground constant) of a Wasserstein distance as the kernels take them: order 1 or 2, ground "l2" or "linf".
    TdaError, before any GPU call, for anything else."""
    if isinstance(order, bool) or order not in (1, 2):
        raise _lib.TdaError(f"wasserstein_q: order must be 1 or 2, not {order!r}")
    if not isinstance(ground, str) or ground not in GROUNDS:
        raise _lib.TdaError(f"wasserstein_q: ground must be 'l2' or 'linf', not {ground!r}")
    return int(order), GROUNDS[ground]


def wasserstein_q_batch(rows_a, cnt_a, rows_b, cnt_b, idx_a=None, idx_b=None, order=2, ground="l2", ctx=None, want_status=False):
    """Wasserstein distance of order 1 or 2 of diagram pairs with the L2 ((d - b) / sqrt 2 to the diagonal) or the
    L-infinity ((d - b) / 2) ground metric (include/tdaeeg.h); arguments and results as wasserstein_batch."""
    order, ground = wasserstein_q_args(order, ground)
    ctx = ctx or get_ctx()
    return _pair_batch(ctx.lib.tda_wasserstein_q_batch, rows_a, cnt_a, rows_b, cnt_b, idx_a, idx_b, ctx, want_status, order, ground)


def landscape_batch(rows, cnt, grid, levels, ctx=None):
    """Persistence landscape and Betti curve of every diagram (include/tdaeeg.h): rows (n, cap, 2), cnt (n,), grid
    (n_grid,) float64 -> (n, levels + 1, n_grid): levels 1..levels, then the Betti curve."""
    ctx = ctx or get_ctx()
    rows = f64(rows); cnt = i32(cnt); grid = f64(grid)
    n, cap, _ = rows.shape
    assert grid.ndim == 1
    levels = int(levels)
    out = np.empty((n, max(levels, 0) + 1, grid.shape[0]))
    ctx.check(ctx.lib.tda_landscape_batch(ctx.h, ptr(rows), ptr(cnt), n, cap, ptr(grid), grid.shape[0], levels, ptr(out)))
    return out


def euler_args(grid, max_dim):
    """The parameters of an Euler characteristic curve as the kernel takes them (include/tdaeeg.h, "Euler characteristic
    curves"): (grid, max_dim) with grid a contiguous 1-D float64 array of 1..MAX_GRID values (any values, any order: a NaN
    grid point holds no edge) and max_dim an int in 1..EC_MAX_DIM.  ValueError, before any GPU call, for anything else."""
    try:
        grid = np.asarray(grid, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("grid: the scales are a 1-D float64 array") from None
    if grid.ndim != 1 or not 1 <= grid.shape[0] <= _lib.MAX_GRID:
        raise ValueError(f"grid: 1..{_lib.MAX_GRID} scales in a 1-D array")
    grid = np.ascontiguousarray(grid)
    if isinstance(max_dim, bool) or not isinstance(max_dim, (int, np.integer)) or not 1 <= max_dim <= _lib.EC_MAX_DIM:
        raise ValueError(f"max_dim must be an integer in 1..{_lib.EC_MAX_DIM}, not {max_dim!r}")
    return grid, int(max_dim)


def euler_dm_batch(dms, grid, max_dim=3, thresh=MAX_EDGE_LENGTH, symmetrise=True, ctx=None):
    """Simplex counts f_0 .. f_max_dim and the Euler characteristic of the Rips complex of every distance matrix at every
    scale of grid (include/tdaeeg.h): dms (n_win, n, n) float64 -> (counts (n_win, max_dim + 2, n_grid) int32, status)."""
    grid, max_dim = euler_args(grid, max_dim)
    ctx = ctx or get_ctx()
    d = f64(dms)
    n_win, n, n2 = d.shape
    assert n == n2, "distance matrices must be square"
    out = np.zeros((n_win, max_dim + 2, grid.shape[0]), np.int32); st = np.zeros(n_win, np.int32)
    ctx.check(ctx.lib.tda_euler_dm_batch(ctx.h, ptr(d), n_win, n, float(thresh), int(bool(symmetrise)), ptr(grid),
                                         grid.shape[0], max_dim, ptr(out), ptr(st)))
    return out, st


def euler_cloud_batch(clouds, grid, max_dim=3, n_pts=None, normalise=True, thresh=MAX_EDGE_LENGTH, ctx=None):
    """The same from explicit clouds (n_win, p_cap, dim) with n_pts rows each, by the keys of cloud_rips_batch.  A window
    with fewer than 3 or more than min(p_cap, MAX_POINTS) points has TDA_WIN_DEGENERATE / TDA_WIN_TOO_LARGE and zeros."""
    grid, max_dim = euler_args(grid, max_dim)
    ctx = ctx or get_ctx()
    pc = f64(clouds)
    n_win, p_cap, dim = pc.shape
    n_pts = i32(np.full(n_win, p_cap) if n_pts is None else n_pts)
    out = np.zeros((n_win, max_dim + 2, grid.shape[0]), np.int32); st = np.zeros(n_win, np.int32)
    ctx.check(ctx.lib.tda_euler_cloud_batch(ctx.h, ptr(pc), ptr(n_pts), n_win, p_cap, dim, int(bool(normalise)), float(thresh),
                                            ptr(grid), grid.shape[0], max_dim, ptr(out), ptr(st)))
    return out, st


def euler_takens_batch(windows, taus, grid, max_dim=3, dim=3, subsample=2, thresh=MAX_EDGE_LENGTH, ctx=None):
    """The same from audio windows (n_win, n_t) and their delays, by the keys of takens_rips_batch: (counts, n_points,
    status)."""
    grid, max_dim = euler_args(grid, max_dim)
    ctx = ctx or get_ctx()
    w = f64(windows)
    n_win, n_t = w.shape
    tau = i32(np.broadcast_to(np.asarray(taus), (n_win,)))
    out = np.zeros((n_win, max_dim + 2, grid.shape[0]), np.int32)
    npts = np.zeros(n_win, np.int32); st = np.zeros(n_win, np.int32)
    ctx.check(ctx.lib.tda_euler_takens_batch(ctx.h, ptr(w), ptr(tau), n_win, n_t, int(dim), int(subsample), float(thresh),
                                             ptr(grid), grid.shape[0], max_dim, ptr(out), ptr(npts), ptr(st)))
    return out, npts, st


def network_args(grid):
    """The grid of the network curves as the kernel takes it (include/tdaeeg.h, "Network curves"): a contiguous 1-D float64
    array of 1..MAX_GRID values, any values in any order, with the refusals of euler_args.  ValueError, before any GPU
    call, for anything else."""
    return euler_args(grid, 1)[0]


def _network_host(n_win, n_grid, n_node, nodal):
    """The zeroed host outputs of the network_*_batch forms: counts, measures, nodal (or None), status."""
    return (np.zeros((n_win, _lib.NET_ROWS, n_grid), np.int32), np.zeros((n_win, _lib.NET_MEASURES, n_grid), np.float64),
            np.zeros((n_win, _lib.NET_NODAL, n_grid, n_node), np.int32) if nodal else None, np.zeros(n_win, np.int32))


def network_dm_batch(dms, grid, nodal=False, thresh=MAX_EDGE_LENGTH, symmetrise=True, ctx=None):
    """The graph measures of the thresholded graph of every distance matrix at every scale of grid (include/tdaeeg.h,
    "Network curves"): dms (n_win, n, n) float64 -> (counts (n_win, NET_ROWS, n_grid) int32, measures (n_win, NET_MEASURES,
    n_grid) float64, nodal (n_win, NET_NODAL, n_grid, n) int32 or None, status).  The rows are named by
    _lib.NET_COUNT_NAMES, NET_MEASURE_NAMES and NET_NODAL_NAMES."""
    grid = network_args(grid)
    ctx = ctx or get_ctx()
    d = f64(dms)
    n_win, n, n2 = d.shape
    assert n == n2, "distance matrices must be square"
    cnt, mea, nod, st = _network_host(n_win, grid.shape[0], n, nodal)
    ctx.check(ctx.lib.tda_network_dm_batch(ctx.h, ptr(d), n_win, n, float(thresh), int(bool(symmetrise)), ptr(grid),
                                           grid.shape[0], ptr(cnt), ptr(mea), ptr(nod), ptr(st)))
    return cnt, mea, nod, st


def network_cloud_batch(clouds, grid, nodal=False, n_pts=None, normalise=True, thresh=MAX_EDGE_LENGTH, ctx=None):
    """The same from explicit clouds (n_win, p_cap, dim) with n_pts rows each, by the keys of cloud_rips_batch; nodal has
    p_cap columns.  A window with fewer than 3 or more than min(p_cap, MAX_POINTS) points has TDA_WIN_DEGENERATE /
    TDA_WIN_TOO_LARGE and zeros."""
    grid = network_args(grid)
    ctx = ctx or get_ctx()
    pc = f64(clouds)
    n_win, p_cap, dim = pc.shape
    n_pts = i32(np.full(n_win, p_cap) if n_pts is None else n_pts)
    cnt, mea, nod, st = _network_host(n_win, grid.shape[0], p_cap, nodal)
    ctx.check(ctx.lib.tda_network_cloud_batch(ctx.h, ptr(pc), ptr(n_pts), n_win, p_cap, dim, int(bool(normalise)),
                                              float(thresh), ptr(grid), grid.shape[0], ptr(cnt), ptr(mea),
                                              ptr(nod), ptr(st)))
    return cnt, mea, nod, st


def network_takens_batch(windows, taus, grid, nodal=False, dim=3, subsample=2, thresh=MAX_EDGE_LENGTH, ctx=None):
    """The same from audio windows (n_win, n_t) and their delays, by the keys of takens_rips_batch: (counts, measures,
    nodal with MAX_POINTS columns or None, n_points, status)."""
    grid = network_args(grid)
    ctx = ctx or get_ctx()
    w = f64(windows)
    n_win, n_t = w.shape
    tau = i32(np.broadcast_to(np.asarray(taus), (n_win,)))
    cnt, mea, nod, st = _network_host(n_win, grid.shape[0], _lib.MAX_POINTS, nodal)
    npts = np.zeros(n_win, np.int32)
    ctx.check(ctx.lib.tda_network_takens_batch(ctx.h, ptr(w), ptr(tau), n_win, n_t, int(dim), int(subsample), float(thresh),
                                               ptr(grid), grid.shape[0], ptr(cnt), ptr(mea), ptr(nod),
                                               ptr(npts), ptr(st)))
    return cnt, mea, nod, npts, st


def recurrence_args(grid, theiler=1, l_min=2, v_min=2):
    """The parameters of the recurrence curves as the kernel takes them (include/tdaeeg.h, "Recurrence curves"): (grid,
    theiler, l_min, v_min) with grid as network_args takes it and the three others ints in 1..MAX_POINTS.  ValueError,
    before any GPU call, for anything else."""
    grid = network_args(grid)
    out = []
    for name, v in (("theiler", theiler), ("l_min", l_min), ("v_min", v_min)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 1 <= v <= _lib.MAX_POINTS:
            raise ValueError(f"{name} must be an integer in 1..{_lib.MAX_POINTS}, not {v!r}")
        out.append(int(v))
    return (grid,) + tuple(out)


def _recurrence_host(n_win, n_grid, n_hist, hist):
    """The zeroed host outputs of the recurrence_*_batch forms: counts, measures, hist (or None), status."""
    return (np.zeros((n_win, _lib.RQA_ROWS, n_grid), np.int32), np.zeros((n_win, _lib.RQA_MEASURES, n_grid), np.float64),
            np.zeros((n_win, 2, n_grid, n_hist), np.int32) if hist else None, np.zeros(n_win, np.int32))


def recurrence_dm_batch(dms, grid, theiler=1, l_min=2, v_min=2, hist=False, thresh=MAX_EDGE_LENGTH, symmetrise=True,
                        ctx=None):
    """Recurrence quantification of every distance matrix at every scale of grid (include/tdaeeg.h, "Recurrence curves"):
    dms (n_win, n, n) float64, the vertices in time order -> (counts (n_win, RQA_ROWS, n_grid) int32, measures (n_win,
    RQA_MEASURES, n_grid) float64, hist (n_win, 2, n_grid, n) int32 or None, status).  The rows are named by
    _lib.RQA_COUNT_NAMES and RQA_MEASURE_NAMES; hist[:, 0, :, l - 1] and hist[:, 1, :, l - 1] count the diagonal and the
    vertical lines of length l."""
    grid, theiler, l_min, v_min = recurrence_args(grid, theiler, l_min, v_min)
    ctx = ctx or get_ctx()
    d = f64(dms)
    n_win, n, n2 = d.shape
    assert n == n2, "distance matrices must be square"
    cnt, mea, his, st = _recurrence_host(n_win, grid.shape[0], n, hist)
    ctx.check(ctx.lib.tda_recurrence_dm_batch(ctx.h, ptr(d), n_win, n, float(thresh), int(bool(symmetrise)), ptr(grid),
                                              grid.shape[0], theiler, l_min, v_min, ptr(cnt), ptr(mea), ptr(his), ptr(st)))
    return cnt, mea, his, st


def recurrence_cloud_batch(clouds, grid, theiler=1, l_min=2, v_min=2, hist=False, n_pts=None, normalise=True,
                           thresh=MAX_EDGE_LENGTH, ctx=None):
    """The same from explicit clouds (n_win, p_cap, dim) with n_pts rows each in time order, by the keys of
    cloud_rips_batch; hist has p_cap columns.  A window with fewer than 3 or more than min(p_cap, MAX_POINTS) points has
    TDA_WIN_DEGENERATE / TDA_WIN_TOO_LARGE and zeros."""
    grid, theiler, l_min, v_min = recurrence_args(grid, theiler, l_min, v_min)
    ctx = ctx or get_ctx()
    pc = f64(clouds)
    n_win, p_cap, dim = pc.shape
    n_pts = i32(np.full(n_win, p_cap) if n_pts is None else n_pts)
    cnt, mea, his, st = _recurrence_host(n_win, grid.shape[0], p_cap, hist)
    ctx.check(ctx.lib.tda_recurrence_cloud_batch(ctx.h, ptr(pc), ptr(n_pts), n_win, p_cap, dim, int(bool(normalise)),
                                                 float(thresh), ptr(grid), grid.shape[0], theiler, l_min, v_min, ptr(cnt),
                                                 ptr(mea), ptr(his), ptr(st)))
    return cnt, mea, his, st


def recurrence_takens_batch(windows, taus, grid, theiler=1, l_min=2, v_min=2, hist=False, dim=3, subsample=2,
                            thresh=MAX_EDGE_LENGTH, ctx=None):
    """The same from signal windows (n_win, n_t) and their delays, by the keys of takens_rips_batch: (counts, measures,
    hist with MAX_POINTS columns or None, n_points, status).  One step of a line is `subsample` samples."""
    grid, theiler, l_min, v_min = recurrence_args(grid, theiler, l_min, v_min)
    ctx = ctx or get_ctx()
    w = f64(windows)
    n_win, n_t = w.shape
    tau = i32(np.broadcast_to(np.asarray(taus), (n_win,)))
    cnt, mea, his, st = _recurrence_host(n_win, grid.shape[0], _lib.MAX_POINTS, hist)
    npts = np.zeros(n_win, np.int32)
    ctx.check(ctx.lib.tda_recurrence_takens_batch(ctx.h, ptr(w), ptr(tau), n_win, n_t, int(dim), int(subsample),
                                                  float(thresh), ptr(grid), grid.shape[0], theiler, l_min, v_min, ptr(cnt),
                                                  ptr(mea), ptr(his), ptr(npts), ptr(st)))
    return cnt, mea, his, npts, st


def generators_args(cyc_cap):
    """The cycle capacity of the generators entry points as the kernel takes it (include/tdaeeg.h, "Generators and
    representative cycles"): an int in 4..MAX_POINTS.  ValueError, before any GPU call, for anything else."""
    if isinstance(cyc_cap, bool) or not isinstance(cyc_cap, (int, np.integer)) or not 4 <= cyc_cap <= _lib.MAX_POINTS:
        raise ValueError(f"cyc_cap must be an integer in 4..{_lib.MAX_POINTS}, not {cyc_cap!r}")
    return int(cyc_cap)


def _gen_host(n_win, n_part, h0, c0, h1, c1, cyc_cap, rips_status, want_part, want_h0, want_work):
    """Row inputs and output arrays of the host forms -> (dict of outputs, the shared C arguments without skip_mask)."""
    cyc_cap = generators_args(cyc_cap)
    h1 = f64(h1); c1 = i32(c1)
    if h1.ndim != 3 or h1.shape[0] != n_win or h1.shape[2] != 2 or h1.shape[1] < 1 or c1.shape != (n_win,):
        raise ValueError("h1: (n_win, h1_cap >= 1, 2) rows and (n_win,) counts")
    h1_cap = h1.shape[1]
    h0_cap = 0
    if h0 is not None:
        h0 = f64(h0); c0 = i32(c0)
        if h0.ndim != 3 or h0.shape[0] != n_win or h0.shape[2] != 2 or h0.shape[1] < 1 or c0.shape != (n_win,):
            raise ValueError("h0: (n_win, h0_cap >= 1, 2) rows and (n_win,) counts")
        h0_cap = h0.shape[1]
    else:
        c0, want_h0 = None, False
    rs = None if rips_status is None else i32(rips_status)
    out = dict(h1_gen=np.empty((n_win, h1_cap, 4), np.int16), h1_flag=np.empty((n_win, h1_cap), np.int32),
               cyc=np.empty((n_win, h1_cap, cyc_cap), np.int16), cyc_len=np.empty((n_win, h1_cap), np.int32),
               status=np.empty(n_win, np.int32))
    if want_part:
        out["part"] = np.empty((n_win, n_part), np.float64)
    if want_h0:
        out["h0_edge"] = np.empty((n_win, h0_cap, 2), np.int16)
    if want_work:
        out["work"] = np.empty((n_win, 4, 2), np.int32)
    rows = (ptr(h0), h0_cap, ptr(c0), ptr(h1), h1_cap, ptr(c1), ptr(rs))
    outs = (cyc_cap, ptr(out["h1_gen"]), ptr(out["h1_flag"]), ptr(out["cyc"]), ptr(out["cyc_len"]), ptr(out.get("part")),
            ptr(out.get("h0_edge")), ptr(out.get("work")))
    return out, rows, outs


def generators_dm_batch(dms, h0, c0, h1, c1, thresh=MAX_EDGE_LENGTH, symmetrise=True, cyc_cap=_lib.MAX_POINTS,
                        rips_status=None, skip_mask=0, part=True, h0_edge=True, work=False, ctx=None):
    """The edges behind the rows of rips_dm_batch(dms, ..., raw=True) and a representative cycle of every H1 row
    (include/tdaeeg.h): dms (n_win, n, n) float64, h0 / c0 (or None) and h1 / c1 the raw rows and counts -> a dict of
    h1_gen (n_win, h1_cap, 4) int16, h1_flag, cyc (n_win, h1_cap, cyc_cap) int16, cyc_len, status and, when asked for,
    part (n_win, n) float64, h0_edge (n_win, h0_cap, 2) int16, work."""
    ctx = ctx or get_ctx()
    d = f64(dms)
    n_win, n, n2 = d.shape
    assert n == n2, "distance matrices must be square"
    out, rows, outs = _gen_host(n_win, n, h0, c0, h1, c1, cyc_cap, rips_status, part, h0_edge, work)
    ctx.check(ctx.lib.tda_generators_dm_batch(ctx.h, ptr(d), n_win, n, float(thresh), int(bool(symmetrise)), *rows,
                                              int(skip_mask), *outs, ptr(out["status"])))
    return out


def generators_cloud_batch(clouds, h0, c0, h1, c1, n_pts=None, normalise=True, thresh=MAX_EDGE_LENGTH,
                           cyc_cap=_lib.MAX_POINTS, rips_status=None, skip_mask=0, part=True, h0_edge=True, work=False,
                           ctx=None):
    """The same for the rows of cloud_rips_batch(clouds, ..., raw=True), by its keys; part has p_cap columns."""
    ctx = ctx or get_ctx()
    pc = f64(clouds)
    n_win, p_cap, dim = pc.shape
    n_pts = i32(np.full(n_win, p_cap) if n_pts is None else n_pts)
    out, rows, outs = _gen_host(n_win, p_cap, h0, c0, h1, c1, cyc_cap, rips_status, part, h0_edge, work)
    ctx.check(ctx.lib.tda_generators_cloud_batch(ctx.h, ptr(pc), ptr(n_pts), n_win, p_cap, dim, int(bool(normalise)),
                                                 float(thresh), *rows, int(skip_mask), *outs, ptr(out["status"])))
    return out


def generators_takens_batch(windows, taus, h0, c0, h1, c1, dim=3, subsample=2, thresh=MAX_EDGE_LENGTH,
                            cyc_cap=_lib.MAX_POINTS, rips_status=None, skip_mask=0, part=True, h0_edge=True, work=False,
                            ctx=None):
    """The same for the rows of takens_rips_batch(windows, taus, ..., raw=True); part has MAX_POINTS columns and the dict
    also holds n_points."""
    ctx = ctx or get_ctx()
    w = f64(windows)
    n_win, n_t = w.shape
    tau = i32(np.broadcast_to(np.asarray(taus), (n_win,)))
    out, rows, outs = _gen_host(n_win, _lib.MAX_POINTS, h0, c0, h1, c1, cyc_cap, rips_status, part, h0_edge, work)
    out["n_points"] = np.empty(n_win, np.int32)
    ctx.check(ctx.lib.tda_generators_takens_batch(ctx.h, ptr(w), ptr(tau), n_win, n_t, int(dim), int(subsample), float(thresh),
                                                  *rows, int(skip_mask), *outs, ptr(out["n_points"]), ptr(out["status"])))
    return out


def image_args(xe, ye, sigma, power):
    """The parameters of a persistence image as the kernels take them: (xe, ye) contiguous 1-D float64, float sigma, int
    power.  ValueError, before any GPU call, for edges that are not finite and strictly ascending or give a side outside
    1..MAX_IMAGE_SIDE, a sigma that is not finite and > 0, a power outside {0, 1, 2}."""
    edges = []
    for name, e in (("xe", xe), ("ye", ye)):
        try:
            e = np.ascontiguousarray(e, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError(f"{name}: the edges are a 1-D float64 array") from None
        if e.ndim != 1 or not 2 <= e.shape[0] <= _lib.MAX_IMAGE_SIDE + 1:
            raise ValueError(f"{name}: 2..{_lib.MAX_IMAGE_SIDE + 1} edges (1..{_lib.MAX_IMAGE_SIDE} pixels) in a 1-D array")
        if not np.isfinite(e).all() or not (np.diff(e) > 0).all():
            raise ValueError(f"{name}: the edges must be finite and strictly ascending")
        edges.append(e)
    try:
        sigma = float(sigma)
    except (TypeError, ValueError):
        raise ValueError("sigma must be a finite number > 0") from None
    if not np.isfinite(sigma) or not sigma > 0:
        raise ValueError("sigma must be a finite number > 0")
    if isinstance(power, bool) or power not in (0, 1, 2):
        raise ValueError("power must be 0, 1 or 2")
    return edges[0], edges[1], sigma, int(power)


def image_batch(rows, cnt, xe, ye, sigma, power=1, ctx=None):
    """Persistence image of every diagram (include/tdaeeg.h): rows (n, cap, 2), cnt (n,), xe (n_x + 1,) birth edges, ye
    (n_y + 1,) persistence edges, float64 -> (n, n_y, n_x).  Edges that are not finite and strictly ascending, a sigma that
    is not finite and > 0 or a power outside {0, 1, 2} are a TdaError."""
    ctx = ctx or get_ctx()
    rows = f64(rows); cnt = i32(cnt); xe = f64(xe); ye = f64(ye)
    n, cap, _ = rows.shape
    assert xe.ndim == 1 and ye.ndim == 1
    n_x, n_y = xe.shape[0] - 1, ye.shape[0] - 1
    out = np.empty((n, max(n_y, 0), max(n_x, 0)))
    ctx.check(ctx.lib.tda_image_batch(ctx.h, ptr(rows), ptr(cnt), n, cap, ptr(xe), n_x, ptr(ye), n_y, float(sigma), int(power),
                                      ptr(out)))
    return out


def frechet_args(cap_out, max_iter):
    """(cap_out, max_iter) of a Frechet mean as the kernel takes them: cap_out >= 1, 1 <= max_iter <= FM_MAX_ITER.
    TdaError, before any GPU call, for anything else."""
    for name, v, hi in (("cap_out", cap_out, None), ("max_iter", max_iter, _lib.FM_MAX_ITER)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 1 or (hi is not None and v > hi):
            raise _lib.TdaError(f"frechet_mean: {name} must be an integer >= 1{'' if hi is None else f' and <= {hi}'}, not {v!r}")
    return int(cap_out), int(max_iter)


def frechet_mean_batch(rows, cnt, seg_off=None, status=None, skip_mask=0, max_iter=32, cap_out=None, ctx=None):
    """Frechet mean and Frechet variance of every group of diagrams in the order-2 Wasserstein metric (include/tdaeeg.h):
    rows (n, cap, 2), cnt (n,), seg_off (n_seg + 1,) int32 or None (every diagram its own group); diagrams whose status
    word has a bit of skip_mask are left out.  Returns mean (n_seg, cap_out, 2) with NaN beyond the count, count, variance,
    iters and status, (n_seg,) each.  cap_out defaults to FM_MAX_POINTS."""
    cap_out, max_iter = frechet_args(_lib.FM_MAX_POINTS if cap_out is None else cap_out, max_iter)
    ctx = ctx or get_ctx()
    rows = f64(rows); cnt = i32(cnt)
    n, cap, _ = rows.shape
    off = None if seg_off is None else i32(seg_off)
    st_in = None if status is None else i32(status)
    assert st_in is None or st_in.shape == (n,)
    n_seg = n if off is None else len(off) - 1
    mean = np.empty((n_seg, cap_out, 2)); mc = np.empty(n_seg, np.int32); var = np.empty(n_seg)
    it = np.empty(n_seg, np.int32); st = np.empty(n_seg, np.int32)
    ctx.check(ctx.lib.tda_frechet_mean_batch(ctx.h, ptr(rows), ptr(cnt), n, cap, ptr(off), n_seg, ptr(st_in), int(skip_mask),
                                             max_iter, ptr(mean), ptr(mc), cap_out, ptr(var), ptr(it), ptr(st)))
    mean[np.arange(cap_out)[None, :] >= mc[:, None]] = np.nan
    return mean, mc, var, it, st


def _directions(dirs):
    """The (M, 2) float64 direction table of the sliced Wasserstein entry points, validated on the host."""
    d = np.asarray(dirs, dtype=np.float64)
    if d.ndim != 2 or d.shape[1] != 2:
        raise _lib.TdaError("libtdaeeg error 1: dirs must have shape (M, 2)")
    if not 1 <= d.shape[0] <= _lib.MAX_DIRECTIONS:
        raise _lib.TdaError("libtdaeeg error 1: 1 <= M <= TDA_MAX_DIRECTIONS directions")
    if not np.isfinite(d).all():
        raise _lib.TdaError("libtdaeeg error 1: directions must be finite")
    return np.ascontiguousarray(d)


def sliced_wasserstein_batch(rows_a, cnt_a, rows_b, cnt_b, dirs, idx_a=None, idx_b=None, ctx=None, want_status=False):
    """Sliced Wasserstein distance of diagram pairs over the (M, 2) direction table `dirs` (include/tdaeeg.h: both diagrams
    augmented with the other's diagonal images, projected as (c * x) + (s * y), sorted, L1 difference, mean over the
    directions); the other arguments and the results as wasserstein_batch.  A pair with more than TDA_SW_MAX_POINTS
    points in all is NaN with status TDA_WIN_TOO_LARGE."""
    ctx = ctx or get_ctx()
    d = _directions(dirs)
    return _pair_batch(ctx.lib.tda_sliced_wasserstein_batch, rows_a, cnt_a, rows_b, cnt_b, idx_a, idx_b, ctx, want_status, ptr(d),
                       d.shape[0])


def sliced_wasserstein_gram(rows, cnt, dirs, ctx=None):
    """(n, n) symmetric matrix of the sliced Wasserstein distances of one set of diagrams: the pairs i < j in one batched
    call, mirrored; the diagonal is 0.0.  NaN where a pair has a status."""
    n = len(cnt)
    iu, ju = np.triu_indices(n, 1)
    G = np.zeros((n, n))
    if len(iu):
        d = sliced_wasserstein_batch(rows, cnt, rows, cnt, dirs, idx_a=iu, idx_b=ju, ctx=ctx)
        G[iu, ju] = d
        G[ju, iu] = d
    else:
        _directions(dirs)
    return G


def diagram_kernel_args(kernel):
    """(ninv, mirror, scale, weight, wc) of a kernel on diagrams as the entry points take them (include/tdaeeg.h):
      ("pss", sigma)     persistence scale-space kernel: ninv = -1 / (8 sigma), mirror 1, scale 1 / (8 pi sigma), weight 1
      ("pwg", sigma, c)  persistence weighted Gaussian kernel: ninv = -1 / (2 sigma^2), mirror 0, scale 1, weight
                         atan(c * persistence)
    sigma and c are finite numbers > 0.  TdaError, before any GPU call, for anything else."""
    def num(v):
        return not isinstance(v, bool) and isinstance(v, (int, float, np.integer, np.floating)) and np.isfinite(v) and v > 0
    bad = _lib.TdaError(f"diagram kernel: ('pss', sigma) or ('pwg', sigma, c) with finite sigma, c > 0, not {kernel!r}")
    if not isinstance(kernel, (tuple, list)) or len(kernel) < 2 or not isinstance(kernel[0], str) or not all(num(v) for v in kernel[1:]):
        raise bad
    try:
        if kernel[0] == "pss" and len(kernel) == 2:
            sigma = float(kernel[1])
            args = (-1.0 / (8.0 * sigma), 1, 1.0 / (8.0 * np.pi * sigma), _lib.TDA_KW_ONE, 0.0)
        elif kernel[0] == "pwg" and len(kernel) == 3:
            sigma, c = float(kernel[1]), float(kernel[2])
            args = (-1.0 / (2.0 * sigma * sigma), 0, 1.0, _lib.TDA_KW_ATAN, c)
        else:
            raise bad
    except ZeroDivisionError:                        # sigma * sigma underflows
        raise bad from None
    if not (np.isfinite(args[0]) and args[0] < 0 and np.isfinite(args[2])):
        raise bad                                    # a sigma so small or so large that ninv or scale is not a finite number < 0
    return args


def _kernel_params(kernel):
    """`kernel` as the five parameters: a named kernel through diagram_kernel_args, or the five values themselves
    (ninv, mirror, scale, weight, wc), which the library checks."""
    if isinstance(kernel, (tuple, list)) and len(kernel) == 5 and not isinstance(kernel[0], str):
        ninv, mirror, scale, weight, wc = kernel
        return float(ninv), int(mirror), float(scale), int(weight), float(wc)
    return diagram_kernel_args(kernel)


def diagram_kernel_batch(rows_a, cnt_a, rows_b, cnt_b, kernel, idx_a=None, idx_b=None, ctx=None, want_status=False):
    """Kernel values and kernel-induced distances of diagram pairs (include/tdaeeg.h): `kernel` as diagram_kernel_args
    takes it (or the five raw parameters); the other arguments as wasserstein_batch.  Returns (dist (n_pairs,), kvals
    (n_pairs, 3) = [k_ab, k_aa, k_bb]) and, with want_status, the status words: a pair whose index is outside its set is
    NaN with TDA_WIN_NO_PAIR."""
    par = _kernel_params(kernel)
    ctx = ctx or get_ctx()
    ra = f64(rows_a); rb = f64(rows_b); ca = i32(cnt_a); cb = i32(cnt_b)
    n_a, cap_a, _ = ra.shape
    n_b, cap_b, _ = rb.shape
    if idx_a is None and idx_b is None:
        assert n_a == n_b
        n_pairs = n_a
    else:
        n_pairs = len(idx_a if idx_a is not None else idx_b)
    ia = None if idx_a is None else i32(idx_a)
    ib = None if idx_b is None else i32(idx_b)
    out = np.empty(n_pairs); kv = np.empty((n_pairs, 3)); st = np.empty(n_pairs, np.int32)
    ctx.check(ctx.lib.tda_diagram_kernel_pairs(ctx.h, ptr(ra), ptr(ca), n_a, cap_a, ptr(rb), ptr(cb), n_b, cap_b, ptr(ia), ptr(ib),
                                               n_pairs, *par, ptr(out), ptr(kv), ptr(st)))
    return (out, kv, st) if want_status else (out, kv)


def diagram_kernel_gram(rows_a, cnt_a, kernel, seg_off_a=None, status_a=None, rows_b=None, cnt_b=None, seg_off_b=None,
                        status_b=None, skip_mask=0, ctx=None):
    """Gram matrix of the mean embeddings of groups of diagrams (include/tdaeeg.h): G[g, h] = the average of the kernel
    over all pairs of a kept diagram of group g and one of group h; NaN for a group without a kept diagram.  seg_off
    (n_seg + 1,) int32 or None (every diagram its own group); diagrams whose status word has a bit of skip_mask are left
    out.  Without rows_b the matrix of set A against itself, symmetric as bytes; with it the (n_seg_a, n_seg_b) cross
    matrix."""
    par = _kernel_params(kernel)
    ctx = ctx or get_ctx()
    ra = f64(rows_a); ca = i32(cnt_a)
    n_a, cap_a, _ = ra.shape
    oa = None if seg_off_a is None else i32(seg_off_a)
    sa = None if status_a is None else i32(status_a)
    n_ga = n_a if oa is None else len(oa) - 1
    if rows_b is None:
        rb = cb = ob = sb = None
        n_b = cap_b = n_gb = 0
        out = np.empty((n_ga, n_ga))
    else:
        rb = f64(rows_b); cb = i32(cnt_b)
        n_b, cap_b, _ = rb.shape
        ob = None if seg_off_b is None else i32(seg_off_b)
        sb = None if status_b is None else i32(status_b)
        n_gb = n_b if ob is None else len(ob) - 1
        out = np.empty((n_ga, n_gb))
        if n_b == 0:                                 # nothing on the B side: every group of it is empty
            diagram_kernel_check(par, cap_a)
            out.fill(np.nan)
            return out
    ctx.check(ctx.lib.tda_diagram_kernel_gram(ctx.h, ptr(ra), ptr(ca), n_a, cap_a, ptr(oa), n_ga, ptr(sa), ptr(rb), ptr(cb), n_b,
                                              cap_b, ptr(ob), n_gb, ptr(sb), int(skip_mask), *par, ptr(out)))
    return out


def diagram_kernel_check(par, *caps):
    """The library's own refusals for five raw parameters and diagram capacities, for a call that launches nothing."""
    ninv, mirror, scale, weight, wc = par
    ok = np.isfinite(ninv) and ninv < 0 and mirror in (0, 1) and np.isfinite(scale) and (
        weight in (_lib.TDA_KW_ONE, _lib.TDA_KW_PERS) or (weight == _lib.TDA_KW_ATAN and np.isfinite(wc)))
    if not ok or any(c < 1 for c in caps):
        raise _lib.TdaError("libtdaeeg error 1: ninv finite and < 0, mirror 0 or 1, scale finite, weight TDA_KW_*, wc finite, "
                            "cap >= 1")


def fisher_args(sigma):
    """ninv = -1 / (2 sigma^2) of the persistence Fisher distance as the entry points take it (include/tdaeeg.h): sigma a
    finite number > 0.  TdaError, before any GPU call, for anything else (a sigma whose ninv is not a finite number < 0
    included)."""
    bad = _lib.TdaError(f"persistence Fisher: sigma must be a finite number > 0, not {sigma!r}")
    if isinstance(sigma, bool) or not isinstance(sigma, (int, float, np.integer, np.floating)) or not np.isfinite(sigma) \
            or not sigma > 0:
        raise bad
    s = float(sigma)
    if s * s == 0.0:                                 # sigma * sigma underflows
        raise bad
    ninv = -1.0 / (2.0 * s * s)
    if not (np.isfinite(ninv) and ninv < 0):
        raise bad
    return ninv


def persistence_fisher_batch(rows_a, cnt_a, rows_b, cnt_b, sigma, idx_a=None, idx_b=None, ctx=None, want_status=False):
    """Persistence Fisher distance of diagram pairs (include/tdaeeg.h: the Fisher information metric between the two
    diagrams smoothed by Gaussians of width sigma on both diagrams and their diagonal images; in [0, pi / 2], exactly 0
    for a diagram against itself); arguments and results as wasserstein_batch.  A pair with more than PF_MAX_POINTS finite
    rows in all is NaN with TDA_WIN_TOO_LARGE, a pair whose index is outside its set NaN with TDA_WIN_NO_PAIR."""
    ninv = fisher_args(sigma)
    ctx = ctx or get_ctx()
    return _pair_batch(ctx.lib.tda_persistence_fisher_batch, rows_a, cnt_a, rows_b, cnt_b, idx_a, idx_b, ctx, want_status, ninv)


def persistence_fisher_gram(rows, cnt, sigma, ctx=None):
    """(n, n) matrix of the persistence Fisher distances of one set of diagrams: the pairs i <= j in one batched call,
    mirrored, so symmetric as bytes; the diagonal is computed, not set (it is 0.0 by the contract).  NaN where a pair has
    a status."""
    fisher_args(sigma)
    n = len(cnt)
    iu, ju = np.triu_indices(n)
    G = np.zeros((n, n))
    if len(iu):
        d = persistence_fisher_batch(rows, cnt, rows, cnt, sigma, idx_a=iu, idx_b=ju, ctx=ctx)
        G[iu, ju] = d
        G[ju, iu] = d
    return G


# ------------------------------------------------------------------ device-tensor API (torch)
def _tp(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class DeviceDiagrams:
    """H0/H1 rows of a batch of windows, resident in HBM."""

    def __init__(self, n_win, h0_cap, h1_cap, device):
        import torch
        kw = dict(device=device)
        self.h0 = torch.empty((n_win, h0_cap, 2), dtype=torch.float64, **kw)
        self.h1 = torch.empty((n_win, h1_cap, 2), dtype=torch.float64, **kw)
        self.c0 = torch.empty(n_win, dtype=torch.int32, **kw)
        self.c1 = torch.empty(n_win, dtype=torch.int32, **kw)
        self.status = torch.empty(n_win, dtype=torch.int32, **kw)
        self.n_points = torch.empty(n_win, dtype=torch.int32, **kw)
        self.h0_cap, self.h1_cap, self.n_win = h0_cap, h1_cap, n_win

    def head(self, n_win):
        """The same buffers for the first n_win windows only (a view: nothing is copied)."""
        v = object.__new__(DeviceDiagrams)
        v.h0, v.h1, v.c0, v.c1 = self.h0[:n_win], self.h1[:n_win], self.c0[:n_win], self.c1[:n_win]
        v.status, v.n_points = self.status[:n_win], self.n_points[:n_win]
        v.h0_cap, v.h1_cap, v.n_win = self.h0_cap, self.h1_cap, n_win
        return v

    def to_lists(self):
        h0, c0 = self.h0.cpu().numpy(), self.c0.cpu().numpy()
        h1, c1 = self.h1.cpu().numpy(), self.c1.cpu().numpy()
        return _diagrams(h0, c0, self.h0_cap), _diagrams(h1, c1, self.h1_cap)


def corr_dist_dev(win_t, dist_t=None, corr_t=None, ctx=None):
    import torch
    ctx = ctx or get_ctx()
    assert win_t.is_cuda and win_t.dtype == torch.float64 and win_t.is_contiguous()
    n_win, n_ch, n_t = win_t.shape
    if dist_t is None:
        dist_t = torch.empty((n_win, n_ch, n_ch), dtype=torch.float64, device=win_t.device)
    ctx.check(ctx.lib.tda_corr_dist_batch_dev(ctx.h, _tp(win_t), n_win, n_ch, n_t, _tp(dist_t), _tp(corr_t), _stream()))
    return dist_t


def rips_dm_dev(dm_t, out=None, thresh=MAX_EDGE_LENGTH, symmetrise=True, h1_cap=DEFAULT_H1_CAP, ctx=None):
    import torch
    ctx = ctx or get_ctx()
    assert dm_t.is_cuda and dm_t.dtype == torch.float64 and dm_t.is_contiguous()
    n_win, n, _ = dm_t.shape
    out = out or DeviceDiagrams(n_win, n, h1_cap, dm_t.device)
    ctx.check(ctx.lib.tda_rips_dm_batch_dev(ctx.h, _tp(dm_t), n_win, n, float(thresh), int(bool(symmetrise)),
                                            _tp(out.h0), out.h0_cap, _tp(out.c0), _tp(out.h1), out.h1_cap,
                                            _tp(out.c1), _tp(out.status), _stream()))
    return out


def eeg_window_dev(win_t, out=None, thresh=MAX_EDGE_LENGTH, h1_cap=DEFAULT_H1_CAP, dist_t=None, corr_t=None, ctx=None):
    """Fused corr -> dist -> Rips of EEG windows (nb2:198-207 + utils.py:135-141), one launch; the matrices are
    written only when dist_t (and corr_t) are given."""
    import torch
    ctx = ctx or get_ctx()
    assert win_t.is_cuda and win_t.dtype == torch.float64 and win_t.is_contiguous()
    n_win, n_ch, n_t = win_t.shape
    out = out or DeviceDiagrams(n_win, n_ch, h1_cap, win_t.device)
    ctx.check(ctx.lib.tda_eeg_window_batch_dev(ctx.h, _tp(win_t), n_win, n_ch, n_t, float(thresh), _tp(dist_t), _tp(corr_t),
                                               _tp(out.h0), out.h0_cap, _tp(out.c0), _tp(out.h1), out.h1_cap, _tp(out.c1),
                                               _tp(out.status), _stream()))
    return out


def eeg_window_sliding_dev(sig_t, win_len=250, step=62, sel_t=None, out=None, thresh=MAX_EDGE_LENGTH,
                           h1_cap=DEFAULT_H1_CAP, dist_t=None, corr_t=None, ctx=None):
    """Fused corr -> dist -> Rips on windows read in place from band-passed recordings sig_t (n_rec, n_ch,
    n_samples) (nb1:314-381 + nb2:198-207 + utils.py:135-141).  sel_t: optional int32 tensor of window indices
    r * n_win_per_rec + k.  Returns (diagrams, n_win_per_rec)."""
    import torch
    ctx = ctx or get_ctx()
    assert sig_t.is_cuda and sig_t.dtype == torch.float64 and sig_t.is_contiguous() and sig_t.dim() == 3
    n_rec, n_ch, n_s = sig_t.shape
    per_rec = (n_s - win_len) // step + 1 if n_s >= win_len else 0
    n_out = int(sel_t.numel()) if sel_t is not None else n_rec * per_rec
    out = out or DeviceDiagrams(n_out, n_ch, h1_cap, sig_t.device)
    assert out.n_win == n_out
    ctx.check(ctx.lib.tda_eeg_window_sliding_dev(ctx.h, _tp(sig_t), n_rec, n_ch, n_s, win_len, step, _tp(sel_t),
                                                 0 if sel_t is None else n_out, float(thresh), _tp(dist_t), _tp(corr_t),
                                                 _tp(out.h0), out.h0_cap, _tp(out.c0), _tp(out.h1), out.h1_cap, _tp(out.c1),
                                                 _tp(out.status), None, _stream()))
    return out, per_rec


def eeg_window_ragged_dev(sig_t, start_t, ld_t, win_len=250, out=None, thresh=MAX_EDGE_LENGTH, h1_cap=DEFAULT_H1_CAP,
                          dist_t=None, corr_t=None, n_ch=47, ctx=None):
    """Fused corr -> dist -> Rips on windows of RAGGED recordings read in place from a window table: window w starts at
    element start_t[w] of sig_t (packed band-passed recordings) and its n_ch rows are ld_t[w] (= L_r) apart; both int64
    device tensors (nb1:314-381 per recording + nb2:198-207 + utils.py:135-141).  Diagrams identical to eeg_window_dev on
    the same windows stacked."""
    import torch
    ctx = ctx or get_ctx()
    assert sig_t.is_cuda and sig_t.dtype == torch.float64 and sig_t.is_contiguous()
    assert start_t.dtype == torch.int64 and ld_t.dtype == torch.int64 and start_t.numel() == ld_t.numel()
    n_win = int(start_t.numel())
    out = out or DeviceDiagrams(n_win, n_ch, h1_cap, sig_t.device)
    assert out.n_win == n_win
    ctx.check(ctx.lib.tda_eeg_window_ragged_dev(ctx.h, _tp(sig_t), _tp(start_t), _tp(ld_t), n_win, n_ch, int(win_len),
                                                float(thresh), _tp(dist_t), _tp(corr_t), _tp(out.h0), out.h0_cap, _tp(out.c0),
                                                _tp(out.h1), out.h1_cap, _tp(out.c1), _tp(out.status), _stream()))
    return out


def gather_windows_dev(src_t, start_t, win_len=250, out_t=None, ctx=None):
    """out_t[w] = src_t[start_t[w] : start_t[w] + win_len] (flat float64 source, int64 device table): the selected
    windows of packed signals as a stack (create_windows + np.linspace, cmp:65,77-80, for ragged recordings)."""
    import torch
    ctx = ctx or get_ctx()
    assert src_t.is_cuda and src_t.dtype == torch.float64 and src_t.is_contiguous() and start_t.dtype == torch.int64
    n_win = int(start_t.numel())
    if out_t is None:
        out_t = torch.empty((n_win, win_len), dtype=torch.float64, device=src_t.device)
    assert out_t.is_contiguous() and out_t.numel() >= n_win * win_len
    ctx.check(ctx.lib.tda_gather_windows_dev(ctx.h, _tp(src_t), _tp(start_t), n_win, int(win_len), _tp(out_t), _stream()))
    return out_t


def takens_rips_dev(win_t, tau_t, out=None, dim=3, subsample=2, thresh=MAX_EDGE_LENGTH, h1_cap=DEFAULT_H1_CAP,
                    ctx=None):
    import torch
    ctx = ctx or get_ctx()
    assert win_t.is_cuda and win_t.dtype == torch.float64 and win_t.is_contiguous()
    assert tau_t.dtype == torch.int32 and tau_t.is_cuda
    n_win, n_t = win_t.shape
    out = out or DeviceDiagrams(n_win, _lib.MAX_POINTS, h1_cap, win_t.device)
    ctx.check(ctx.lib.tda_takens_rips_batch_dev(ctx.h, _tp(win_t), _tp(tau_t), n_win, n_t, dim, subsample,
                                                float(thresh), _tp(out.h0), out.h0_cap, _tp(out.c0), _tp(out.h1),
                                                out.h1_cap, _tp(out.c1), _tp(out.n_points), _tp(out.status),
                                                _stream()))
    return out


class DeviceLandmarks:
    """Landmark rows, indices, insertion radii and covering radius of a batch of windows, resident in HBM (include/tdaeeg.h,
    "Landmark Rips").  Allocated zeroed: rows and entries from n_lm on are never written."""

    def __init__(self, n_win, n_perm, dim, device):
        import torch
        n_perm, dim, _ = landmark_args(n_perm, dim)
        kw = dict(device=device)
        self.lm = torch.zeros((n_win, n_perm, dim), dtype=torch.float64, **kw)
        self.idx = torch.zeros((n_win, n_perm), dtype=torch.int32, **kw)
        self.lam = torch.zeros((n_win, n_perm), dtype=torch.float64, **kw)
        self.r_cover = torch.zeros(n_win, dtype=torch.float64, **kw)
        self.n_lm = torch.zeros(n_win, dtype=torch.int32, **kw)
        self.n_full = torch.zeros(n_win, dtype=torch.int32, **kw)
        self.n_win, self.n_perm, self.dim = n_win, n_perm, dim

    def head(self, n_win):
        """The same buffers for the first n_win windows only (a view: nothing is copied)."""
        v = object.__new__(DeviceLandmarks)
        for name in ("lm", "idx", "lam", "r_cover", "n_lm", "n_full"):
            setattr(v, name, getattr(self, name)[:n_win])
        v.n_win, v.n_perm, v.dim = n_win, self.n_perm, self.dim
        return v

    def _args(self):
        return (self.n_perm, _tp(self.lm), _tp(self.idx), _tp(self.lam), _tp(self.r_cover), _tp(self.n_lm), _tp(self.n_full))


def _landmark_dev_out(lm, n_win, n_perm, dim, device):
    lm = lm or DeviceLandmarks(n_win, n_perm, dim, device)
    assert lm.n_win == n_win and lm.dim == dim, "landmark buffers of another shape"
    return lm


def takens_landmarks_dev(win_t, tau_t, lm=None, dim=3, subsample=1, n_perm=128, ctx=None):
    """Greedy permutation of the normalised Takens cloud of every window, into lm (a DeviceLandmarks; n_perm is lm's when
    lm is given).  Enqueue only."""
    import torch
    ctx = ctx or get_ctx()
    assert win_t.is_cuda and win_t.dtype == torch.float64 and win_t.is_contiguous()
    assert tau_t.dtype == torch.int32 and tau_t.is_cuda
    n_win, n_t = win_t.shape
    _, dim, subsample = landmark_args(lm.n_perm if lm else n_perm, dim, subsample)
    lm = _landmark_dev_out(lm, n_win, n_perm, dim, win_t.device)
    n_perm, *bufs = lm._args()
    ctx.check(ctx.lib.tda_takens_landmarks_dev(ctx.h, _tp(win_t), _tp(tau_t), n_win, n_t, dim, subsample, n_perm, *bufs,
                                               _stream()))
    return lm


def cloud_landmarks_dev(pc_t, n_pts_t, lm=None, normalise=True, n_perm=128, ctx=None):
    """The same from explicit clouds pc_t (n_win, p_cap, dim) float64 with n_pts_t (n_win) int32 rows each."""
    import torch
    ctx = ctx or get_ctx()
    assert pc_t.is_cuda and pc_t.dtype == torch.float64 and pc_t.is_contiguous() and pc_t.dim() == 3
    assert n_pts_t.dtype == torch.int32 and n_pts_t.is_cuda
    n_win, p_cap, dim = pc_t.shape
    landmark_args(lm.n_perm if lm else n_perm, dim)
    lm = _landmark_dev_out(lm, n_win, n_perm, dim, pc_t.device)
    n_perm, *bufs = lm._args()
    ctx.check(ctx.lib.tda_cloud_landmarks_dev(ctx.h, _tp(pc_t), _tp(n_pts_t), n_win, p_cap, dim, int(bool(normalise)), n_perm,
                                              *bufs, _stream()))
    return lm


def takens_rips_landmarks_dev(win_t, tau_t, out=None, lm=None, dim=3, subsample=1, n_perm=128, thresh=MAX_EDGE_LENGTH,
                              h1_cap=DEFAULT_H1_CAP, ctx=None):
    """takens_rips_dev for clouds of up to LM_MAX_POINTS points: the landmarks into lm, then the cloud Rips on them into
    out (out.n_points receives n_lm).  Returns (out, lm)."""
    import torch
    ctx = ctx or get_ctx()
    assert win_t.is_cuda and win_t.dtype == torch.float64 and win_t.is_contiguous()
    assert tau_t.dtype == torch.int32 and tau_t.is_cuda
    n_win, n_t = win_t.shape
    _, dim, subsample = landmark_args(lm.n_perm if lm else n_perm, dim, subsample)
    lm = _landmark_dev_out(lm, n_win, n_perm, dim, win_t.device)
    out = out or DeviceDiagrams(n_win, _lib.MAX_POINTS, h1_cap, win_t.device)
    assert out.n_win == n_win
    n_perm, *bufs = lm._args()
    ctx.check(ctx.lib.tda_takens_rips_landmarks_dev(ctx.h, _tp(win_t), _tp(tau_t), n_win, n_t, dim, subsample, n_perm,
                                                    float(thresh), *bufs, _tp(out.h0), out.h0_cap, _tp(out.c0), _tp(out.h1),
                                                    out.h1_cap, _tp(out.c1), _tp(out.n_points), _tp(out.status), _stream()))
    return out, lm


def _sublevel_shape(sig_t, n_t, win_start_t, win_ld_t, n_ch):
    """(n_win, n_ch, n_t) of a sublevel call on device tensors: stacked (n_sig, n_t) / (n_win, n_ch, n_t), or tables."""
    import torch
    assert sig_t.is_cuda and sig_t.dtype == torch.float64 and sig_t.is_contiguous()
    if win_start_t is None and win_ld_t is None:
        assert sig_t.dim() in (2, 3)
        return (sig_t.shape[0], 1, sig_t.shape[1]) if sig_t.dim() == 2 else tuple(sig_t.shape)
    assert win_start_t.dtype == torch.int64 and win_ld_t.dtype == torch.int64 and win_start_t.numel() == win_ld_t.numel()
    assert win_start_t.is_contiguous() and win_ld_t.is_contiguous() and n_ch is not None and n_t is not None
    return int(win_start_t.numel()), int(n_ch), int(n_t)


def sublevel_dev(sig_t, n_t=None, win_start_t=None, win_ld_t=None, n_ch=None, cap=None, dgm_t=None, cnt_t=None, idx_t=None,
                 status_t=None, want_index=False, ctx=None):
    """sublevel_batch on device tensors: one launch on torch's current stream, nothing allocated when dgm_t, cnt_t and
    status_t (and idx_t, if indices are wanted) are given.  win_start_t / win_ld_t: optional int64 device tables, the ones of
    eeg_window_ragged_dev.  Returns (dgm_t, cnt_t, idx_t or None, status_t); buffers made here are NaN / -1 outside rows
    [0, cnt)."""
    import torch
    ctx = ctx or get_ctx()
    n_win, n_ch, n_t = _sublevel_shape(sig_t, n_t, win_start_t, win_ld_t, n_ch)
    n_sig = n_win * max(n_ch, 0)
    if cap is None:
        cap = dgm_t.shape[1] if dgm_t is not None else sublevel_rows(n_t)
    dev = sig_t.device
    if dgm_t is None:
        dgm_t = torch.full((n_sig, max(cap, 0), 2), float("nan"), dtype=torch.float64, device=dev)
    if idx_t is None and want_index:
        idx_t = torch.full((n_sig, max(cap, 0), 2), -1, dtype=torch.int32, device=dev)
    cnt_t = torch.zeros(n_sig, dtype=torch.int32, device=dev) if cnt_t is None else cnt_t
    status_t = torch.zeros(n_sig, dtype=torch.int32, device=dev) if status_t is None else status_t
    assert dgm_t.is_contiguous() and dgm_t.dtype == torch.float64 and dgm_t.numel() >= n_sig * max(cap, 0) * 2
    assert idx_t is None or (idx_t.is_contiguous() and idx_t.dtype == torch.int32 and idx_t.numel() >= n_sig * max(cap, 0) * 2)
    assert cnt_t.numel() >= n_sig and status_t.numel() >= n_sig and cnt_t.dtype == status_t.dtype == torch.int32
    ctx.check(ctx.lib.tda_sublevel_batch_dev(ctx.h, _tp(sig_t), _tp(win_start_t), _tp(win_ld_t), n_win, n_ch, n_t, _tp(dgm_t),
                                             int(cap), _tp(cnt_t), _tp(idx_t), _tp(status_t), _stream()))
    return dgm_t, cnt_t, idx_t, status_t


SL_SCRATCH_BYTES = 128 << 20      # sublevel_features_dev: bound of the diagram rows of one chunk


class SublevelScratch:
    """The bounded scratch of sublevel_features_dev: the diagram rows and counts of ONE chunk of windows.  The diagrams of
    47 channels come to 95 KB per window of 250 samples, 10 GB for 106,200 windows, so the features are taken chunk by
    chunk: chunk_windows = the windows whose rows fit into max_bytes (at least one), fixed here, and with it the number of
    launches for any given number of windows -- a captured graph of the calls holds."""

    def __init__(self, n_ch, n_t, device, max_bytes=SL_SCRATCH_BYTES, n_win=None):
        import torch
        self.n_ch, self.n_t, self.cap = int(n_ch), int(n_t), sublevel_rows(n_t)
        per_win = self.n_ch * self.cap * 16
        self.chunk_windows = max(1, int(max_bytes) // per_win)
        if n_win is not None:                        # never more than the caller's batch
            self.chunk_windows = max(1, min(self.chunk_windows, int(n_win)))
        n = self.chunk_windows * self.n_ch
        self.dgm = torch.empty((n, self.cap, 2), dtype=torch.float64, device=device)
        self.cnt = torch.empty(n, dtype=torch.int32, device=device)

    def n_chunks(self, n_win):
        return -(-int(n_win) // self.chunk_windows)


def sublevel_features_dev(sig_t, n_t=None, win_start_t=None, win_ld_t=None, n_ch=None, out_t=None, status_t=None, scratch=None,
                          max_bytes=SL_SCRATCH_BYTES, ctx=None):
    """The 11 extract_features values of the sublevel-set diagram of every signal, (n_win, n_ch, 11) float64: per chunk of
    scratch.chunk_windows windows one sublevel launch into the scratch and one tda_features_batch_dev launch on it, on
    torch's current stream; the rows never exist for more than a chunk.  A signal with a sample that is not finite is NaN
    (status_t, (n_win, n_ch) int32, holds its TDA_WIN_NOT_FINITE).  Arguments as sublevel_dev; scratch: a SublevelScratch
    of this (n_ch, n_t), made here from max_bytes when None.  Nothing is allocated when out_t, status_t and scratch are
    given, but the NaN mask."""
    import torch
    ctx = ctx or get_ctx()
    n_win, n_ch, n_t = _sublevel_shape(sig_t, n_t, win_start_t, win_ld_t, n_ch)
    dev = sig_t.device
    scratch = scratch or SublevelScratch(n_ch, n_t, dev, max_bytes, n_win=n_win)
    assert (scratch.n_ch, scratch.n_t) == (n_ch, n_t), "scratch of another signal shape"
    if out_t is None:
        out_t = torch.empty((n_win, n_ch, _lib.N_FEATURES), dtype=torch.float64, device=dev)
    if status_t is None:
        status_t = torch.empty((n_win, n_ch), dtype=torch.int32, device=dev)
    assert out_t.is_contiguous() and out_t.shape == (n_win, n_ch, _lib.N_FEATURES) and out_t.dtype == torch.float64
    assert status_t.is_contiguous() and status_t.shape == (n_win, n_ch) and status_t.dtype == torch.int32
    cw = scratch.chunk_windows
    stacked = sig_t.view(n_win, n_ch, n_t) if win_start_t is None else None
    for w0 in range(0, n_win, cw):
        w1 = min(w0 + cw, n_win)
        if stacked is not None:
            sublevel_dev(stacked[w0:w1], dgm_t=scratch.dgm, cnt_t=scratch.cnt, status_t=status_t[w0:w1], ctx=ctx)
        else:
            sublevel_dev(sig_t, n_t, win_start_t[w0:w1], win_ld_t[w0:w1], n_ch, dgm_t=scratch.dgm, cnt_t=scratch.cnt,
                         status_t=status_t[w0:w1], ctx=ctx)
        n = (w1 - w0) * n_ch
        features_dev(scratch.dgm[:n], scratch.cnt[:n], out_t[w0:w1], ctx=ctx)
    out_t.masked_fill_((status_t != 0).unsqueeze(-1), float("nan"))
    return out_t


_PLV_G = {}                 # (n_t, device) -> the resident Hilbert table of plv_dist_dev


def plv_g_table(n_t, device):
    """preprocess._hilbert_g(n_t) resident on `device`: uploaded once per (n_t, device) and kept (the first call copies from
    the host, so it stays out of a graph capture: run a step eagerly once, as pipeline.Lanes does)."""
    import torch
    from .preprocess import _hilbert_g
    device = torch.device(device)
    key = (int(n_t), device.type, device.index if device.index is not None else torch.cuda.current_device())
    if key not in _PLV_G:
        _PLV_G[key] = torch.from_numpy(_hilbert_g(int(n_t))).to(device)
    return _PLV_G[key]


def _dev_windows(sig_t, n_t, win_start_t, win_ld_t, n_ch):
    """The window arguments of plv_dist_dev / connectivity_dist_dev checked: (n_win, n_ch, n_t) of stacked windows or of a
    flat tensor with its int64 device tables."""
    import torch
    assert sig_t.is_cuda and sig_t.dtype == torch.float64 and sig_t.is_contiguous()
    if win_start_t is None and win_ld_t is None:
        assert sig_t.dim() == 3
        n_win, n_ch, n_t = sig_t.shape
    else:
        assert win_start_t.dtype == torch.int64 and win_ld_t.dtype == torch.int64 and win_start_t.numel() == win_ld_t.numel()
        assert win_start_t.is_contiguous() and win_ld_t.is_contiguous() and n_ch is not None and n_t is not None
        n_win, n_ch, n_t = int(win_start_t.numel()), int(n_ch), int(n_t)
    return n_win, n_ch, n_t


def plv_dist_dev(sig_t, n_t=None, win_start_t=None, win_ld_t=None, n_ch=None, method="euclidean", out=None, plv_t=None,
                 status_t=None, want_plv=False, ctx=None):
    """plv_dist_batch on device tensors: one launch on torch's current stream.  sig_t (n_win, n_ch, n_t), or flat with the
    int64 device tables win_start_t / win_ld_t (those of eeg_window_ragged_dev) and n_ch, n_t.  out: the (n_win, n_ch, n_ch)
    distance matrices; plv_t: the PLV matrices (made when want_plv; not touched when absent).  Nothing is allocated when
    out and status_t are given and the table of this (n_t, device) is resident (plv_g_table).  Returns
    (out, plv_t or None, status_t)."""
    import torch
    m = plv_method(method)
    ctx = ctx or get_ctx()
    n_win, n_ch, n_t = _dev_windows(sig_t, n_t, win_start_t, win_ld_t, n_ch)
    dev = sig_t.device
    nc = max(n_ch, 0)
    if out is None:
        out = torch.empty((n_win, nc, nc), dtype=torch.float64, device=dev)
    if plv_t is None and want_plv:
        plv_t = torch.empty((n_win, nc, nc), dtype=torch.float64, device=dev)
    status_t = torch.zeros(n_win, dtype=torch.int32, device=dev) if status_t is None else status_t
    assert out.is_contiguous() and out.dtype == torch.float64 and out.numel() >= n_win * nc * nc
    assert plv_t is None or (plv_t.is_contiguous() and plv_t.dtype == torch.float64 and plv_t.numel() >= n_win * nc * nc)
    assert status_t.numel() >= n_win and status_t.dtype == torch.int32 and status_t.is_contiguous()
    g_t = plv_g_table(max(n_t, 1), dev)
    ctx.check(ctx.lib.tda_plv_dist_batch_dev(ctx.h, _tp(sig_t), _tp(win_start_t), _tp(win_ld_t), n_win, n_ch, n_t, _tp(g_t), m,
                                             _tp(out), _tp(plv_t), _tp(status_t), _stream()))
    return out, plv_t, status_t


def connectivity_dist_dev(sig_t, n_t=None, win_start_t=None, win_ld_t=None, n_ch=None, measure=None, method="euclidean",
                          out=None, value_t=None, status_t=None, want_value=False, ctx=None):
    """connectivity_dist_batch on device tensors: one launch on torch's current stream.  sig_t and the tables as plv_dist_dev
    takes them.  out: the (n_win, n_ch, n_ch) distance matrices; value_t: the measure's matrices (made when want_value; not
    touched when absent).  Nothing is allocated when out and status_t are given and the table of this (n_t, device) is
    resident (plv_g_table, shared with plv_dist_dev).  Returns (out, value_t or None, status_t)."""
    import torch
    k, m = connectivity_measure(measure), _dist_method(method)
    ctx = ctx or get_ctx()
    n_win, n_ch, n_t = _dev_windows(sig_t, n_t, win_start_t, win_ld_t, n_ch)
    dev = sig_t.device
    nc = max(n_ch, 0)
    if out is None:
        out = torch.empty((n_win, nc, nc), dtype=torch.float64, device=dev)
    if value_t is None and want_value:
        value_t = torch.empty((n_win, nc, nc), dtype=torch.float64, device=dev)
    status_t = torch.zeros(n_win, dtype=torch.int32, device=dev) if status_t is None else status_t
    assert out.is_contiguous() and out.dtype == torch.float64 and out.numel() >= n_win * nc * nc
    assert value_t is None or (value_t.is_contiguous() and value_t.dtype == torch.float64 and value_t.numel() >= n_win * nc * nc)
    assert status_t.numel() >= n_win and status_t.dtype == torch.int32 and status_t.is_contiguous()
    g_t = plv_g_table(max(n_t, 1), dev)
    ctx.check(ctx.lib.tda_connectivity_dist_batch_dev(ctx.h, _tp(sig_t), _tp(win_start_t), _tp(win_ld_t), n_win, n_ch, n_t,
                                                      _tp(g_t), k, m, _tp(out), _tp(value_t), _tp(status_t), _stream()))
    return out, value_t, status_t


def permutation_sums_dev(D_t, lab_t, out_t=None, n1_t=None, ctx=None, n_perm=None, work_t=None):
    """permutation_sums_batch on device tensors: two launches on torch's current stream, no synchronisation.  D_t
    (n_mat, n, ld) or (n, ld) float64, contiguous; lab_t the packed labels (pack_labels, viewed as int64), (n_words, n).
    n_perm: the relabellings of lab_t that count (default: those of out_t, else all 64 * n_words bits).  out_t
    (n_mat, 3, n_perm) float64, n1_t (n_perm) int32 and work_t (at least _lib.pt_work_doubles(n_mat, n, n_perm) float64) are
    made when absent; with all three given nothing is allocated.  Returns (out_t, n1_t)."""
    import torch
    ctx = ctx or get_ctx()
    assert D_t.is_cuda and D_t.dtype == torch.float64 and D_t.is_contiguous()
    assert lab_t.is_cuda and lab_t.dtype == torch.int64 and lab_t.is_contiguous() and lab_t.dim() == 2
    n_words, n = (int(x) for x in lab_t.shape)
    n_mat, ld = _perm_shape(tuple(D_t.shape), n)
    if n_perm is None:
        n_perm = int(out_t.shape[-1]) if out_t is not None else 64 * n_words
    n_perm = int(n_perm)
    assert _lib.pt_words(max(n_perm, 1)) <= n_words, "lab_t has fewer words than n_perm needs"
    dev = D_t.device
    if out_t is None:
        out_t = torch.empty((n_mat, 3, max(n_perm, 0)), dtype=torch.float64, device=dev)
    if n1_t is None:
        n1_t = torch.empty(max(n_perm, 0), dtype=torch.int32, device=dev)
    need = _lib.pt_work_doubles(n_mat, n, max(n_perm, 0))
    if work_t is None:
        work_t = torch.empty(max(need, 1), dtype=torch.float64, device=dev)
    assert out_t.is_contiguous() and out_t.dtype == torch.float64 and out_t.numel() >= n_mat * 3 * n_perm
    assert n1_t.is_contiguous() and n1_t.dtype == torch.int32 and n1_t.numel() >= n_perm
    assert work_t.is_contiguous() and work_t.dtype == torch.float64
    # the kernel takes the words of relabelling group g at lab + g * n: a lab_t with more words than n_perm needs is fine
    ctx.check(ctx.lib.tda_perm_sums_batch_dev(ctx.h, _tp(D_t), n_mat, n, ld, _tp(lab_t), n_perm, _tp(work_t),
                                              int(work_t.numel()), _tp(out_t), _tp(n1_t), _stream()))
    return out_t, n1_t


def tau_dev(win_t, max_lag=None, tau_t=None, ctx=None):
    import torch
    ctx = ctx or get_ctx()
    n_win, n_t = win_t.shape
    if tau_t is None:
        tau_t = torch.empty(n_win, dtype=torch.int32, device=win_t.device)
    ctx.check(ctx.lib.tda_tau_batch_dev(ctx.h, _tp(win_t), n_win, n_t, -1 if max_lag is None else int(max_lag),
                                        _tp(tau_t), _stream()))
    return tau_t


def tau_segments_dev(win_t, seg_off_t, max_lag=None, tau_seg_t=None, tau_win_t=None, ctx=None):
    """cmp:83 / mvm:56: tau of every (recording, band) group from its first window; tau_win_t (optional, (n_win,)
    int32) receives the group's value for every window."""
    import torch
    ctx = ctx or get_ctx()
    n_win, n_t = win_t.shape
    n_seg = seg_off_t.numel() - 1
    if tau_seg_t is None:
        tau_seg_t = torch.empty(n_seg, dtype=torch.int32, device=win_t.device)
    ctx.check(ctx.lib.tda_tau_segments_dev(ctx.h, _tp(win_t), _tp(seg_off_t), n_seg, n_t,
                                           -1 if max_lag is None else int(max_lag), _tp(tau_seg_t), _tp(tau_win_t),
                                           _stream()))
    return tau_seg_t


class DeviceEmbedding:
    """The outputs of ami_dev and fnn_dev for a batch of windows, resident in HBM (include/tdaeeg.h, "Delay and dimension
    selection"): ami (n_win, n_lag) float64, tau (n_win,) int32, ami_status, and, when asked for, joint (n_win, n_lag,
    n_bins, n_bins) int32; counts (n_win, d_max, 4) int32, frac (n_win, d_max) float64, dim (n_win,) int32, fnn_status and,
    when asked for, nn (n_win, d_max, n_t) int32.  n_lag = 0 or d_max = 0 leaves that half out."""

    def __init__(self, n_win, n_lag, d_max, device, n_bins=0, n_t=0):
        import torch
        kw = dict(device=device)
        i32t, f64t = torch.int32, torch.float64
        self.ami = torch.empty((n_win, n_lag), dtype=f64t, **kw) if n_lag else None
        self.tau = torch.empty(n_win, dtype=i32t, **kw) if n_lag else None
        self.ami_status = torch.empty(n_win, dtype=i32t, **kw) if n_lag else None
        self.joint = torch.empty((n_win, n_lag, n_bins, n_bins), dtype=i32t, **kw) if n_lag and n_bins else None
        self.counts = torch.empty((n_win, d_max, _lib.FNN_COLS), dtype=i32t, **kw) if d_max else None
        self.frac = torch.empty((n_win, d_max), dtype=f64t, **kw) if d_max else None
        self.dim = torch.empty(n_win, dtype=i32t, **kw) if d_max else None
        self.fnn_status = torch.empty(n_win, dtype=i32t, **kw) if d_max else None
        self.nn = torch.empty((n_win, d_max, n_t), dtype=i32t, **kw) if d_max and n_t else None
        self.n_win, self.n_lag, self.d_max = n_win, n_lag, d_max

    def to_host(self):
        return {k: getattr(self, k).cpu().numpy() for k in ("ami", "tau", "ami_status", "joint", "counts", "frac", "dim",
                                                            "fnn_status", "nn") if getattr(self, k) is not None}


def ami_dev(win_t, max_lag=None, n_bins=16, joint=False, out=None, ctx=None):
    """ami_batch on device tensors: win_t (n_win, n_t) float64 -> a DeviceEmbedding (out, when given, needs n_lag = the
    resolved max_lag + 1 and, for joint=True, its joint block); nothing else is allocated."""
    import torch
    ctx = ctx or get_ctx()
    assert win_t.is_cuda and win_t.dtype == torch.float64 and win_t.is_contiguous() and win_t.dim() == 2
    n_win, n_t = (int(v) for v in win_t.shape)
    lag, n_bins = ami_args(n_t, max_lag, n_bins)
    if out is None:
        out = DeviceEmbedding(n_win, lag + 1, 0, win_t.device, n_bins if joint else 0)
    assert out.n_win >= n_win and out.n_lag == lag + 1 and out.ami.is_contiguous()
    assert not joint or (out.joint is not None and tuple(out.joint.shape[1:]) == (lag + 1, n_bins, n_bins))
    ctx.check(ctx.lib.tda_ami_batch_dev(ctx.h, _tp(win_t), n_win, n_t, lag, n_bins, _tp(out.ami), _tp(out.tau),
                                        _tp(out.joint if joint else None), _tp(out.ami_status), _stream()))
    return out


def ami_segments_dev(win_t, seg_off_t, max_lag=None, n_bins=16, tau_seg_t=None, tau_win_t=None, ctx=None):
    """tau_segments_dev with the first minimum of the average mutual information in place of the zero crossing of the
    autocorrelation: the delay of every (recording, band) group from its first window, compute_tau's fallback
    max(max_lag // 10, 1) where there is no minimum; tau_win_t (optional, (n_win,) int32) receives the group's value for
    every window, ready for the Takens entry points."""
    import torch
    ctx = ctx or get_ctx()
    assert win_t.is_cuda and win_t.dtype == torch.float64 and win_t.is_contiguous() and win_t.dim() == 2
    assert seg_off_t.dtype == torch.int32 and seg_off_t.is_contiguous()
    n_win, n_t = (int(v) for v in win_t.shape)
    lag, n_bins = ami_args(n_t, max_lag, n_bins)
    n_seg = seg_off_t.numel() - 1
    if tau_seg_t is None:
        tau_seg_t = torch.empty(n_seg, dtype=torch.int32, device=win_t.device)
    assert tau_seg_t.dtype == torch.int32 and tau_seg_t.numel() >= n_seg
    assert tau_win_t is None or (tau_win_t.dtype == torch.int32 and tau_win_t.numel() >= n_win)
    ctx.check(ctx.lib.tda_ami_segments_dev(ctx.h, _tp(win_t), _tp(seg_off_t), n_seg, n_t, lag, n_bins, _tp(tau_seg_t),
                                           _tp(tau_win_t), _stream()))
    return tau_seg_t


def fnn_dev(win_t, tau_t, d_max=5, theiler=1, r_tol=10.0, a_tol=2.0, frac_tol=0.05, nn=False, out=None, ctx=None):
    """fnn_batch on device tensors: win_t (n_win, n_t) float64, tau_t (n_win,) int32 -> a DeviceEmbedding (out, when given,
    needs d_max and, for nn=True, its nn block); nothing else is allocated."""
    import torch
    ctx = ctx or get_ctx()
    assert win_t.is_cuda and win_t.dtype == torch.float64 and win_t.is_contiguous() and win_t.dim() == 2
    n_win, n_t = (int(v) for v in win_t.shape)
    assert tau_t.is_cuda and tau_t.dtype == torch.int32 and tau_t.is_contiguous() and tau_t.numel() >= n_win
    par = fnn_args(n_t, d_max, theiler, r_tol, a_tol, frac_tol)
    if out is None:
        out = DeviceEmbedding(n_win, 0, par[0], win_t.device, 0, n_t if nn else 0)
    assert out.n_win >= n_win and out.d_max == par[0] and out.counts.is_contiguous()
    assert not nn or (out.nn is not None and tuple(out.nn.shape[1:]) == (par[0], n_t))
    ctx.check(ctx.lib.tda_fnn_batch_dev(ctx.h, _tp(win_t), _tp(tau_t), n_win, n_t, *par, _tp(out.counts), _tp(out.frac),
                                        _tp(out.dim), _tp(out.nn if nn else None), _tp(out.fnn_status), _stream()))
    return out


def recording_rows_dev(w0_t, w1_t, tau_seg_t, fe0_t, fe1_t, seg_off_t, out_t=None, status_a=None, status_b=None,
                       seg_flags=None, ctx=None):
    """(n_seg, 48) rows [nanmean W_H0, nanmean W_H1, tau, n_windows, 44 aggregated features] in one launch.
    seg_flags (optional, (n_seg,) int32): per group, OR of the class-overflow bits of the two status arrays."""
    import torch
    ctx = ctx or get_ctx()
    n_seg = seg_off_t.numel() - 1
    if out_t is None:
        out_t = torch.empty((n_seg, 4 + 4 * _lib.N_FEATURES), dtype=torch.float64, device=w0_t.device)
    assert out_t.is_contiguous()
    ctx.check(ctx.lib.tda_recording_rows_dev(ctx.h, _tp(w0_t), _tp(w1_t), _tp(tau_seg_t), _tp(fe0_t), _tp(fe1_t),
                                             _tp(seg_off_t), n_seg, _tp(out_t), _tp(status_a), _tp(status_b),
                                             _tp(seg_flags), _stream()))
    return out_t


_COLS_DEV = {}


def _cols_dev(cols, ld, device):
    """The column list on the device, uploaded once per (list, device): temporal_corr_dev must not copy inside a capture."""
    import torch
    key = (tuple(int(c) for c in cols), int(ld), str(device))
    t = _COLS_DEV.get(key)
    if t is None:
        t = _COLS_DEV[key] = torch.from_numpy(_check_cols(cols, ld)).to(device)
    return t


def temporal_corr_dev(fa_t, fe_t, seg_off_t, status_b=None, cols=SPEARMAN_COLS, out_t=None, ctx=None):
    """temporal_corr_batch on device tensors: fa_t, fe_t (n_win, ld) float64 (pipeline.Workspace's fa1 / fe1), seg_off_t
    int32, status_b the audio Rips status words or None -> out_t (n_seg, 2 * len(cols)) float64, [r, p] per column (for
    the default columns the order of drivers.DETAILED_COLUMNS[8:]).  One launch on torch's current stream; cols may
    also be an int32 device tensor."""
    import torch
    ctx = ctx or get_ctx()
    assert fa_t.is_cuda and fa_t.dtype == torch.float64 and fa_t.is_contiguous() and fa_t.dim() == 2
    assert fe_t.dtype == torch.float64 and fe_t.is_contiguous() and fe_t.shape == fa_t.shape
    assert seg_off_t.dtype == torch.int32 and seg_off_t.is_contiguous()
    assert status_b is None or (status_b.dtype == torch.int32 and status_b.is_contiguous() and status_b.numel() >= fa_t.shape[0])
    cols_t = cols if isinstance(cols, torch.Tensor) else _cols_dev(cols, fa_t.shape[1], fa_t.device)
    assert cols_t.dtype == torch.int32 and cols_t.is_cuda
    n_seg, n_cols = seg_off_t.numel() - 1, int(cols_t.numel())
    if out_t is None:
        out_t = torch.empty((n_seg, 2 * n_cols), dtype=torch.float64, device=fa_t.device)
    assert out_t.is_contiguous() and out_t.numel() >= n_seg * 2 * n_cols
    ctx.check(ctx.lib.tda_temporal_corr_dev(ctx.h, _tp(fa_t), _tp(fe_t), fa_t.shape[1], _tp(cols_t), n_cols, _tp(seg_off_t),
                                            n_seg, _tp(status_b), _tp(out_t), _stream()))
    return out_t


def features_dev(rows_t, cnt_t, feat_t=None, ctx=None):
    import torch
    ctx = ctx or get_ctx()
    n, cap, _ = rows_t.shape
    if feat_t is None:
        feat_t = torch.empty((n, _lib.N_FEATURES), dtype=torch.float64, device=rows_t.device)
    ctx.check(ctx.lib.tda_features_batch_dev(ctx.h, _tp(rows_t), _tp(cnt_t), n, cap, _tp(feat_t), _stream()))
    return feat_t


def diagram_finish_dev(sets, ctx=None):
    """ONE launch over up to four diagram sets: sets = [(rows_t (n, cap, 2), cnt_t (n,), order: bool, feat_t or
    None), ...] -- H1 rows into ripser's order where order is set, extract_features where feat_t is given."""
    ctx = ctx or get_ctx()
    arr = (_lib.DiagramSet * len(sets))()
    n = sets[0][0].shape[0]
    for i, (rows_t, cnt_t, order, feat_t) in enumerate(sets):
        assert rows_t.shape[0] == n and rows_t.is_contiguous()
        arr[i].rows = rows_t.data_ptr(); arr[i].cnt = cnt_t.data_ptr(); arr[i].cap = rows_t.shape[1]
        arr[i].order = int(bool(order)); arr[i].feat = feat_t.data_ptr() if feat_t is not None else None
    ctx.check(ctx.lib.tda_diagram_finish_dev(ctx.h, C.cast(arr, C.c_void_p), len(sets), n, _stream()))


def aggregate_dev(f0_t, f1_t, seg_off_t, out_t=None, ctx=None):
    import torch
    ctx = ctx or get_ctx()
    n_seg = seg_off_t.numel() - 1
    if out_t is None:
        out_t = torch.empty((n_seg, 4 * _lib.N_FEATURES), dtype=torch.float64, device=f0_t.device)
    ctx.check(ctx.lib.tda_aggregate_batch_dev(ctx.h, _tp(f0_t), _tp(f1_t), _tp(seg_off_t), n_seg, _tp(out_t),
                                              _stream()))
    return out_t


def segment_nanmean_dev(x_t, seg_off_t, out_t=None, ctx=None):
    import torch
    ctx = ctx or get_ctx()
    n_seg = seg_off_t.numel() - 1
    if out_t is None:
        out_t = torch.empty(n_seg, dtype=torch.float64, device=x_t.device)
    ctx.check(ctx.lib.tda_segment_nanmean_dev(ctx.h, _tp(x_t), _tp(seg_off_t), n_seg, _tp(out_t), _stream()))
    return out_t


def _pair_dev(entry, rows_a, cnt_a, rows_b, cnt_b, idx_a, idx_b, out_t, status_t, ctx, *extra):
    """The marshalling of the device-tensor pair distances: the entry point `entry` with `extra` arguments before out / status."""
    import torch
    n_pairs = rows_a.shape[0] if idx_a is None and idx_b is None else (idx_a if idx_a is not None else idx_b).numel()
    if out_t is None:
        out_t = torch.empty(n_pairs, dtype=torch.float64, device=rows_a.device)
    if status_t is None:
        status_t = torch.empty(n_pairs, dtype=torch.int32, device=rows_a.device)
    ctx.check(entry(ctx.h, _tp(rows_a), _tp(cnt_a), rows_a.shape[1], _tp(rows_b), _tp(cnt_b), rows_b.shape[1], _tp(idx_a), _tp(idx_b),
                    n_pairs, *extra, _tp(out_t), _tp(status_t), _stream()))
    return out_t, status_t


def wasserstein_dev(rows_a, cnt_a, rows_b, cnt_b, idx_a=None, idx_b=None, out_t=None, status_t=None, ctx=None):
    ctx = ctx or get_ctx()
    return _pair_dev(ctx.lib.tda_wasserstein_batch_dev, rows_a, cnt_a, rows_b, cnt_b, idx_a, idx_b, out_t, status_t, ctx)


def bottleneck_dev(rows_a, cnt_a, rows_b, cnt_b, idx_a=None, idx_b=None, out_t=None, status_t=None, ctx=None):
    """bottleneck_batch on device tensors: one launch on torch's current stream, nothing allocated when out_t and
    status_t are given.  out_t is NaN where status_t != 0."""
    ctx = ctx or get_ctx()
    return _pair_dev(ctx.lib.tda_bottleneck_batch_dev, rows_a, cnt_a, rows_b, cnt_b, idx_a, idx_b, out_t, status_t, ctx)


def wasserstein_q_dev(rows_a, cnt_a, rows_b, cnt_b, idx_a=None, idx_b=None, order=2, ground="l2", out_t=None, status_t=None,
                      ctx=None):
    """wasserstein_q_batch on device tensors: one launch on torch's current stream, nothing allocated when out_t and
    status_t are given.  out_t is NaN where status_t != 0."""
    order, ground = wasserstein_q_args(order, ground)
    ctx = ctx or get_ctx()
    return _pair_dev(ctx.lib.tda_wasserstein_q_batch_dev, rows_a, cnt_a, rows_b, cnt_b, idx_a, idx_b, out_t, status_t, ctx, order,
                     ground)


def persistence_fisher_dev(rows_a, cnt_a, rows_b, cnt_b, sigma, idx_a=None, idx_b=None, out_t=None, status_t=None, ctx=None):
    """persistence_fisher_batch on device tensors: one launch on torch's current stream, nothing allocated when out_t and
    status_t are given.  out_t is NaN where status_t != 0."""
    ninv = fisher_args(sigma)
    ctx = ctx or get_ctx()
    n_a, n_b = rows_a.shape[0], rows_b.shape[0]
    assert rows_a.is_contiguous() and rows_b.is_contiguous()

    def entry(h, a, ca, cap_a, b, cb, cap_b, *rest):     # the entry point also takes the sizes of the two sets
        return ctx.lib.tda_persistence_fisher_batch_dev(h, a, ca, n_a, cap_a, b, cb, n_b, cap_b, *rest)
    return _pair_dev(entry, rows_a, cnt_a, rows_b, cnt_b, idx_a, idx_b, out_t, status_t, ctx, ninv)


def persistence_fisher_gram_dev(rows, cnt, sigma, ctx=None):
    """persistence_fisher_gram on device tensors: the pairs i <= j in one launch with index lists built on the device,
    mirrored; an (n, n) float64 device tensor equal to persistence_fisher_gram bit for bit."""
    import torch
    fisher_args(sigma)
    n = rows.shape[0]
    G = torch.zeros((n, n), dtype=torch.float64, device=rows.device)
    if n:
        iu = torch.triu_indices(n, n, 0, device=rows.device)
        d, _ = persistence_fisher_dev(rows, cnt, rows, cnt, sigma, iu[0].to(torch.int32).contiguous(),
                                      iu[1].to(torch.int32).contiguous(), ctx=ctx)
        G[iu[0], iu[1]] = d
        G[iu[1], iu[0]] = d
    return G


def landscape_mean_dev(rows_t, cnt_t, grid_t, levels, seg_off_t=None, status_t=None, skip_mask=0, out_t=None, ctx=None):
    """Group means of [landscape levels 1..levels, Betti curve] of device diagrams (include/tdaeeg.h): one launch on
    torch's current stream, nothing allocated when out_t is given.  seg_off_t (n_seg + 1,) int32, or None: every diagram
    its own group.  Diagrams whose status_t word has a bit of skip_mask are left out; a group without a kept diagram is
    NaN.  out_t: (n_seg, levels + 1, n_grid)."""
    import torch
    ctx = ctx or get_ctx()
    n, cap, _ = rows_t.shape
    n_seg = n if seg_off_t is None else seg_off_t.numel() - 1
    n_grid, levels = grid_t.numel(), int(levels)
    if out_t is None:
        out_t = torch.empty((n_seg, max(levels, 0) + 1, n_grid), dtype=torch.float64, device=rows_t.device)
    assert rows_t.is_contiguous() and out_t.is_contiguous() and grid_t.is_contiguous()
    ctx.check(ctx.lib.tda_landscape_mean_dev(ctx.h, _tp(rows_t), _tp(cnt_t), cap, n, _tp(seg_off_t), n_seg, _tp(status_t),
                                             int(skip_mask), _tp(grid_t), n_grid, levels, _tp(out_t), _stream()))
    return out_t


def _euler_dev_args(grid_t, max_dim, n_win, out_t, status_t, device):
    """Checks of the euler_*_dev forms: grid_t a contiguous 1-D float64 device tensor of 1..MAX_GRID scales, max_dim as
    euler_args; out_t / status_t are allocated when None (they may be larger than the batch: the tail is not touched)."""
    import torch
    if not (grid_t.is_cuda and grid_t.dtype == torch.float64 and grid_t.dim() == 1 and grid_t.is_contiguous()):
        raise ValueError("grid_t: a contiguous 1-D float64 device tensor")
    n_grid = int(grid_t.numel())
    if not 1 <= n_grid <= _lib.MAX_GRID:
        raise ValueError(f"grid_t: 1..{_lib.MAX_GRID} scales")
    if isinstance(max_dim, bool) or not isinstance(max_dim, (int, np.integer)) or not 1 <= max_dim <= _lib.EC_MAX_DIM:
        raise ValueError(f"max_dim must be an integer in 1..{_lib.EC_MAX_DIM}, not {max_dim!r}")
    max_dim = int(max_dim)
    if out_t is None:
        out_t = torch.empty((n_win, max_dim + 2, n_grid), dtype=torch.int32, device=device)
    if status_t is None:
        status_t = torch.empty(n_win, dtype=torch.int32, device=device)
    assert out_t.dtype == torch.int32 and out_t.is_contiguous() and out_t.numel() >= n_win * (max_dim + 2) * n_grid
    assert status_t.dtype == torch.int32 and status_t.is_contiguous() and status_t.numel() >= n_win
    return n_grid, max_dim, out_t, status_t


def euler_mean_dev(counts_t, n_win, max_dim, n_grid, seg_off_t=None, status_in=None, skip_mask=0, mean_t=None, ctx=None):
    """Group means of the int32 blocks of euler_*_dev (include/tdaeeg.h): counts_t holds (n_win, max_dim + 2, n_grid);
    seg_off_t (n_seg + 1,) int32, or None: every window its own group.  Windows whose status_in word has a bit of skip_mask
    are left out; a group without a kept window is NaN.  mean_t: (n_seg, max_dim + 2, n_grid) float64.  One launch on
    torch's current stream, nothing allocated when mean_t is given."""
    import torch
    ctx = ctx or get_ctx()
    n_seg = n_win if seg_off_t is None else seg_off_t.numel() - 1
    if mean_t is None:
        mean_t = torch.empty((n_seg, max(int(max_dim), 0) + 2, max(int(n_grid), 0)), dtype=torch.float64, device=counts_t.device)
    assert counts_t.dtype == torch.int32 and counts_t.is_contiguous() and mean_t.is_contiguous()
    ctx.check(ctx.lib.tda_euler_mean_dev(ctx.h, _tp(counts_t), int(n_win), int(max_dim), int(n_grid), _tp(seg_off_t), n_seg,
                                         _tp(status_in), int(skip_mask), _tp(mean_t), _stream()))
    return mean_t


def _euler_dev_mean(out_t, status_t, n_win, max_dim, n_grid, mean_t, seg_off_t, status_in, skip_mask, ctx):
    """The optional second launch of the euler_*_dev forms: asked for by mean_t (a tensor, or True to have one allocated)
    or by seg_off_t.  status_in defaults to the status words the first launch has just written."""
    if mean_t is None and seg_off_t is None:
        return None
    return euler_mean_dev(out_t, n_win, max_dim, n_grid, seg_off_t, status_t if status_in is None else status_in, skip_mask,
                          None if mean_t is True else mean_t, ctx)


def euler_dm_dev(dm_t, grid_t, max_dim=3, thresh=MAX_EDGE_LENGTH, symmetrise=True, out_t=None, status_t=None, mean_t=None,
                 seg_off_t=None, status_in=None, skip_mask=0, ctx=None):
    """euler_dm_batch on device tensors: dm_t (n_win, n, n) float64, grid_t (n_grid,) float64 -> (out_t (n_win, max_dim + 2,
    n_grid) int32, status_t, mean or None).  One launch on torch's current stream (two with the group means), nothing
    allocated when the outputs are given."""
    import torch
    ctx = ctx or get_ctx()
    assert dm_t.is_cuda and dm_t.dtype == torch.float64 and dm_t.is_contiguous()
    n_win, n, n2 = dm_t.shape
    assert n == n2, "distance matrices must be square"
    n_grid, max_dim, out_t, status_t = _euler_dev_args(grid_t, max_dim, n_win, out_t, status_t, dm_t.device)
    ctx.check(ctx.lib.tda_euler_dm_batch_dev(ctx.h, _tp(dm_t), n_win, n, float(thresh), int(bool(symmetrise)), _tp(grid_t),
                                             n_grid, max_dim, _tp(out_t), _tp(status_t), _stream()))
    return out_t, status_t, _euler_dev_mean(out_t, status_t, n_win, max_dim, n_grid, mean_t, seg_off_t, status_in, skip_mask, ctx)


def euler_cloud_dev(pc_t, n_pts_t, grid_t, max_dim=3, normalise=True, thresh=MAX_EDGE_LENGTH, out_t=None, status_t=None,
                    mean_t=None, seg_off_t=None, status_in=None, skip_mask=0, ctx=None):
    """euler_cloud_batch on device tensors: pc_t (n_win, p_cap, dim) float64, n_pts_t (n_win,) int32."""
    import torch
    ctx = ctx or get_ctx()
    assert pc_t.is_cuda and pc_t.dtype == torch.float64 and pc_t.is_contiguous() and n_pts_t.dtype == torch.int32
    n_win, p_cap, dim = pc_t.shape
    n_grid, max_dim, out_t, status_t = _euler_dev_args(grid_t, max_dim, n_win, out_t, status_t, pc_t.device)
    ctx.check(ctx.lib.tda_euler_cloud_batch_dev(ctx.h, _tp(pc_t), _tp(n_pts_t), n_win, p_cap, dim, int(bool(normalise)),
                                                float(thresh), _tp(grid_t), n_grid, max_dim, _tp(out_t), _tp(status_t),
                                                _stream()))
    return out_t, status_t, _euler_dev_mean(out_t, status_t, n_win, max_dim, n_grid, mean_t, seg_off_t, status_in, skip_mask, ctx)


def euler_takens_dev(win_t, tau_t, grid_t, max_dim=3, dim=3, subsample=2, thresh=MAX_EDGE_LENGTH, out_t=None, status_t=None,
                     n_points_t=None, mean_t=None, seg_off_t=None, status_in=None, skip_mask=0, ctx=None):
    """euler_takens_batch on device tensors: win_t (n_win, n_t) float64, tau_t (n_win,) int32; n_points_t (optional, int32)
    receives the points per window."""
    import torch
    ctx = ctx or get_ctx()
    assert win_t.is_cuda and win_t.dtype == torch.float64 and win_t.is_contiguous()
    assert tau_t.dtype == torch.int32 and tau_t.is_cuda
    n_win, n_t = win_t.shape
    n_grid, max_dim, out_t, status_t = _euler_dev_args(grid_t, max_dim, n_win, out_t, status_t, win_t.device)
    ctx.check(ctx.lib.tda_euler_takens_batch_dev(ctx.h, _tp(win_t), _tp(tau_t), n_win, n_t, int(dim), int(subsample),
                                                 float(thresh), _tp(grid_t), n_grid, max_dim, _tp(out_t), _tp(n_points_t),
                                                 _tp(status_t), _stream()))
    return out_t, status_t, _euler_dev_mean(out_t, status_t, n_win, max_dim, n_grid, mean_t, seg_off_t, status_in, skip_mask, ctx)


def euler_eeg_windows_dev(win_t, grid_t, max_dim=3, thresh=MAX_EDGE_LENGTH, dist_t=None, out_t=None, status_t=None, mean_t=None,
                          seg_off_t=None, status_in=None, skip_mask=0, ctx=None):
    """corr_dist_dev followed by euler_dm_dev on EEG windows win_t (n_win, n_ch, n_t): the curves of exactly the matrix
    whose diagrams eeg_window_dev gives, so curve and diagram belong to one complex.  dist_t (optional) receives the
    matrices."""
    dist_t = corr_dist_dev(win_t, dist_t, ctx=ctx)
    return euler_dm_dev(dist_t, grid_t, max_dim, thresh, True, out_t, status_t, mean_t, seg_off_t, status_in, skip_mask, ctx)


class DeviceNetworkCurves:
    """The outputs of the network_*_dev forms for a batch of windows, resident in HBM (include/tdaeeg.h, "Network curves"):
    counts (n_win, NET_ROWS, n_grid) int32, measures (n_win, NET_MEASURES, n_grid) float64, status (n_win,) int32 and, when
    asked for, nodal (n_win, NET_NODAL, n_grid, n_node) int32; mean_counts, mean_measures and mean_nodal (float64, a row
    per group) are set by the group-mean launches."""

    def __init__(self, n_win, n_grid, n_node, device, nodal=False):
        import torch
        kw = dict(device=device)
        self.counts = torch.empty((n_win, _lib.NET_ROWS, n_grid), dtype=torch.int32, **kw)
        self.measures = torch.empty((n_win, _lib.NET_MEASURES, n_grid), dtype=torch.float64, **kw)
        self.nodal = torch.empty((n_win, _lib.NET_NODAL, n_grid, n_node), dtype=torch.int32, **kw) if nodal else None
        self.status = torch.empty(n_win, dtype=torch.int32, **kw)
        self.mean_counts = self.mean_measures = self.mean_nodal = None
        self.n_win, self.n_grid, self.n_node = n_win, n_grid, n_node

    def to_host(self):
        """The same arrays as numpy, in a dict."""
        return {k: getattr(self, k).cpu().numpy() for k in ("counts", "measures", "nodal", "status", "mean_counts",
                                                            "mean_measures", "mean_nodal") if getattr(self, k) is not None}


def network_mean_dev(counts_t, measures_t, nodal_t, n_win, n_grid, n_node, seg_off_t=None, status_in=None, skip_mask=0,
                     mean_counts_t=None, mean_measures_t=None, mean_nodal_t=None, ctx=None):
    """Group means of the blocks of network_*_dev (include/tdaeeg.h): each of counts_t, measures_t, nodal_t may be None and
    then has no mean.  seg_off_t (n_seg + 1,) int32, or None: every window its own group.  Windows whose status_in word has
    a bit of skip_mask are left out; a group without a kept window is NaN.  Returns (mean_counts, mean_measures,
    mean_nodal), float64 with a row per group; up to three launches on torch's current stream, nothing allocated when the
    means are given."""
    import torch
    ctx = ctx or get_ctx()
    n_win, n_grid, n_node = int(n_win), int(n_grid), int(n_node)
    n_seg = n_win if seg_off_t is None else seg_off_t.numel() - 1
    shapes = ((_lib.NET_ROWS, max(n_grid, 0)), (_lib.NET_MEASURES, max(n_grid, 0)), (_lib.NET_NODAL, max(n_grid, 0), max(n_node, 0)))
    ins, means = [counts_t, measures_t, nodal_t], [mean_counts_t, mean_measures_t, mean_nodal_t]
    for k, (t, dt) in enumerate(zip(ins, (torch.int32, torch.float64, torch.int32))):
        if t is None:
            continue
        assert t.dtype == dt and t.is_contiguous()
        if means[k] is None:
            means[k] = torch.empty((n_seg,) + shapes[k], dtype=torch.float64, device=t.device)
        assert means[k].dtype == torch.float64 and means[k].is_contiguous()
    ctx.check(ctx.lib.tda_network_mean_dev(ctx.h, _tp(counts_t), _tp(measures_t), _tp(nodal_t), n_win, n_grid, n_node,
                                           _tp(seg_off_t), n_seg, _tp(status_in), int(skip_mask), _tp(means[0]), _tp(means[1]),
                                           _tp(means[2]), _stream()))
    return tuple(means)


def _network_dev(grid_t, n_win, n_node, nodal, out, device):
    """Checks of the network_*_dev forms: grid_t a contiguous 1-D float64 device tensor of 1..MAX_GRID scales; out is
    allocated when None (it may be larger than the batch: the tail is not touched)."""
    import torch
    if not (grid_t.is_cuda and grid_t.dtype == torch.float64 and grid_t.dim() == 1 and grid_t.is_contiguous()):
        raise ValueError("grid_t: a contiguous 1-D float64 device tensor")
    n_grid = int(grid_t.numel())
    if not 1 <= n_grid <= _lib.MAX_GRID:
        raise ValueError(f"grid_t: 1..{_lib.MAX_GRID} scales")
    if out is None:
        out = DeviceNetworkCurves(n_win, n_grid, n_node, device, nodal)
    assert out.n_win >= n_win and (out.n_grid, out.n_node) == (n_grid, n_node)
    assert not nodal or out.nodal is not None, "nodal=True needs an out with a nodal tensor"
    return n_grid, out


def _network_dev_mean(out, n_win, nodal, mean, seg_off_t, status_in, skip_mask, ctx):
    """The optional group-mean launches of the network_*_dev forms: asked for by mean=True or by seg_off_t.  status_in
    defaults to the status words the first launch has just written."""
    if mean or seg_off_t is not None:
        out.mean_counts, out.mean_measures, out.mean_nodal = network_mean_dev(
            out.counts, out.measures, out.nodal if nodal else None, n_win, out.n_grid, out.n_node, seg_off_t,
            out.status if status_in is None else status_in, skip_mask, out.mean_counts, out.mean_measures,
            out.mean_nodal if nodal else None, ctx)
    return out


def network_dm_dev(dm_t, grid_t, nodal=False, thresh=MAX_EDGE_LENGTH, symmetrise=True, out=None, mean=False, seg_off_t=None,
                   status_in=None, skip_mask=0, ctx=None):
    """network_dm_batch on device tensors: dm_t (n_win, n, n) float64, grid_t (n_grid,) float64 -> a DeviceNetworkCurves.
    One launch on torch's current stream (up to three more with the group means), nothing allocated when out is given."""
    import torch
    ctx = ctx or get_ctx()
    assert dm_t.is_cuda and dm_t.dtype == torch.float64 and dm_t.is_contiguous()
    n_win, n, n2 = dm_t.shape
    assert n == n2, "distance matrices must be square"
    n_grid, out = _network_dev(grid_t, n_win, n, nodal, out, dm_t.device)
    ctx.check(ctx.lib.tda_network_dm_batch_dev(ctx.h, _tp(dm_t), n_win, n, float(thresh), int(bool(symmetrise)), _tp(grid_t),
                                               n_grid, _tp(out.counts), _tp(out.measures), _tp(out.nodal if nodal else None),
                                               _tp(out.status), _stream()))
    return _network_dev_mean(out, n_win, nodal, mean, seg_off_t, status_in, skip_mask, ctx)


def network_cloud_dev(pc_t, n_pts_t, grid_t, nodal=False, normalise=True, thresh=MAX_EDGE_LENGTH, out=None, mean=False,
                      seg_off_t=None, status_in=None, skip_mask=0, ctx=None):
    """network_cloud_batch on device tensors: pc_t (n_win, p_cap, dim) float64, n_pts_t (n_win,) int32."""
    import torch
    ctx = ctx or get_ctx()
    assert pc_t.is_cuda and pc_t.dtype == torch.float64 and pc_t.is_contiguous() and n_pts_t.dtype == torch.int32
    n_win, p_cap, dim = pc_t.shape
    n_grid, out = _network_dev(grid_t, n_win, p_cap, nodal, out, pc_t.device)
    ctx.check(ctx.lib.tda_network_cloud_batch_dev(ctx.h, _tp(pc_t), _tp(n_pts_t), n_win, p_cap, dim, int(bool(normalise)),
                                                  float(thresh), _tp(grid_t), n_grid, _tp(out.counts), _tp(out.measures),
                                                  _tp(out.nodal if nodal else None), _tp(out.status), _stream()))
    return _network_dev_mean(out, n_win, nodal, mean, seg_off_t, status_in, skip_mask, ctx)


def network_takens_dev(win_t, tau_t, grid_t, nodal=False, dim=3, subsample=2, thresh=MAX_EDGE_LENGTH, out=None,
                       n_points_t=None, mean=False, seg_off_t=None, status_in=None, skip_mask=0, ctx=None):
    """network_takens_batch on device tensors: win_t (n_win, n_t) float64, tau_t (n_win,) int32; n_points_t (optional,
    int32) receives the points per window.  nodal has MAX_POINTS columns."""
    import torch
    ctx = ctx or get_ctx()
    assert win_t.is_cuda and win_t.dtype == torch.float64 and win_t.is_contiguous()
    assert tau_t.dtype == torch.int32 and tau_t.is_cuda
    n_win, n_t = win_t.shape
    n_grid, out = _network_dev(grid_t, n_win, _lib.MAX_POINTS, nodal, out, win_t.device)
    ctx.check(ctx.lib.tda_network_takens_batch_dev(ctx.h, _tp(win_t), _tp(tau_t), n_win, n_t, int(dim), int(subsample),
                                                   float(thresh), _tp(grid_t), n_grid, _tp(out.counts), _tp(out.measures),
                                                   _tp(out.nodal if nodal else None), _tp(n_points_t), _tp(out.status),
                                                   _stream()))
    return _network_dev_mean(out, n_win, nodal, mean, seg_off_t, status_in, skip_mask, ctx)


def network_eeg_windows_dev(win_t, grid_t, nodal=False, thresh=MAX_EDGE_LENGTH, dist_t=None, out=None, mean=False,
                            seg_off_t=None, status_in=None, skip_mask=0, ctx=None):
    """corr_dist_dev followed by network_dm_dev on EEG windows win_t (n_win, n_ch, n_t): the graph measures of exactly the
    matrix whose diagrams eeg_window_dev gives, so the baseline and the diagram belong to one filtration.  dist_t
    (optional) receives the matrices."""
    dist_t = corr_dist_dev(win_t, dist_t, ctx=ctx)
    return network_dm_dev(dist_t, grid_t, nodal, thresh, True, out, mean, seg_off_t, status_in, skip_mask, ctx)


class DeviceRecurrenceCurves:
    """The outputs of the recurrence_*_dev forms for a batch of windows, resident in HBM (include/tdaeeg.h, "Recurrence
    curves"): counts (n_win, RQA_ROWS, n_grid) int32, measures (n_win, RQA_MEASURES, n_grid) float64, status (n_win,) int32
    and, when asked for, hist (n_win, 2, n_grid, n_hist) int32; mean_counts, mean_measures and mean_hist (float64, a row
    per group) are set by the group-mean launches."""

    def __init__(self, n_win, n_grid, n_hist, device, hist=False):
        import torch
        kw = dict(device=device)
        self.counts = torch.empty((n_win, _lib.RQA_ROWS, n_grid), dtype=torch.int32, **kw)
        self.measures = torch.empty((n_win, _lib.RQA_MEASURES, n_grid), dtype=torch.float64, **kw)
        self.hist = torch.empty((n_win, 2, n_grid, n_hist), dtype=torch.int32, **kw) if hist else None
        self.status = torch.empty(n_win, dtype=torch.int32, **kw)
        self.mean_counts = self.mean_measures = self.mean_hist = None
        self.n_win, self.n_grid, self.n_hist = n_win, n_grid, n_hist

    def to_host(self):
        """The same arrays as numpy, in a dict."""
        return {k: getattr(self, k).cpu().numpy() for k in ("counts", "measures", "hist", "status", "mean_counts",
                                                            "mean_measures", "mean_hist") if getattr(self, k) is not None}


def recurrence_mean_dev(counts_t, measures_t, hist_t, n_win, n_grid, n_hist, seg_off_t=None, status_in=None, skip_mask=0,
                        mean_counts_t=None, mean_measures_t=None, mean_hist_t=None, ctx=None):
    """Group means of the blocks of recurrence_*_dev (include/tdaeeg.h), by the rules of network_mean_dev: each of
    counts_t, measures_t, hist_t may be None and then has no mean.  Returns (mean_counts, mean_measures, mean_hist),
    float64 with a row per group; up to three launches on torch's current stream, nothing allocated when the means are
    given."""
    import torch
    ctx = ctx or get_ctx()
    n_win, n_grid, n_hist = int(n_win), int(n_grid), int(n_hist)
    n_seg = n_win if seg_off_t is None else seg_off_t.numel() - 1
    shapes = ((_lib.RQA_ROWS, max(n_grid, 0)), (_lib.RQA_MEASURES, max(n_grid, 0)), (2, max(n_grid, 0), max(n_hist, 0)))
    ins, means = [counts_t, measures_t, hist_t], [mean_counts_t, mean_measures_t, mean_hist_t]
    for k, (t, dt) in enumerate(zip(ins, (torch.int32, torch.float64, torch.int32))):
        if t is None:
            continue
        assert t.dtype == dt and t.is_contiguous()
        if means[k] is None:
            means[k] = torch.empty((n_seg,) + shapes[k], dtype=torch.float64, device=t.device)
        assert means[k].dtype == torch.float64 and means[k].is_contiguous()
    ctx.check(ctx.lib.tda_recurrence_mean_dev(ctx.h, _tp(counts_t), _tp(measures_t), _tp(hist_t), n_win, n_grid, n_hist,
                                              _tp(seg_off_t), n_seg, _tp(status_in), int(skip_mask), _tp(means[0]),
                                              _tp(means[1]), _tp(means[2]), _stream()))
    return tuple(means)


def _recurrence_dev(grid_t, theiler, l_min, v_min, n_win, n_hist, hist, out, device):
    """Checks of the recurrence_*_dev forms: grid_t a contiguous 1-D float64 device tensor of 1..MAX_GRID scales, the three
    ints as recurrence_args takes them; out is allocated when None (it may be larger than the batch: the tail is not
    touched)."""
    import torch
    if not (grid_t.is_cuda and grid_t.dtype == torch.float64 and grid_t.dim() == 1 and grid_t.is_contiguous()):
        raise ValueError("grid_t: a contiguous 1-D float64 device tensor")
    n_grid = int(grid_t.numel())
    if not 1 <= n_grid <= _lib.MAX_GRID:
        raise ValueError(f"grid_t: 1..{_lib.MAX_GRID} scales")
    _, theiler, l_min, v_min = recurrence_args(np.zeros(1), theiler, l_min, v_min)
    if out is None:
        out = DeviceRecurrenceCurves(n_win, n_grid, n_hist, device, hist)
    assert out.n_win >= n_win and (out.n_grid, out.n_hist) == (n_grid, n_hist)
    assert not hist or out.hist is not None, "hist=True needs an out with a hist tensor"
    return n_grid, (theiler, l_min, v_min), out


def _recurrence_dev_mean(out, n_win, hist, mean, seg_off_t, status_in, skip_mask, ctx):
    """The optional group-mean launches of the recurrence_*_dev forms: asked for by mean=True or by seg_off_t.  status_in
    defaults to the status words the first launch has just written."""
    if mean or seg_off_t is not None:
        out.mean_counts, out.mean_measures, out.mean_hist = recurrence_mean_dev(
            out.counts, out.measures, out.hist if hist else None, n_win, out.n_grid, out.n_hist, seg_off_t,
            out.status if status_in is None else status_in, skip_mask, out.mean_counts, out.mean_measures,
            out.mean_hist if hist else None, ctx)
    return out


def recurrence_dm_dev(dm_t, grid_t, theiler=1, l_min=2, v_min=2, hist=False, thresh=MAX_EDGE_LENGTH, symmetrise=True,
                      out=None, mean=False, seg_off_t=None, status_in=None, skip_mask=0, ctx=None):
    """recurrence_dm_batch on device tensors: dm_t (n_win, n, n) float64, grid_t (n_grid,) float64 -> a
    DeviceRecurrenceCurves.  One launch on torch's current stream (up to three more with the group means), nothing
    allocated when out is given."""
    import torch
    ctx = ctx or get_ctx()
    assert dm_t.is_cuda and dm_t.dtype == torch.float64 and dm_t.is_contiguous()
    n_win, n, n2 = dm_t.shape
    assert n == n2, "distance matrices must be square"
    n_grid, par, out = _recurrence_dev(grid_t, theiler, l_min, v_min, n_win, n, hist, out, dm_t.device)
    ctx.check(ctx.lib.tda_recurrence_dm_batch_dev(ctx.h, _tp(dm_t), n_win, n, float(thresh), int(bool(symmetrise)),
                                                  _tp(grid_t), n_grid, *par, _tp(out.counts), _tp(out.measures),
                                                  _tp(out.hist if hist else None), _tp(out.status), _stream()))
    return _recurrence_dev_mean(out, n_win, hist, mean, seg_off_t, status_in, skip_mask, ctx)


def recurrence_cloud_dev(pc_t, n_pts_t, grid_t, theiler=1, l_min=2, v_min=2, hist=False, normalise=True,
                         thresh=MAX_EDGE_LENGTH, out=None, mean=False, seg_off_t=None, status_in=None, skip_mask=0, ctx=None):
    """recurrence_cloud_batch on device tensors: pc_t (n_win, p_cap, dim) float64, n_pts_t (n_win,) int32."""
    import torch
    ctx = ctx or get_ctx()
    assert pc_t.is_cuda and pc_t.dtype == torch.float64 and pc_t.is_contiguous() and n_pts_t.dtype == torch.int32
    n_win, p_cap, dim = pc_t.shape
    n_grid, par, out = _recurrence_dev(grid_t, theiler, l_min, v_min, n_win, p_cap, hist, out, pc_t.device)
    ctx.check(ctx.lib.tda_recurrence_cloud_batch_dev(ctx.h, _tp(pc_t), _tp(n_pts_t), n_win, p_cap, dim, int(bool(normalise)),
                                                     float(thresh), _tp(grid_t), n_grid, *par, _tp(out.counts),
                                                     _tp(out.measures), _tp(out.hist if hist else None), _tp(out.status),
                                                     _stream()))
    return _recurrence_dev_mean(out, n_win, hist, mean, seg_off_t, status_in, skip_mask, ctx)


def recurrence_takens_dev(win_t, tau_t, grid_t, theiler=1, l_min=2, v_min=2, hist=False, dim=3, subsample=2,
                          thresh=MAX_EDGE_LENGTH, out=None, n_points_t=None, mean=False, seg_off_t=None, status_in=None,
                          skip_mask=0, ctx=None):
    """recurrence_takens_batch on device tensors: win_t (n_win, n_t) float64, tau_t (n_win,) int32; n_points_t (optional,
    int32) receives the points per window.  hist has MAX_POINTS columns."""
    import torch
    ctx = ctx or get_ctx()
    assert win_t.is_cuda and win_t.dtype == torch.float64 and win_t.is_contiguous()
    assert tau_t.dtype == torch.int32 and tau_t.is_cuda
    n_win, n_t = win_t.shape
    n_grid, par, out = _recurrence_dev(grid_t, theiler, l_min, v_min, n_win, _lib.MAX_POINTS, hist, out, win_t.device)
    ctx.check(ctx.lib.tda_recurrence_takens_batch_dev(ctx.h, _tp(win_t), _tp(tau_t), n_win, n_t, int(dim), int(subsample),
                                                      float(thresh), _tp(grid_t), n_grid, *par, _tp(out.counts),
                                                      _tp(out.measures), _tp(out.hist if hist else None), _tp(n_points_t),
                                                      _tp(out.status), _stream()))
    return _recurrence_dev_mean(out, n_win, hist, mean, seg_off_t, status_in, skip_mask, ctx)


class DeviceGenerators:
    """The outputs of the generators_*_dev forms for a batch of windows, resident in HBM (include/tdaeeg.h, "Generators
    and representative cycles"): h1_gen (n_win, h1_cap, 4) int16, h1_flag (n_win, h1_cap) int32, cyc (n_win, h1_cap,
    cyc_cap) int16, cyc_len (n_win, h1_cap) int32, status (n_win,) int32 and, when asked for, part (n_win, n_part) float64,
    h0_edge (n_win, h0_cap, 2) int16, work (n_win, 4, 2) int32; mean is set by the group-mean launch.  cyc=False (with
    part=False) leaves the cycle buffer out: edges, lengths and flags only."""

    def __init__(self, n_win, h0_cap, h1_cap, cyc_cap, n_part, device, part=True, h0_edge=True, work=False, cyc=True):
        import torch
        kw = dict(device=device)
        self.h1_gen = torch.empty((n_win, h1_cap, 4), dtype=torch.int16, **kw)
        self.h1_flag = torch.empty((n_win, h1_cap), dtype=torch.int32, **kw)
        self.cyc = torch.empty((n_win, h1_cap, cyc_cap), dtype=torch.int16, **kw) if cyc else None
        assert cyc or not part, "part is summed over the cycles: it needs cyc"
        self.cyc_len = torch.empty((n_win, h1_cap), dtype=torch.int32, **kw)
        self.status = torch.empty(n_win, dtype=torch.int32, **kw)
        self.part = torch.empty((n_win, n_part), dtype=torch.float64, **kw) if part else None
        self.h0_edge = torch.empty((n_win, h0_cap, 2), dtype=torch.int16, **kw) if h0_edge else None
        self.work = torch.empty((n_win, 4, 2), dtype=torch.int32, **kw) if work else None
        self.mean = None
        self.n_win, self.h0_cap, self.h1_cap, self.cyc_cap, self.n_part = n_win, h0_cap, h1_cap, cyc_cap, n_part

    def to_host(self):
        """The same arrays as numpy, in a dict keyed like generators_dm_batch's."""
        return {k: getattr(self, k).cpu().numpy() for k in ("h1_gen", "h1_flag", "cyc", "cyc_len", "part", "h0_edge", "work",
                                                            "status", "mean") if getattr(self, k) is not None}


def _gen_rows_dev(dgm):
    """The row tensors of a DeviceDiagrams, or of a tuple (h0_t, c0_t, h1_t, c1_t) with h0_t / c0_t None for no H0 rows."""
    import torch
    h0, c0, h1, c1 = (dgm.h0, dgm.c0, dgm.h1, dgm.c1) if isinstance(dgm, DeviceDiagrams) else dgm
    assert h1.is_cuda and h1.dtype == torch.float64 and h1.is_contiguous() and h1.dim() == 3 and h1.shape[2] == 2
    assert c1.dtype == torch.int32 and c1.is_contiguous()
    if h0 is not None:
        assert h0.dtype == torch.float64 and h0.is_contiguous() and h0.dim() == 3 and h0.shape[2] == 2
        assert c0 is not None and c0.dtype == torch.int32 and c0.is_contiguous()
    return h0, c0, h1, c1


def _gen_dev(n_win, n_part, dgm, cyc_cap, rips_status, part, h0_edge, work, out, device):
    """Checks and output buffers of the generators_*_dev forms -> (out, the shared tail of the C arguments).  out may be
    larger than the batch: the tail is not touched."""
    cyc_cap = generators_args(cyc_cap)
    h0, c0, h1, c1 = _gen_rows_dev(dgm)
    assert h1.shape[0] >= n_win and c1.numel() >= n_win and (h0 is None or (h0.shape[0] >= n_win and c0.numel() >= n_win))
    h1_cap = int(h1.shape[1])
    h0_cap = int(h0.shape[1]) if h0 is not None else 0
    if h1_cap < 1:
        raise ValueError("the H1 rows need h1_cap >= 1")
    if h0 is None:
        h0_edge = False
    if rips_status is None and isinstance(dgm, DeviceDiagrams):
        rips_status = dgm.status
    if out is None:
        out = DeviceGenerators(n_win, h0_cap, h1_cap, cyc_cap, n_part, device, part, h0_edge, work)
    assert out.n_win >= n_win and (out.h0_cap, out.h1_cap, out.cyc_cap, out.n_part) == (h0_cap, h1_cap, cyc_cap, n_part)
    tail = (_tp(h0), h0_cap, _tp(c0), _tp(h1), h1_cap, _tp(c1), _tp(rips_status))
    outs = (cyc_cap, _tp(out.h1_gen), _tp(out.h1_flag), _tp(out.cyc), _tp(out.cyc_len), _tp(out.part), _tp(out.h0_edge),
            _tp(out.work))
    return out, tail, outs


def generators_mean_dev(part_t, n_win, n, seg_off_t=None, status_in=None, skip_mask=0, mean_t=None, ctx=None):
    """Group means of the participation rows of generators_*_dev (include/tdaeeg.h): part_t holds (n_win, n) float64;
    seg_off_t (n_seg + 1,) int32, or None: every window its own group.  Windows whose status_in word has a bit of skip_mask
    are left out; a group without a kept window is NaN.  mean_t: (n_seg, n) float64.  One launch on torch's current
    stream, nothing allocated when mean_t is given."""
    import torch
    ctx = ctx or get_ctx()
    n_seg = n_win if seg_off_t is None else seg_off_t.numel() - 1
    if mean_t is None:
        mean_t = torch.empty((n_seg, max(int(n), 0)), dtype=torch.float64, device=part_t.device)
    assert part_t.dtype == torch.float64 and part_t.is_contiguous() and mean_t.is_contiguous()
    ctx.check(ctx.lib.tda_generators_mean_dev(ctx.h, _tp(part_t), int(n_win), int(n), _tp(seg_off_t), n_seg, _tp(status_in),
                                              int(skip_mask), _tp(mean_t), _stream()))
    return mean_t


def _gen_dev_mean(out, n_win, seg_off_t, status_in, mean_skip, ctx):
    """The optional second launch of the generators_*_dev forms, asked for by seg_off_t: the group means of part over the
    windows whose status_in word (default: none skipped) has no bit of mean_skip."""
    if seg_off_t is not None:
        assert out.part is not None, "the group means need part"
        out.mean = generators_mean_dev(out.part, n_win, out.n_part, seg_off_t, status_in, mean_skip, ctx=ctx)
    return out


def generators_dm_dev(dm_t, dgm, thresh=MAX_EDGE_LENGTH, symmetrise=True, cyc_cap=_lib.MAX_POINTS, rips_status=None,
                      skip_mask=0, part=True, h0_edge=True, work=False, out=None, seg_off_t=None, status_in=None,
                      mean_skip=0, ctx=None):
    """generators_dm_batch on device tensors: dm_t (n_win, n, n) float64 and the diagrams rips_dm_dev / eeg_window_dev
    wrote for it -- dgm an engine.DeviceDiagrams (its status words are rips_status then) or the raw row tensors (h0_t, c0_t,
    h1_t, c1_t).  Returns a DeviceGenerators.  One launch on torch's current stream (two with seg_off_t: the group means of
    part), nothing allocated when out is given."""
    import torch
    ctx = ctx or get_ctx()
    assert dm_t.is_cuda and dm_t.dtype == torch.float64 and dm_t.is_contiguous()
    n_win, n, n2 = dm_t.shape
    assert n == n2, "distance matrices must be square"
    out, rows, outs = _gen_dev(n_win, n, dgm, cyc_cap, rips_status, part, h0_edge, work, out, dm_t.device)
    ctx.check(ctx.lib.tda_generators_dm_batch_dev(ctx.h, _tp(dm_t), n_win, n, float(thresh), int(bool(symmetrise)), *rows,
                                                  int(skip_mask), *outs, _tp(out.status), _stream()))
    return _gen_dev_mean(out, n_win, seg_off_t, status_in, mean_skip, ctx)


def generators_cloud_dev(pc_t, n_pts_t, dgm, normalise=True, thresh=MAX_EDGE_LENGTH, cyc_cap=_lib.MAX_POINTS,
                         rips_status=None, skip_mask=0, part=True, h0_edge=True, work=False, out=None, seg_off_t=None,
                         status_in=None, mean_skip=0, ctx=None):
    """generators_cloud_batch on device tensors: pc_t (n_win, p_cap, dim) float64, n_pts_t (n_win,) int32."""
    import torch
    ctx = ctx or get_ctx()
    assert pc_t.is_cuda and pc_t.dtype == torch.float64 and pc_t.is_contiguous() and n_pts_t.dtype == torch.int32
    n_win, p_cap, dim = pc_t.shape
    out, rows, outs = _gen_dev(n_win, p_cap, dgm, cyc_cap, rips_status, part, h0_edge, work, out, pc_t.device)
    ctx.check(ctx.lib.tda_generators_cloud_batch_dev(ctx.h, _tp(pc_t), _tp(n_pts_t), n_win, p_cap, dim, int(bool(normalise)),
                                                     float(thresh), *rows, int(skip_mask), *outs, _tp(out.status), _stream()))
    return _gen_dev_mean(out, n_win, seg_off_t, status_in, mean_skip, ctx)


def generators_takens_dev(win_t, tau_t, dgm, dim=3, subsample=2, thresh=MAX_EDGE_LENGTH, cyc_cap=_lib.MAX_POINTS,
                          rips_status=None, skip_mask=0, part=True, h0_edge=True, work=False, out=None, n_points_t=None,
                          seg_off_t=None, status_in=None, mean_skip=0, ctx=None):
    """generators_takens_batch on device tensors: win_t (n_win, n_t) float64, tau_t (n_win,) int32; n_points_t (optional,
    int32) receives the points per window.  part has MAX_POINTS columns."""
    import torch
    ctx = ctx or get_ctx()
    assert win_t.is_cuda and win_t.dtype == torch.float64 and win_t.is_contiguous()
    assert tau_t.dtype == torch.int32 and tau_t.is_cuda
    n_win, n_t = win_t.shape
    out, rows, outs = _gen_dev(n_win, _lib.MAX_POINTS, dgm, cyc_cap, rips_status, part, h0_edge, work, out, win_t.device)
    ctx.check(ctx.lib.tda_generators_takens_batch_dev(ctx.h, _tp(win_t), _tp(tau_t), n_win, n_t, int(dim), int(subsample),
                                                      float(thresh), *rows, int(skip_mask), *outs, _tp(n_points_t),
                                                      _tp(out.status), _stream()))
    return _gen_dev_mean(out, n_win, seg_off_t, status_in, mean_skip, ctx)


def generators_eeg_windows_dev(win_t, thresh=MAX_EDGE_LENGTH, h1_cap=DEFAULT_H1_CAP, cyc_cap=_lib.MAX_POINTS, skip_mask=0,
                               part=True, h0_edge=True, work=False, dist_t=None, dgm=None, out=None, seg_off_t=None,
                               status_in=None, mean_skip=0, ctx=None):
    """eeg_window_dev with its dist output, then generators_dm_dev on the matrices and the diagrams that one launch wrote:
    edges and cycles of exactly the rows the fused EEG kernel gives.  Returns (diagrams, DeviceGenerators); dist_t
    (optional) receives the matrices."""
    import torch
    n_win, n_ch, _ = win_t.shape
    if dist_t is None:
        dist_t = torch.empty((n_win, n_ch, n_ch), dtype=torch.float64, device=win_t.device)
    dgm = eeg_window_dev(win_t, dgm, thresh, h1_cap, dist_t=dist_t, ctx=ctx)
    return dgm, generators_dm_dev(dist_t, dgm, thresh, True, cyc_cap, None, skip_mask, part, h0_edge, work, out, seg_off_t,
                                  status_in, mean_skip, ctx)


def frechet_mean_dev(rows_t, cnt_t, seg_off_t=None, status_t=None, skip_mask=0, max_iter=32, cap_out=None, out=None, ctx=None):
    """frechet_mean_batch on device tensors: one launch on torch's current stream, nothing allocated when out is given.
    out: the tensors (mean (n_seg, cap_out, 2) float64, count, variance float64, iters, status) -- int32 where not said
    otherwise; the rows of mean beyond the count are left as they were (the NaN padding is the caller's).  Returns out."""
    import torch
    ctx = ctx or get_ctx()
    n, cap, _ = rows_t.shape
    n_seg = n if seg_off_t is None else seg_off_t.numel() - 1
    if out is None:
        cap_out, max_iter = frechet_args(_lib.FM_MAX_POINTS if cap_out is None else cap_out, max_iter)
        dev = rows_t.device
        out = (torch.full((n_seg, cap_out, 2), float("nan"), dtype=torch.float64, device=dev),
               torch.empty(n_seg, dtype=torch.int32, device=dev), torch.empty(n_seg, dtype=torch.float64, device=dev),
               torch.empty(n_seg, dtype=torch.int32, device=dev), torch.empty(n_seg, dtype=torch.int32, device=dev))
    else:
        cap_out, max_iter = frechet_args(out[0].shape[1], max_iter)
    mean_t, mc_t, var_t, it_t, st_t = out
    assert rows_t.is_contiguous() and all(o.is_contiguous() for o in out)
    ctx.check(ctx.lib.tda_frechet_mean_dev(ctx.h, _tp(rows_t), _tp(cnt_t), cap, n, _tp(seg_off_t), n_seg, _tp(status_t),
                                           int(skip_mask), max_iter, _tp(mean_t), _tp(mc_t), cap_out, _tp(var_t), _tp(it_t),
                                           _tp(st_t), _stream()))
    return out


def image_mean_dev(rows_t, cnt_t, xe_t, ye_t, sigma, power, seg_off_t=None, status_t=None, skip_mask=0, out_t=None, ctx=None):
    """Group means of the persistence images of device diagrams (include/tdaeeg.h): one launch on torch's current stream,
    nothing allocated when out_t is given.  xe_t (n_x + 1,), ye_t (n_y + 1,) float64 edges on the device; seg_off_t
    (n_seg + 1,) int32, or None: every diagram its own group.  Diagrams whose status_t word has a bit of skip_mask are left
    out; a group without a kept diagram is NaN.  out_t: (n_seg, n_y, n_x)."""
    import torch
    ctx = ctx or get_ctx()
    n, cap, _ = rows_t.shape
    n_seg = n if seg_off_t is None else seg_off_t.numel() - 1
    n_x, n_y = xe_t.numel() - 1, ye_t.numel() - 1
    if out_t is None:
        out_t = torch.empty((n_seg, max(n_y, 0), max(n_x, 0)), dtype=torch.float64, device=rows_t.device)
    assert rows_t.is_contiguous() and out_t.is_contiguous() and xe_t.is_contiguous() and ye_t.is_contiguous()
    ctx.check(ctx.lib.tda_image_mean_dev(ctx.h, _tp(rows_t), _tp(cnt_t), cap, n, _tp(seg_off_t), n_seg, _tp(status_t),
                                         int(skip_mask), _tp(xe_t), n_x, _tp(ye_t), n_y, float(sigma), int(power),
                                         _tp(out_t), _stream()))
    return out_t


def sliced_wasserstein_dev(rows_a, cnt_a, rows_b, cnt_b, dirs_t, idx_a=None, idx_b=None, out_t=None, status_t=None, ctx=None):
    """sliced_wasserstein_batch on device tensors (dirs_t: (M, 2) float64, resident): one launch on torch's current stream,
    nothing allocated when out_t and status_t are given.  out_t is NaN where status_t != 0.  The directions cannot be
    looked at here: validate them on the host before the upload."""
    import torch
    ctx = ctx or get_ctx()
    if dirs_t.dim() != 2 or dirs_t.shape[1] != 2 or dirs_t.dtype != torch.float64 or not dirs_t.is_contiguous():
        raise _lib.TdaError("libtdaeeg error 1: dirs_t must be a contiguous (M, 2) float64 tensor")
    return _pair_dev(ctx.lib.tda_sliced_wasserstein_batch_dev, rows_a, cnt_a, rows_b, cnt_b, idx_a, idx_b, out_t, status_t, ctx,
                     _tp(dirs_t), dirs_t.shape[0])


def diagram_kernel_dev(rows_a, cnt_a, rows_b, cnt_b, kernel, idx_a=None, idx_b=None, out_t=None, status_t=None, kvals_t=None,
                       ctx=None):
    """diagram_kernel_batch on device tensors: one launch on torch's current stream, nothing allocated when out_t and
    status_t are given.  kvals_t: an optional (n_pairs, 3) float64 tensor for [k_ab, k_aa, k_bb].  Returns (out_t,
    status_t); out_t is NaN where status_t != 0."""
    import torch
    par = _kernel_params(kernel)
    ctx = ctx or get_ctx()
    n_pairs = rows_a.shape[0] if idx_a is None and idx_b is None else (idx_a if idx_a is not None else idx_b).numel()
    if out_t is None:
        out_t = torch.empty(n_pairs, dtype=torch.float64, device=rows_a.device)
    if status_t is None:
        status_t = torch.empty(n_pairs, dtype=torch.int32, device=rows_a.device)
    assert rows_a.is_contiguous() and rows_b.is_contiguous() and (kvals_t is None or kvals_t.is_contiguous())
    ctx.check(ctx.lib.tda_diagram_kernel_pairs_dev(ctx.h, _tp(rows_a), _tp(cnt_a), rows_a.shape[0], rows_a.shape[1], _tp(rows_b),
                                                   _tp(cnt_b), rows_b.shape[0], rows_b.shape[1], _tp(idx_a), _tp(idx_b), n_pairs,
                                                   *par, _tp(out_t), _tp(kvals_t), _tp(status_t), _stream()))
    return out_t, status_t


def diagram_kernel_gram_dev(rows_a, cnt_a, kernel, seg_off_a=None, status_a=None, rows_b=None, cnt_b=None, seg_off_b=None,
                            status_b=None, skip_mask=0, out_t=None, ctx=None):
    """diagram_kernel_gram on device tensors: one launch on torch's current stream, nothing allocated when out_t is given.
    out_t: (n_seg_a, n_seg_a) without rows_b, (n_seg_a, n_seg_b) with it."""
    import torch
    par = _kernel_params(kernel)
    ctx = ctx or get_ctx()
    n_a, cap_a, _ = rows_a.shape
    n_ga = n_a if seg_off_a is None else seg_off_a.numel() - 1
    n_b = cap_b = 0
    n_gb = n_ga
    if rows_b is not None:
        n_b, cap_b, _ = rows_b.shape
        n_gb = n_b if seg_off_b is None else seg_off_b.numel() - 1
    if out_t is None:
        out_t = torch.empty((n_ga, n_gb), dtype=torch.float64, device=rows_a.device)
    assert rows_a.is_contiguous() and out_t.is_contiguous() and tuple(out_t.shape) == (n_ga, n_gb)
    if rows_b is not None and n_b == 0:              # nothing on the B side: every group of it is empty
        diagram_kernel_check(par, cap_a)
        return out_t.fill_(float("nan"))
    assert rows_b is None or rows_b.is_contiguous()
    ctx.check(ctx.lib.tda_diagram_kernel_gram_dev(ctx.h, _tp(rows_a), _tp(cnt_a), n_a, cap_a, _tp(seg_off_a), n_ga, _tp(status_a),
                                                  _tp(rows_b), _tp(cnt_b), n_b, cap_b, _tp(seg_off_b),
                                                  n_gb if rows_b is not None else 0, _tp(status_b), int(skip_mask), *par,
                                                  _tp(out_t), _stream()))
    return out_t


def group_table(seg_off_t, n):
    """(n,) int32: the group of each of the n members of a segment table, made on the device without a host
    synchronisation: what wasserstein_cross_dev takes as grp_a.  Plans that know their tables upload it instead."""
    import torch
    pos = torch.arange(n, dtype=seg_off_t.dtype, device=seg_off_t.device)
    return torch.searchsorted(seg_off_t[1:].contiguous(), pos, right=True).to(torch.int32)


def wasserstein_cross_dev(rows_a, cnt_a, seg_off_a, rows_b, cnt_b, seg_off_b, status_b, partner_seg, grp_a=None, out_t=None,
                          status_t=None, ctx=None):
    """mvm:86-95 for every (recording, band) group at once: A diagram w at position i of group g is paired with B
    diagram seg_off_b[p] + i of group p = partner_seg[g]; out[w] = NaN and status[w] = TDA_WIN_NO_PAIR where there is
    none (p < 0, the B group is shorter, or the B diagram is degenerate).  All tables int32 device tensors; grp_a:
    (n_a,) group of every A diagram (group_table(seg_off_a, n_a) when not given)."""
    import torch
    ctx = ctx or get_ctx()
    n_a, n_b = rows_a.shape[0], rows_b.shape[0]
    n_seg_a, n_seg_b = seg_off_a.numel() - 1, seg_off_b.numel() - 1
    for t in (seg_off_a, seg_off_b, status_b, partner_seg):
        assert t.dtype == torch.int32 and t.is_cuda and t.is_contiguous()
    assert partner_seg.numel() == n_seg_a and status_b.numel() >= n_b and cnt_a.numel() >= n_a and cnt_b.numel() >= n_b
    if grp_a is None:
        grp_a = group_table(seg_off_a, n_a)
    assert grp_a.dtype == torch.int32 and grp_a.numel() >= n_a and grp_a.is_contiguous()
    if out_t is None:
        out_t = torch.empty(n_a, dtype=torch.float64, device=rows_a.device)
    if status_t is None:
        status_t = torch.empty(n_a, dtype=torch.int32, device=rows_a.device)
    assert out_t.numel() >= n_a and status_t.numel() >= n_a
    ctx.check(ctx.lib.tda_wasserstein_cross_dev(ctx.h, _tp(rows_a), _tp(cnt_a), rows_a.shape[1], n_a, _tp(grp_a), _tp(seg_off_a),
                                                n_seg_a, _tp(rows_b), _tp(cnt_b), rows_b.shape[1], n_b, _tp(seg_off_b), n_seg_b,
                                                _tp(status_b), _tp(partner_seg), _tp(out_t), _tp(status_t), _stream()))
    return out_t, status_t


def cross_rows_dev(w_m, st_m, w_x, st_x, seg_off_a, out_t=None, status_a=None, seg_flags=None, ctx=None):
    """(n_seg, 4) rows [nanmean matched, nanmean mismatched, matched pairs, mismatched pairs] from the outputs of two
    wasserstein_cross_dev calls over the same A side (mvm:89-95).  seg_flags (optional, (n_seg,) int32): per group, OR of
    status_a (the A side's Rips status) and the solver status words, without TDA_WIN_NO_PAIR / TDA_WIN_DEGENERATE."""
    import torch
    ctx = ctx or get_ctx()
    n_seg = seg_off_a.numel() - 1
    if out_t is None:
        out_t = torch.empty((n_seg, 4), dtype=torch.float64, device=w_m.device)
    assert out_t.is_contiguous() and out_t.numel() >= 4 * n_seg and seg_off_a.dtype == torch.int32
    ctx.check(ctx.lib.tda_cross_rows_dev(ctx.h, _tp(w_m), _tp(st_m), _tp(w_x), _tp(st_x), _tp(seg_off_a), n_seg, _tp(out_t),
                                         _tp(status_a), _tp(seg_flags), _stream()))
    return out_t


MATCH_COLS = 6              # [w_own, n_own_pairs, n_valid, n_less, n_equal, null_mean]


def wasserstein_matrix_dev(rows_a, cnt_a, seg_off_a, cls_a, rows_b, cnt_b, seg_off_b, status_b, n_col, out_t=None,
                           pairs_t=None, flags_t=None, ctx=None):
    """mvm:86-95 of every A group against EVERY candidate column at once.  The B groups are class-major: the group of
    (class k, column c) is k * n_col + c, so seg_off_b has n_cls * n_col + 1 entries; cls_a (n_seg_a,) names the class
    (band) of every A group.  Returns out (n_seg_a, n_col) float64, pairs and flags (n_seg_a, n_col) int32: entry (g, c)
    is the mismatched mean, pair count and flags that wasserstein_cross_dev with partner_seg[g] = cls_a[g] * n_col + c
    and cross_rows_dev give, bit for bit.  All tables int32 device tensors."""
    import torch
    ctx = ctx or get_ctx()
    n_a, n_b = rows_a.shape[0], rows_b.shape[0]
    n_seg_a, n_col = seg_off_a.numel() - 1, int(n_col)
    n_cls = (seg_off_b.numel() - 1) // n_col if n_col else 0
    for t in (seg_off_a, cls_a, seg_off_b, status_b):
        assert t.dtype == torch.int32 and t.is_cuda and t.is_contiguous()
    assert seg_off_b.numel() == n_cls * n_col + 1 and cls_a.numel() == n_seg_a
    assert status_b.numel() >= n_b and cnt_a.numel() >= n_a and cnt_b.numel() >= n_b
    if out_t is None:
        out_t = torch.empty((n_seg_a, n_col), dtype=torch.float64, device=rows_a.device)
    if pairs_t is None:
        pairs_t = torch.empty((n_seg_a, n_col), dtype=torch.int32, device=rows_a.device)
    if flags_t is None:
        flags_t = torch.empty((n_seg_a, n_col), dtype=torch.int32, device=rows_a.device)
    for t in (out_t, pairs_t, flags_t):
        assert t.is_contiguous() and t.numel() >= n_seg_a * n_col
    ctx.check(ctx.lib.tda_wasserstein_matrix_dev(ctx.h, _tp(rows_a), _tp(cnt_a), rows_a.shape[1], n_a, _tp(seg_off_a), n_seg_a,
                                                 _tp(cls_a), _tp(rows_b), _tp(cnt_b), rows_b.shape[1], n_b, _tp(seg_off_b),
                                                 n_cls, n_col, _tp(status_b), _tp(out_t), _tp(pairs_t), _tp(flags_t), _stream()))
    return out_t, pairs_t, flags_t


def match_rows_dev(out_t, pairs_t, flags_t, own_col, rows_t=None, status_a=None, seg_off_a=None, seg_flags=None, ctx=None):
    """(n_seg_a, 6) rows [w_own, n_own_pairs, n_valid, n_less, n_equal, null_mean] from the (n_seg_a, n_col) outputs of
    wasserstein_matrix_dev and own_col (n_seg_a,) int32, the column of every group's own audio or -1.  seg_flags
    (optional, (n_seg_a,) int32): per group, OR of the row's flags and of status_a over the group (seg_off_a), without
    TDA_WIN_NO_PAIR / TDA_WIN_DEGENERATE."""
    import torch
    ctx = ctx or get_ctx()
    n_seg_a = own_col.numel()
    n_col = out_t.numel() // n_seg_a if n_seg_a else 0
    assert own_col.dtype == torch.int32 and out_t.is_contiguous() and pairs_t.is_contiguous() and flags_t.is_contiguous()
    assert status_a is None or (seg_off_a is not None and seg_off_a.numel() == n_seg_a + 1)
    if rows_t is None:
        rows_t = torch.empty((n_seg_a, MATCH_COLS), dtype=torch.float64, device=own_col.device)
    assert rows_t.is_contiguous() and rows_t.numel() >= MATCH_COLS * n_seg_a
    ctx.check(ctx.lib.tda_match_rows_dev(ctx.h, _tp(out_t), _tp(pairs_t), _tp(flags_t), n_seg_a, n_col, _tp(own_col),
                                         _tp(status_a), _tp(seg_off_a), _tp(rows_t), _tp(seg_flags), _stream()))
    return rows_t


# ------------------------------------------------------------------ sliced Wasserstein from prepared diagrams
class SlicedTable:
    """What sliced_prepare_dev leaves on the device: `table` (flat float64, 2 * n_dirs doubles per slot row), `slot_off`
    ((n_dgm + 1,) int64), `m` ((n_dgm,) int32: rows after cleaning, -1 where a diagram was not prepared) and n_dirs.  Two
    tables can meet in sliced_wasserstein_prepared_dev / sliced_matrix_dev when they were made with the same directions."""

    def __init__(self, table, slot_off, m, n_dirs):
        self.table, self.slot_off, self.m, self.n_dirs = table, slot_off, m, int(n_dirs)

    @property
    def n_dgm(self):
        return self.m.numel()


def sliced_slots_dev(cnt, cap, out=None):
    """(n_dgm + 1,) int64 slot table of sliced_prepare_dev: the exclusive scan of max(min(cnt, cap), 1), made on the device
    without a host synchronisation.  Its last element is the number of table rows the diagrams need.  out: a contiguous
    int64 tensor of n_dgm + 1 elements to fill."""
    import torch
    slot_off = torch.empty(cnt.numel() + 1, dtype=torch.int64, device=cnt.device) if out is None else out
    assert slot_off.dtype == torch.int64 and slot_off.numel() == cnt.numel() + 1 and slot_off.is_contiguous()
    slot_off[:1] = 0
    torch.cumsum(torch.clamp(cnt, 1, int(cap)), 0, out=slot_off[1:])
    return slot_off


def sliced_prepare_dev(rows, cnt, dirs_t, table_t=None, slot_off=None, m_t=None, ctx=None):
    """Sort every diagram once for the sliced Wasserstein distance (tda_sliced_prepare_dev): per diagram and direction of
    dirs_t ((M, 2) float64, resident, validated on the host before the upload) the ascending projections of its rows and of
    its diagonal images.  One launch on torch's current stream.  slot_off: (n_dgm + 1,) int64 (default sliced_slots_dev:
    packed, as many rows as a diagram can have after cleaning); table_t: flat float64 of 2 * M doubles per row (default:
    n_dgm * cap rows, which holds any slot table of this kind without a look at its total).  Returns a SlicedTable."""
    import torch
    ctx = ctx or get_ctx()
    if dirs_t.dim() != 2 or dirs_t.shape[1] != 2 or dirs_t.dtype != torch.float64 or not dirs_t.is_contiguous():
        raise _lib.TdaError("libtdaeeg error 1: dirs_t must be a contiguous (M, 2) float64 tensor")
    n_dgm, cap, n_dirs = rows.shape[0], rows.shape[1], dirs_t.shape[0]
    assert rows.is_contiguous() and cnt.dtype == torch.int32 and cnt.numel() >= n_dgm
    if slot_off is None:
        slot_off = sliced_slots_dev(cnt[:n_dgm], cap)
    assert slot_off.dtype == torch.int64 and slot_off.is_contiguous() and slot_off.numel() == n_dgm + 1
    if table_t is None:
        table_t = torch.empty(2 * n_dirs * n_dgm * cap, dtype=torch.float64, device=rows.device)
    assert table_t.dtype == torch.float64 and table_t.is_contiguous()
    table_rows = table_t.numel() // (2 * n_dirs) if n_dirs else 0
    if m_t is None:
        m_t = torch.empty(n_dgm, dtype=torch.int32, device=rows.device)
    assert m_t.dtype == torch.int32 and m_t.is_contiguous() and m_t.numel() >= n_dgm
    ctx.check(ctx.lib.tda_sliced_prepare_dev(ctx.h, _tp(rows), _tp(cnt), cap, n_dgm, _tp(dirs_t), n_dirs, _tp(slot_off),
                                             _tp(table_t), table_rows, _tp(m_t), _stream()))
    return SlicedTable(table_t, slot_off, m_t[:n_dgm], n_dirs)


def sliced_wasserstein_prepared_dev(ta, tb, idx_a=None, idx_b=None, out_t=None, status_t=None, ctx=None):
    """The sliced Wasserstein distance of pairs of prepared diagrams (SlicedTable ta, tb of the same directions): two
    merges and a sum per pair and direction, the bytes sliced_wasserstein_dev gives for the same pair.  idx_a / idx_b:
    int32 device tensors or None (identity).  out_t is NaN where status_t != 0."""
    import torch
    ctx = ctx or get_ctx()
    if ta.n_dirs != tb.n_dirs:
        raise _lib.TdaError("libtdaeeg error 1: the two tables were prepared with different numbers of directions")
    n_pairs = ta.n_dgm if idx_a is None and idx_b is None else (idx_a if idx_a is not None else idx_b).numel()
    for t in (idx_a, idx_b):
        assert t is None or (t.dtype == torch.int32 and t.is_contiguous() and t.numel() >= n_pairs)
    dev = ta.table.device
    if out_t is None:
        out_t = torch.empty(n_pairs, dtype=torch.float64, device=dev)
    if status_t is None:
        status_t = torch.empty(n_pairs, dtype=torch.int32, device=dev)
    ctx.check(ctx.lib.tda_sliced_prepared_pairs_dev(ctx.h, _tp(ta.table), _tp(ta.slot_off), _tp(ta.m), ta.n_dgm, _tp(tb.table),
                                                    _tp(tb.slot_off), _tp(tb.m), tb.n_dgm, _tp(idx_a), _tp(idx_b), n_pairs,
                                                    ta.n_dirs, _tp(out_t), _tp(status_t), _stream()))
    return out_t, status_t


def sliced_wasserstein_gram_dev(rows, cnt, dirs_t, ctx=None):
    """sliced_wasserstein_gram on device tensors by the prepared route: one sliced_prepare_dev, the pairs i < j through
    sliced_wasserstein_prepared_dev with index lists built on the device, mirrored, zero diagonal; an (n, n) float64
    device tensor equal to sliced_wasserstein_gram bit for bit (NaN where a pair has a status)."""
    import torch
    n = rows.shape[0]
    G = torch.zeros((n, n), dtype=torch.float64, device=rows.device)
    t = sliced_prepare_dev(rows, cnt, dirs_t, ctx=ctx)
    if n > 1:
        iu = torch.triu_indices(n, n, 1, device=rows.device)
        d, _ = sliced_wasserstein_prepared_dev(t, t, iu[0].to(torch.int32).contiguous(), iu[1].to(torch.int32).contiguous(), ctx=ctx)
        G[iu[0], iu[1]] = d
        G[iu[1], iu[0]] = d
    return G


def sliced_matrix_dev(ta, seg_off_a, cls_a, tb, seg_off_b, status_b, n_col, out_t=None, pairs_t=None, flags_t=None, ctx=None):
    """wasserstein_matrix_dev with the sliced Wasserstein distance, from prepared diagrams (SlicedTable ta: the A side, tb:
    the bank): the same tables, pairing rules and entries -- out (n_seg_a, n_col) float64 the mean over the pairs of
    (group g, column c), pairs and flags int32 -- and the value of a pair is sliced_wasserstein_prepared_dev's."""
    import torch
    ctx = ctx or get_ctx()
    if ta.n_dirs != tb.n_dirs:
        raise _lib.TdaError("libtdaeeg error 1: the two tables were prepared with different numbers of directions")
    n_seg_a, n_col = seg_off_a.numel() - 1, int(n_col)
    n_cls = (seg_off_b.numel() - 1) // n_col if n_col else 0
    for t in (seg_off_a, cls_a, seg_off_b, status_b):
        assert t.dtype == torch.int32 and t.is_cuda and t.is_contiguous()
    assert seg_off_b.numel() == n_cls * n_col + 1 and cls_a.numel() == n_seg_a and status_b.numel() >= tb.n_dgm
    dev = ta.table.device
    if out_t is None:
        out_t = torch.empty((n_seg_a, n_col), dtype=torch.float64, device=dev)
    if pairs_t is None:
        pairs_t = torch.empty((n_seg_a, n_col), dtype=torch.int32, device=dev)
    if flags_t is None:
        flags_t = torch.empty((n_seg_a, n_col), dtype=torch.int32, device=dev)
    for t in (out_t, pairs_t, flags_t):
        assert t.is_contiguous() and t.numel() >= n_seg_a * n_col
    ctx.check(ctx.lib.tda_sliced_matrix_dev(ctx.h, _tp(ta.table), _tp(ta.slot_off), _tp(ta.m), ta.n_dgm, _tp(seg_off_a), n_seg_a,
                                            _tp(cls_a), _tp(tb.table), _tp(tb.slot_off), _tp(tb.m), tb.n_dgm, _tp(seg_off_b),
                                            n_cls, n_col, _tp(status_b), ta.n_dirs, _tp(out_t), _tp(pairs_t), _tp(flags_t),
                                            _stream()))
    return out_t, pairs_t, flags_t
