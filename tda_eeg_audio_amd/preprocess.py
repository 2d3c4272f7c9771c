"""
preprocess.py -- front ends of the hot path ("next" rows 2-3), same names as
the reference:

  design_bandpass_filter, apply_bandpass_filter, create_sliding_windows
        notebooks/1_preprocesamiento.ipynb:209-263, 314-381  (EEG: zero-phase Butterworth per channel)
  bandpass_filter
        scripts/utils.py:66-74                               (audio envelope: filtfilt per band)
  eeg_to_distances
        preprocess_file (nb1:388-494) + process_file_graphs (nb2:158-218) fused: raw EEG (47, L) ->
        per band: band-pass on the GPU -> correlation/distance of the sliding windows read in place;
        neither the filtered windows stack (n_win, 47, 250) nor its 4x overlap ever exist.

Filter DESIGN (scipy.signal.butter, sosfilt_zi / lfilter_zi, pad length) is host-side preparation
done with scipy, exactly as the reference does; the recursions run in csrc/filters.hip and are
bit-identical to scipy.signal.sosfiltfilt / filtfilt.
"""
import ctypes as C

import numpy as np
from scipy import signal

from . import engine
from ._lib import f64, get_ctx, ptr

FREQ_BANDS = {"delta": (0.5, 4), "theta": (4, 8), "alpha": (8, 13), "beta": (13, 30), "gamma": (30, 50)}
FILTER_ORDER = 4            # nb1:128
WINDOW_SIZE_SEC = 1.0       # nb1:131
OVERLAP_PERCENT = 0.75      # nb1:132


def design_bandpass_filter(lowcut, highcut, fs, order=4):
    """nb1:209-233."""
    nyquist = 0.5 * fs
    return signal.butter(order, [lowcut / nyquist, highcut / nyquist], btype="band", output="sos")


def _sos_plan(sos):
    sos = np.ascontiguousarray(sos, dtype=np.float64)
    n_sections = sos.shape[0]
    ntaps = 2 * n_sections + 1
    ntaps -= min((sos[:, 2] == 0).sum(), (sos[:, 5] == 0).sum())      # scipy.signal.sosfiltfilt
    return sos, np.ascontiguousarray(signal.sosfilt_zi(sos)), int(ntaps * 3)


class SosBank:
    """SOS filters applied in ONE launch, packed for the C entries once: `sos` (n, n_sec, 6) and `zi` (n, n_sec, 2) stacked
    per filter (_sos_plan), and what a launch takes once for all its filters: `n_sec` and `edge`, sosfiltfilt's pad length."""

    def __init__(self, designs):
        plans = [_sos_plan(sos) for sos in designs]
        self.n, self.n_sec, self.edge = len(plans), plans[0][0].shape[0], plans[0][2]
        assert all(p[0].shape[0] == self.n_sec and p[2] == self.edge for p in plans), "the filters of a bank share their structure"
        self.sos = np.ascontiguousarray(np.stack([p[0] for p in plans]))
        self.zi = np.ascontiguousarray(np.stack([p[1] for p in plans]))

    @classmethod
    def bandpass(cls, bands, fs, order=FILTER_ORDER):
        """design_bandpass_filter (nb1:209-233) of every (lowcut, highcut) of `bands`."""
        return cls([design_bandpass_filter(lo, hi, fs, order) for lo, hi in bands])


class BaBank:
    """(b, a) filters applied by filtfilt in ONE launch, packed for the C entries once: `B`, `A` (n, ntaps) zero-padded to
    the longest filter, `Z` (n, ntaps - 1) scipy.signal.lfilter_zi of the padded pairs, `edge` = 3 * ntaps (filtfilt's)."""

    def __init__(self, bas):
        bas = [(np.atleast_1d(b), np.atleast_1d(a)) for b, a in bas]
        self.n, self.ntaps = len(bas), max(max(len(b), len(a)) for b, a in bas)
        self.edge = 3 * self.ntaps
        self.B, self.A, self.Z = (np.zeros((self.n, m)) for m in (self.ntaps, self.ntaps, self.ntaps - 1))
        for f, (b, a) in enumerate(bas):
            self.B[f, :len(b)] = b; self.A[f, :len(a)] = a
            self.Z[f] = signal.lfilter_zi(self.B[f], self.A[f])


def sosfiltfilt(sos, x, ctx=None):
    """scipy.signal.sosfiltfilt(sos, x, axis=-1) for a (n_sig, n_samples) float64 array."""
    ctx = ctx or get_ctx()
    x = f64(x)
    one = x.ndim == 1
    x2 = x.reshape(1, -1) if one else x
    sos, zi, edge = _sos_plan(sos)
    if x2.shape[1] <= edge:
        raise ValueError(f"The length of the input vector x must be greater than padlen, which is {edge}.")
    y = np.empty_like(x2)
    ctx.check(ctx.lib.tda_sosfiltfilt(ctx.h, ptr(x2), x2.shape[0], x2.shape[1], ptr(sos), ptr(zi), sos.shape[0], edge,
                                      ptr(y)))
    return y[0] if one else y


def filtfilt(b, a, x, ctx=None):
    """scipy.signal.filtfilt(b, a, x, axis=-1) (default odd padding) for (n_sig, n_samples) float64."""
    ctx = ctx or get_ctx()
    fb = BaBank([(b, a)])
    ntaps, edge = fb.ntaps, fb.edge
    x = f64(x)
    one = x.ndim == 1
    x2 = x.reshape(1, -1) if one else x
    if x2.shape[1] <= edge:
        raise ValueError(f"The length of the input vector x must be greater than padlen, which is {edge}.")
    y = np.empty_like(x2)
    ctx.check(ctx.lib.tda_filtfilt(ctx.h, ptr(x2), x2.shape[0], x2.shape[1], ptr(fb.B), ptr(fb.A), ptr(fb.Z), ntaps, edge, ptr(y)))
    return y[0] if one else y


def apply_bandpass_filter(data, lowcut, highcut, fs, order=4):
    """nb1:236-263 -- all channels in one launch instead of a Python loop over channels."""
    return sosfiltfilt(design_bandpass_filter(lowcut, highcut, fs, order), np.asarray(data, dtype=np.float64))


def _envelope_edges(low, high, fs):
    nyq = fs / 2
    return max(low / nyq, 0.001), min(high / nyq, 0.999)


def envelope_bandpass(bands, fs):
    """The (b, a) designs of bandpass_filter (utils.py:66-74, with its clamps) for every (low, high) of `bands`."""
    return [signal.butter(4, list(_envelope_edges(lo, hi, fs)), btype="band") for lo, hi in bands]


def bandpass_filter(s, fs, low, high):
    """scripts/utils.py:66-74."""
    lo, hi = _envelope_edges(low, high, fs)
    if lo >= hi:
        return s
    (b, a), = envelope_bandpass([(low, high)], fs)
    return filtfilt(b, a, s)


def create_sliding_windows(data, window_size, overlap, fs):
    """nb1:314-381 -- (n_windows, n_channels, window_samples) stack and window centre times (host slicing;
    the GPU path never builds this stack, see eeg_to_distances)."""
    data = np.asarray(data)
    n_channels, n_samples = data.shape
    window_samples = int(window_size * fs)
    step_samples = int(window_samples * (1 - overlap))
    n_windows = (n_samples - window_samples) // step_samples + 1
    if n_windows <= 0:
        return np.zeros((0, n_channels, window_samples)), np.zeros(0)
    idx = np.arange(n_windows)[:, None] * step_samples + np.arange(window_samples)[None, :]
    windows = np.ascontiguousarray(data[:, idx].transpose(1, 0, 2))
    times = (np.arange(n_windows) * step_samples + window_samples // 2) / fs
    return windows, times


def bandpass_dev(x_t, lowcut, highcut, fs, order=FILTER_ORDER, y_t=None, work_t=None, ctx=None):
    """apply_bandpass_filter (nb1:236-263) on device tensors: x_t (n_sig, n_samples) float64 -- every channel of every
    recording of equal length in ONE launch (bandpass_bank_ragged_dev: different lengths); returns y_t (same shape).
    work_t: optional (n_sig, n_samples + 2*edge)."""
    import torch
    ctx = ctx or get_ctx()
    assert x_t.is_cuda and x_t.dtype == torch.float64 and x_t.is_contiguous() and x_t.dim() == 2
    n_sig, n_s = x_t.shape
    sos, zi, edge = _sos_plan(design_bandpass_filter(lowcut, highcut, fs, order))
    if n_s <= edge:
        raise ValueError(f"The length of the input vector x must be greater than padlen, which is {edge}.")
    if y_t is None:
        y_t = torch.empty_like(x_t)
    if work_t is None or work_t.numel() < n_sig * (n_s + 2 * edge):
        work_t = torch.empty((n_sig, n_s + 2 * edge), dtype=torch.float64, device=x_t.device)
    ctx.check(ctx.lib.tda_sosfiltfilt_dev(ctx.h, C.c_void_p(x_t.data_ptr()), n_sig, n_s, ptr(sos), ptr(zi), sos.shape[0], edge,
                                          C.c_void_p(y_t.data_ptr()), C.c_void_p(work_t.data_ptr()),
                                          C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    return y_t


def recordings_to_features(raw_t, fs, sel_t=None, n_sel_per_rec=None, freq_bands=FREQ_BANDS, window_size=WINDOW_SIZE_SEC,
                           overlap=OVERLAP_PERCENT, order=FILTER_ORDER, ctx=None):
    """The EEG half of the corpus from RAW recordings, on the GPU end to end (preprocess_file nb1:388-494 +
    process_file_graphs nb2:158-218 + the hot loop and aggregation of process_file_features v2:404-436):
    raw_t (n_rec, n_ch, n_samples) float64 in HBM, recordings of equal length (recordings_to_features_ragged takes
    recordings of different lengths) -> per band: zero-phase band-pass of
    all n_rec * n_ch channels in one launch -> fused window kernel on the sliding windows read in place (the
    (n_win, n_ch, 250) stacks and the distance matrices never exist) -> H1 row order + extract_features -> mean / std
    over each recording's windows.  sel_t: optional int32 window list (r * n_win_per_rec + k, n_sel_per_rec per
    recording, recording-major) -- the drivers' window selection.  Returns (n_rec, 44 * n_bands) float64 tensor in the
    column order of features/feature_names.txt, and the status words of the windows, OR-ed over the bands."""
    import torch
    from . import engine
    ctx = ctx or get_ctx()
    n_rec, n_ch, n_s = raw_t.shape
    win = int(window_size * fs)
    step = int(win * (1 - overlap))
    per_rec = (n_s - win) // step + 1 if n_s >= win else 0
    k = per_rec if sel_t is None else int(n_sel_per_rec)
    n_out = n_rec * k
    dev = raw_t.device
    flat = raw_t.view(n_rec * n_ch, n_s)
    y = torch.empty_like(flat)
    work = None
    dgm = engine.DeviceDiagrams(n_out, n_ch, engine.DEFAULT_H1_CAP, dev)
    fe0 = torch.empty((n_out, 11), dtype=torch.float64, device=dev)
    fe1 = torch.empty_like(fe0)
    seg = torch.arange(0, n_out + 1, k, dtype=torch.int32, device=dev)
    X = torch.empty((n_rec, len(freq_bands), 44), dtype=torch.float64, device=dev)
    status = torch.zeros(n_out, dtype=torch.int32, device=dev)
    with ctx.deferred():
        for bi, (name, (lo, hi)) in enumerate(freq_bands.items()):
            sos, zi, edge = _sos_plan(design_bandpass_filter(lo, hi, fs, order))
            if work is None:
                work = torch.empty((n_rec * n_ch, n_s + 2 * edge + 64), dtype=torch.float64, device=dev)
            bandpass_dev(flat, lo, hi, fs, order, y_t=y, work_t=work, ctx=ctx)
            engine.eeg_window_sliding_dev(y.view(n_rec, n_ch, n_s), win, step, sel_t=sel_t, out=dgm, ctx=ctx)
            engine.diagram_finish_dev([(dgm.h0, dgm.c0, False, fe0), (dgm.h1, dgm.c1, True, fe1)], ctx=ctx)
            X[:, bi].copy_(engine.aggregate_dev(fe0, fe1, seg, ctx=ctx))
            status |= dgm.status                 # (the next band overwrites the words)
    return X.view(n_rec, len(freq_bands) * 44), status


def filtfilt_dev(x_t, b, a, y_t=None, work_t=None, ctx=None):
    """scipy.signal.filtfilt(b, a, x, axis=-1) on device tensors: x_t (n_sig, n_samples) float64, one launch (the band-pass
    of the audio envelope, utils.py:66-74, for every recording of a shard at once)."""
    import torch
    ctx = ctx or get_ctx()
    assert x_t.is_cuda and x_t.dtype == torch.float64 and x_t.is_contiguous() and x_t.dim() == 2
    fb = BaBank([(b, a)])
    ntaps, edge = fb.ntaps, fb.edge
    n_sig, n_s = x_t.shape
    if n_s <= edge:
        raise ValueError(f"The length of the input vector x must be greater than padlen, which is {edge}.")
    if y_t is None:
        y_t = torch.empty_like(x_t)
    if work_t is None or work_t.numel() < n_sig * (n_s + 2 * edge):
        work_t = torch.empty((n_sig, n_s + 2 * edge), dtype=torch.float64, device=x_t.device)
    ctx.check(ctx.lib.tda_filtfilt_dev(ctx.h, C.c_void_p(x_t.data_ptr()), n_sig, n_s, ptr(fb.B), ptr(fb.A), ptr(fb.Z), ntaps, edge,
                                       C.c_void_p(y_t.data_ptr()), C.c_void_p(work_t.data_ptr()),
                                       C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    return y_t


def bandpass_bank_dev(x_t, bands, fs=None, order=FILTER_ORDER, y_t=None, work_t=None, ctx=None):
    """apply_bandpass_filter (nb1:236-263) for ALL bands in one launch: x_t (n_sig, n_samples) -> y_t (n_bands, n_sig,
    n_samples), bit-identical to one bandpass_dev call per band.  bands: iterable of (lowcut, highcut) (designed here for
    `fs` and `order`) or the SosBank prepared once."""
    import torch
    ctx = ctx or get_ctx()
    assert x_t.is_cuda and x_t.dtype == torch.float64 and x_t.is_contiguous() and x_t.dim() == 2
    n_sig, n_s = x_t.shape
    bank = bands if isinstance(bands, SosBank) else SosBank.bandpass(bands, fs, order)
    sos, zi, nf, n_sec, edge = bank.sos, bank.zi, bank.n, bank.n_sec, bank.edge
    if n_s <= edge:
        raise ValueError(f"The length of the input vector x must be greater than padlen, which is {edge}.")
    if y_t is None:
        y_t = torch.empty((nf, n_sig, n_s), dtype=torch.float64, device=x_t.device)
    if work_t is None or work_t.numel() < nf * n_sig * (n_s + 2 * edge):
        work_t = torch.empty((nf, n_sig, n_s + 2 * edge), dtype=torch.float64, device=x_t.device)
    ctx.check(ctx.lib.tda_sosfiltfilt_bank_dev(ctx.h, C.c_void_p(x_t.data_ptr()), n_sig, n_s, ptr(sos), ptr(zi), nf, n_sec, edge,
                                               C.c_void_p(y_t.data_ptr()), C.c_void_p(work_t.data_ptr()),
                                               C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    return y_t


def filtfilt_bank_dev(x_t, bas, y_t=None, work_t=None, ctx=None):
    """scipy.signal.filtfilt for a bank of (b, a) pairs on signals of equal length in one launch (filtfilt_bank_ragged_dev:
    different lengths): x_t (n_sig, n_samples) -> y_t
    (n_filters, n_sig, n_samples) -- bandpass_filter (utils.py:66-74) of the audio envelope for all bands (cmp:63-64).
    bas: list of (b, a), or the BaBank prepared once."""
    import torch
    ctx = ctx or get_ctx()
    assert x_t.is_cuda and x_t.dtype == torch.float64 and x_t.is_contiguous() and x_t.dim() == 2
    n_sig, n_s = x_t.shape
    bank = bas if isinstance(bas, BaBank) else BaBank(bas)
    nf, ntaps, edge = bank.n, bank.ntaps, bank.edge
    if n_s <= edge:
        raise ValueError(f"The length of the input vector x must be greater than padlen, which is {edge}.")
    if y_t is None:
        y_t = torch.empty((nf, n_sig, n_s), dtype=torch.float64, device=x_t.device)
    if work_t is None or work_t.numel() < nf * n_sig * (n_s + 2 * edge):
        work_t = torch.empty((nf, n_sig, n_s + 2 * edge), dtype=torch.float64, device=x_t.device)
    ctx.check(ctx.lib.tda_filtfilt_bank_dev(ctx.h, C.c_void_p(x_t.data_ptr()), n_sig, n_s, ptr(bank.B), ptr(bank.A), ptr(bank.Z), nf, ntaps,
                                            edge, C.c_void_p(y_t.data_ptr()), C.c_void_p(work_t.data_ptr()),
                                            C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    return y_t


# --------------------------------------------------------------------------------------------
# ragged ("packed") recordings: one recording after the other, each at its own length
# --------------------------------------------------------------------------------------------
def pack_recordings(arrays):
    """list of (n_ch, L_r) (or (L_r,)) float64 arrays -> (pinned flat float64 tensor, lengths int64): recording r is an
    (n_ch, L_r) row-major block at element n_ch * off[r], off the exclusive prefix sum of the lengths -- the layout of
    every ragged entry point (bandpass_bank_ragged_dev, recordings.RaggedRecordingPass)."""
    import torch
    arrs = [np.ascontiguousarray(a, dtype=np.float64) for a in arrays]
    assert len({a.shape[:-1] for a in arrs}) <= 1, "all recordings need the same channel count"
    lengths = np.array([a.shape[-1] for a in arrs], dtype=np.int64)
    flat = torch.empty(int(sum(a.size for a in arrs)), dtype=torch.float64).pin_memory()
    fv = flat.numpy()
    o = 0
    for a in arrs:
        fv[o:o + a.size] = a.ravel()
        o += a.size
    return flat, lengths


class RaggedTables:
    """Lengths and offsets of packed signals: host int64 copies (`len_h`, `off_h`: exclusive prefix sum, n + 1 entries) and
    the device tables the ragged kernels read (`len_t`, `off_t`), uploaded once."""

    def __init__(self, lengths, device):
        import torch
        self.len_h = np.ascontiguousarray(lengths, dtype=np.int64)
        self.off_h = np.concatenate([[0], np.cumsum(self.len_h)]).astype(np.int64)
        self.n, self.total = len(self.len_h), int(self.off_h[-1])
        self.len_t = torch.from_numpy(self.len_h).to(device)
        self.off_t = torch.from_numpy(self.off_h).to(device)


def _tables(lengths, device):
    return lengths if isinstance(lengths, RaggedTables) else RaggedTables(lengths, device)


def bandpass_bank_ragged_dev(x_t, lengths, bands, fs=None, n_ch=47, order=FILTER_ORDER, y_t=None, work_t=None, ctx=None):
    """apply_bandpass_filter (nb1:236-263) for ALL bands in one launch on RAGGED recordings: x_t flat float64 (packed,
    recording r an (n_ch, L_r) block at n_ch * off[r]; see pack_recordings), lengths: L_r (numpy) or RaggedTables,
    bands: (lowcut, highcut) pairs or a SosBank, as for bandpass_bank_dev.
    Returns y_t (n_bands, n_ch * sum(L)) in the same layout per band, every channel bit-identical to
    scipy.signal.sosfiltfilt on that channel alone.  work_t: optional, n_bands * n_ch * (sum(L) + 2*edge*n_rec) elements."""
    import torch
    ctx = ctx or get_ctx()
    assert x_t.is_cuda and x_t.dtype == torch.float64 and x_t.is_contiguous()
    tb = _tables(lengths, x_t.device)
    assert x_t.numel() >= n_ch * tb.total
    bank = bands if isinstance(bands, SosBank) else SosBank.bandpass(bands, fs, order)
    sos, zi, nf, n_sec, edge = bank.sos, bank.zi, bank.n, bank.n_sec, bank.edge
    if tb.n and int(tb.len_h.min()) <= edge:
        raise ValueError(f"The length of the input vector x must be greater than padlen, which is {edge}.")
    if y_t is None:
        y_t = torch.empty((nf, n_ch * tb.total), dtype=torch.float64, device=x_t.device)
    n_work = nf * n_ch * (tb.total + 2 * edge * tb.n)
    if work_t is None or work_t.numel() < n_work:
        work_t = torch.empty(n_work, dtype=torch.float64, device=x_t.device)
    ctx.check(ctx.lib.tda_sosfiltfilt_bank_ragged_dev(ctx.h, C.c_void_p(x_t.data_ptr()), tb.n, n_ch, C.c_void_p(tb.len_t.data_ptr()),
                                                      C.c_void_p(tb.off_t.data_ptr()), ptr(tb.len_h), ptr(sos), ptr(zi), nf, n_sec,
                                                      edge, C.c_void_p(y_t.data_ptr()), C.c_void_p(work_t.data_ptr()),
                                                      C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    return y_t


def filtfilt_bank_ragged_dev(x_t, lengths, bas, y_t=None, work_t=None, ctx=None):
    """scipy.signal.filtfilt for a bank of (b, a) pairs (ntaps <= 9) in one launch on RAGGED signals: x_t flat float64,
    signal s = L_s samples at off[s] (packed; lengths numpy or RaggedTables) -> y_t (n_filters, sum(L)) in the same
    layout -- bandpass_filter (utils.py:66-74, cmp:63-64) of the envelopes of recordings of different lengths, each
    bit-identical to scipy.signal.filtfilt on that signal alone.  bas: list of (b, a) or a BaBank.  work_t: optional,
    n_filters * (sum(L) + 2*edge*n)."""
    import torch
    ctx = ctx or get_ctx()
    assert x_t.is_cuda and x_t.dtype == torch.float64 and x_t.is_contiguous()
    tb = _tables(lengths, x_t.device)
    assert x_t.numel() >= tb.total
    bank = bas if isinstance(bas, BaBank) else BaBank(bas)
    nf, ntaps, edge = bank.n, bank.ntaps, bank.edge
    if tb.n and int(tb.len_h.min()) <= edge:
        raise ValueError(f"The length of the input vector x must be greater than padlen, which is {edge}.")
    if y_t is None:
        y_t = torch.empty((nf, tb.total), dtype=torch.float64, device=x_t.device)
    n_work = nf * (tb.total + 2 * edge * tb.n)
    if work_t is None or work_t.numel() < n_work:
        work_t = torch.empty(n_work, dtype=torch.float64, device=x_t.device)
    ctx.check(ctx.lib.tda_filtfilt_bank_ragged_dev(ctx.h, C.c_void_p(x_t.data_ptr()), tb.n, C.c_void_p(tb.len_t.data_ptr()),
                                                   C.c_void_p(tb.off_t.data_ptr()), ptr(tb.len_h), ptr(bank.B), ptr(bank.A), ptr(bank.Z),
                                                   nf, ntaps, edge, C.c_void_p(y_t.data_ptr()), C.c_void_p(work_t.data_ptr()),
                                                   C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    return y_t


def n_windows(n_samples, window_size=WINDOW_SIZE_SEC, overlap=OVERLAP_PERCENT, fs=250):
    """Sliding windows of a recording of n_samples (scalar or array): nb1:341, 0 below one window."""
    win = int(window_size * fs)
    step = int(win * (1 - overlap))
    n = np.asarray(n_samples, dtype=np.int64)
    return np.where(n >= win, (n - win) // step + 1, 0)


def recordings_to_features_ragged(raw_packed_t, lengths, fs, sel=None, n_ch=47, freq_bands=FREQ_BANDS,
                                  window_size=WINDOW_SIZE_SEC, overlap=OVERLAP_PERCENT, order=FILTER_ORDER, ctx=None):
    """recordings_to_features for RAGGED recordings: raw_packed_t flat float64 in HBM (recording r an (n_ch, L_r) block
    at n_ch * off[r]; pack_recordings), lengths L_r.  Per recording, the sliding windows at its own length (nb1:341), or
    sel[r] (optional list of per-recording window-index arrays, sizes may differ -- the drivers' selection).  All bands
    band-passed in ONE launch, then per band the fused window kernel on a window table (no stacks, no matrices), H1
    order + extract_features, mean / std per recording.  Returns (n_rec, 44 * n_bands) float64 tensor -- NaN rows for
    recordings without a window -- and the status words of the windows (recording-major, in table order), OR-ed over
    the bands.  Each row equals recordings_to_features on that recording alone, bit for bit."""
    import torch
    from . import engine
    ctx = ctx or get_ctx()
    dev = raw_packed_t.device
    tb = _tables(lengths, dev)
    win = int(window_size * fs)
    step = int(win * (1 - overlap))
    per_rec = n_windows(tb.len_h, window_size, overlap, fs)
    picks = [np.arange(int(n)) for n in per_rec] if sel is None else [np.asarray(s, dtype=np.int64).ravel() for s in sel]
    assert len(picks) == tb.n and all(((p >= 0) & (p < n)).all() for p, n in zip(picks, per_rec)), "window index out of range"
    k = np.array([len(p) for p in picks], dtype=np.int64)
    live = np.flatnonzero(k > 0)
    n_out = int(k.sum())
    nb = len(freq_bands)
    X = torch.full((tb.n, nb, 44), float("nan"), dtype=torch.float64, device=dev)
    status = torch.zeros(n_out, dtype=torch.int32, device=dev)
    if n_out == 0:
        return X.view(tb.n, nb * 44), status
    y = bandpass_bank_ragged_dev(raw_packed_t, tb, list(freq_bands.values()), fs, n_ch=n_ch, order=order, ctx=ctx)
    band_len = n_ch * tb.total
    start0 = np.concatenate([n_ch * tb.off_h[r] + picks[r] * step for r in live]).astype(np.int64)
    ld = torch.from_numpy(np.repeat(tb.len_h[live], k[live]).astype(np.int64)).to(dev)
    seg = torch.from_numpy(np.concatenate([[0], np.cumsum(k[live])]).astype(np.int32)).to(dev)
    live_t = torch.from_numpy(live).to(dev)
    dgm = engine.DeviceDiagrams(n_out, n_ch, engine.DEFAULT_H1_CAP, dev)
    fe0 = torch.empty((n_out, 11), dtype=torch.float64, device=dev)
    fe1 = torch.empty_like(fe0)
    with ctx.deferred():
        for bi in range(nb):
            start = torch.from_numpy(start0 + bi * band_len).to(dev)
            engine.eeg_window_ragged_dev(y, start, ld, win, out=dgm, ctx=ctx)
            engine.diagram_finish_dev([(dgm.h0, dgm.c0, False, fe0), (dgm.h1, dgm.c1, True, fe1)], ctx=ctx)
            X[:, bi].index_copy_(0, live_t, engine.aggregate_dev(fe0, fe1, seg, ctx=ctx))
            status |= dgm.status                 # (the next band overwrites the words)
    return X.view(tb.n, nb * 44), status


def eeg_to_distances(eeg, fs, freq_bands=FREQ_BANDS, window_size=WINDOW_SIZE_SEC, overlap=OVERLAP_PERCENT,
                     order=FILTER_ORDER, want_corr=False, ctx=None):
    """raw EEG (n_ch, n_samples) -> {band: (n_win, n_ch, n_ch) distance matrices}; everything between the
    raw samples and the matrices stays in HBM (torch tensors, one stream)."""
    import torch
    ctx = ctx or get_ctx()
    dev = torch.device("cuda", ctx.device)
    x = torch.from_numpy(f64(eeg)).to(dev)
    n_ch, n_s = x.shape
    win = int(window_size * fs)
    step = int(win * (1 - overlap))
    out = {}
    for name, (lo, hi) in freq_bands.items():
        sos, zi, edge = _sos_plan(design_bandpass_filter(lo, hi, fs, order))
        y = torch.empty_like(x)
        work = torch.empty((n_ch, n_s + 2 * edge), dtype=torch.float64, device=dev)
        ctx.check(ctx.lib.tda_sosfiltfilt_dev(ctx.h, C.c_void_p(x.data_ptr()), n_ch, n_s, ptr(sos), ptr(zi), sos.shape[0],
                                              edge, C.c_void_p(y.data_ptr()), C.c_void_p(work.data_ptr()),
                                              C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        n_win = (n_s - win) // step + 1 if n_s >= win else 0
        if n_win <= 0:
            continue
        corr_t = torch.empty((n_win, n_ch, n_ch), dtype=torch.float64, device=dev) if want_corr else None
        dist_t = engine.corr_dist_sliding_dev(y, win, step, corr_t=corr_t, ctx=ctx)
        out[name] = (corr_t.cpu().numpy(), dist_t.cpu().numpy()) if want_corr else dist_t.cpu().numpy()
    return out


# --------------------------------------------------------------------------------------------
# audio front end (scripts/utils.py:47-79)
# --------------------------------------------------------------------------------------------
FS_AUDIO, FS_EEG = 44100, 250


def _resample_plan(n_in, up, down, window=("kaiser", 5.0)):
    """The FIR design and bookkeeping of scipy.signal.resample_poly (constant padding, cval 0)."""
    import math
    g_ = math.gcd(up, down)
    up //= g_; down //= g_
    n_out = n_in * up
    n_out = n_out // down + bool(n_out % down)
    max_rate = max(up, down)
    half_len = 10 * max_rate
    h = signal.firwin(2 * half_len + 1, 1.0 / max_rate, window=window).astype(np.float64)
    h *= up
    n_pre_pad = down - half_len % down
    n_post_pad = 0
    n_pre_remove = (half_len + n_pre_pad) // down

    def _output_len(len_h, in_len, up_, down_):
        return (((in_len - 1) * up_ + len_h) - 1) // down_ + 1
    while _output_len(len(h) + n_pre_pad + n_post_pad, n_in, up, down) < n_out + n_pre_remove:
        n_post_pad += 1
    h = np.concatenate((np.zeros(n_pre_pad), h, np.zeros(n_post_pad)))
    return np.ascontiguousarray(h), up, down, n_pre_remove, n_out


def resample_audio(audio, fs_audio=FS_AUDIO, fs_target=FS_EEG, ctx=None):
    """scripts/utils.py:77-79 -- scipy.signal.resample_poly(audio, fs_target, fs_audio)."""
    ctx = ctx or get_ctx()
    x = f64(np.asarray(audio).ravel())
    if fs_audio == fs_target:
        return x.copy()
    h, up, down, n_pre_remove, n_out = _resample_plan(len(x), int(fs_target), int(fs_audio))
    y = np.empty(n_out)
    ctx.check(ctx.lib.tda_upfirdn(ctx.h, ptr(x), len(x), ptr(h), len(h), up, down, n_pre_remove, n_out, ptr(y)))
    return y


def _hilbert_g(n):
    """g = imag(ifft(h)) of scipy.signal.hilbert at length n: the analytic signal's imaginary part is x (*) g."""
    hh = np.zeros(n)
    if n % 2 == 0:
        hh[0] = hh[n // 2] = 1; hh[1:n // 2] = 2
    else:
        hh[0] = 1; hh[1:(n + 1) // 2] = 2
    return np.ascontiguousarray(np.fft.ifft(hh).imag)


def hilbert_envelope(s, ctx=None):
    """np.abs(scipy.signal.hilbert(s)) (utils.py:58-59)."""
    ctx = ctx or get_ctx()
    x = f64(np.asarray(s).ravel())
    n = len(x)
    g = _hilbert_g(n)
    env = np.empty(n)
    ctx.check(ctx.lib.tda_hilbert_envelope(ctx.h, ptr(x), n, ptr(g), ptr(env)))
    return env


def compute_envelope(s, fs, ctx=None):
    """scripts/utils.py:56-63 -- Hilbert envelope, then 4th-order low-pass (zero-phase)."""
    return filtfilt(*envelope_lowpass(fs), hilbert_envelope(s, ctx=ctx), ctx=ctx)


def audio_to_band_windows(audio, fs_audio=FS_AUDIO, freq_bands=FREQ_BANDS, ctx=None):
    """cmp:53-65 -- 44.1 kHz audio -> 250 Hz envelope -> per band zero-phase band-pass -> 1 s windows
    (step 62): {band: (n_win, 250)}."""
    from .utils import create_windows
    rs = resample_audio(audio, fs_audio, FS_EEG, ctx=ctx)
    env = compute_envelope(rs, FS_EEG, ctx=ctx)
    win = int(1.0 * FS_EEG)
    step = int(win * (1 - 0.75))
    return {name: create_windows(bandpass_filter(env, FS_EEG, lo, hi), win, step) for name, (lo, hi) in freq_bands.items()}


# --------------------------------------------------------------------------------------------
# audio front end for RAGGED recordings: every recording of a shard in one launch per stage
# --------------------------------------------------------------------------------------------
HILBERT_RAGGED_MAX = 8192       # longest signal of tda_hilbert_envelope_ragged_dev (it and its g table live in LDS)
LOWPASS_ORDER = 4               # utils.py:60-62


def envelope_lowpass(fs=FS_EEG):
    """(b, a) of compute_envelope's low-pass (utils.py:60-62)."""
    nyq = fs / 2
    return signal.butter(LOWPASS_ORDER, min(50, nyq * 0.9) / nyq, btype="low")


class HilbertTables:
    """The g tables of hilbert_envelope for packed signals of lengths `lengths` (numpy only): one table per DISTINCT
    length, packed back to back in `g`; `g_off[s]` is signal s's table."""

    def __init__(self, lengths):
        self.len_h = np.ascontiguousarray(lengths, dtype=np.int64)
        self.lengths, inv = np.unique(self.len_h, return_inverse=True)
        start = np.concatenate([[0], np.cumsum(self.lengths)]).astype(np.int64)
        self.g = np.concatenate([_hilbert_g(int(n)) for n in self.lengths]) if len(self.lengths) else np.zeros(0)
        self.g_off = np.ascontiguousarray(start[:-1][inv.ravel()], dtype=np.int64)


class AudioPlan:
    """The host plan of the ragged audio front end (envelopes_ragged_dev), numpy only: from the lengths La of packed
    44.1 kHz recordings,
      n_out, out_off   envelope lengths ceil(La * up / down) (resample_poly's) and their exclusive prefix sum
      h, hp, nq        resample_poly's filter (_resample_plan) and its polyphase table hp[p, q] = h[p + up*q], nq taps per
                       phase.  _resample_plan pads h with n_post_pad zeros that depend on the input length; zero taps
                       only add exact +-0 products to a finite input, so the table padded for the longest input
                       (n_in_max, default max(La)) serves every length.
      n_pre_remove, up, down
      hilbert          HilbertTables of the envelope lengths.
      lowpass          compute_envelope's low-pass at fs (envelope_lowpass) as a one-filter BaBank.
    upload(device) adds the device tables (uploaded once): in_tb / out_tb (RaggedTables of La / n_out), hp_t, g_t, g_off_t."""

    def __init__(self, audio_lengths, fs_audio=FS_AUDIO, fs=FS_EEG, n_in_max=None):
        self.La = np.ascontiguousarray(audio_lengths, dtype=np.int64).ravel()
        if len(self.La) and int(self.La.min()) < 1:
            raise ValueError("every recording needs at least one audio sample")
        if int(fs_audio) == int(fs):
            raise ValueError("the ragged front end resamples: fs_audio must differ from fs")
        n_max = max(int(self.La.max()) if len(self.La) else 1, int(n_in_max or 1))
        self.h, self.up, self.down, self.n_pre_remove, _ = _resample_plan(n_max, int(fs), int(fs_audio))
        self.nq = -(-len(self.h) // self.up)
        hp = np.zeros(self.nq * self.up)
        hp[:len(self.h)] = self.h
        self.hp = np.ascontiguousarray(hp.reshape(self.nq, self.up).T)
        n_out = self.La * self.up
        self.n_out = n_out // self.down + (n_out % self.down > 0)
        self.out_off = np.concatenate([[0], np.cumsum(self.n_out)]).astype(np.int64)
        self.hilbert = HilbertTables(self.n_out)
        self.lowpass = BaBank([envelope_lowpass(fs)])
        self.device = None

    def upload(self, device):
        import torch
        self.device = device
        self.in_tb = RaggedTables(self.La, device)
        self.out_tb = RaggedTables(self.n_out, device)
        self.hp_t = torch.from_numpy(self.hp).to(device)
        self.g_t = torch.from_numpy(self.hilbert.g).to(device)
        self.g_off_t = torch.from_numpy(self.hilbert.g_off).to(device)
        return self


def _audio_plan(audio_lengths, device, fs_audio=FS_AUDIO, fs=FS_EEG):
    if isinstance(audio_lengths, AudioPlan):
        return audio_lengths if audio_lengths.device is not None else audio_lengths.upload(device)
    return AudioPlan(audio_lengths, fs_audio, fs).upload(device)


def resample_bank_ragged_dev(x_t, plan, y_t=None, ctx=None):
    """resample_audio (utils.py:77-79, scipy.signal.resample_poly) of RAGGED signals in one launch: x_t flat float64,
    signal s = plan.La[s] samples at plan.in_tb.off_h[s] (packed); plan: AudioPlan or the audio lengths.  Returns y_t
    (sum n_out,) float64, signal s's output at plan.out_off[s]."""
    import torch
    ctx = ctx or get_ctx()
    assert x_t.is_cuda and x_t.dtype == torch.float64 and x_t.is_contiguous()
    P = _audio_plan(plan, x_t.device)
    assert x_t.numel() >= P.in_tb.total
    if y_t is None:
        y_t = torch.empty(P.out_tb.total, dtype=torch.float64, device=x_t.device)
    assert y_t.is_contiguous() and y_t.numel() >= P.out_tb.total
    ctx.check(ctx.lib.tda_resample_poly_ragged_dev(ctx.h, C.c_void_p(x_t.data_ptr()), P.in_tb.n, C.c_void_p(P.in_tb.len_t.data_ptr()),
                                                   C.c_void_p(P.in_tb.off_t.data_ptr()), ptr(P.in_tb.len_h),
                                                   C.c_void_p(P.out_tb.off_t.data_ptr()), C.c_void_p(P.hp_t.data_ptr()), P.nq,
                                                   P.up, P.down, P.n_pre_remove, C.c_void_p(y_t.data_ptr()),
                                                   C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    return y_t


def hilbert_envelope_ragged_dev(x_t, lengths, env_t=None, g_tables=None, ctx=None):
    """hilbert_envelope (np.abs(scipy.signal.hilbert(s)), utils.py:58-59) of RAGGED signals in one launch: x_t flat float64,
    signal s = L_s samples at off[s] (lengths numpy or RaggedTables; L_s <= HILBERT_RAGGED_MAX).  g_tables: optional
    (g_t, g_off_t) device tables of HilbertTables(lengths) (built here otherwise).  Returns env_t in the layout of x_t."""
    import torch
    ctx = ctx or get_ctx()
    assert x_t.is_cuda and x_t.dtype == torch.float64 and x_t.is_contiguous()
    tb = _tables(lengths, x_t.device)
    assert x_t.numel() >= tb.total
    if g_tables is None:
        ht = HilbertTables(tb.len_h)
        g_tables = (torch.from_numpy(ht.g).to(x_t.device), torch.from_numpy(ht.g_off).to(x_t.device))
    g_t, g_off_t = g_tables
    if env_t is None:
        env_t = torch.empty(tb.total, dtype=torch.float64, device=x_t.device)
    assert env_t.is_contiguous() and env_t.numel() >= tb.total
    ctx.check(ctx.lib.tda_hilbert_envelope_ragged_dev(ctx.h, C.c_void_p(x_t.data_ptr()), tb.n, C.c_void_p(tb.len_t.data_ptr()),
                                                      C.c_void_p(tb.off_t.data_ptr()), ptr(tb.len_h), C.c_void_p(g_t.data_ptr()),
                                                      C.c_void_p(g_off_t.data_ptr()), C.c_void_p(env_t.data_ptr()),
                                                      C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    return env_t


def envelopes_ragged_dev(audio_packed_t, audio_lengths, fs_audio=FS_AUDIO, fs=FS_EEG, out_t=None, work_t=None, ctx=None):
    """compute_envelope(resample_audio(a), fs) (utils.py:56-63, 77-79; cmp:53-55) for every recording of a RAGGED set,
    in HBM end to end: audio_packed_t flat float64 (recording s = La_s samples at the exclusive prefix sum of La;
    pack_recordings of 1-D arrays), audio_lengths numpy or AudioPlan.  Three launches: the polyphase resampler, the
    Hilbert envelope, the low-pass (the plan's `lowpass` bank) through filtfilt_bank_ragged_dev.  Returns (env_t flat
    float64, the envelope lengths n_out, numpy int64), envelope s at the exclusive prefix sum of n_out.  Raises ValueError
    as scipy does when an envelope is not longer than the low-pass pad length (15).  work_t: optional, 3 * sum(n_out) +
    2 * 15 * n_rec elements."""
    import torch
    ctx = ctx or get_ctx()
    P = _audio_plan(audio_lengths, audio_packed_t.device, fs_audio, fs)
    edge = P.lowpass.edge
    if P.out_tb.n and int(P.n_out.min()) <= edge:
        raise ValueError(f"The length of the input vector x must be greater than padlen, which is {edge}.")
    T, n = P.out_tb.total, P.out_tb.n
    n_work = 3 * T + 2 * edge * n
    if work_t is None or work_t.numel() < n_work:
        work_t = torch.empty(n_work, dtype=torch.float64, device=audio_packed_t.device)
    if out_t is None:
        out_t = torch.empty(T, dtype=torch.float64, device=audio_packed_t.device)
    rs, hil, fwork = work_t[:T], work_t[T:2 * T], work_t[2 * T:n_work]
    resample_bank_ragged_dev(audio_packed_t, P, y_t=rs, ctx=ctx)
    hilbert_envelope_ragged_dev(rs, P.out_tb, env_t=hil, g_tables=(P.g_t, P.g_off_t), ctx=ctx)
    filtfilt_bank_ragged_dev(hil, P.out_tb, P.lowpass, y_t=out_t, work_t=fwork, ctx=ctx)
    return out_t, P.n_out
