"""
recordings.py -- process_recording (scripts/tda_eeg_audio_comparison.py:45-124) for a whole set of recordings, FROM HOST
MEMORY: raw EEG (n_rec, 47, L) float64 and the 250 Hz audio envelope (n_rec, L) float64 (compute_envelope of the
resampled audio, utils.py:56-63 -- preprocess.compute_envelope) in pinned host buffers go in, the (n_rec, 5, 48) result
rows [W_H0, W_H1, tau, n_windows, 44 aggregated EEG features] come back to the host.

ONE shard driver (_ShardedPass.run / _verify) serves every pass of this module.  Per shard of recordings:
    H2D of the shard on the copy stream (1.73 MB of EEG per recording, not the 33 MB of its five window stacks)
    the shard's step on the main stream of its buffer set, the envelopes' filters on the set's side stream
    D2H of the shard's rows on a stream of its own
and the upload of shard k + 1 overlaps the compute of shard k (n_sets buffer sets); a shard is verified (class-overflow
flags of its groups) after the later ones have been queued, run again with the full ladder if a flag is set, and its
rows are withheld if any status bit is left.  The passes differ in how a shard is cut out of the host input and in its step:
    RecordingPass             recordings of equal length; the step the benchmark's `recordings` leg times:
        zero-phase band-pass of all 47 x n_rec EEG channels, all five bands in ONE launch   (nb1:236-263)
        zero-phase band-pass of the n_rec envelopes, all five bands in one launch, beside it  (utils.py:66-74, cmp:64)
        the selected 1 s windows of the band-passed envelopes                 (create_windows + np.linspace, cmp:65,77-80)
        ONE run_step over the (band, recording) groups of the shard: the EEG windows are read IN PLACE from the
        band-passed recordings (fused window kernel on sliding windows: neither the (n_win, 47, 250) stacks nor the
        distance matrices exist), tau from the first selected window of every group, Takens + Rips, finish,
        Wasserstein H0 / H1, rows
    RaggedRecordingPass       recordings of different lengths, packed back to back (preprocess.pack_recordings)
    RaggedAudioRecordingPass  the same from the raw 44.1 kHz audio instead of the envelopes
    ControlPass               the matched-vs-mismatched control (scripts/matched_vs_mismatched.py)
    MatchMismatchPass         the same control against the audio of EVERY candidate recording: the whole distance matrix
The filter banks are designed and packed once per pass (preprocess.SosBank / BaBank) and handed to every shard's step.
The rows equal pipeline.run_step on the stacked windows of the same band-passed signals bit for bit
(tests/test_gpu_frontend.py::test_recording_pass_equals_stacked_windows).
RecordingPass and the ragged passes take the optional outputs of pipeline.step_outputs, by its keywords (each is
described there), and return each enabled one per (recording, band) beside the rows, in pinned host memory: <name>_h
(n_rec, 5) + shape, e.g. corr_h (n_rec, 5, 10) -- the group's block of the step's Workspace, NaN for a recording without a
window.  They are computed on the device from the step's own diagrams and feature matrices; drivers.comparison_rows /
comparison_summary turn rows and corr_h into the script's table and statistics.
"""
import numpy as np

from . import engine, pipeline, preprocess
from ._lib import TdaError, get_ctx

MAX_WINDOWS = 15            # cmp:39


def select_windows(n_win, max_windows=MAX_WINDOWS):
    """cmp:77-80."""
    return np.linspace(0, n_win - 1, max_windows, dtype=int) if n_win > max_windows else np.arange(n_win)


class _ShardedPass:
    """The shard driver of every pass: state, `run` and `_verify`.  A subclass supplies
      _begin(raw_h, second_h)       checks the host inputs; returns the shards of this run, a list of ranges (r0, r1) of
                                    recordings (kept as self.ranges)
      _upload(st, i, raw_h, second_h)   shard i into buffer set st (on the copy stream)
      _shard_step(st, i)            everything between the upload and st["rows"] (on st["main"]; filters on st["side"])
      _rips_step(st, i, retry)      the part of the step that a flagged shard repeats with retry="auto"
      _rows(st, i, res)             the result of _rips_step -> st["rows"], and the Workspace's block of every output of
                                    self.outputs -> st[name]
      _flags_ws(st, i)              the Workspace (or view) whose seg_flags / flags_host are shard i's; None for a shard
                                    without a window (nothing to verify)
      _more_back(st, r0, r1, nb)    optional: further per-recording outputs of the shard to the host beside the rows
                                    (non_blocking = nb)."""

    ROW_COLS = pipeline.RESULT_COLS     # width of a row

    def __init__(self, device, ctx, fs, bands, takens=None, **outputs):
        self.ctx = ctx or get_ctx()
        # takens=(dim, subsample, n_perm): the audio stage of every Workspace runs on greedy landmarks (pipeline.Workspace)
        self.takens = None if takens is None else tuple(int(v) for v in takens)
        self.dev, self.fs = device, fs
        self.bands = list(dict(bands).values())
        # the optional outputs (pipeline.step_outputs: self.outputs is the table, validated here, once); output_kw: the
        # enabled ones as keywords for every pipeline.Workspace, each also an attribute; host buffer of `name`:
        # self.<name>_h, made by `run`
        self.outputs = pipeline.step_outputs(**outputs)
        self.output_kw = {pipeline.OUTPUT_BY_NAME[o.name].keyword: pipeline.OUTPUT_BY_NAME[o.name].arg(o.params)
                          for o in self.outputs}
        for spec in pipeline.OUTPUTS:
            setattr(self, spec.keyword, self.output_kw.get(spec.keyword, spec.off))
            setattr(self, spec.name + "_h", None)
        # the filter banks, designed and packed once: the EEG's band-passes (nb1:209-233) and the envelopes' (utils.py:66-74)
        self.eeg_bank = preprocess.SosBank.bandpass(self.bands, fs, preprocess.FILTER_ORDER)
        self.env_bank = preprocess.BaBank(preprocess.envelope_bandpass(self.bands, fs))

    def _make_sets(self, n_sets, buffers):
        """buffers() -> the tensors and the Workspace ("ws") of one buffer set.  Buffer sets = shards in flight (upload,
        filters, step, download of consecutive shards overlap).  A stream pair per set: the filters of shard k + 1 (chains
        of dependent operations on few waves) run beside the Rips kernels of shard k (which fill the vector units).  Which
        hardware queue a stream lands on depends on how many were made before it, and a pass' speed on that: the order
        stays per set the Workspace's own, main, side; then copy, then back.  st[name] (rows of st["rows"], bands, the
        output's shape) of every output of self.outputs is made here."""
        import torch
        self.n_sets = int(n_sets)
        self.set = []
        for _ in range(self.n_sets):
            st = buffers()
            for o in self.outputs:
                st[o.name] = torch.empty(st["rows"].shape[:2] + o.shape, dtype=torch.float64, device=self.dev)
            st.update(main=torch.cuda.Stream(device=self.dev), side=torch.cuda.Stream(device=self.dev),
                      up=torch.cuda.Event(), done=torch.cuda.Event(), down=torch.cuda.Event())
            self.set.append(st)
        self.copy = torch.cuda.Stream(device=self.dev)                 # uploads
        self.back = torch.cuda.Stream(device=self.dev)                 # rows back (its own stream: the download of shard k waits
                                                                       # for the compute of k, the upload of k + 1 must not)
        self.repairs = 0

    def run(self, raw_h, second_h, rows_h=None):
        """The two pinned float64 host inputs of the pass -> rows_h (n_rec, n_bands, ROW_COLS), pinned, complete when the
        call returns; so is self.<name>_h, pinned (n_rec, n_bands) + shape, of every output of self.outputs."""
        import torch
        self.ranges = self._begin(raw_h, second_h)
        n_rec, nb = self.ranges[-1][1] if self.ranges else 0, len(self.bands)
        if rows_h is None:
            rows_h = torch.empty((n_rec, nb, self.ROW_COLS), dtype=torch.float64).pin_memory()
        for o in self.outputs:
            if getattr(self, o.name + "_h") is None or getattr(self, o.name + "_h").shape[0] != n_rec:
                setattr(self, o.name + "_h", torch.empty((n_rec, nb) + o.shape, dtype=torch.float64).pin_memory())
        pend = []
        try:
            for i, (r0, r1) in enumerate(self.ranges):
                st = self.set[i % self.n_sets]
                with torch.cuda.stream(self.copy):
                    if i >= self.n_sets:            # the shard before in this buffer set has read it and its rows are out
                        self.copy.wait_event(st["done"])
                        self.copy.wait_event(st["down"])
                    self._upload(st, i, raw_h, second_h)
                    st["up"].record(self.copy)
                with torch.cuda.stream(st["main"]):
                    st["main"].wait_event(st["up"])
                    self._shard_step(st, i)
                    st["done"].record(st["main"])
                with torch.cuda.stream(self.back):
                    self.back.wait_event(st["done"])
                    self._back(st, r0, r1, rows_h, True)
                    st["down"].record(self.back)
                pend.append(i)
                if len(pend) >= self.n_sets:        # (the GPU has the later shards to work on while the host looks at this
                    self._verify(pend.pop(0), rows_h)           # one; its buffer set is the next to be reused)
            while pend:
                self._verify(pend.pop(0), rows_h)
        except BaseException:
            torch.cuda.synchronize(self.dev)        # shards still in flight read the buffer sets the next run fills
            raise
        self.back.synchronize()
        return rows_h

    def _back(self, st, r0, r1, rows_h, non_blocking):
        """The rows of a shard, its block of every output and what the _more_back hook adds, to the host on the current stream."""
        rows_h[r0:r1].copy_(st["rows"][:r1 - r0], non_blocking=non_blocking)
        for o in self.outputs:
            getattr(self, o.name + "_h")[r0:r1].copy_(st[o.name][:r1 - r0], non_blocking=non_blocking)
        self._more_back(st, r0, r1, non_blocking)

    def _more_back(self, st, r0, r1, non_blocking):
        pass

    def _verify(self, i, rows_h):
        """Verify, then publish: a shard whose step left a class-overflow flag (run_step copies the flags of its groups
        to pinned memory) is run again with the full ladder -- rare -- and its rows replace the ones already copied; any
        status bit still left withholds the rows (and every output: they take the path of the rows)."""
        import torch
        st = self.set[i % self.n_sets]
        r0, r1 = self.ranges[i]
        st["down"].synchronize()
        ws = self._flags_ws(st, i)
        if ws is None:
            return
        fl = ws.flags_host
        if bool((fl & 2).any()):
            self.repairs += 1
            with torch.cuda.stream(st["main"]):
                self._rows(st, i, self._rips_step(st, i, "auto"))
                self._back(st, r0, r1, rows_h, False)
                fl.copy_(ws.seg_flags, non_blocking=True)
                st["main"].synchronize()
        if bool(fl.any()):
            raise TdaError(f"window status bits {int(np.bitwise_or.reduce(fl.numpy())):#x} left in shard {i}: rows withheld")


class RecordingPass(_ShardedPass):
    """Recordings of EQUAL length: `run` takes raw_h (n_rec, n_ch, L) and env_h (n_rec, L), pinned float64, in shards of
    `shard` recordings; the idle rows of a short last shard repeat its first recording (their groups repeat real ones:
    their flags say nothing new)."""

    def __init__(self, n_samples, shard, device, ctx=None, n_ch=47, fs=250, bands=preprocess.FREQ_BANDS,
                 max_windows=MAX_WINDOWS, window_sec=1.0, overlap=0.75, n_sets=None, takens=None, **outputs):
        """**outputs: the optional outputs, by the keywords of pipeline.step_outputs; `run` also fills self.<name>_h of each
        (_ShardedPass.run).  corr_h is in the order of drivers.DETAILED_COLUMNS[8:].  The rows are the same either way.
        takens=(dim, subsample, n_perm): handed to every pipeline.Workspace -- the audio diagrams come from n_perm greedy
        landmarks of the (dim, subsample) Takens cloud; the columns of the rows keep their meaning."""
        import os
        import torch
        super().__init__(device, ctx, fs, bands, takens, **outputs)
        self.S, self.L, self.n_ch = int(shard), int(n_samples), n_ch
        self.win = int(window_sec * fs)
        self.step = int(self.win * (1 - overlap))                      # cmp:57-58: 62
        self.per_rec = (self.L - self.win) // self.step + 1 if self.L >= self.win else 0
        assert self.per_rec > 0, "recordings shorter than one window"
        self.pick = select_windows(self.per_rec, max_windows)
        self.k = len(self.pick)
        S, L, k, nb = self.S, self.L, self.k, len(self.bands)
        edge, edge_a = self.eeg_bank.edge, self.env_bank.edge
        f64 = dict(dtype=torch.float64, device=device)
        # the (band, recording) groups of a shard are the "recordings" of ONE batch: window (b * S + r) * per_rec + pick
        sel = ((np.arange(nb * S)[:, None]) * self.per_rec + self.pick[None, :]).astype(np.int32).ravel()
        self.sel_t = torch.from_numpy(sel).to(device)
        self.pick_t = torch.from_numpy(self.pick.astype(np.int64)).to(device)
        seg_off = np.arange(0, nb * S * k + 1, k, dtype=np.int32)
        self._make_sets(n_sets or os.environ.get("TDA_REC_SETS", "2"), lambda: dict(
            raw=torch.empty((S, n_ch, L), **f64), env=torch.empty((S, L), **f64),
            y=torch.empty((nb, S * n_ch, L), **f64), ya=torch.empty((nb, S, L), **f64),
            aw=torch.empty((nb * S * k, self.win), **f64), rows=torch.empty((S, nb, pipeline.RESULT_COLS), **f64),
            ws=pipeline.Workspace(nb * S * k, seg_off, device, n_ch=n_ch, takens=self.takens, **self.output_kw),
            work=torch.empty((nb, S * n_ch, L + 2 * edge), **f64), worka=torch.empty((nb, S, L + 2 * edge_a), **f64)))

    def _begin(self, raw_h, env_h):
        n_rec = raw_h.shape[0]
        assert raw_h.shape[1:] == (self.n_ch, self.L) and env_h.shape == (n_rec, self.L)
        return [(s0, min(s0 + self.S, n_rec)) for s0 in range(0, n_rec, self.S)]

    def _upload(self, st, i, raw_h, env_h):
        s0, s1 = self.ranges[i]
        n = s1 - s0
        st["raw"][:n].copy_(raw_h[s0:s1], non_blocking=True)
        st["env"][:n].copy_(env_h[s0:s1], non_blocking=True)
        if n < self.S:                              # a short last shard: the idle rows repeat its first recording
            st["raw"][n:].copy_(st["raw"][:1].expand(self.S - n, -1, -1))
            st["env"][n:].copy_(st["env"][:1].expand(self.S - n, -1))

    def _flags_ws(self, st, i):
        return st["ws"]

    def _rips_step(self, st, i, retry):
        nb = len(self.bands)
        return pipeline.run_step(None, st["aw"], st["ws"], ctx=self.ctx, max_lag=self.win // 2, retry=retry,
                                 eeg_sliding=(st["y"].view(nb * self.S, self.n_ch, self.L), self.win, self.step, self.sel_t))

    def _shard_step(self, st, i):
        import torch
        ctx, S, k, nb = self.ctx, self.S, self.k, len(self.bands)
        st["side"].wait_stream(st["main"])
        with torch.cuda.stream(st["side"]):
            preprocess.filtfilt_bank_dev(st["env"], self.env_bank, y_t=st["ya"], work_t=st["worka"], ctx=ctx)
            # create_windows + the selection: a strided view of the band-passed envelopes, gathered into the stack the
            # tau / Takens kernels read (2 KB per window: plumbing)
            st["aw"].view(nb * S, k, self.win).copy_(
                st["ya"].view(nb * S, self.L).unfold(1, self.win, self.step).index_select(1, self.pick_t))
        preprocess.bandpass_bank_dev(st["raw"].view(S * self.n_ch, self.L), self.eeg_bank, y_t=st["y"], work_t=st["work"], ctx=ctx)
        st["main"].wait_stream(st["side"])
        self._rows(st, i, self._rips_step(st, i, "one"))

    def _rows(self, st, i, res):
        """(nb * S, 48) band-major groups -> the shard's rows; the same for the Workspace's block of every output."""
        for dst, src in [(st["rows"], res)] + [(st[o.name], getattr(st["ws"], o.name)) for o in self.outputs]:
            dst.copy_(src.unflatten(0, (len(self.bands), self.S)).transpose(0, 1))


# ------------------------------------------------------------------------------------------------------------
# recordings of DIFFERENT lengths (the study's corpus: 46 distinct lengths, 2,663 .. 5,741 samples)
# ------------------------------------------------------------------------------------------------------------
DEFAULT_SHARD_SAMPLES = 1_100_000      # EEG samples per shard (~236 recordings of the corpus; 52 MB of raw EEG)
DEFAULT_SHARD_BYTES = 1 << 30          # bytes uploaded per shard of RaggedAudioRecordingPass (EEG + 44.1 kHz audio: ~120
                                       # recordings of the corpus, 11 shards)


class RaggedPlan:
    """The host plan of RaggedRecordingPass, numpy only (tests/test_ragged_plan.py checks it without a GPU).
    Per recording r (cmp:70-80 at its own length): n_win[r] = min(per_rec(L_r), per_rec(Le_r)) (nb1:341 for the EEG and
    for the envelope), picks[r] = the selected windows, k[r] = len(picks[r]).  shards: contiguous ranges [r0, r1) of
    recordings closed at a budget of EEG samples (a shard exceeds it only when it holds a single recording) -- or, with
    shard_bytes, at a budget of bytes uploaded: 8 * (n_ch * L_r + La_r) per recording, La the audio lengths
    (RaggedAudioRecordingPass; default Le).  Per shard:
      eeg_off / env_off  exclusive prefix sums of L / Le within the shard (the packed layout of its upload)
      live               local indices of the recordings with k > 0 (the others get a NaN row, n_windows = 0)
      seg_off            groups of k windows, band-major: group (b, j) = band b of live recording j
      eeg_start, eeg_ld  window table of the band-passed EEG (n_bands, n_ch * sum L): element offset of the first sample,
                         row stride L_r
      env_start          window table of the band-passed envelopes (n_bands, sum Le)."""

    def __init__(self, eeg_lengths, env_lengths=None, shard_samples=DEFAULT_SHARD_SAMPLES, n_ch=47, n_bands=5, fs=250,
                 window_sec=1.0, overlap=0.75, max_windows=MAX_WINDOWS, shard_bytes=None, audio_lengths=None):
        self.L = np.asarray(eeg_lengths, dtype=np.int64).ravel()
        self.Le = self.L.copy() if env_lengths is None else np.asarray(env_lengths, dtype=np.int64).ravel()
        assert self.L.shape == self.Le.shape
        self.n_rec, self.n_ch, self.nb = len(self.L), int(n_ch), int(n_bands)
        self.win = int(window_sec * fs)
        self.step = int(self.win * (1 - overlap))                      # cmp:57-58: 62
        self._select(window_sec, overlap, fs, max_windows)
        if shard_bytes is None:
            cost, budget = self.L, shard_samples
        else:
            La = self.Le if audio_lengths is None else np.asarray(audio_lengths, dtype=np.int64).ravel()
            assert La.shape == self.L.shape
            cost, budget = 8 * (self.n_ch * self.L + La), shard_bytes
        self.cost = cost
        self.shards = []
        r0, acc = 0, 0
        for r in range(self.n_rec):
            if r > r0 and acc + cost[r] > budget:
                self.shards.append((r0, r))
                r0, acc = r, 0
            acc += int(cost[r])
        if self.n_rec:
            self.shards.append((r0, self.n_rec))
        self.tables = [self._shard_tables(a, b) for a, b in self.shards]

    def _select(self, window_sec, overlap, fs, max_windows):
        """The windows of every recording: n_win, picks, k, empty (a plan with another rule: ControlPlan)."""
        self.n_win = np.minimum(preprocess.n_windows(self.L, window_sec, overlap, fs),
                                preprocess.n_windows(self.Le, window_sec, overlap, fs))          # cmp:71
        self.picks = [select_windows(int(n), max_windows) for n in self.n_win]                  # cmp:77-80
        self.k = np.array([len(p) for p in self.picks], dtype=np.int64)
        self.empty = np.flatnonzero(self.k == 0)                                                 # the reference's None

    def _shard_tables(self, r0, r1):
        L, Le, k = self.L[r0:r1], self.Le[r0:r1], self.k[r0:r1]
        eeg_off = np.concatenate([[0], np.cumsum(L)]).astype(np.int64)
        env_off = np.concatenate([[0], np.cumsum(Le)]).astype(np.int64)
        live = np.flatnonzero(k > 0)
        kl = k[live]
        seg_off = np.concatenate([[0], np.cumsum(np.tile(kl, self.nb))]).astype(np.int32)
        # one band's window offsets, recording-major over the live recordings, then the bands behind each other
        pick_off = np.concatenate([self.picks[r0 + j] * self.step for j in live]).astype(np.int64) if len(live) else \
            np.zeros(0, np.int64)
        e1 = self.n_ch * np.repeat(eeg_off[live], kl) + pick_off
        a1 = np.repeat(env_off[live], kl) + pick_off
        band = np.arange(self.nb, dtype=np.int64)[:, None]
        return dict(eeg_off=eeg_off, env_off=env_off, live=live, seg_off=seg_off,
                    eeg_start=(band * self.n_ch * eeg_off[-1] + e1[None, :]).ravel(),
                    eeg_ld=np.tile(np.repeat(L[live], kl), self.nb).astype(np.int64),
                    env_start=(band * env_off[-1] + a1[None, :]).ravel())


class RaggedRecordingPass(_ShardedPass):
    """RecordingPass for recordings of DIFFERENT lengths: raw EEG packed back to back (recording r an (n_ch, L_r) block at
    n_ch * off[r]) and the 250 Hz envelopes packed the same way with their own lengths (Le_r, default L_r), both in pinned
    host memory (preprocess.pack_recordings).  `run` returns the (n_rec, n_bands, 48) rows of process_recording
    (cmp:45-124) at every recording's own length, in the caller's order; a recording without a window (the reference
    returns None) gets a NaN row with n_windows = 0 and is listed in `empty`.
    Planned once at construction (RaggedPlan): shards are contiguous ranges of recordings (one H2D copy per tensor and
    shard), the buffer sets are sized by the largest shard, and every shard's window tables and segment table are
    uploaded once.  Per shard: the ragged SOS bank of all EEG channels and the ragged (b, a) bank of the envelopes (one
    launch each), the selected envelope windows gathered into the stack the tau / Takens kernels read, ONE run_step over
    the (band, recording) groups with the EEG windows read in place through the window table, rows scattered to the
    recordings.  Upload / compute / download overlap and verify-then-publish are the shared driver's (_ShardedPass)."""

    ROW_ZERO = 3                        # the columns of the NaN row of a recording without a window that are 0: n_windows

    def __init__(self, eeg_lengths, env_lengths=None, device=None, shard_samples=DEFAULT_SHARD_SAMPLES, n_sets=2, ctx=None,
                 n_ch=47, fs=250, bands=preprocess.FREQ_BANDS, max_windows=MAX_WINDOWS, window_sec=1.0, overlap=0.75,
                 plan=None, takens=None, **outputs):
        """**outputs: the optional outputs (pipeline.step_outputs), as RecordingPass takes them; NaN for a recording without
        a window.  takens=(dim, subsample, n_perm): as RecordingPass takes it."""
        import torch
        super().__init__(device if device is not None else torch.device("cuda", torch.cuda.current_device()), ctx, fs, bands,
                         takens, **outputs)
        self.n_ch = n_ch
        nb = len(self.bands)
        # plan: a RaggedPlan made by a subclass (RaggedAudioRecordingPass plans its shards by bytes)
        if plan is None:
            plan = RaggedPlan(eeg_lengths, env_lengths, shard_samples, n_ch, nb, fs, window_sec, overlap, max_windows)
        self.plan = P = plan
        self.win, self.step, self.n_rec, self.empty = P.win, P.step, P.n_rec, P.empty
        self.edge, self.edge_a = self.eeg_bank.edge, self.env_bank.edge
        short = np.flatnonzero((P.L <= self.edge) | (P.Le <= self.edge_a))
        if len(short):
            raise ValueError(f"recording(s) {short[:8].tolist()} not longer than the filters' pad length "
                             f"({self.edge} EEG / {self.edge_a} envelope samples)")
        self.eeg_off = np.concatenate([[0], np.cumsum(P.L)]).astype(np.int64)
        self.env_off = np.concatenate([[0], np.cumsum(P.Le)]).astype(np.int64)
        self.second = ("env", self.env_off)         # the per-recording host input uploaded beside the EEG: buffer, offsets
        i64 = dict(dtype=torch.int64, device=self.dev)
        f64 = dict(dtype=torch.float64, device=self.dev)
        # per shard, uploaded once: length tables of the two banks, window tables, segment tables (a Workspace view)
        self.shards = []
        for (r0, r1), t in zip(P.shards, P.tables):
            self.shards.append(dict(
                r0=r0, r1=r1, n=r1 - r0, T=int(t["eeg_off"][-1]), Te=int(t["env_off"][-1]), seg_off=t["seg_off"],
                eeg_tb=preprocess.RaggedTables(P.L[r0:r1], self.dev), env_tb=preprocess.RaggedTables(P.Le[r0:r1], self.dev),
                eeg_start=torch.from_numpy(t["eeg_start"]).to(**i64), eeg_ld=torch.from_numpy(t["eeg_ld"]).to(**i64),
                env_start=torch.from_numpy(t["env_start"]).to(**i64), live=torch.from_numpy(t["live"]).to(**i64),
                n_live=len(t["live"]), n_win=int(t["seg_off"][-1])))
        S = max(d["n"] for d in self.shards) if self.shards else 1
        T = max((d["T"] for d in self.shards), default=1)
        Te = max((d["Te"] for d in self.shards), default=1)
        n_win = max((d["n_win"] for d in self.shards), default=0)
        n_seg = max((nb * d["n_live"] for d in self.shards), default=0)

        def buffers():
            # the Workspace of a buffer set is sized by the largest shard; each shard gets a view with its own seg tables
            ws = pipeline.Workspace(n_win, np.concatenate([np.zeros(n_seg, np.int32), [n_win]]).astype(np.int32), self.dev,
                                    n_ch=n_ch, takens=self.takens, **self.output_kw)
            return dict(
                raw=torch.empty(n_ch * T, **f64), env=torch.empty(Te, **f64),
                y=torch.empty(nb * n_ch * T, **f64), ya=torch.empty(nb * Te, **f64),
                work=torch.empty(nb * n_ch * (T + 2 * self.edge * S), **f64), worka=torch.empty(nb * (Te + 2 * self.edge_a * S), **f64),
                aw=torch.empty((max(n_win, 1), self.win), **f64), rows=torch.empty((S, nb, self.ROW_COLS), **f64),
                ws=ws, views=[ws.view(d["seg_off"]) for d in self.shards])
        self._make_sets(n_sets, buffers)

    def _begin(self, raw_packed_h, second_packed_h):
        assert raw_packed_h.numel() == self.n_ch * self.eeg_off[-1] and second_packed_h.numel() == self.second[1][-1]
        return self.plan.shards

    def _upload(self, st, i, raw_packed_h, second_packed_h):
        key, sec_off = self.second
        r0, r1 = self.ranges[i]
        e0, e1 = self.n_ch * int(self.eeg_off[r0]), self.n_ch * int(self.eeg_off[r1])
        st["raw"][:e1 - e0].copy_(raw_packed_h.view(-1)[e0:e1], non_blocking=True)
        a0, a1 = int(sec_off[r0]), int(sec_off[r1])
        st[key][:a1 - a0].copy_(second_packed_h.view(-1)[a0:a1], non_blocking=True)

    def _flags_ws(self, st, i):
        return st["views"][i] if self.shards[i]["n_win"] else None

    def _rips_step(self, st, i, retry):
        d = self.shards[i]
        return pipeline.run_step(None, st["aw"][:d["n_win"]], st["views"][i], ctx=self.ctx, max_lag=self.win // 2, retry=retry,
                                 eeg_table=(st["y"], d["eeg_start"], d["eeg_ld"], self.win))

    def _rows(self, st, i, res):
        """(n_bands * n_live, ROW_COLS) band-major -> the shard's rows; recordings without a window: NaN, with 0 in the
        columns ROW_ZERO.  The same (all NaN) for the block of every output in the shard's view."""
        self._scatter(i, st["rows"], res, self.ROW_ZERO)
        for o in self.outputs:
            self._scatter(i, st[o.name], getattr(st["views"][i], o.name))

    def _scatter(self, i, dst, src, zero=None):
        """src, band-major over the live recordings of shard i, to the recordings in dst; NaN (0 in the columns `zero`) for
        the ones without a window."""
        d = self.shards[i]
        dst = dst[:d["n"]]
        if d["n_live"] < d["n"]:
            dst.fill_(float("nan"))
            if zero is not None:
                dst[:, :, zero] = 0.0
        if d["n_live"]:
            dst.index_copy_(0, d["live"], src.unflatten(0, (len(self.bands), d["n_live"])).transpose(0, 1))

    def _front_end(self, st, i):
        """Whatever makes st["env"] from the upload, on the side stream (here the envelopes ARE the upload)."""

    def _shard_step(self, st, i):
        import torch
        ctx, d, nb = self.ctx, self.shards[i], len(self.bands)
        if d["n_win"] == 0:                                            # no recording of the shard has a window
            self._rows(st, i, None)
            return
        st["side"].wait_stream(st["main"])
        with torch.cuda.stream(st["side"]):
            self._front_end(st, i)
            preprocess.filtfilt_bank_ragged_dev(st["env"], d["env_tb"], self.env_bank, y_t=st["ya"], work_t=st["worka"], ctx=ctx)
            engine.gather_windows_dev(st["ya"], d["env_start"], self.win, out_t=st["aw"], ctx=ctx)
        preprocess.bandpass_bank_ragged_dev(st["raw"], d["eeg_tb"], self.eeg_bank, n_ch=self.n_ch, y_t=st["y"],
                                            work_t=st["work"], ctx=ctx)
        st["main"].wait_stream(st["side"])
        self._rows(st, i, self._rips_step(st, i, "one"))


class RaggedAudioRecordingPass(RaggedRecordingPass):
    """RaggedRecordingPass from the reference's own inputs: raw EEG packed as for RaggedRecordingPass and the raw 44.1 kHz
    mono float64 audio of each recording (what load_audio returns) packed back to back, both in pinned host memory
    (preprocess.pack_recordings takes 1-D arrays).  Per shard the AUDIO is uploaded instead of the envelopes, and the
    front end of process_recording (cmp:53-55: resample_audio, then compute_envelope) runs on the side stream ahead of
    the envelopes' band-pass bank: the ragged polyphase resampler, the ragged Hilbert envelope and the low-pass, one
    launch each (preprocess.envelopes_ragged_dev).  Envelope lengths are the resampled lengths ceil(La * 250 / 44100).
    Audio is ~3.75x the bytes of the EEG, so shards are planned by bytes uploaded (RaggedPlan shard_bytes).  Everything
    else -- buffer sets sized by the largest shard, upload / compute / download overlap, verify-then-publish, NaN rows
    for recordings without a window -- is RaggedRecordingPass's; the rows equal RaggedRecordingPass.run fed the
    envelopes of envelopes_ragged_dev bit for bit."""

    def __init__(self, eeg_lengths, audio_lengths, device=None, shard_bytes=DEFAULT_SHARD_BYTES, n_sets=2, ctx=None, n_ch=47,
                 fs=250, fs_audio=preprocess.FS_AUDIO, bands=preprocess.FREQ_BANDS, max_windows=MAX_WINDOWS, window_sec=1.0,
                 overlap=0.75, takens=None, **outputs):
        """**outputs, takens: as RaggedRecordingPass takes them (pipeline.step_outputs lists the optional outputs)."""
        import torch
        A = preprocess.AudioPlan(audio_lengths, fs_audio, fs)
        long_ = np.flatnonzero(A.n_out > preprocess.HILBERT_RAGGED_MAX)
        if len(long_):
            raise ValueError(f"recording(s) {long_[:8].tolist()} longer than {preprocess.HILBERT_RAGGED_MAX} envelope samples")
        plan = RaggedPlan(eeg_lengths, A.n_out, n_ch=n_ch, n_bands=len(dict(bands)), fs=fs, window_sec=window_sec,
                          overlap=overlap, max_windows=max_windows, shard_bytes=shard_bytes, audio_lengths=A.La)
        super().__init__(eeg_lengths, A.n_out, device, n_sets=n_sets, ctx=ctx, n_ch=n_ch, fs=fs, bands=bands,
                         max_windows=max_windows, window_sec=window_sec, overlap=overlap, plan=plan, takens=takens, **outputs)
        self.audio_plan = A
        self.audio_off = np.concatenate([[0], np.cumsum(A.La)]).astype(np.int64)
        self.second = ("audio", self.audio_off)
        # the filter and Hilbert tables once; per shard its own length / offset tables (AudioPlan of the shard's lengths,
        # its filter designed for the longest audio of the whole set: the same taps in every shard)
        for d in self.shards:
            d["audio"] = preprocess.AudioPlan(A.La[d["r0"]:d["r1"]], fs_audio, fs, n_in_max=int(A.La.max())).upload(self.dev)
        Ta = max((int(self.audio_off[d["r1"]] - self.audio_off[d["r0"]]) for d in self.shards), default=1)
        S = max((d["n"] for d in self.shards), default=1)
        Te = max((d["Te"] for d in self.shards), default=1)
        edge_lp = A.lowpass.edge
        for st in self.set:
            st["audio"] = torch.empty(Ta, dtype=torch.float64, device=self.dev)
            st["front"] = torch.empty(3 * Te + 2 * edge_lp * S, dtype=torch.float64, device=self.dev)

    def _front_end(self, st, i):
        d = self.shards[i]
        preprocess.envelopes_ragged_dev(st["audio"], d["audio"], out_t=st["env"], work_t=st["front"], ctx=self.ctx)

    def run(self, raw_packed_h, audio_packed_h, rows_h=None):
        """raw_packed_h: flat pinned float64, n_ch * sum(L); audio_packed_h: flat pinned float64, sum(La).  Returns rows_h
        (n_rec, n_bands, 48), pinned, complete when the call returns."""
        return super().run(raw_packed_h, audio_packed_h, rows_h)


# ------------------------------------------------------------------------------------------------------------
# the control experiment (scripts/matched_vs_mismatched.py): every recording's EEG against its own audio and against the
# audio of a recording of the other condition of the same infant
# ------------------------------------------------------------------------------------------------------------
def mismatch_partners(names, conditions):
    """mvm:98-118, host only.  names: file names or stems of the recordings; conditions: the condition of each (two
    distinct values, mvm's "slow" / "fast").  Subject = the part of the stem before the first "_" (mvm:102).  Returns
    int64 (n_rec,): the index of the recording whose audio is the mismatched one -- the first file, in sorted order, of
    the same subject in the other condition (mvm:100,113-114) -- or -1 where the subject has no recording there (mvm:106
    leaves such subjects out).  The same name may occur in both conditions: a recording is (condition, name)."""
    names = [str(n) for n in names]
    conditions = [str(c) for c in conditions]
    assert len(names) == len(conditions)
    files = [n if n.lower().endswith(".mat") else n + ".mat" for n in names]           # mvm sorts the *.mat paths
    conds = sorted(set(conditions))
    if len(conds) > 2:
        raise ValueError(f"two conditions expected, got {conds}")
    first = {}                                                                           # (condition, subject) -> index
    for r in sorted(range(len(files)), key=lambda r: files[r]):
        first.setdefault((conditions[r], files[r][:-4].split("_")[0]), r)
    other = {conds[0]: conds[-1], conds[-1]: conds[0]} if len(conds) == 2 else {}
    return np.array([first.get((other.get(c), f[:-4].split("_")[0]), -1) for f, c in zip(files, conditions)], dtype=np.int64)


class ControlPlan(RaggedPlan):
    """The host plan of ControlPass, numpy only (tests/test_control_plan.py checks it without a GPU).  What differs from
    RaggedPlan is mvm's: per recording r the EEG windows are selected from the EEG's own window count (mvm:74-78; k_e,
    picks_e) and the audio windows from the envelope's own (mvm:44-49; k_a, picks_a) -- cmp:71 takes both from the
    minimum -- and partner[r] (mismatch_partners, or any table: a shuffle for a permutation null) names the recording
    whose audio is the mismatched one, -1 for none.  Shards as RaggedPlan makes them.  Per shard, beside RaggedPlan's
    eeg_off / env_off / live / eeg_start / eeg_ld (by k_e and picks_e):
      seg_off_e (= seg_off)  EEG groups of k_e windows, band-major over the live recordings (k_e > 0); grp_e: the group
                             of every EEG window
      live_a, seg_off_a      audio groups of k_a windows, band-major over the recordings with k_a > 0
      env_start              window table of the band-passed envelopes by picks_a
      partner_own            per EEG group the audio group of the same (recording, band), -1 when k_a = 0
      partner_bank           per EEG group the bank group of (partner, band), -1 without a partner (or one with k_a = 0)
    The bank, once per pass: U the sorted distinct partners, bank the ones of them with k_a > 0 (bank_pos[r]: position
    in `bank` or -1), bank_off the offsets of their packed envelopes, seg_off_bank (band-major over `bank`) and
    bank_start, the window table of their band-passed envelopes."""

    def __init__(self, eeg_lengths, env_lengths=None, partner=None, shard_samples=DEFAULT_SHARD_SAMPLES, n_ch=47, n_bands=5,
                 fs=250, window_sec=1.0, overlap=0.75, max_windows=MAX_WINDOWS):
        n_rec = len(np.asarray(eeg_lengths).ravel())
        self.partner = np.full(n_rec, -1, np.int64) if partner is None else np.asarray(partner, dtype=np.int64).ravel()
        assert self.partner.shape == (n_rec,) and ((self.partner >= -1) & (self.partner < n_rec)).all()
        super().__init__(eeg_lengths, env_lengths, shard_samples, n_ch, n_bands, fs, window_sec, overlap, max_windows)

    def _select(self, window_sec, overlap, fs, max_windows):
        self.n_win_e = preprocess.n_windows(self.L, window_sec, overlap, fs)                     # mvm:72
        self.n_win_a = preprocess.n_windows(self.Le, window_sec, overlap, fs)                    # mvm:44
        self.picks_e = [select_windows(int(n), max_windows) for n in self.n_win_e]              # mvm:74-77
        self.picks_a = [select_windows(int(n), max_windows) for n in self.n_win_a]              # mvm:46-49
        self.k_e = np.array([len(p) for p in self.picks_e], dtype=np.int64)
        self.k_a = np.array([len(p) for p in self.picks_a], dtype=np.int64)
        # RaggedPlan's names are the EEG's: a recording without an EEG window has no row (mvm:73)
        self.n_win, self.picks, self.k = self.n_win_e, self.picks_e, self.k_e
        self.empty = np.flatnonzero(self.k_e == 0)
        self.U = self._bank_members()
        self.bank = self.U[self.k_a[self.U] > 0]
        self.bank_pos = np.full(self.n_rec, -1, np.int64)
        self.bank_pos[self.bank] = np.arange(len(self.bank))
        kb = self.k_a[self.bank]
        self.bank_off = np.concatenate([[0], np.cumsum(self.Le[self.bank])]).astype(np.int64)
        self.seg_off_bank = np.concatenate([[0], np.cumsum(np.tile(kb, self.nb))]).astype(np.int32)
        pick_off = np.concatenate([self.picks_a[u] * self.step for u in self.bank]).astype(np.int64) if len(self.bank) else \
            np.zeros(0, np.int64)
        b1 = np.repeat(self.bank_off[:-1], kb) + pick_off
        self.bank_start = (np.arange(self.nb, dtype=np.int64)[:, None] * self.bank_off[-1] + b1[None, :]).ravel()

    def _bank_members(self):
        """The recordings whose audio diagrams the bank may hold, in the bank's order."""
        return np.unique(self.partner[self.partner >= 0])

    def _shard_tables(self, r0, r1):
        t = super()._shard_tables(r0, r1)                                # the EEG side: k = k_e, picks = picks_e
        n, nb = r1 - r0, self.nb
        live, ka = t["live"], self.k_a[r0:r1]
        live_a = np.flatnonzero(ka > 0)
        kla = ka[live_a]
        pick_off = np.concatenate([self.picks_a[r0 + j] * self.step for j in live_a]).astype(np.int64) if len(live_a) else \
            np.zeros(0, np.int64)
        a1 = np.repeat(t["env_off"][live_a], kla) + pick_off
        band = np.arange(nb, dtype=np.int64)[:, None]
        pos_a = np.full(n, -1, np.int64)
        pos_a[live_a] = np.arange(len(live_a))
        own = pos_a[live]
        pr = self.partner[r0 + live]
        pb = np.where(pr >= 0, self.bank_pos[np.maximum(pr, 0)], -1)
        seg_off_e = t["seg_off"]
        t.update(seg_off_e=seg_off_e, grp_e=np.repeat(np.arange(len(seg_off_e) - 1), np.diff(seg_off_e)).astype(np.int32),
                 live_a=live_a, seg_off_a=np.concatenate([[0], np.cumsum(np.tile(kla, nb))]).astype(np.int32),
                 env_start=(band * t["env_off"][-1] + a1[None, :]).ravel(),
                 partner_own=np.where(own >= 0, band * len(live_a) + own[None, :], -1).astype(np.int32).ravel(),
                 partner_bank=np.where(pb >= 0, band * len(self.bank) + pb[None, :], -1).astype(np.int32).ravel())
        return t


CONTROL_COLS = 4            # [w_matched, w_mismatched, n_matched, n_mismatched]


class ControlPass(RaggedRecordingPass):
    """The control experiment (scripts/matched_vs_mismatched.py:120-172) as a batched pass FROM HOST MEMORY: the inputs of
    RaggedRecordingPass (raw EEG packed back to back, 250 Hz envelopes packed with their own lengths, both pinned) and a
    partner table (mismatch_partners) go in, the (n_rec, n_bands, 4) rows [w_matched, w_mismatched, n_matched,
    n_mismatched] come back: per (recording, band) the mean H1 Wasserstein distance between the EEG diagrams and the
    diagrams of the recording's own audio, and of its partner's audio, paired by position (mvm:86-95), with the number of
    pairs of each.  A recording without an EEG window (mvm:73) gets a NaN row with zero counts; a (recording, band)
    without a pair NaN (mvm:90).
    Phase 1, once per run: the envelopes of the distinct partners with a window (the bank: 90 recordings for the study's
    table, sized by the table for any other) are staged, uploaded in one copy, band-passed, windowed and taken through
    tau / Takens / Rips under the full ladder into a DeviceDiagrams that lives for the whole pass.
    Phase 2, per shard: RaggedRecordingPass's pipeline (its run, _shard_step, _verify and buffer sets) with another Rips
    step: the EEG windows by the EEG's own count, the audio windows by the envelope's own count, two
    engine.wasserstein_cross_dev launches that resolve their pairs on the device from the plan's tables (own audio,
    then the bank) and engine.cross_rows_dev.  No index array is built per shard and nothing synchronises with the host
    between the Rips stages and the rows.
    The 250 Hz envelopes are the upload (the _front_end hook is RaggedRecordingPass's).
    The pass keeps an audio bank of its own, embedded as the reference embeds it (dim 3, subsample 2, every point): the
    landmark route (takens=, RecordingPass) is not offered here."""

    ROW_COLS = CONTROL_COLS
    ROW_ZERO = slice(2, None)           # the pair counts

    def __init__(self, eeg_lengths, env_lengths=None, partner=None, device=None, shard_samples=DEFAULT_SHARD_SAMPLES, n_sets=2,
                 ctx=None, n_ch=47, fs=250, bands=preprocess.FREQ_BANDS, max_windows=MAX_WINDOWS, window_sec=1.0, overlap=0.75,
                 correlations=False, plan=None):
        import torch
        from ._lib import MAX_POINTS
        if correlations:
            # its EEG and audio windows are selected apart (mvm:44-49,74-78) and paired by position with two audios:
            # there is no series of (audio, EEG) window pairs in cmp's sense
            raise ValueError(f"{type(self).__name__} has no temporal correlations (correlations=True): use RaggedRecordingPass")
        # plan: a ControlPlan made by a subclass (MatchMismatchPass)
        if plan is None:
            plan = ControlPlan(eeg_lengths, env_lengths, partner, shard_samples, n_ch, len(dict(bands)), fs, window_sec, overlap,
                               max_windows)
        super().__init__(eeg_lengths, env_lengths, device, n_sets=n_sets, ctx=ctx, n_ch=n_ch, fs=fs, bands=bands,
                         max_windows=max_windows, window_sec=window_sec, overlap=overlap, plan=plan)
        P, dev, nb = plan, self.dev, len(self.bands)
        i32 = dict(dtype=torch.int32, device=dev)
        f64 = dict(dtype=torch.float64, device=dev)
        up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(device=dev, dtype=dt)      # noqa: E731
        for d, t in zip(self.shards, P.tables):
            d.update(seg_off_a=up(t["seg_off_a"], torch.int32), grp_e=up(t["grp_e"], torch.int32),
                     partner_own=up(t["partner_own"], torch.int32), partner_bank=up(t["partner_bank"], torch.int32),
                     n_win_a=int(t["seg_off_a"][-1]))
        n_e = max((d["n_win"] for d in self.shards), default=0)
        n_a = max((d["n_win_a"] for d in self.shards), default=0)
        n_seg = max((nb * d["n_live"] for d in self.shards), default=0)
        for st in self.set:
            # the audio side of a shard has its own window count: its own stack, tau tables and -- where the Workspace's
            # audio diagrams (sized by the EEG's count) do not hold it -- diagrams
            st["aw"] = torch.empty((max(n_a, 1), self.win), **f64)
            st["caud"] = st["ws"].aud if n_a <= st["ws"].aud.n_win else engine.DeviceDiagrams(n_a, MAX_POINTS, st["ws"].aud.h1_cap, dev)
            st["tau_seg"], st["tau_win"] = torch.empty(max(n_a, 1), **i32), torch.empty(max(n_a, 1), **i32)
            st["wm"], st["wx"] = torch.empty(max(n_e, 1), **f64), torch.empty(max(n_e, 1), **f64)
            st["sm"], st["sx"] = torch.empty(max(n_e, 1), **i32), torch.empty(max(n_e, 1), **i32)
            st["res"] = torch.empty((max(n_seg, 1), CONTROL_COLS), **f64)
        self.bits = torch.tensor([1, 2, 8, 16], **i32)                  # every TDA_WIN_* bit but DEGENERATE (a result)
        # the bank
        Tb, n_b = int(P.bank_off[-1]), int(P.seg_off_bank[-1])
        self.n_bank_win = n_b
        self.bank = engine.DeviceDiagrams(n_b, MAX_POINTS, engine.DEFAULT_H1_CAP, dev)
        self.bank_seg_off = up(P.seg_off_bank, torch.int32)
        self.bank_start = up(P.bank_start, torch.int64)
        self.bank_tb = preprocess.RaggedTables(P.Le[P.bank], dev)
        self.bank_stage = torch.empty(max(Tb, 1), dtype=torch.float64).pin_memory()
        self.bank_buf = dict(env=torch.empty(max(Tb, 1), **f64), ya=torch.empty(nb * max(Tb, 1), **f64),
                             work=torch.empty(nb * (Tb + 2 * self.edge_a * max(len(P.bank), 1)), **f64),
                             aw=torch.empty((max(n_b, 1), self.win), **f64), tau_seg=torch.empty(max(n_b, 1), **i32),
                             tau_win=torch.empty(max(n_b, 1), **i32))
        self.bank_stream = self.set[0]["main"]                           # (no stream of its own: the Rips retry lists are per stream)
        self.bank_ready = torch.cuda.Event()
        self.bank_flags = torch.zeros(1, **i32)
        self.bank_flags_host = torch.zeros(1, dtype=torch.int32).pin_memory()

    def _or_bits(self, status_t):
        """OR of the status words of a Rips call without TDA_WIN_DEGENERATE, on the device (0-d int32)."""
        import torch
        if status_t.numel() == 0:
            return torch.zeros((), dtype=torch.int32, device=self.dev)
        return (status_t.unsqueeze(1) & self.bits).amax(0).sum().to(torch.int32)

    def _audio_diagrams(self, aw, seg_off_t, tau_seg, tau_win, out):
        """mvm:56-61 for the groups of a window stack: tau from the first window of every group, Takens + Rips, the H1
        rows into ripser's order (the finishing step of pipeline.run_step: a diagram is row for row the per-call API's)."""
        engine.tau_segments_dev(aw, seg_off_t, self.win // 2, tau_seg, tau_win, ctx=self.ctx)
        engine.takens_rips_dev(aw, tau_win, out, ctx=self.ctx)
        engine.diagram_finish_dev([(out.h1, out.c1, True, None)], ctx=self.ctx)

    def _phase1(self, env_f):
        """The bank: one staging copy of the partners' envelopes, their band-pass bank, windows and diagrams."""
        import torch
        P, B, ctx = self.plan, self.bank_buf, self.ctx
        if self.n_bank_win == 0:
            self.bank_ready.record(self.bank_stream)
            return
        sv, ev = self.bank_stage.numpy(), env_f.numpy()
        for j, u in enumerate(P.bank):
            sv[P.bank_off[j]:P.bank_off[j + 1]] = ev[self.env_off[u]:self.env_off[u + 1]]
        Tb = int(P.bank_off[-1])
        with torch.cuda.stream(self.bank_stream):
            for st in self.set[1:]:                                      # a run before this one may still read the bank
                self.bank_stream.wait_stream(st["main"])
            B["env"][:Tb].copy_(self.bank_stage[:Tb], non_blocking=True)
            preprocess.filtfilt_bank_ragged_dev(B["env"][:Tb], self.bank_tb, self.env_bank, y_t=B["ya"], work_t=B["work"], ctx=ctx)
            engine.gather_windows_dev(B["ya"], self.bank_start, self.win, out_t=B["aw"], ctx=ctx)
            with ctx.deferred():                                         # (the retry policy is the default: the full ladder)
                self._audio_diagrams(B["aw"][:self.n_bank_win], self.bank_seg_off, B["tau_seg"], B["tau_win"], self.bank)
            self.bank_flags.copy_(self._or_bits(self.bank.status).view(1))
            self.bank_flags_host.copy_(self.bank_flags, non_blocking=True)
            self.bank_ready.record(self.bank_stream)

    def _rips_step(self, st, i, retry):
        """Both Rips stages of a shard, the two cross Wasserstein launches and the rows: (n_bands * n_live, 4)."""
        import torch
        ctx, d, v = self.ctx, self.shards[i], st["views"][i]
        n_e, n_a = d["n_win"], d["n_win_a"]
        aud = st["caud"].head(n_a)
        with ctx.deferred(retry):
            engine.eeg_window_ragged_dev(st["y"], d["eeg_start"], d["eeg_ld"], self.win, out=v.eeg, n_ch=v.eeg.h0_cap, ctx=ctx)
            if n_a:
                self._audio_diagrams(st["aw"][:n_a], d["seg_off_a"], st["tau_seg"], st["tau_win"], aud)
        engine.diagram_finish_dev([(v.eeg.h1, v.eeg.c1, True, None)], ctx=ctx)
        torch.cuda.current_stream().wait_event(self.bank_ready)
        wm, sm, wx, sx = st["wm"][:n_e], st["sm"][:n_e], st["wx"][:n_e], st["sx"][:n_e]
        engine.wasserstein_cross_dev(v.eeg.h1, v.eeg.c1, v.seg_off, aud.h1, aud.c1, d["seg_off_a"], aud.status,
                                     d["partner_own"], grp_a=d["grp_e"], out_t=wm, status_t=sm, ctx=ctx)
        engine.wasserstein_cross_dev(v.eeg.h1, v.eeg.c1, v.seg_off, self.bank.h1, self.bank.c1, self.bank_seg_off,
                                     self.bank.status, d["partner_bank"], grp_a=d["grp_e"], out_t=wx, status_t=sx, ctx=ctx)
        res = engine.cross_rows_dev(wm, sm, wx, sx, v.seg_off, out_t=st["res"][:v.n_seg], status_a=v.eeg.status,
                                    seg_flags=v.seg_flags, ctx=ctx)
        if n_a:                                                          # the audio side's flags ask for the ladder too
            v.seg_flags.bitwise_or_(self._or_bits(aud.status))
        if retry != "auto":
            v.flags_host.copy_(v.seg_flags, non_blocking=True)
        return res

    def run(self, raw_packed_h, env_packed_h, rows_h=None):
        """raw_packed_h: flat pinned float64, n_ch * sum(L); env_packed_h: flat pinned float64, sum(Le).  Returns rows_h
        (n_rec, n_bands, 4) [w_matched, w_mismatched, n_matched, n_mismatched], pinned, complete when the call returns."""
        assert env_packed_h.numel() == self.env_off[-1]
        self._phase1(env_packed_h.view(-1))
        rows_h = super().run(raw_packed_h, env_packed_h, rows_h)
        self.bank_ready.synchronize()
        if int(self.bank_flags_host[0]):
            raise TdaError(f"window status bits {int(self.bank_flags_host[0]):#x} left in the partners' diagrams: rows withheld")
        return rows_h


# ------------------------------------------------------------------------------------------------------------
# match-mismatch: every recording's EEG against the audio of every candidate recording
# ------------------------------------------------------------------------------------------------------------
class MatchMismatchPlan(ControlPlan):
    """The host plan of MatchMismatchPass, numpy only (tests/test_match_mismatch_plan.py checks it without a GPU): a
    ControlPlan whose bank is the candidate list.  candidates: distinct recording indices whose audio forms the columns
    of the matrix, in the order given (default: every recording, in order); column c is always candidates[c], and
    own_col[r] is the position of r in `candidates` or -1.  The window selection is ControlPlan's (EEG windows from the
    EEG's own count, audio windows from the envelope's own: mvm:44-49, 74-78).  The bank holds the candidates with an
    audio window (k_a > 0) in the order of the columns, with ControlPlan's bank_off / seg_off_bank / bank_start; a
    candidate without one keeps its column with an EMPTY group:
      seg_off_col   (n_bands * n_col + 1) offsets into the bank's windows, band-major over the columns -- the group of
                    (band b, column c) is b * n_col + c
    and per shard, beside ControlPlan's tables:
      cls_e         the band of every EEG group (seg_off_e is band-major over the live recordings)
      own_col_e     the own column of every EEG group, -1 for a recording that is no candidate."""

    def __init__(self, eeg_lengths, env_lengths=None, candidates=None, shard_samples=DEFAULT_SHARD_SAMPLES, n_ch=47, n_bands=5,
                 fs=250, window_sec=1.0, overlap=0.75, max_windows=MAX_WINDOWS):
        n_rec = len(np.asarray(eeg_lengths).ravel())
        self.candidates = np.arange(n_rec, dtype=np.int64) if candidates is None else np.asarray(candidates, dtype=np.int64).ravel()
        assert ((self.candidates >= 0) & (self.candidates < n_rec)).all(), "candidates are recording indices"
        assert len(np.unique(self.candidates)) == len(self.candidates), "a recording is a candidate once"
        self.n_col = len(self.candidates)
        self.own_col = np.full(n_rec, -1, np.int64)
        self.own_col[self.candidates] = np.arange(self.n_col)
        super().__init__(eeg_lengths, env_lengths, None, shard_samples, n_ch, n_bands, fs, window_sec, overlap, max_windows)
        self.seg_off_col = np.concatenate([[0], np.cumsum(np.tile(self.k_a[self.candidates], self.nb))]).astype(np.int32)

    def _bank_members(self):
        return self.candidates

    def _shard_tables(self, r0, r1):
        t = super()._shard_tables(r0, r1)
        live = t["live"]
        t.update(cls_e=np.repeat(np.arange(self.nb), len(live)).astype(np.int32),
                 own_col_e=np.tile(self.own_col[r0 + live], self.nb).astype(np.int32))
        return t


MATCH_COLS = engine.MATCH_COLS      # [w_own, n_own_pairs, n_valid, n_less, n_equal, null_mean]


class MatchMismatchPass(ControlPass):
    """The control experiment against EVERY candidate audio, as a batched pass FROM HOST MEMORY: ControlPass's inputs and a
    candidate list go in; per (recording r, band b) the mean H1 Wasserstein distance between the EEG diagrams of r and the
    audio diagrams of every candidate c, paired by position (mvm:86-95), comes back as dist_h (n_rec, n_bands, n_col)
    float64 with the pair counts pairs_h (int32), and `run` returns rows_h (n_rec, n_bands, 6) = [w_own, n_own_pairs,
    n_valid, n_less, n_equal, null_mean] (engine.match_rows_dev): the matched distance (the own column, mvm:136-137), how
    many of the other candidates with a finite distance lie below / at it (midrank of the true audio: 1 + n_less +
    n_equal / 2 among n_valid + 1) and their mean.  The reference's mismatched column, any permutation null and the
    match-mismatch score follow from dist_h without another run (drivers.match_mismatch_summary).
    Phase 1, once per run, is ControlPass's with the candidates as the bank.  Phase 2, per shard: the shard driver's
    upload of the EEG and its band-pass bank, the EEG diagrams (ControlPass's EEG stage), ONE
    engine.wasserstein_matrix_dev launch against the bank and one engine.match_rows_dev launch.  The own audio is a
    column of the bank, so no envelope is uploaded, filtered or taken through Rips per shard.  A recording without an EEG
    window gets NaN, zero counts and zero pairs; a candidate without an audio window an all-NaN column with 0 pairs.
    sliced=dirs, an (M, 2) table of directions (engine._directions validates it; utils.default_directions makes one): the
    same matrix with the sliced Wasserstein distance (include/tdaeeg.h) in the place of the Wasserstein distance, by the
    prepared route: after phase 1 the bank's H1 diagrams are sorted once per run (engine.sliced_prepare_dev; the table is
    sized from one host read of the slot scan's total), and per shard, inside the step the repair redoes, the shard's EEG
    H1 diagrams are prepared into the buffer set's table, one engine.sliced_matrix_dev launch makes the matrix and one
    engine.match_rows_dev launch its rows.  `run` then also fills slc_dist_h (n_rec, n_bands, n_col) float64, slc_pairs_h
    (the same shape, int32) and slc_rows_h (n_rec, n_bands, 6), pinned, with the meaning of dist_h / pairs_h / rows_h.  A
    status bit of a sliced entry withholds the rows as one of a Wasserstein entry does.  Off by default: rows_h, dist_h and
    pairs_h are the same bytes with and without it.
    As ControlPass, the pass embeds its audio bank as the reference does; the landmark route (takens=) is not offered."""

    ROW_COLS = MATCH_COLS
    ROW_ZERO = slice(1, 5)              # the counts

    def __init__(self, eeg_lengths, env_lengths=None, candidates=None, device=None, shard_samples=DEFAULT_SHARD_SAMPLES,
                 n_sets=2, ctx=None, n_ch=47, fs=250, bands=preprocess.FREQ_BANDS, max_windows=MAX_WINDOWS, window_sec=1.0,
                 overlap=0.75, correlations=False, sliced=None):
        import torch
        plan = MatchMismatchPlan(eeg_lengths, env_lengths, candidates, shard_samples, n_ch, len(dict(bands)), fs, window_sec,
                                 overlap, max_windows)
        super().__init__(eeg_lengths, env_lengths, None, device, shard_samples, n_sets, ctx, n_ch, fs, bands, max_windows,
                         window_sec, overlap, correlations, plan=plan)
        P, dev, nb = plan, self.dev, len(self.bands)
        self.candidates, self.own_col, self.n_col = P.candidates, P.own_col, P.n_col
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)           # noqa: E731
        for d, t in zip(self.shards, P.tables):
            d.update(cls_e=up(t["cls_e"]), own_col_e=up(t["own_col_e"]))
        self.col_seg_off = up(P.seg_off_col)
        S = max((d["n"] for d in self.shards), default=1)
        n_seg = max((nb * d["n_live"] for d in self.shards), default=0)
        shape = (max(n_seg, 1), max(self.n_col, 1))
        for st in self.set:
            # the per-shard audio stage of ControlPass does not exist here: its buffers go
            for key in ("env", "ya", "worka", "aw", "caud", "tau_seg", "tau_win", "wm", "wx", "sm", "sx"):
                st[key] = None
            st["mat"] = torch.empty(shape, dtype=torch.float64, device=dev)
            st["mat_pairs"], st["mat_flags"] = (torch.empty(shape, dtype=torch.int32, device=dev) for _ in range(2))
            st["res"] = torch.empty((max(n_seg, 1), MATCH_COLS), dtype=torch.float64, device=dev)
            st["dist"] = torch.empty((S, nb, self.n_col), dtype=torch.float64, device=dev)
            st["pairs"] = torch.empty((S, nb, self.n_col), dtype=torch.int32, device=dev)
        self.dist_h = self.pairs_h = None
        # sliced=dirs: the direction table once, per buffer set the EEG side's table and the second matrix
        self.slc_dirs, self.slc_dirs_t, self.slc_bank, self.slc_bank_table = None, None, None, None
        self.slc_dist_h = self.slc_pairs_h = self.slc_rows_h = None
        if sliced is not None:
            self.slc_dirs = engine._directions(sliced)
            self.slc_dirs_t = torch.from_numpy(self.slc_dirs).to(dev)
            self.slc_ready = torch.cuda.Event()
            M = self.slc_dirs.shape[0]
            n_e = max((d["n_win"] for d in self.shards), default=0)
            for st in self.set:
                cap = st["ws"].eeg.h1_cap
                st["slc_table"] = torch.empty(2 * M * max(n_e, 1) * cap, dtype=torch.float64, device=dev)
                st["slc_slot"] = torch.zeros(max(n_e, 1) + 1, dtype=torch.int64, device=dev)
                st["slc_m"] = torch.empty(max(n_e, 1), dtype=torch.int32, device=dev)
                st["slc_mat"] = torch.empty(shape, dtype=torch.float64, device=dev)
                st["slc_mat_pairs"], st["slc_mat_flags"] = (torch.empty(shape, dtype=torch.int32, device=dev) for _ in range(2))
                st["slc_res"] = torch.empty((max(n_seg, 1), MATCH_COLS), dtype=torch.float64, device=dev)
                st["slc_seg_flags"] = torch.zeros(max(n_seg, 1), dtype=torch.int32, device=dev)
                st["slc_dist"] = torch.empty((S, nb, self.n_col), dtype=torch.float64, device=dev)
                st["slc_pairs"] = torch.empty((S, nb, self.n_col), dtype=torch.int32, device=dev)
                st["slc_rows"] = torch.empty((S, nb, MATCH_COLS), dtype=torch.float64, device=dev)

    def _phase1(self, env_f):
        """ControlPass's bank; with sliced=dirs its H1 diagrams are then sorted once (one host read: the rows of the table)."""
        import torch
        super()._phase1(env_f)
        if self.slc_dirs is None:
            return
        with torch.cuda.stream(self.bank_stream):
            M, cap = self.slc_dirs.shape[0], self.bank.h1.shape[1]
            slot_off = engine.sliced_slots_dev(self.bank.c1, cap)
            need = 2 * M * int(slot_off[-1])                             # (the read: once per run, not per shard)
            if self.slc_bank_table is None or self.slc_bank_table.numel() < need:
                self.slc_bank_table = torch.empty(max(need, 1), dtype=torch.float64, device=self.dev)
            self.slc_bank = engine.sliced_prepare_dev(self.bank.h1, self.bank.c1, self.slc_dirs_t, table_t=self.slc_bank_table,
                                                      slot_off=slot_off, ctx=self.ctx)
            self.slc_ready.record(self.bank_stream)

    def _upload(self, st, i, raw_packed_h, env_packed_h):
        r0, r1 = self.ranges[i]
        e0, e1 = self.n_ch * int(self.eeg_off[r0]), self.n_ch * int(self.eeg_off[r1])
        st["raw"][:e1 - e0].copy_(raw_packed_h.view(-1)[e0:e1], non_blocking=True)

    def _shard_step(self, st, i):
        d = self.shards[i]
        if d["n_win"] == 0:                                            # no recording of the shard has a window
            self._rows(st, i, None)
            return
        preprocess.bandpass_bank_ragged_dev(st["raw"], d["eeg_tb"], self.eeg_bank, n_ch=self.n_ch, y_t=st["y"],
                                            work_t=st["work"], ctx=self.ctx)
        self._rows(st, i, self._rips_step(st, i, "one"))

    def _rips_step(self, st, i, retry):
        """The EEG's Rips stage of a shard, the matrix against the bank and its rows: (n_bands * n_live, 6)."""
        import torch
        ctx, d, v = self.ctx, self.shards[i], st["views"][i]
        with ctx.deferred(retry):
            engine.eeg_window_ragged_dev(st["y"], d["eeg_start"], d["eeg_ld"], self.win, out=v.eeg, n_ch=v.eeg.h0_cap, ctx=ctx)
        engine.diagram_finish_dev([(v.eeg.h1, v.eeg.c1, True, None)], ctx=ctx)
        torch.cuda.current_stream().wait_event(self.bank_ready)
        n = v.n_seg * self.n_col
        mat, mp, mf = (st[k].view(-1)[:n].view(v.n_seg, self.n_col) for k in ("mat", "mat_pairs", "mat_flags"))
        engine.wasserstein_matrix_dev(v.eeg.h1, v.eeg.c1, v.seg_off, d["cls_e"], self.bank.h1, self.bank.c1, self.col_seg_off,
                                      self.bank.status, self.n_col, out_t=mat, pairs_t=mp, flags_t=mf, ctx=ctx)
        res = engine.match_rows_dev(mat, mp, mf, d["own_col_e"], rows_t=st["res"][:v.n_seg], status_a=v.eeg.status,
                                    seg_off_a=v.seg_off, seg_flags=v.seg_flags, ctx=ctx)
        if self.slc_dirs is not None:
            # the same matrix with the sliced distance: the shard's EEG diagrams sorted once, then merges against the bank
            torch.cuda.current_stream().wait_event(self.slc_ready)
            n_e = v.eeg.h1.shape[0]
            slot = engine.sliced_slots_dev(v.eeg.c1[:n_e], v.eeg.h1.shape[1], out=st["slc_slot"][:n_e + 1])
            ta = engine.sliced_prepare_dev(v.eeg.h1, v.eeg.c1, self.slc_dirs_t, table_t=st["slc_table"], slot_off=slot,
                                           m_t=st["slc_m"], ctx=ctx)
            smat, smp, smf = (st[k].view(-1)[:n].view(v.n_seg, self.n_col) for k in ("slc_mat", "slc_mat_pairs", "slc_mat_flags"))
            engine.sliced_matrix_dev(ta, v.seg_off, d["cls_e"], self.slc_bank, self.col_seg_off, self.bank.status, self.n_col,
                                     out_t=smat, pairs_t=smp, flags_t=smf, ctx=ctx)
            sfl = st["slc_seg_flags"][:v.n_seg]
            engine.match_rows_dev(smat, smp, smf, d["own_col_e"], rows_t=st["slc_res"][:v.n_seg], seg_flags=sfl, ctx=ctx)
            v.seg_flags.bitwise_or_(sfl)                                 # a flagged sliced entry withholds the rows too
        if retry != "auto":
            v.flags_host.copy_(v.seg_flags, non_blocking=True)
        return res

    def _rows(self, st, i, res):
        """The rows as ControlPass scatters them, and the matrix of the shard, (n_bands * n_live, n_col) band-major, to
        the recordings: dist NaN and 0 pairs for a recording without a window."""
        super()._rows(st, i, res)
        d, nb = self.shards[i], len(self.bands)
        dist, pairs = st["dist"][:d["n"]], st["pairs"][:d["n"]]
        if d["n_live"] < d["n"]:
            dist.fill_(float("nan"))
            pairs.zero_()
        if d["n_live"] and self.n_col:
            n = nb * d["n_live"] * self.n_col
            for dst, key in ((dist, "mat"), (pairs, "mat_pairs")):
                dst.index_copy_(0, d["live"], st[key].view(-1)[:n].view(nb, d["n_live"], self.n_col).transpose(0, 1))
        if self.slc_dirs is None:
            return
        sdist, spairs, srows = st["slc_dist"][:d["n"]], st["slc_pairs"][:d["n"]], st["slc_rows"][:d["n"]]
        if d["n_live"] < d["n"]:
            sdist.fill_(float("nan"))
            spairs.zero_()
            srows.fill_(float("nan"))
            srows[:, :, self.ROW_ZERO] = 0.0
        if d["n_live"] and res is not None:
            srows.index_copy_(0, d["live"], st["slc_res"][:nb * d["n_live"]].view(nb, d["n_live"], MATCH_COLS).transpose(0, 1))
            if self.n_col:
                n = nb * d["n_live"] * self.n_col
                for dst, key in ((sdist, "slc_mat"), (spairs, "slc_mat_pairs")):
                    dst.index_copy_(0, d["live"], st[key].view(-1)[:n].view(nb, d["n_live"], self.n_col).transpose(0, 1))

    def _more_back(self, st, r0, r1, non_blocking):
        self.dist_h[r0:r1].copy_(st["dist"][:r1 - r0], non_blocking=non_blocking)
        self.pairs_h[r0:r1].copy_(st["pairs"][:r1 - r0], non_blocking=non_blocking)
        if self.slc_dirs is not None:
            self.slc_dist_h[r0:r1].copy_(st["slc_dist"][:r1 - r0], non_blocking=non_blocking)
            self.slc_pairs_h[r0:r1].copy_(st["slc_pairs"][:r1 - r0], non_blocking=non_blocking)
            self.slc_rows_h[r0:r1].copy_(st["slc_rows"][:r1 - r0], non_blocking=non_blocking)

    def run(self, raw_packed_h, env_packed_h, rows_h=None):
        """raw_packed_h: flat pinned float64, n_ch * sum(L); env_packed_h: flat pinned float64, sum(Le).  Returns rows_h
        (n_rec, n_bands, 6), pinned, and fills self.dist_h (n_rec, n_bands, n_col) float64 and self.pairs_h (the same shape,
        int32), pinned, in list order -- with sliced=dirs also self.slc_dist_h, self.slc_pairs_h and self.slc_rows_h; all
        complete when the call returns."""
        import torch
        shape = (self.n_rec, len(self.bands), self.n_col)
        if self.dist_h is None:
            self.dist_h = torch.empty(shape, dtype=torch.float64).pin_memory()
            self.pairs_h = torch.empty(shape, dtype=torch.int32).pin_memory()
        if self.slc_dirs is not None and self.slc_dist_h is None:
            self.slc_dist_h = torch.empty(shape, dtype=torch.float64).pin_memory()
            self.slc_pairs_h = torch.empty(shape, dtype=torch.int32).pin_memory()
            self.slc_rows_h = torch.empty((self.n_rec, len(self.bands), MATCH_COLS), dtype=torch.float64).pin_memory()
        return super().run(raw_packed_h, env_packed_h, rows_h)
