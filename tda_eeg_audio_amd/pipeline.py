"""
pipeline.py -- the end-to-end per-window unit of the reference, batched on one GPU.

Counterpart of the hot loop of process_recording (scripts/tda_eeg_audio_comparison.py:77-122):
for every selected window  corr->dist (nb2:198-207) -> Rips(EEG) (cmp:93) ; tau once per
recording-band from its first selected window (cmp:83) -> Takens -> Rips(audio) (cmp:89-92) ->
Wasserstein H0 and H1 (cmp:95-96) -> features of the H1 diagrams (cmp:98-99); then per
recording-band np.nanmean of the distances (cmp:117-118) and the mean/std feature aggregation of
process_file_features (scripts/tda_eeg_classification_v2.py:429-436).

Everything stays in HBM; each stage is one C-ABI launch on torch's current stream.  torch is
only the allocator / stream owner here.
"""
import collections
import functools
import inspect

import numpy as np

from . import _lib, engine

RESULT_COLS = 4 + 44      # [w_h0, w_h1, tau, n_windows] + 44 aggregated EEG features per recording-band
# a group's block of each optional output (OUTPUTS, below, describes them)
CORR_COLS = 2 * len(engine.SPEARMAN_COLS)      # corr: [r, p] of the five series (cmp:104-114)
BOTT_COLS = 2             # bott: [b_h0, b_h1], the means of the bottleneck distances
SLC_COLS = 2              # slc: [s_h0, s_h1], the means of the sliced Wasserstein distances
WQ_COLS = 2               # wq: [q_h0, q_h1], the means of that Wasserstein distance
LAND_SETS = 3             # land: the diagram sets EEG H0, EEG H1, audio H1, in this order
IMG_SETS = 3              # img: the same three diagram sets, in the same order
FM_SETS = 3               # fm: the same three diagram sets, in the same order
KD_COLS = 2               # kd: [k_h0, k_h1], the means of the kernel-induced distances
PF_COLS = 2               # pf: [f_h0, f_h1], the means of the persistence Fisher distances
SL_COLS = 22              # sl: the 11 features of the audio window's sublevel-set diagram, then of the EEG channels'
PL_COLS = 24              # pl: the 11 features of H0, then of H1, of the PLV-distance Rips complex, then [w_h0, w_h1]

Output = collections.namedtuple("Output", "name shape params")      # a record of step_outputs


def _head(buf, n):
    """The first n windows (or groups) of a buffer: a tensor, a tuple of tensors or an engine.DeviceDiagrams / DeviceLandmarks."""
    if buf is None:
        return None
    if isinstance(buf, tuple):
        return tuple(t[:n] for t in buf)
    return buf.head(n) if hasattr(buf, "head") else buf[:n]


class Workspace:
    """Pre-allocated device buffers for a batch of n_win windows grouped into recordings."""

    lm = takens = None
    # (the attributes of the optional outputs, None where the output is off, are set from OUTPUTS, below)

    def __init__(self, n_win, seg_off, device, n_ch=47, h1_cap=engine.DEFAULT_H1_CAP, *, takens=None,
                 sublevel_bytes=engine.SL_SCRATCH_BYTES, **outputs):
        """**outputs: the keywords of step_outputs, validated there (TypeError for any other keyword); `outputs` keeps its
        table.  run_step also fills every enabled output, the group in front: `<name>` (n_seg,) + shape.  What else a
        record of OUTPUTS allocates here -- per-window buffers, tables uploaded once -- stands in its paragraph of
        step_outputs' docstring; its validated parameters are the attribute named like its keyword.
        sublevel_bytes: the bound on the scratch of the `sl` output.
        takens=None: the audio stage as the reference runs it (dim 3, subsample 2, every point; at most 128 points).
        takens=(dim, subsample, n_perm): the audio stage embeds with these and runs Rips on n_perm greedy landmarks
        (engine.takens_rips_landmarks_dev), for clouds of up to LM_MAX_POINTS points; `lm` (an engine.DeviceLandmarks,
        allocated here) then holds the landmarks of every window, lm.r_cover their covering radius and lm.n_full the size
        of the whole cloud.  No column of `result` changes meaning.  TdaError for parameters outside their limits."""
        import torch
        self.n_win, self.device = n_win, device
        if takens is not None:
            dim, subsample, n_perm = takens
            n_perm, dim, subsample = engine.landmark_args(n_perm, dim, subsample)
            self.takens = (dim, subsample, n_perm)
            self.lm = engine.DeviceLandmarks(n_win, n_perm, dim, device)
        seg_off = np.asarray(seg_off, np.int32)
        assert seg_off[0] == 0 and seg_off[-1] == n_win
        self.n_seg = len(seg_off) - 1
        self.seg_off = torch.from_numpy(seg_off).to(device)
        rec_id = np.repeat(np.arange(self.n_seg), np.diff(seg_off))
        self.rec_id = torch.from_numpy(rec_id.astype(np.int64)).to(device)
        self.first_idx = torch.from_numpy(seg_off[:-1].astype(np.int64)).to(device)
        f64 = dict(dtype=torch.float64, device=device)
        self.eeg = engine.DeviceDiagrams(n_win, n_ch, h1_cap, device)
        self.aud = engine.DeviceDiagrams(n_win, 128, h1_cap, device)
        self.tau_seg = torch.empty(self.n_seg, dtype=torch.int32, device=device)
        self.tau_win = torch.empty(n_win, dtype=torch.int32, device=device)
        self.seg_flags = torch.zeros(self.n_seg, dtype=torch.int32, device=device)     # class-overflow bits per group
        self.flags_host = torch.zeros(self.n_seg, dtype=torch.int32).pin_memory()
        self.w0 = torch.empty(n_win, **f64); self.w1 = torch.empty(n_win, **f64)
        self.ws0 = torch.empty(n_win, dtype=torch.int32, device=device)
        self.ws1 = torch.empty(n_win, dtype=torch.int32, device=device)
        self.fe0 = torch.empty((n_win, 11), **f64); self.fe1 = torch.empty((n_win, 11), **f64)
        self.fa1 = torch.empty((n_win, 11), **f64)
        self.result = torch.empty((self.n_seg, RESULT_COLS), **f64)
        self.outputs = step_outputs(**outputs)
        self.sublevel_bytes, self.n_ch = int(sublevel_bytes), n_ch
        for o in self.outputs:
            spec = OUTPUT_BY_NAME[o.name]
            setattr(self, spec.keyword, True if o.params is None else o.params)
            if len(o.shape) == 1:
                setattr(self, o.name, torch.empty((self.n_seg,) + o.shape, **f64))
            else:
                # a block per diagram set: stored set-major, one contiguous (n_seg, ...) block per launch (<name>_sets);
                # `<name>` is the same memory seen group-major
                sets = torch.empty((o.shape[0], self.n_seg) + o.shape[1:], **f64)
                setattr(self, o.name + "_sets", sets)
                setattr(self, o.name, sets.permute(1, 0, 2, 3))
            for attr, make in {**spec.per_window, **spec.per_group, **spec.tables}.items():
                setattr(self, attr, make(self))             # its further buffers, and its tables, uploaded once
        self.n_win_seg = torch.from_numpy(np.diff(seg_off).astype(np.float64)).to(device)
        self.side_stream = torch.cuda.Stream(device=device)
        import os
        # TDA_OVERLAP=1: EEG chain on a side stream.  Off by default since round 3: a step that forks takes two of the
        # four hardware queues, so only two lanes make progress at a time and their audio kernels end together,
        # leaving the CUs to the (latency-bound, nearly empty) widening passes -- measured with tools/share_ab.sh:
        # one stream per lane is +1.5 % on the full corpus and +9-12 % on the share a rank of eight holds
        self.overlap = os.environ.get("TDA_OVERLAP", "0") != "0"
        # fused EEG window kernel (corr -> dist -> Rips in one launch, the matrix stays in LDS); "0": the two-kernel
        # path through ws.dist (also taken when the channel count is outside the fused kernel's 33..48)
        self.fused = os.environ.get("TDA_FUSED_EEG", "1") != "0" and 33 <= n_ch <= 48
        self.dist = None if self.fused else torch.empty((n_win, n_ch, n_ch), **f64)

    def view(self, seg_off):
        """A Workspace over the first seg_off[-1] windows and len(seg_off) - 1 groups of THIS one's buffers, with segment
        tables of its own (uploaded once, here): one buffer set sized by the largest shard of
        recordings.RaggedRecordingPass serves every shard through one view per shard.  Views share every buffer, so only
        one of them may be in flight at a time."""
        import copy
        import torch
        seg_off = np.asarray(seg_off, np.int32)
        n_win, n_seg = int(seg_off[-1]), len(seg_off) - 1
        assert seg_off[0] == 0 and (np.diff(seg_off) >= 0).all() and n_win <= self.n_win and n_seg <= self.n_seg
        v = copy.copy(self)
        v.n_win, v.n_seg = n_win, n_seg
        v.seg_off = torch.from_numpy(seg_off).to(self.device)
        v.rec_id = torch.from_numpy(np.repeat(np.arange(n_seg), np.diff(seg_off)).astype(np.int64)).to(self.device)
        v.first_idx = torch.from_numpy(seg_off[:-1].astype(np.int64)).to(self.device)
        v.n_win_seg = torch.from_numpy(np.diff(seg_off).astype(np.float64)).to(self.device)
        on = [OUTPUT_BY_NAME[o.name] for o in self.outputs]
        for name in ["eeg", "aud", "lm", "tau_win", "w0", "w1", "ws0", "ws1", "fe0", "fe1", "fa1", "dist",
                     *(a for spec in on for a in spec.per_window)]:
            setattr(v, name, _head(getattr(self, name), n_win))
        for name in ["tau_seg", "seg_flags", "flags_host", "result", *(a for spec in on for a in spec.per_group)]:
            setattr(v, name, _head(getattr(self, name), n_seg))
        for o in self.outputs:
            if len(o.shape) == 1:
                setattr(v, o.name, getattr(self, o.name)[:n_seg])
            else:
                sets = getattr(self, o.name + "_sets")[:, :n_seg]
                setattr(v, o.name + "_sets", sets)
                setattr(v, o.name, sets.permute(1, 0, 2, 3))
        return v


def run_step(eeg_win, audio_win, ws, ctx=None, max_lag=125, timers=None, retry="auto", eeg_sliding=None, eeg_table=None):
    """One pass of the hot path over the batch.  eeg_win (n_win,47,250) f64, audio_win (n_win,250)
    f64, both resident in HBM.  Returns ws.result (n_seg, 48).
    eeg_sliding = (sig_t (n_rec, 47, L), win_len, step, sel_t): the EEG windows are read IN PLACE from band-passed
    recordings instead (window sel_t[i] = r * n_win_per_rec + k; eeg_win is ignored) -- recordings.RecordingPass.
    eeg_table = (sig_t, start_t, ld_t, win_len): the EEG windows are read in place from packed band-passed recordings of
    different lengths through a window table (engine.eeg_window_ragged_dev) -- recordings.RaggedRecordingPass.
    `timers`: optional dict of
    (start,end) torch.cuda.Event pairs per stage, recorded on the launch stream.
    retry="auto": every Rips call launches its widening passes (exact by itself).  retry="first": first passes
    only; retry="one": first passes plus ONE widening pass each (TDA_RETRY_ONE_STEP: the wide rungs of the ladder
    wait for a nearly empty CU even when they have nothing to redo).  In both cases the class-overflow bits that are
    left are copied to ws.flags_host (pinned) at the end of the step and the caller re-runs the step with
    retry="auto" if any is set (pipeline.Lanes does: verify, then publish)."""
    import torch
    ctx = ctx or _lib.get_ctx()
    with ctx.deferred(retry):                    # one finishing pass for the three diagram sets of the batch
        return _run_step(eeg_win, audio_win, ws, ctx, max_lag, timers, retry, eeg_sliding, eeg_table)


def _run_step(eeg_win, audio_win, ws, ctx, max_lag, timers, retry, eeg_sliding=None, eeg_table=None):
    import torch

    def stage(name, fn):
        if timers is None or name not in timers:
            return fn()
        s, e = timers[name]
        s.record()
        r = fn()
        e.record()
        return r

    # The EEG chain (corr->dist->Rips) and the audio chain (tau->Takens->Rips) are independent until
    # the Wasserstein step; with ws.overlap the EEG kernels run on a side stream (see Workspace: not the default,
    # the other lanes fill the tails better than a fork inside the step does).
    main = torch.cuda.current_stream()
    side = ws.side_stream if ws.overlap else main
    if ws.overlap:
        side.wait_stream(main)
    with torch.cuda.stream(side):
        if eeg_table is not None:
            sig_t, start_t, ld_t, win_len = eeg_table
            stage("eeg_window", lambda: engine.eeg_window_ragged_dev(sig_t, start_t, ld_t, win_len, out=ws.eeg,
                                                                     n_ch=ws.eeg.h0_cap, ctx=ctx))
        elif eeg_sliding is not None:
            sig_t, win_len, step, sel_t = eeg_sliding
            stage("eeg_window", lambda: engine.eeg_window_sliding_dev(sig_t, win_len, step, sel_t=sel_t, out=ws.eeg, ctx=ctx))
        elif ws.fused and eeg_win.shape[2] <= 256:
            stage("eeg_window", lambda: engine.eeg_window_dev(eeg_win, ws.eeg, ctx=ctx))
        else:
            if ws.dist is None:
                ws.dist = torch.empty((ws.n_win, eeg_win.shape[1], eeg_win.shape[1]), dtype=torch.float64, device=ws.device)
            stage("corr_dist", lambda: engine.corr_dist_dev(eeg_win, ws.dist, None, ctx=ctx))
            stage("rips_eeg", lambda: engine.rips_dm_dev(ws.dist, ws.eeg, ctx=ctx))
    # tau from the first selected window of each recording-band (cmp:83), written per group and per window
    stage("tau", lambda: engine.tau_segments_dev(audio_win, ws.seg_off, max_lag, ws.tau_seg, ws.tau_win, ctx=ctx))
    if ws.takens is None:
        stage("rips_audio", lambda: engine.takens_rips_dev(audio_win, ws.tau_win, ws.aud, ctx=ctx))
    else:
        dim, subsample, _ = ws.takens
        stage("rips_audio", lambda: engine.takens_rips_landmarks_dev(audio_win, ws.tau_win, ws.aud, ws.lm, dim=dim,
                                                                     subsample=subsample, ctx=ctx))
    if ws.overlap:
        main.wait_stream(side)
    # H1 rows of both Rips stages into ripser's order + extract_features of EEG H0 / EEG H1 / audio H1
    # (cmp:98-99, v2:415-416): one launch, one wavefront per diagram
    stage("finish", lambda: engine.diagram_finish_dev([(ws.eeg.h0, ws.eeg.c0, False, ws.fe0),
                                                        (ws.eeg.h1, ws.eeg.c1, True, ws.fe1),
                                                        (ws.aud.h1, ws.aud.c1, True, ws.fa1)], ctx=ctx))
    # the optional outputs that are on, in LAUNCH_ORDER around the two Wasserstein stages of `result`
    on = {o.name for o in ws.outputs}
    inputs = (eeg_win, audio_win, eeg_sliding, eeg_table)
    for name in LAUNCH_ORDER:
        if name is None:
            stage("wasserstein_h0", lambda: engine.wasserstein_dev(ws.eeg.h0, ws.eeg.c0, ws.aud.h0, ws.aud.c0,
                                                                   out_t=ws.w0, status_t=ws.ws0, ctx=ctx))
            stage("wasserstein_h1", lambda: engine.wasserstein_dev(ws.eeg.h1, ws.eeg.c1, ws.aud.h1, ws.aud.c1,
                                                                   out_t=ws.w1, status_t=ws.ws1, ctx=ctx))
        elif name in on:
            OUTPUT_BY_NAME[name].launch(ws, ctx, stage, inputs)
    # per recording-band rows: nanmean of the distances (cmp:117-118), tau, window count, mean/std of the EEG
    # features (v2:429-436) -- one launch
    stage("reduce", lambda: engine.recording_rows_dev(ws.w0, ws.w1, ws.tau_seg, ws.fe0, ws.fe1, ws.seg_off, ws.result,
                                                      ws.eeg.status, ws.aud.status, ws.seg_flags, ctx=ctx))
    if retry != "auto":
        ws.flags_host.copy_(ws.seg_flags, non_blocking=True)
    return ws.result


def pair_means(ws, ctx, stage, name, launch, d, ds, means):
    """Stages name_h0 / name_h1: the H0 and the H1 diagram pairs of every window through `launch` (d[k], status ds[k]);
    then means[:, k], the means of recording_rows_dev's windows: masked on the device, one nanmean launch per leg."""
    import torch
    legs = ((ws.eeg.h0, ws.eeg.c0, ws.aud.h0, ws.aud.c0), (ws.eeg.h1, ws.eeg.c1, ws.aud.h1, ws.aud.c1))
    for k, leg in enumerate(legs):
        stage(f"{name}_h{k}", lambda: launch(*leg, out_t=d[k], status_t=ds[k], ctx=ctx))
    out = (ws.aud.status & (_lib.TDA_WIN_DEGENERATE | _lib.TDA_WIN_TOO_LARGE)) != 0
    nan = torch.full((), float("nan"), dtype=torch.float64, device=ws.device)
    for k in range(2):
        seg_mean = engine.segment_nanmean_dev(torch.where(out | (ds[k] != 0), nan, d[k]), ws.seg_off, ctx=ctx)
        means[:, k].copy_(seg_mean)


def _set_means_stage(ws, ctx, audio, launch, out_sets):
    """One launch per diagram set, EEG H0, EEG H1 and (audio=True) audio H1, each writing only the group means of its set,
    out_sets[s]; launch: the engine's launcher with the output's own parameters bound."""
    sets = [(ws.eeg.h0, ws.eeg.c0, None, 0), (ws.eeg.h1, ws.eeg.c1, None, 0)]
    if audio:
        sets.append((ws.aud.h1, ws.aud.c1, ws.aud.status, _lib.TDA_WIN_DEGENERATE | _lib.TDA_WIN_TOO_LARGE))
    for s, (rows, cnt, status, mask) in enumerate(sets):
        launch(rows, cnt, seg_off_t=ws.seg_off, status_t=status, skip_mask=mask, out_t=out_sets[s], ctx=ctx)


def _eeg_window_table(ws, eeg_win, eeg_sliding, eeg_table):
    """Where the step's EEG kernel reads its windows, for the kernels that take a window table: (sig_t, the table keywords of
    engine.sublevel_features_dev / plv_dist_dev -- none for stacked windows --, n_t).  For eeg_sliding the table is derived
    here, on the device, from its arguments."""
    import torch
    n_ch = ws.n_ch
    if eeg_table is not None:
        sig_t, start_t, ld_t, win_len = eeg_table
        tab = dict(n_t=int(win_len), win_start_t=start_t, win_ld_t=ld_t, n_ch=n_ch)
    elif eeg_sliding is not None:
        sig_t, win_len, step, sel_t = eeg_sliding
        n_rec, ch, L = sig_t.shape
        assert ch == n_ch
        per_rec = (L - win_len) // step + 1 if L >= win_len else 0
        sel = torch.arange(n_rec * per_rec, device=ws.device) if sel_t is None else sel_t.to(torch.int64)
        start_t = torch.div(sel, max(per_rec, 1), rounding_mode="floor") * (n_ch * L) + (sel % max(per_rec, 1)) * step
        tab = dict(n_t=int(win_len), win_start_t=start_t.contiguous(), win_ld_t=torch.full_like(start_t, L), n_ch=n_ch)
    else:
        sig_t, tab = eeg_win, {}
    return sig_t, tab, (tab["n_t"] if tab else eeg_win.shape[-1])


def _phase_locking_stage(ws, ctx, eeg_win, eeg_sliding, eeg_table):
    """ws.pl of the step: the phase-locking distance matrix of every EEG window (read where the step's EEG kernel reads it),
    Rips on it, the finishing pass (H1 rows into ripser's order, the features of H0 and H1), the Wasserstein distances to the
    audio diagrams, then the 24 group means.  The Rips call runs its whole ladder whatever the step's retry policy (the
    policy is put back afterwards): it is exact by itself, so no class-overflow bit of it has to travel to the host."""
    import torch
    n_win = ws.n_win
    sig_t, tab, _ = _eeg_window_table(ws, eeg_win, eeg_sliding, eeg_table)
    engine.plv_dist_dev(sig_t, method=engine.METHOD_NAMES[ws.phase_locking], out=ws.pl_dist, status_t=ws.pl_st, ctx=ctx, **tab)
    bad = ws.pl_st != 0
    torch.where(bad[:, None, None], ws.pl_line, ws.pl_dist, out=ws.pl_dist)
    policy = ctx.retry_policy
    ctx.set_retry_policy(ctx.RETRY_AUTO)
    try:
        engine.rips_dm_dev(ws.pl_dist, ws.pl_dgm, ctx=ctx)
    finally:
        ctx.set_retry_policy(policy)
    engine.diagram_finish_dev([(ws.pl_dgm.h0, ws.pl_dgm.c0, False, ws.pl_f0), (ws.pl_dgm.h1, ws.pl_dgm.c1, True, ws.pl_f1)],
                              ctx=ctx)
    engine.wasserstein_dev(ws.pl_dgm.h0, ws.pl_dgm.c0, ws.aud.h0, ws.aud.c0, out_t=ws.pl_w0, status_t=ws.pl_ws0, ctx=ctx)
    engine.wasserstein_dev(ws.pl_dgm.h1, ws.pl_dgm.c1, ws.aud.h1, ws.aud.c1, out_t=ws.pl_w1, status_t=ws.pl_ws1, ctx=ctx)
    nan = torch.full((), float("nan"), dtype=torch.float64, device=ws.device)
    bad = bad | (ws.pl_dgm.status != 0)
    out = bad | ((ws.aud.status & (_lib.TDA_WIN_DEGENERATE | _lib.TDA_WIN_TOO_LARGE)) != 0)
    cols = ws.pl_cols[:PL_COLS * n_win].view(PL_COLS, n_win)
    cols[:11].copy_(torch.where(bad[:, None], nan, ws.pl_f0).t())
    cols[11:22].copy_(torch.where(bad[:, None], nan, ws.pl_f1).t())
    cols[22].copy_(torch.where(out | (ws.pl_ws0 != 0), nan, ws.pl_w0))
    cols[23].copy_(torch.where(out | (ws.pl_ws1 != 0), nan, ws.pl_w1))
    for k in range(PL_COLS):
        ws.pl[:, k].copy_(engine.segment_nanmean_dev(cols[k], ws.seg_off, ctx=ctx))


def _sublevel_stage(ws, ctx, eeg_win, audio_win, eeg_sliding, eeg_table):
    """ws.sl of the step: the features of the sublevel-set diagrams of the audio windows and of the EEG channels (read where
    the step's EEG kernel reads them: stacked, or in place through the window table, which for eeg_sliding is derived here,
    on the device, from its arguments), then the 22 group means."""
    import torch
    n_win, n_ch = ws.n_win, ws.n_ch

    def scratch(ch, n_t):
        if (ch, n_t) not in ws.sl_scratch:
            ws.sl_scratch[(ch, n_t)] = engine.SublevelScratch(ch, n_t, ws.device, ws.sublevel_bytes, n_win=ws.sl_n_win)
        return ws.sl_scratch[(ch, n_t)]

    engine.sublevel_features_dev(audio_win.view(n_win, 1, -1), out_t=ws.sl_fa, status_t=ws.sl_sa,
                                 scratch=scratch(1, audio_win.shape[-1]), ctx=ctx)
    sig_t, tab, n_t = _eeg_window_table(ws, eeg_win, eeg_sliding, eeg_table)
    engine.sublevel_features_dev(sig_t, out_t=ws.sl_fe, status_t=ws.sl_se, scratch=scratch(n_ch, n_t), ctx=ctx, **tab)
    cols = ws.sl_cols[:SL_COLS * n_win].view(SL_COLS, n_win)
    cols[:11].copy_(ws.sl_fa.view(n_win, 11).t())
    cols[11:].copy_(ws.sl_fe.mean(dim=1).t())                        # np.mean over the channels: NaN if any is flagged
    for k in range(SL_COLS):
        ws.sl[:, k].copy_(engine.segment_nanmean_dev(cols[k], ws.seg_off, ctx=ctx))


def _frechet_stage(ws, ctx, audio):
    """ws.fm of the step, (n_seg, cap + 2, 2) per set: one launch per diagram set into ws.fm_out, then the set's block --
    the mean with NaN beyond its count, [count, variance], [iterations, status]."""
    import torch
    cap, max_iter = ws.frechet

    def launch(rows, cnt, seg_off_t, status_t, skip_mask, out_t, ctx):
        mean, mc, var, it, st = engine.frechet_mean_dev(rows, cnt, seg_off_t=seg_off_t, status_t=status_t, skip_mask=skip_mask,
                                                        max_iter=max_iter, out=ws.fm_out, ctx=ctx)
        live = torch.arange(cap, device=ws.device)[None, :, None] < mc[:, None, None]
        out_t[:, :cap] = torch.where(live, mean, torch.full((), float("nan"), dtype=torch.float64, device=ws.device))
        out_t[:, cap, 0] = mc; out_t[:, cap, 1] = var
        out_t[:, cap + 1, 0] = it; out_t[:, cap + 1, 1] = st
    _set_means_stage(ws, ctx, audio, launch, ws.fm_sets)


# ------------------------------------------------------------------------------------------------------------
# the optional outputs: one record each.  What is particular to an output stands in its record and in the functions the
# record names, nowhere else: Workspace, run_step, run_features_step and the passes of recordings.py go through OUTPUTS
# ------------------------------------------------------------------------------------------------------------
# A record of OUTPUTS:
#   name, keyword  the Workspace attribute of its block (n_seg,) + shape, and the keyword that turns it on; the Workspace
#                  attribute named like the keyword keeps the validated parameters (True if it has none), `off` otherwise
#   doc, validate(v)   its paragraph of step_outputs' docstring; for v other than None: None if v leaves it off, else
#                  (shape of a group's block, validated parameters)
#   stages, launch(ws, ctx, stage, inputs)   its part of run_step, timed under these names by stage(name, fn); inputs =
#                  (eeg_win, audio_win, eeg_sliding, eeg_table).  Parameters and tables are read from `ws` at step time
#   set_stage(ws, ctx, audio)   of a set mean: its launches; run_features_step runs it with audio=False (the EEG sets alone)
#   arg(params)    a value of the keyword that validates to these parameters again (recordings.py hands it to Workspace)
#   per_window, per_group, tables   {attribute: make(ws)} of what else it owns in a Workspace, None while it is off: buffers
#                  with a row per window, tuples of buffers with a row per group (Workspace.view slices both), and tables,
#                  parameters and scratch that views share
OutputSpec = collections.namedtuple(
    "OutputSpec", "name keyword doc validate stages launch off set_stage arg per_window per_group tables",
    defaults=(None, None, lambda params: True if params is None else params, {}, {}, {}))


def _empty(dtype, ws, *shape):
    import torch
    return torch.empty(shape, dtype=getattr(torch, dtype), device=ws.device)


_f64, _i32 = functools.partial(_empty, "float64"), functools.partial(_empty, "int32")


def _dev(ws, array):
    import torch
    return torch.from_numpy(array).to(ws.device)


def _switch(*shape):
    """validate of an output without parameters."""
    return lambda value: (shape, None) if value else None


def _pair_distance(name, keyword, doc, validate, prefix, stage_name, launcher, extra=lambda ws: {}, **more):
    """A distance between the H0 / H1 diagram pairs of every window and its group means (pair_means): the engine's
    `launcher` with the further keywords extra(ws); per window the distances <prefix>0 / <prefix>1 and their status words
    <prefix>s0 / <prefix>s1."""
    d, ds = (prefix + "0", prefix + "1"), (prefix + "s0", prefix + "s1")

    def launch(ws, ctx, stage, inputs):
        pair_means(ws, ctx, stage, stage_name, functools.partial(launcher, **extra(ws)), [getattr(ws, a) for a in d],
                   [getattr(ws, a) for a in ds], getattr(ws, name))
    doc += f".\n            Workspace: the distances of every window `{d[0]}` / `{d[1]}` (n_win), status words `{ds[0]}` / `{ds[1]}`"
    per_window = {**{a: lambda ws: _f64(ws, ws.n_win) for a in d}, **{a: lambda ws: _i32(ws, ws.n_win) for a in ds}}
    return OutputSpec(name, keyword, doc, validate, (stage_name + "_h0", stage_name + "_h1"), launch, per_window=per_window,
                      **more)


def _set_means(name, keyword, doc, validate, stage_name, launcher=None, extra=None, set_stage=None, **more):
    """Group means over the three diagram sets, the EEG sets alone in run_features_step: set_stage(ws, ctx, audio), by
    default _set_means_stage with the engine's `launcher` and the further keywords extra(ws)."""
    if set_stage is None:
        def set_stage(ws, ctx, audio):
            _set_means_stage(ws, ctx, audio, functools.partial(launcher, **extra(ws)), getattr(ws, name + "_sets"))
    return OutputSpec(name, keyword, doc, validate, (stage_name,),
                      lambda ws, ctx, stage, inputs: stage(stage_name, lambda: set_stage(ws, ctx, audio=True)),
                      set_stage=set_stage, **more)


def _landscapes(value):
    grid, levels = value
    grid = np.ascontiguousarray(grid, dtype=np.float64)
    if grid.ndim != 1 or not 1 <= grid.shape[0] <= _lib.MAX_GRID or not 1 <= int(levels) <= _lib.MAX_LANDSCAPES:
        raise ValueError(f"landscapes=(grid, levels): a 1-D grid of 1..{_lib.MAX_GRID} points and 1..{_lib.MAX_LANDSCAPES} levels")
    return (LAND_SETS, int(levels) + 1, grid.shape[0]), (grid, int(levels))


def _images(value):
    xe, ye, sigma, power = engine.image_args(*value)
    return (IMG_SETS, ye.shape[0] - 1, xe.shape[0] - 1), (xe, ye, sigma, power)


def _frechet(value):
    try:
        cap, max_iter = value
        cap, max_iter = engine.frechet_args(cap, max_iter)
        if cap > _lib.FM_MAX_POINTS:
            raise ValueError
    except (TypeError, ValueError, _lib.TdaError):
        raise ValueError(f"frechet=(cap, max_iter): integers, 1 <= cap <= {_lib.FM_MAX_POINTS}, "
                         f"1 <= max_iter <= {_lib.FM_MAX_ITER}") from None
    return (FM_SETS, cap + 2, 2), (cap, max_iter)


def _engine_checked(check, message, shape, params, catch=_lib.TdaError):
    """validate through an argument check of the engine: what it raises of `catch` becomes ValueError(message)."""
    def validate(value):
        try:
            check(value)
        except catch:
            raise ValueError(message) from None
        return shape, params(value)
    return validate


OUTPUTS = [
    OutputSpec("corr", "correlations", """\
      corr  correlations=True: (CORR_COLS,) Spearman [r, p] of the five feature series of engine.SPEARMAN_COLS, audio H1
            against EEG H1 (cmp:104-114; engine.temporal_corr_dev)""",
               _switch(CORR_COLS), ("temporal_corr",),
               # over the windows that reach the distances (cmp:90-91,104-114)
               lambda ws, ctx, stage, inputs: stage("temporal_corr", lambda: engine.temporal_corr_dev(
                   ws.fa1, ws.fe1, ws.seg_off, ws.aud.status, cols=ws.corr_cols, out_t=ws.corr, ctx=ctx)), off=False,
               tables=dict(corr_cols=lambda ws: _dev(ws, np.array(engine.SPEARMAN_COLS, np.int32)))),
    _pair_distance("bott", "bottleneck", """\
      bott  bottleneck=True: (BOTT_COLS,) np.nanmean of the bottleneck distances of the H0 / H1 diagram pairs
            (engine.bottleneck_dev) over the windows the Wasserstein means of `result` run over -- a window whose audio
            cloud is degenerate or too large (cmp:90-91), or whose pair has a status, counts as NaN""",
                   _switch(BOTT_COLS), "b", "bottleneck", engine.bottleneck_dev, off=False),
    _set_means("land", "landscapes", """\
      land  landscapes=(grid, levels): (LAND_SETS, levels + 1, n_grid) mean persistence landscape (levels 1..levels) and
            mean Betti curve (last row) on the float64 grid, of the EEG H0, the EEG H1 and the audio H1 diagrams
            (engine.landscape_mean_dev).  The EEG sets average every window of the group, as the feature aggregation does
            (v2:429-436); the audio set leaves out the windows whose cloud is degenerate or too large; a group without
            such a window is NaN.  ValueError unless the grid is 1-D with 1..MAX_GRID points and 1 <= levels <= MAX_LANDSCAPES""",
               _landscapes, "landscape", engine.landscape_mean_dev, lambda ws: dict(grid_t=ws.land_grid, levels=ws.land_levels),
               tables=dict(land_grid=lambda ws: _dev(ws, ws.landscapes[0]), land_levels=lambda ws: ws.landscapes[1])),
    _set_means("img", "images", """\
      img   images=(xe, ye, sigma, power): (IMG_SETS, n_y, n_x) mean persistence image of the same sets, windows and audio
            mask on the birth edges xe (n_x + 1) and persistence edges ye (n_y + 1) (engine.image_mean_dev; engine.image_args)""",
               _images, "image", engine.image_mean_dev,
               lambda ws: dict(xe_t=ws.img_xe, ye_t=ws.img_ye, sigma=ws.images[2], power=ws.images[3]),
               tables=dict(img_xe=lambda ws: _dev(ws, ws.images[0]), img_ye=lambda ws: _dev(ws, ws.images[1]))),
    _pair_distance("slc", "sliced", """\
      slc   sliced=dirs, (M, 2) finite directions, 1 <= M <= TDA_MAX_DIRECTIONS (engine._directions): (SLC_COLS,) np.nanmean
            of the sliced Wasserstein distances of the H0 / H1 pairs (engine.sliced_wasserstein_dev) under the rule of `bott`;
            the directions are uploaded once (`sliced_dirs`)""",
                   lambda value: ((SLC_COLS,), engine._directions(value)), "s", "sliced", engine.sliced_wasserstein_dev,
                   lambda ws: dict(dirs_t=ws.sliced_dirs), tables=dict(sliced_dirs=lambda ws: _dev(ws, ws.sliced))),
    _pair_distance("wq", "wasserstein_q", """\
      wq    wasserstein_q=(order, ground), order 1 or 2 and ground "l2" or "linf": (WQ_COLS,) np.nanmean of that Wasserstein
            distance of the H0 / H1 pairs (engine.wasserstein_q_dev) under the rule of `bott`.  ValueError for anything else""",
                   _engine_checked(lambda value: engine.wasserstein_q_args(*value),
                                   "wasserstein_q=(order, ground): order 1 or 2, ground 'l2' or 'linf'", (WQ_COLS,),
                                   lambda value: (int(value[0]), value[1]), catch=(TypeError, ValueError, _lib.TdaError)),
                   "q", "wasserstein_q", engine.wasserstein_q_dev,
                   lambda ws: dict(order=ws.wasserstein_q[0], ground=ws.wasserstein_q[1])),
    _set_means("fm", "frechet", """\
      fm    frechet=(cap, max_iter), 1 <= cap <= FM_MAX_POINTS and 1 <= max_iter <= FM_MAX_ITER: (FM_SETS, cap + 2, 2), per
            diagram set of `land` (same windows, same audio mask) the Frechet mean of the group's diagrams in the order-2
            Wasserstein metric (engine.frechet_mean_dev): rows 0..cap-1 the mean, NaN beyond its count; row cap
            [count, Frechet variance]; row cap + 1 [iterations, status word].  ValueError for anything else""",
               _frechet, "frechet", set_stage=_frechet_stage,
               # what the kernel writes for one diagram set, packed into the set's float64 block after its launch
               per_group=dict(fm_out=lambda ws: (_f64(ws, ws.n_seg, ws.frechet[0], 2), _i32(ws, ws.n_seg), _f64(ws, ws.n_seg),
                                                 _i32(ws, ws.n_seg), _i32(ws, ws.n_seg)))),
    _pair_distance("kd", "kernel_distance", """\
      kd    kernel_distance=("pss", sigma) or ("pwg", sigma, c) (engine.diagram_kernel_args): (KD_COLS,) np.nanmean of the
            distance that kernel on diagrams induces between the H0 / H1 pairs (engine.diagram_kernel_dev) under the rule of
            `bott`.  ValueError for anything else""",
                   _engine_checked(engine.diagram_kernel_args,
                                   "kernel_distance=('pss', sigma) or ('pwg', sigma, c): finite sigma, c > 0", (KD_COLS,),
                                   lambda value: (value[0],) + tuple(float(v) for v in value[1:])),
                   "k", "kernel_distance", engine.diagram_kernel_dev, lambda ws: dict(kernel=ws.kernel_distance)),
    _pair_distance("pf", "fisher", """\
      pf    fisher=sigma, a finite number > 0 (engine.fisher_args): (PF_COLS,) np.nanmean of the persistence Fisher distances
            of the H0 / H1 pairs (engine.persistence_fisher_dev) under the rule of `bott`.  ValueError for anything else""",
                   _engine_checked(engine.fisher_args, "fisher=sigma: a finite number > 0", (PF_COLS,), float),
                   "f", "fisher", engine.persistence_fisher_dev, lambda ws: dict(sigma=ws.fisher)),
    OutputSpec("sl", "sublevel", """\
      sl    sublevel=True: (SL_COLS,) from the sublevel-set (lower-star) H0 diagrams of the signals themselves
            (engine.sublevel_features_dev; include/tdaeeg.h).  Columns 0..10: np.nanmean over the group's windows of the 11
            extract_features values of the audio window's diagram.  Columns 11..21: np.nanmean over the windows of the
            np.mean over the channels of the same 11 values of the EEG channels' diagrams, one diagram per channel.  A
            signal with a sample that is not finite counts as NaN.  Every window of the group takes part: no Rips status
            is looked at.
            Workspace: per window the features it averages, `sl_fa` (n_win, 1, 11) of the audio window and `sl_fe`
            (n_win, n_ch, 11) of the EEG channels (NaN where `sl_sa` / `sl_se` flag the signal).  The diagrams exist only
            chunk by chunk, in scratch of at most sublevel_bytes of rows per signal kind (engine.SublevelScratch, made at
            the first step, when the window length is known)""",
               _switch(SL_COLS), ("sublevel",),
               lambda ws, ctx, stage, inputs: stage("sublevel", lambda: _sublevel_stage(ws, ctx, *inputs)), off=False,
               per_window=dict(sl_fa=lambda ws: _f64(ws, ws.n_win, 1, 11), sl_fe=lambda ws: _f64(ws, ws.n_win, ws.n_ch, 11),
                               sl_sa=lambda ws: _i32(ws, ws.n_win, 1), sl_se=lambda ws: _i32(ws, ws.n_win, ws.n_ch)),
               # the 22 per-window series, one contiguous row each; (n_ch, n_t) -> engine.SublevelScratch, shared by views
               tables=dict(sl_cols=lambda ws: _f64(ws, SL_COLS * ws.n_win), sl_scratch=lambda ws: {},
                           sl_n_win=lambda ws: ws.n_win)),
    OutputSpec("pl", "phase_locking", """\
      pl    phase_locking=method, one of "euclidean", "abs", "standard", "sqrt" (True: "euclidean"; the parameter kept is
            the method number): (PL_COLS,) from the Rips diagrams of the phase-locking distance of the EEG window's channels
            (engine.plv_dist_dev -> rips_dm_dev; include/tdaeeg.h, "Phase-locking value").  Columns 0..10: np.nanmean over
            the group's windows of the 11 extract_features values of H0; columns 11..21: the same for H1; every window of
            the group takes part, as for the EEG sets.  Columns 22, 23: np.nanmean of the reference's Wasserstein distance
            (engine.wasserstein_dev) between that diagram and the audio diagram of the same window, H0 and H1, under the
            rule of `bott`.  A window with a PLV or Rips status counts as NaN.  ValueError for anything else.
            Workspace: per window what it averages: `pl_f0` / `pl_f1` (n_win, 11), the features of the H0 / H1 diagram
            `pl_dgm` (an engine.DeviceDiagrams) of the phase-locking distance matrix `pl_dist` (n_win, n_ch, n_ch), `pl_w0` /
            `pl_w1` (n_win), its Wasserstein distances to the audio diagram, with the status words `pl_st` (the PLV
            kernel's), `pl_dgm.status` (Rips) and `pl_ws0` / `pl_ws1` (the distances').  A window flagged by the PLV kernel is
            handed to Rips as points on a line (`pl_line`), its NaN block in `pl_dist` replaced, and counts as NaN""",
               lambda value: None if value is False else ((PL_COLS,), engine.plv_method(value)), ("phase_locking",),
               lambda ws, ctx, stage, inputs: stage("phase_locking",
                                                    lambda: _phase_locking_stage(ws, ctx, inputs[0], inputs[2], inputs[3])),
               arg=lambda method: engine.METHOD_NAMES[method],
               per_window=dict(pl_dist=lambda ws: _f64(ws, ws.n_win, ws.n_ch, ws.n_ch), pl_st=lambda ws: _i32(ws, ws.n_win),
                               pl_dgm=lambda ws: engine.DeviceDiagrams(ws.n_win, ws.n_ch, ws.eeg.h1_cap, ws.device),
                               pl_f0=lambda ws: _f64(ws, ws.n_win, 11), pl_f1=lambda ws: _f64(ws, ws.n_win, 11),
                               pl_w0=lambda ws: _f64(ws, ws.n_win), pl_w1=lambda ws: _f64(ws, ws.n_win),
                               pl_ws0=lambda ws: _i32(ws, ws.n_win), pl_ws1=lambda ws: _i32(ws, ws.n_win)),
               # pl_cols: the 24 per-window series, one contiguous row each; pl_line: |j - k| / n_ch, points on a line
               tables=dict(pl_cols=lambda ws: _f64(ws, PL_COLS * ws.n_win),
                           pl_line=lambda ws: _dev(ws, np.abs(np.subtract.outer(np.arange(ws.n_ch), np.arange(ws.n_ch))) / ws.n_ch))),
]
OUTPUT_BY_NAME = {spec.name: spec for spec in OUTPUTS}
# The launches of a step do not come in the table's order but in this one, the outputs that are on; None stands for the
# two Wasserstein stages of `result`.  Captured graphs and the stage timers depend on it
LAUNCH_ORDER = ("corr", "land", "img", None, "bott", "slc", "wq", "kd", "pf", "fm", "sl", "pl")
# (kept for its readers: the per-window buffers of the pair distances, in the order in which the distances were added)
Workspace.PAIR_BUFFERS = tuple(a for name in ("bott", "slc", "wq", "pf", "kd") for a in OUTPUT_BY_NAME[name].per_window)
for _spec in OUTPUTS:                                       # everything an output owns is None while it is off
    for _attr in (_spec.name, _spec.name + "_sets", *_spec.per_window, *_spec.per_group, *_spec.tables):
        setattr(Workspace, _attr, None)
    setattr(Workspace, _spec.keyword, _spec.off)


def step_outputs(*args, **kw):
    given = _KEYWORDS.bind(*args, **kw).arguments           # TypeError for an unknown keyword
    out = []
    for spec in OUTPUTS:
        value = given.get(spec.keyword)
        checked = None if value is None else spec.validate(value)
        if checked is not None:
            out.append(Output(spec.name, *checked))
    return out


step_outputs.__signature__ = _KEYWORDS = inspect.Signature(
    [inspect.Parameter(spec.keyword, inspect.Parameter.POSITIONAL_OR_KEYWORD, default=spec.off) for spec in OUTPUTS])
step_outputs.__doc__ = """The optional per-group outputs of a step: one Output(name, shape of a group's block, validated
    params) per enabled one, in the fixed order of OUTPUTS (%s), which is also the order of the positional arguments.
    numpy only.  Workspace, the shard driver and the passes of recordings.py size, slice, scatter and copy every optional
    output from this table; `result` is the same either way.
%s""" % (", ".join(OUTPUT_BY_NAME), "\n".join(s.doc for s in OUTPUTS))


class Batch:
    """Handle of a submitted batch: `result()` waits for it, repairs it if a window ran out of class bits, runs the
    `post` callback and returns its value (or the lane's result rows, valid until the lane is used again)."""

    def __init__(self, lanes, lane, inputs, post, event):
        self.lanes, self.lane, self.inputs, self.post, self.event = lanes, lane, inputs, post, event
        self.done, self.value, self.repaired = False, None, False

    def result(self):
        if not self.done:
            self.lanes._finalize(self.lane)
        return self.value


class Lanes:
    """`depth` independent (Workspace, stream pair) lanes.  Consecutive batches (recording-bands are
    independent, cmp:77-122 runs them one after the other) go to alternating lanes, so that the
    thin tail of one batch's grids -- 710 workgroups on 256 CUs is 1.4 rounds of the audio Rips
    kernel -- is filled by the head of the next batch instead of leaving CUs idle.  Every lane owns
    its buffers.

    graph=True: the launches of a step are captured once per (lane, input buffers) into a HIP graph
    and replayed afterwards, which takes the per-step host work from ~0.35 ms to ~0.06 ms.  Inputs are
    baked in by address, so feed the lanes from a fixed ring of device buffers.

    defer_retries=True: a step launches only the first pass of the two Rips stages.  Their widening
    passes redo just the windows that ran out of class bits -- rarely any -- but each is a launch
    that needs a large share of a CU before it can even look, and on a full GPU that stalls the lane
    (5-6 % of the throughput).  Instead the overflow bits of the batch travel to pinned host memory
    with the step; when the lane comes up again (`depth` batches later, so the wait is normally
    over) they are inspected, the batch is re-run with the full ladder if any is set, and only then
    is it published through `post` / `Batch.result()` (verify, then publish)."""

    def __init__(self, depth, n_win, seg_off, device, graph=False, defer_retries=True, **kw):
        import torch
        self.depth = max(1, int(depth))
        self.ws = [Workspace(n_win, seg_off, device, **kw) for _ in range(self.depth)]
        self.streams = [torch.cuda.Stream(device=device) for _ in range(self.depth)]
        self.k = 0
        self.graph = bool(graph)
        self.defer = defer_retries if defer_retries == "one" else bool(defer_retries)
        self.graphs = {}
        self.pending = [None] * self.depth
        self.repairs = 0
        self.before_step = None      # optional callable(lane index): runs before a step is launched or captured

    def _finalize(self, i):
        import torch
        b = self.pending[i]
        if b is None:
            return
        self.pending[i] = None
        st, ws = self.streams[i], self.ws[i]
        b.event.synchronize()
        eeg_win, audio_win, ctx, max_lag = b.inputs
        with torch.cuda.stream(st):
            if self.defer and bool(ws.flags_host.any()):
                if bool((ws.flags_host & 2).any()):                        # class overflow left by the short ladder: rare
                    run_step(eeg_win, audio_win, ws, ctx=ctx, max_lag=max_lag, retry="auto")
                    b.repaired = True
                    self.repairs += 1
                    ws.flags_host.copy_(ws.seg_flags, non_blocking=True)
                    st.synchronize()
                # verify before publishing: the full ladder ends in a pass without a capacity limit, so no overflow can be
                # left; a truncated H1 diagram (h1_cap), an oversized cloud or a kernel that gave up are not repairable
                # here -- the rows are not what the reference would give and must not go out
                if bool(ws.flags_host.any()):
                    from ._lib import TdaError
                    bits = int(np.bitwise_or.reduce(ws.flags_host.numpy()))
                    raise TdaError(f"window status bits {bits:#x} left in {int((ws.flags_host != 0).sum())} recording-band "
                                   "group(s) (1: H1 rows truncated, 2: class overflow, 8: not converged, 16: too many points): "
                                   "rows withheld")
            b.value = b.post(ws.result) if b.post is not None else ws.result
        b.done = True

    def submit(self, eeg_win, audio_win, ctx=None, max_lag=125, timers=None, post=None, sync_inputs=True, lane=None):
        """Enqueue one step on the next lane and return its Batch handle.  The batch that used the lane before
        is finalized first (see class docstring).  `post(result)` runs on the lane's stream when the batch is
        finalized (e.g. the all-gather of the result rows).  `timers` forces an eager (uncaptured) step.
        sync_inputs=False skips the wait on the caller's stream (inputs already complete in HBM)."""
        import torch
        i = self.k % self.depth if lane is None else int(lane) % self.depth      # lane=: a fixed batch -> lane map
        self.k += 1                                                              # (one captured graph per batch)
        self._finalize(i)
        st, ws = self.streams[i], self.ws[i]
        if sync_inputs:                                      # inputs produced on the caller's stream; pass False when
            st.wait_stream(torch.cuda.current_stream())     # they are resident and unchanged (costs ~0.07 ms per step)
        retry = ("one" if self.defer == "one" else "first") if self.defer else "auto"
        key = (i, eeg_win.data_ptr(), audio_win.data_ptr(), int(max_lag), id(ctx))
        if self.graph and timers is None:
            g = self.graphs.get(key)
            if g is None:
                if self.before_step is not None:
                    self.before_step(i)
                with torch.cuda.stream(st):                  # eager once: lazy initialisations stay out of the capture
                    run_step(eeg_win, audio_win, ws, ctx=ctx, max_lag=max_lag, retry=retry)
                st.synchronize()
                if self.before_step is not None:
                    self.before_step(i)
                g = torch.cuda.CUDAGraph()
                # thread_local: calls made by other threads meanwhile (e.g. the event queries of the RCCL watchdog
                # at N > 1) must not invalidate the capture
                with torch.cuda.graph(g, stream=st, capture_error_mode="thread_local"):
                    run_step(eeg_win, audio_win, ws, ctx=ctx, max_lag=max_lag, retry=retry)
                self.graphs[key] = g
            with torch.cuda.stream(st):
                g.replay()
        else:
            if self.before_step is not None:
                self.before_step(i)
            with torch.cuda.stream(st):
                run_step(eeg_win, audio_win, ws, ctx=ctx, max_lag=max_lag, timers=timers, retry=retry)
        ev = torch.cuda.Event()
        ev.record(st)
        b = Batch(self, i, (eeg_win, audio_win, ctx, max_lag), post, ev)
        self.pending[i] = b
        return b

    def drain(self):
        """Finalize every batch still in flight and make the caller's stream wait for the lanes."""
        import torch
        for i in range(self.depth):
            self._finalize(i)
        cur = torch.cuda.current_stream()
        for st in self.streams:
            cur.wait_stream(st)


class CorpusPass:
    """One rank's share of a corpus-shaped pass: the loops of run_analysis / process_recording
    (scripts/tda_eeg_audio_comparison.py:131-138, 63-122) turned inside out.  The rank's recordings are
    resident in HBM as ONE batch per band -- eeg[b]: (n_rec * wpr, 47, 250), aud[b]: (n_rec * wpr, 250),
    window (r * wpr + w) = the w-th selected window of local recording r -- and a pass is one `run_step` per band,
    fed through `Lanes` (band b always on lane b % depth, so each band's launches are captured once).  The
    (n_rec, n_bands, 48) block of result rows is all-gathered ONCE per pass (dist.all_gather_rows: RCCL over xGMI
    on the GPU box), which replaces the reference's serial loop over recordings and the partial-file merge of
    scripts/tda_eeg_classification_v2.py:608-638."""

    def __init__(self, eeg, aud, wpr, device, ctx, depth=3, graph=True, my_recs=None, shards=None, n_total=None,
                 gather=True, seg_off=None, merge_bands=False, **lane_kw):
        """merge_bands: all bands of the rank's share as ONE batch per pass (band-major groups) instead of one batch
        per band -- five times the windows per launch, which matters when the share is small (a rank of eight holds
        2,655 windows per band: 5.2 rounds of the audio kernel)."""
        import torch
        self.ctx = ctx
        self.n_bands = len(eeg)
        n_win = eeg[0].shape[0]
        assert all(e.shape[0] == n_win for e in eeg) and all(a.shape[0] == n_win for a in aud)
        if seg_off is None:                       # wpr selected windows per recording-band
            assert n_win % wpr == 0
            seg_off = np.arange(0, n_win + 1, wpr, dtype=np.int32)
        seg_off = np.asarray(seg_off, np.int32)
        self.n_rec = len(seg_off) - 1
        if merge_bands and self.n_bands > 1:
            base = getattr(eeg[0], "_base", None)
            step_b = eeg[0].numel() * eeg[0].element_size()
            if base is not None and base.is_contiguous() and all(e.is_contiguous() and e.data_ptr() == eeg[0].data_ptr() + b * step_b
                                                                   for b, e in enumerate(eeg)) \
                    and base.numel() == self.n_bands * eeg[0].numel() and base.data_ptr() == eeg[0].data_ptr():
                eeg_all = base.view(self.n_bands * n_win, *eeg[0].shape[1:])          # the bands already lie back to back
            else:
                eeg_all = torch.cat(list(eeg))
            aud_all = torch.cat(list(aud))
            seg_all = np.concatenate([[0]] + [seg_off[1:] + b * n_win for b in range(self.n_bands)]).astype(np.int32)
            self.batches = [(eeg_all, aud_all, list(range(self.n_bands)))]
            seg_off, n_win = seg_all, self.n_bands * n_win
        else:
            self.batches = [(eeg[b], aud[b], [b]) for b in range(self.n_bands)]
        self.eeg, self.aud = [b[0] for b in self.batches], [b[1] for b in self.batches]
        self.n_win = n_win                        # windows per batch (= per launch of every stage)
        # big batches: ONE widening pass rides along with every Rips call (a few windows in ten thousand need it, and
        # it fits beside the other kernels); the wide rungs of the ladder, which would wait for a nearly empty CU
        # even with nothing to redo, run only for a batch whose flags are still set when it is verified
        lane_kw.setdefault("defer_retries", "one")
        self.lanes = Lanes(depth, n_win, seg_off, device, graph=graph, **lane_kw)
        self.blocks = [torch.empty((self.n_rec, self.n_bands, RESULT_COLS), dtype=torch.float64, device=device)
                       for _ in range(3)]
        self.my_recs, self.shards, self.n_total = my_recs, shards, n_total
        self.gather = gather and shards is not None and len(shards) > 1
        self.passes = 0
        self.gathered = None
        self._open = {}
        self._gather_events = []

    def _post(self, k, i, result):
        """Runs on the lane's stream when batch i of pass k has been verified: its rows join the pass' block; the
        last batch to arrive (any order) all-gathers the block."""
        import torch
        blk = self.blocks[k % len(self.blocks)]
        bands = self.batches[i][2]
        if len(bands) == 1:
            blk[:, bands[0]].copy_(result)
        else:                                     # groups are band-major: (band, recording) -> (recording, band)
            blk.copy_(result.view(len(bands), self.n_rec, RESULT_COLS).transpose(0, 1))
        st = self._open.setdefault(k, {"left": len(self.batches), "events": []})
        ev = torch.cuda.Event()
        ev.record()
        st["events"].append(ev)
        st["left"] -= 1
        if st["left"] == 0:
            cur = torch.cuda.current_stream()
            for e in st["events"]:
                cur.wait_event(e)
            del self._open[k]
            flat = blk.view(self.n_rec, self.n_bands * RESULT_COLS)
            if self.gather:
                from . import dist as tdist
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                self.gathered = tdist.all_gather_rows(flat, self.my_recs, self.shards, self.n_total)
                e1.record()
                self._gather_events = (self._gather_events + [(e0, e1)])[-16:]
            else:
                self.gathered = flat.clone() if len(self.batches) == 1 else flat
        return None

    def step(self, timers=None):
        """Enqueue one pass (one batch per band, or one in all).  timers: optional {batch index: stage-event dict} --
        those batches are launched eagerly with per-stage events (see run_step)."""
        import functools
        k = self.passes
        self.passes += 1
        for i, (e, a, _) in enumerate(self.batches):
            # one batch per pass: passes alternate over the lanes; otherwise batch i always on lane i mod depth
            lane = (k if len(self.batches) == 1 else i)
            self.lanes.submit(e, a, ctx=self.ctx, post=functools.partial(self._post, k, i), sync_inputs=False,
                              lane=lane, timers=(timers or {}).get(i))

    def prime(self):
        """Untimed set-up: every lane launches its step once eagerly and captures it, so that no later pass pays for
        a capture (with one batch per pass the lanes take turns, and the first `depth` passes would each capture)."""
        for _ in range(self.lanes.depth if len(self.batches) == 1 else 1):
            self.step()
        return self.finish()

    def allgather_ms(self):
        """Mean duration of the all-gather of a pass (events on the lane's stream), None on one rank."""
        import torch
        if not self._gather_events:
            return None
        torch.cuda.synchronize()
        return round(float(np.mean([a.elapsed_time(b) for a, b in self._gather_events])), 4)

    def finish(self):
        """Verify and publish everything in flight; returns the rows of the last pass:
        (n_total or n_rec, n_bands * 48), recordings in the reference's order."""
        self.lanes.drain()
        return self.gathered


def run_features_step(eeg_win, ws, ctx=None):
    """The EEG half alone, as process_file_features needs it (scripts/tda_eeg_classification_v2.py:404-436,
    BASELINE.json configs[2]): corr->dist -> Rips -> 11 features of H0 and of H1 -> mean/std over the windows of
    every (recording, band) group.  Returns ws.feat44 (n_seg, 44)."""
    import torch
    ctx = ctx or _lib.get_ctx()
    with ctx.deferred():
        if ws.fused and eeg_win.shape[2] <= 256:
            engine.eeg_window_dev(eeg_win, ws.eeg, ctx=ctx)
        else:
            if ws.dist is None:
                ws.dist = torch.empty((ws.n_win, eeg_win.shape[1], eeg_win.shape[1]), dtype=torch.float64, device=ws.device)
            engine.corr_dist_dev(eeg_win, ws.dist, None, ctx=ctx)
            engine.rips_dm_dev(ws.dist, ws.eeg, ctx=ctx)
    engine.diagram_finish_dev([(ws.eeg.h0, ws.eeg.c0, False, ws.fe0), (ws.eeg.h1, ws.eeg.c1, True, ws.fe1)], ctx=ctx)
    on = {o.name for o in ws.outputs}
    for name in LAUNCH_ORDER:                            # the two EEG sets of the set means; the audio set is not touched
        if name in on and OUTPUT_BY_NAME[name].set_stage is not None:
            OUTPUT_BY_NAME[name].set_stage(ws, ctx, audio=False)
    if not hasattr(ws, "feat44"):
        ws.feat44 = torch.empty((ws.n_seg, 44), dtype=torch.float64, device=ws.device)
    engine.aggregate_dev(ws.fe0, ws.fe1, ws.seg_off, ws.feat44, ctx=ctx)
    return ws.feat44


STAGES = ["eeg_window", "corr_dist", "rips_eeg", "tau", "rips_audio", "finish", "wasserstein_h0", "wasserstein_h1", "reduce"]
# (every optional output adds the stages of its record of OUTPUTS, at its place in LAUNCH_ORDER)
