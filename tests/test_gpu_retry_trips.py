"""
The Rips retry passes with more flagged windows than workgroups.

Every first-pass Rips kernel takes one window per workgroup.  The widening passes and the last rung run on a small fixed
grid (RETRY_GRID, RETRY_GRID_WIDE, TOT_SLOTS in csrc/rips.hip) and every workgroup walks the list of the flagged windows:
entries b, b + grid, ... (RETRY_SCAN_BEGIN).  That loop is the only place where a workgroup meets the LDS (keys, vmax,
bucket cursors, class tables, the MFMA accumulator image, mean[] / sdev[], the stored / alive bit maps of the last rung)
and, for the last rung, the HBM slot of the class vectors that an earlier window of its own left behind.  Every test here
flags at least 2 * grid + 1 windows -- the grids are read from the #define lines, so a later change of a grid moves the
tests with it -- and so some workgroup makes three trips.

Method (that of test_gpu_parity.py::test_widening_passes_redo_exactly_the_flagged_windows): the diagrams of an ordinary
RETRY_AUTO call are the reference; a fresh, poisoned DeviceDiagrams gets TDA_WIN_CLASS_OVERFLOW by hand on every window
or on every second one; the rung under test is selected with set_class_words + RETRY_ONLY (or RETRY_LAST_RUNG) and called
twice with the retry counter armed.  Everything is compared exactly: there is no tolerance in this file.
"""
import os
import re

import numpy as np
import pytest

from oracle import brute, port
from tda_eeg_audio_amd import engine, synth

gpu = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
RIPS_HIP = os.path.join(os.path.dirname(HERE), "tda_eeg_audio_amd", "csrc", "rips.hip")
OVERFLOW = 2                  # TDA_WIN_CLASS_OVERFLOW (include/tdaeeg.h)
POISON = -7.25                # rows and matrices no pass may touch
PATTERNS = ["all", "every_second"]
WHITE_BATCHES = 16            # natural case: 8.9 % of white-noise windows have more than 64 classes alive at once (CPU
                              # oracle, 4,000 windows): 16 (2 grid + 1) windows give about 1.4 (2 grid + 1) flagged ones


def _grids():
    """RETRY_GRID, RETRY_GRID_WIDE, TOT_SLOTS as csrc/rips.hip defines them."""
    src = open(RIPS_HIP).read()
    out = []
    for name in ("RETRY_GRID", "RETRY_GRID_WIDE", "TOT_SLOTS"):
        m = re.search(r"^#define[ \t]+%s[ \t]+(\d+)\b" % name, src, re.M)
        assert m, f"#define {name} <number> not found in rips.hip"
        out.append(int(m.group(1)))
    return tuple(out)


def _three_trips(grid):
    """The smallest number of flagged windows with which a workgroup of `grid` makes three trips."""
    return 2 * grid + 1


def _flags(grid, pattern):
    """The windows of a call and which of them are flagged: 2 grid + 1 flagged ones in either pattern."""
    k = _three_trips(grid)
    if pattern == "all":
        return np.ones(k, bool)
    f = np.zeros(2 * k, bool)
    f[::2] = True
    return f


def _sample(f, k=12):
    """k of the flagged windows f (in list order up to the order of the wave-aggregated append): the first and the last
    one and a spread over the first, middle and last third, i.e. over the first, second and third trip."""
    n, q = len(f), k // 3
    pos = [np.linspace(a, b, q).astype(int) for a, b in ((0, n // 3 - 1), (n // 3, 2 * n // 3 - 1), (2 * n // 3, n - 1))]
    return f[np.unique(np.concatenate(pos))]


def test_retry_grids_are_named_and_every_case_makes_three_trips():
    g, gw, slots = _grids()
    assert g >= 1 and gw >= 1 and slots >= 1
    src = open(RIPS_HIP).read()
    exprs = re.findall(r"\bint rgrid\s*=([^;]*);", src)
    assert len(exprs) >= 1, exprs                       # the flavours' rungs hand their retry grid to launch_pass
    for e in exprs:
        assert "RETRY_GRID" in e and not re.search(r"\b(64|512)\b", e), e
    # the last rungs (matrices, fused EEG, clouds) are launched by launch_pass under PASS_LAST, whose grid is dim3(TOT_SLOTS)
    host = src[src.index("// host side"):]
    last = [s for s in host.split(";") if re.search(r"\w+_total_kernel\s*<", s)]
    assert len(last) >= 1
    for s in last:
        assert re.search(r"\blaunch_pass\(\s*ctx,\s*\w+_total_kernel<[^()]*>,\s*PASS_LAST,", s), s
    grids = [e for e in re.findall(r"\bdim3 grid\s*=([^;]*);", host) if "PASS_LAST" in e]
    assert len(grids) >= 1 and len(re.findall(r"\bhipLaunchKernelGGL\(kern, grid,", host)) >= 1
    for e in grids:
        assert re.match(r"\s*pass == PASS_LAST \? dim3\(TOT_SLOTS\) :", e), e
    for grid in (g, gw, slots):
        for pattern in PATTERNS:
            f = _flags(grid, pattern)
            assert int(f.sum()) >= 2 * grid + 1 and len(_sample(np.nonzero(f)[0])) >= 12
            pos = np.searchsorted(np.nonzero(f)[0], _sample(np.nonzero(f)[0]))
            assert (pos >= grid).any() and (pos >= 2 * grid).any()      # second and third trip are in the sample
    # the shared EEG batch serves both grids; the natural white-noise batch is sized from the measured rate
    assert 2 * _three_trips(max(g, gw)) >= len(_flags(gw, "every_second"))
    assert 0.075 * WHITE_BATCHES * _three_trips(g) > 2 * g             # (rate less three standard errors)


# ------------------------------------------------------------------ the common method
def _ref_of(d):
    """Reference diagrams of an ordinary call: (H0 lists, H1 lists, c0, c1); every status word must be 0."""
    import torch
    torch.cuda.synchronize()
    st = d.status.cpu().numpy()
    assert not st.any(), (np.nonzero(st)[0][:8], st[st != 0][:8])
    r0, r1 = d.to_lists()
    return r0, r1, d.c0.cpu().numpy(), d.c1.cpu().numpy()


def _redo(ctx, call, out, flagged, policy, words):
    """Poison `out`, flag the chosen windows by hand and run call(out) twice under `policy` with `words` class words for
    distance matrices (None: the default) and the retry counter armed.  Returns the counter after either call."""
    import torch
    dev = out.status.device
    out.status.zero_(); out.c0.fill_(-5); out.c1.fill_(-5); out.h0.fill_(POISON); out.h1.fill_(POISON)
    out.status[torch.from_numpy(np.nonzero(flagged)[0]).to(dev)] = OVERFLOW
    ctr = torch.zeros(4, dtype=torch.int64, device=dev)
    try:
        if words is not None:
            ctx.set_class_words(words, 1)
        ctx.set_retry_policy(policy)
        ctx.set_retry_counter(ctr.data_ptr())
        call(out)
        torch.cuda.synchronize()
        first = ctr.cpu().numpy().copy()
        call(out)                                       # the list is empty now
        torch.cuda.synchronize()
        second = ctr.cpu().numpy().copy()
    finally:
        ctx.set_retry_counter(None)
        ctx.set_retry_policy(ctx.RETRY_AUTO)
        ctx.set_class_words(2, 1)
    return first, second


def _check(out, ref, flagged, counters, slot, exact, tag):
    """Flagged windows: the reference's counts and rows (sorted multisets), every one of them.  The others: untouched.
    Counter `slot` (include/tdaeeg.h: 0 matrices, 1 clouds, 2 last rung): the flagged count after the first call -- and
    nothing anywhere else when `exact` -- and the same after the second.  Returns the host copies (h0, h1, c0, c1)."""
    r0, r1, rc0, rc1 = ref
    st, c0, c1 = out.status.cpu().numpy(), out.c0.cpu().numpy(), out.c1.cpu().numpy()
    h0, h1 = out.h0.cpu().numpy(), out.h1.cpu().numpy()
    f, u = np.nonzero(flagged)[0], ~flagged
    assert not st.any(), (tag, np.nonzero(st)[0][:8], st[st != 0][:8])
    assert np.array_equal(c0[f], rc0[f]) and np.array_equal(c1[f], rc1[f]), tag
    for w in f:
        assert np.array_equal(brute.sort_rows(h0[w, :c0[w]]), brute.sort_rows(r0[w])), (tag, "H0", int(w))
        assert np.array_equal(brute.sort_rows(h1[w, :c1[w]]), brute.sort_rows(r1[w])), (tag, "H1", int(w))
    assert (c0[u] == -5).all() and (c1[u] == -5).all(), tag
    assert (h0[u] == POISON).all() and (h1[u] == POISON).all(), tag
    first, second = counters
    if exact:
        want = [0, 0, 0, 0]
        want[slot] = len(f)
        assert first.tolist() == want, (tag, first)
    else:
        assert first[slot] >= len(f), (tag, first)
    assert np.array_equal(second, first), (tag, first, second)
    return h0, h1, c0, c1


def _equals_oracle(got, w, o, tag):
    h0, h1, c0, c1 = got
    assert np.array_equal(brute.sort_rows(h0[w, :c0[w]]), brute.sort_rows(o[0])), (tag, "H0 oracle", int(w))
    assert np.array_equal(brute.sort_rows(h1[w, :c1[w]]), brute.sort_rows(o[1])), (tag, "H1 oracle", int(w))


def _latent(rng, n_rec, n_s, n_ch=47):
    """EEG-like recordings (synth.eeg_windows' model: eight latent sources, a mixing matrix per recording)."""
    A = rng.standard_normal((n_rec, n_ch, 8))
    return A @ rng.standard_normal((n_rec, 8, n_s)) + 0.5 * rng.standard_normal((n_rec, n_ch, n_s))


# ------------------------------------------------------------------ shared inputs and their references (computed once)
@pytest.fixture(scope="module")
def eeg(ctx):
    """EEG-like windows for both flag patterns of the larger grid, their matrices and the diagrams of ordinary calls.  A
    window with a zero-variance channel and one with a duplicated channel in every run of 64 windows (even indices: both
    patterns flag them), so that whichever order the waves of the collection append in, some of them are met on a
    workgroup's second and third trip."""
    import torch
    dev = torch.device("cuda", ctx.device)
    g, gw, _ = _grids()
    n = 2 * _three_trips(max(g, gw))
    W = synth.eeg_windows(n, seed=17, windows_per_recording=15)
    W[6::64, 7] = 0.5                                   # zero-variance channel
    W[10::64, 12] = W[10::64, 3]                        # duplicated channel: zero-length edge
    wt = torch.from_numpy(W).to(dev)
    dist = torch.empty((n, 47, 47), dtype=torch.float64, device=dev)
    corr = torch.empty_like(dist)
    engine.corr_dist_dev(wt, dist, corr, ctx=ctx)
    return dict(W=W, wt=wt, dist=dist, corr=corr, dev=dev,
                ref_dm=_ref_of(engine.rips_dm_dev(dist, ctx=ctx)), ref_fused=_ref_of(engine.eeg_window_dev(wt, ctx=ctx)))


# ------------------------------------------------------------------ a. tda_rips_dm_batch_dev, n = 47
@gpu
@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("words", [1, 2, 4])
def test_dm_widening_rungs_three_trips(ctx, eeg, words, pattern):
    """rips_dm_kernel<1, 2 | 4 | 8, u64, RETRY>: 128 and 256 class bits on RETRY_GRID workgroups, 512 bits on
    RETRY_GRID_WIDE, as the first rung behind a first pass of `words` class words."""
    g, gw, _ = _grids()
    grid = gw if 2 * words >= 8 else g
    flagged = _flags(grid, pattern)
    n = len(flagged)
    assert int(flagged.sum()) >= 2 * grid + 1
    dm = eeg["dist"][:n]
    out = engine.DeviceDiagrams(n, 47, engine.DEFAULT_H1_CAP, eeg["dev"])
    counters = _redo(ctx, lambda o: engine.rips_dm_dev(dm, o, ctx=ctx), out, flagged, ctx.RETRY_ONLY, words)
    got = _check(out, eeg["ref_dm"], flagged, counters, 0, True, (words, pattern))
    for w in _sample(np.nonzero(flagged)[0]):
        _equals_oracle(got, w, port.rips_dm(port.corr_dist(eeg["W"][w])[1]), (words, pattern))


# ------------------------------------------------------------------ b. tda_rips_dm_batch_dev, n > 64
@gpu
@pytest.mark.parametrize("pattern", PATTERNS)
def test_dm_two_word_rung_three_trips(ctx, pattern):
    """rips_dm_kernel<2, 2, u64, RETRY> (n > 64: two vertex words) behind a first pass of one class word; matrices as in
    test_rips_dm_larger_n_two_word_path.  A window the 128 bits do not hold goes on to the last rung: counter >=."""
    import torch
    dev = torch.device("cuda", ctx.device)
    g, _, _ = _grids()
    flagged = _flags(g, pattern)
    n, pts = len(flagged), 70
    assert int(flagged.sum()) >= 2 * g + 1
    rng = np.random.default_rng(12)
    d = np.empty((n, pts, pts))
    for w in range(n):
        X = rng.standard_normal((pts, 3))
        d[w] = np.sqrt(((X[:, None] - X[None]) ** 2).sum(-1))
    dm = torch.from_numpy(d).to(dev)
    ref = _ref_of(engine.rips_dm_dev(dm, thresh=10.0, h1_cap=1024, ctx=ctx))
    out = engine.DeviceDiagrams(n, pts, 1024, dev)
    counters = _redo(ctx, lambda o: engine.rips_dm_dev(dm, o, thresh=10.0, ctx=ctx), out, flagged, ctx.RETRY_ONLY, 1)
    got = _check(out, ref, flagged, counters, 0, False, pattern)
    for w in _sample(np.nonzero(flagged)[0]):
        _equals_oracle(got, w, port.rips_dm(d[w], thresh=10.0), pattern)


# ------------------------------------------------------------------ c. fused kernel, stacked source
@gpu
@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("words", [0, 1, 2])
def test_fused_stacked_rungs_three_trips(ctx, eeg, words, pattern):
    """eeg_window_kernel<3, RES, 1 | 2 | 8, RETRY>: 64 and 128 class bits on RETRY_GRID workgroups, 512 bits on
    RETRY_GRID_WIDE, each as the first rung of launch_eeg_ladder; with the matrices written in the 128-bit case."""
    import torch
    g, gw, _ = _grids()
    grid = gw if words == 2 else g
    flagged = _flags(grid, pattern)
    n = len(flagged)
    assert int(flagged.sum()) >= 2 * grid + 1
    f = np.nonzero(flagged)[0]
    assert ((f % 64) == 6).sum() >= 2 and ((f % 64) == 10).sum() >= 2          # degenerate windows, in two waves' shares
    wt = eeg["wt"][:n]
    d2 = c2 = None
    if words == 1:
        d2 = torch.full((n, 47, 47), POISON, dtype=torch.float64, device=eeg["dev"])
        c2 = torch.full_like(d2, POISON)
    out = engine.DeviceDiagrams(n, 47, engine.DEFAULT_H1_CAP, eeg["dev"])
    counters = _redo(ctx, lambda o: engine.eeg_window_dev(wt, o, dist_t=d2, corr_t=c2, ctx=ctx), out, flagged,
                     ctx.RETRY_ONLY, words)
    got = _check(out, eeg["ref_fused"], flagged, counters, 0, True, (words, pattern))
    if d2 is not None:
        ft, ut = torch.from_numpy(f).to(eeg["dev"]), torch.from_numpy(np.nonzero(~flagged)[0]).to(eeg["dev"])
        assert torch.equal(d2[ft], eeg["dist"][ft]) and torch.equal(c2[ft], eeg["corr"][ft])
        assert bool((d2[ut] == POISON).all()) and bool((c2[ut] == POISON).all())
    for w in _sample(f):
        _equals_oracle(got, w, port.rips_dm(port.corr_dist(eeg["W"][w])[1]), (words, pattern))


# ------------------------------------------------------------------ d. fused kernel, sliding source with a selection
@gpu
@pytest.mark.parametrize("pattern", PATTERNS)
def test_fused_sliding_selection_three_trips(ctx, pattern):
    """WindowSource::at with a shuffled selection inside the loop over the list: windows read in place from recordings of
    1,200 samples, the 128-bit rung."""
    import torch
    dev = torch.device("cuda", ctx.device)
    g, _, _ = _grids()
    flagged = _flags(g, pattern)
    n, n_s = len(flagged), 1200
    assert int(flagged.sum()) >= 2 * g + 1
    per_rec = (n_s - 250) // 62 + 1
    n_rec = -(-n // per_rec)
    rng = np.random.default_rng(41)
    sig = _latent(rng, n_rec, n_s)
    sel = rng.permutation(n_rec * per_rec)[:n].astype(np.int32)
    sig_t, sel_t = torch.from_numpy(sig).to(dev), torch.from_numpy(sel).to(dev)
    ref = _ref_of(engine.eeg_window_sliding_dev(sig_t, 250, 62, sel_t=sel_t, ctx=ctx)[0])
    out = engine.DeviceDiagrams(n, 47, engine.DEFAULT_H1_CAP, dev)
    counters = _redo(ctx, lambda o: engine.eeg_window_sliding_dev(sig_t, 250, 62, sel_t=sel_t, out=o, ctx=ctx), out, flagged,
                     ctx.RETRY_ONLY, 1)
    got = _check(out, ref, flagged, counters, 0, True, pattern)
    for w in _sample(np.nonzero(flagged)[0]):
        r, k = divmod(int(sel[w]), per_rec)
        _equals_oracle(got, w, port.rips_dm(port.corr_dist(sig[r][:, 62 * k:62 * k + 250])[1]), pattern)


# ------------------------------------------------------------------ e. fused kernel, ragged source
@gpu
@pytest.mark.parametrize("pattern", PATTERNS)
def test_fused_ragged_three_trips(ctx, pattern):
    """RaggedWindowSource inside the loop: six recordings of three lengths, dealt window by window, so that the row stride
    changes from one trip of a workgroup to the next; every window starts at an odd element offset; the 128-bit rung."""
    import torch
    dev = torch.device("cuda", ctx.device)
    g, _, _ = _grids()
    flagged = _flags(g, pattern)
    n = len(flagged)
    assert int(flagged.sum()) >= 2 * g + 1
    lengths = [1201, 1334, 1507] * 2
    assert g % len(lengths) % 3 != 0 and 2 * g % len(lengths) % 3 != 0    # b, b + grid, b + 2 grid: three row strides
    rng = np.random.default_rng(43)
    recs = [_latent(rng, 1, L)[0] for L in lengths]
    off = 47 * np.concatenate([[0], np.cumsum(lengths)])
    rec = np.arange(n) % len(lengths)
    first = np.array([2 * (w // len(lengths)) + 1 - off[rec[w]] % 2 for w in range(n)])     # start within the recording
    assert all(first[w] + 250 <= lengths[rec[w]] for w in range(n))
    start = off[rec] + first
    assert (start % 2 == 1).all()
    sig_t = torch.from_numpy(np.concatenate([r.ravel() for r in recs])).to(dev)
    start_t = torch.from_numpy(start.astype(np.int64)).to(dev)
    ld_t = torch.from_numpy(np.array(lengths, np.int64)[rec]).to(dev)
    ref = _ref_of(engine.eeg_window_ragged_dev(sig_t, start_t, ld_t, 250, ctx=ctx))
    out = engine.DeviceDiagrams(n, 47, engine.DEFAULT_H1_CAP, dev)
    counters = _redo(ctx, lambda o: engine.eeg_window_ragged_dev(sig_t, start_t, ld_t, 250, out=o, ctx=ctx), out, flagged,
                     ctx.RETRY_ONLY, 1)
    got = _check(out, ref, flagged, counters, 0, True, pattern)
    for w in _sample(np.nonzero(flagged)[0]):
        win = recs[rec[w]][:, first[w]:first[w] + 250]
        _equals_oracle(got, w, port.rips_dm(port.corr_dist(win)[1]), pattern)


# ------------------------------------------------------------------ f. last rung, distance matrices
@gpu
@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("kind", ["latent", "white", "ties"])
def test_last_rung_matrices_three_trips(ctx, kind, pattern):
    """rips_dm_total_kernel: TOT_SLOTS workgroups, each with one HBM slot for the class vectors and the stored / alive bit
    maps in LDS, on 2 TOT_SLOTS + 1 windows flagged by hand: EEG-like and white-noise 47 x 47 matrices, tie-heavy
    40 x 40 ones."""
    import torch
    dev = torch.device("cuda", ctx.device)
    _, _, slots = _grids()
    flagged = _flags(slots, pattern)
    n = len(flagged)
    assert int(flagged.sum()) >= 2 * slots + 1
    if kind == "ties":
        q = np.round(np.random.default_rng(5).random((n, 40, 40)) * 6) / 6
        d = (q + q.transpose(0, 2, 1)) / 2
        for i in range(n):
            np.fill_diagonal(d[i], 0.0)
    else:
        d = engine.corr_dist_batch(synth.eeg_windows(n, seed=9, kind=kind), want_corr=False, ctx=ctx)
    dm = torch.from_numpy(np.ascontiguousarray(d)).to(dev)
    ref = _ref_of(engine.rips_dm_dev(dm, h1_cap=1100, ctx=ctx))
    out = engine.DeviceDiagrams(n, d.shape[1], 1100, dev)
    counters = _redo(ctx, lambda o: engine.rips_dm_dev(dm, o, ctx=ctx), out, flagged, ctx.RETRY_LAST_RUNG, None)
    got = _check(out, ref, flagged, counters, 2, True, (kind, pattern))
    for w in _sample(np.nonzero(flagged)[0]):
        _equals_oracle(got, w, port.rips_dm(d[w]), (kind, pattern))


# ------------------------------------------------------------------ g. last rung, point clouds
@gpu
@pytest.mark.parametrize("pattern", PATTERNS)
def test_last_rung_clouds_three_trips(ctx, pattern):
    """rips_cloud_total_kernel on audio windows of two bands: the flagged windows alternate between gamma (tau = 2, 123
    points) and delta (tau = 24 ... 82, 43 ... 101 points) in runs of TOT_SLOTS, so the clouds a slot sees on its
    three trips differ in size.  (At most 64 flagged windows: one wave collects them, the list is in window order.)"""
    import torch
    dev = torch.device("cuda", ctx.device)
    _, _, slots = _grids()
    flagged = _flags(slots, pattern)
    n = len(flagged)
    f = np.nonzero(flagged)[0]
    assert len(f) >= 2 * slots + 1
    pools = [synth.audio_windows(n, "gamma", seed=31), synth.audio_windows(n, "delta", seed=32)]
    band = (np.searchsorted(f, np.arange(n)) // slots) % 2          # by position in the list
    aw = np.stack([pools[band[w]][w] for w in range(n)])
    wt = torch.from_numpy(aw).to(dev)
    tau_t = engine.tau_dev(wt, max_lag=125, ctx=ctx)
    ref_d = engine.takens_rips_dev(wt, tau_t, h1_cap=1024, ctx=ctx)
    ref = _ref_of(ref_d)
    pts = ref_d.n_points.cpu().numpy()
    for b in range(slots):
        mine = pts[f[b::slots]]
        assert len(mine) >= 2 and len(set(mine.tolist())) >= 2, (b, mine)       # the slot's clouds differ in size
    out = engine.DeviceDiagrams(n, 128, 1024, dev)
    counters = _redo(ctx, lambda o: engine.takens_rips_dev(wt, tau_t, o, ctx=ctx), out, flagged, ctx.RETRY_LAST_RUNG, None)
    got = _check(out, ref, flagged, counters, 2, True, pattern)
    tau = tau_t.cpu().numpy()
    for w in _sample(f):
        (o, _) = port.audio_persistence(aw[w], int(tau[w]))
        _equals_oracle(got, w, o, pattern)


# ------------------------------------------------------------------ g2. last rung, fused EEG kernel
@gpu
@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("source", ["stacked", "sliding", "table"])
def test_last_rung_fused_three_trips(ctx, source, pattern):
    """eeg_window_total_kernel behind each window source: TOT_SLOTS workgroups recompute 2 TOT_SLOTS + 1 windows flagged by
    hand from the samples (48 channels, white noise and EEG-like in turn), each with the MFMA accumulator image, the
    keys and the bit maps of the last rung in the LDS that its earlier window left behind; the matrices are written for
    the flagged windows only."""
    import torch
    dev = torch.device("cuda", ctx.device)
    _, _, slots = _grids()
    flagged = _flags(slots, pattern)
    n = len(flagged)
    f = np.nonzero(flagged)[0]
    assert len(f) >= 2 * slots + 1
    m = n + (n & 1)                                                 # recordings of two windows each
    W = synth.eeg_windows(m, seed=21, n_ch=48, kind="white")
    W[1::2] = synth.eeg_windows(m, seed=22, n_ch=48, windows_per_recording=5)[1::2]
    sig = np.ascontiguousarray(W.reshape(m // 2, 2, 48, 250).transpose(0, 2, 1, 3).reshape(m // 2, 48, 500))
    sig_t = torch.from_numpy(sig).to(dev)
    if source == "stacked":
        wt = torch.from_numpy(W[:n]).to(dev)
        call = lambda o, **kw: engine.eeg_window_dev(wt, o, ctx=ctx, **kw)
    elif source == "sliding":
        sel_t = torch.arange(n, dtype=torch.int32, device=dev)
        call = lambda o, **kw: engine.eeg_window_sliding_dev(sig_t, 250, 250, sel_t=sel_t, out=o, ctx=ctx, **kw)[0]
    else:
        w = np.arange(n)
        start_t = torch.from_numpy((48 * 500 * (w // 2) + 250 * (w % 2)).astype(np.int64)).to(dev)
        ld_t = torch.full((n,), 500, dtype=torch.int64, device=dev)
        call = lambda o, **kw: engine.eeg_window_ragged_dev(sig_t.reshape(-1), start_t, ld_t, 250, out=o, n_ch=48, ctx=ctx, **kw)
    oc, od = port.corr_dist_batch(W[:n])
    ref = _ref_of(call(engine.DeviceDiagrams(n, 48, engine.DEFAULT_H1_CAP, dev)))
    d2 = torch.full((n, 48, 48), POISON, dtype=torch.float64, device=dev)
    c2 = torch.full_like(d2, POISON)
    out = engine.DeviceDiagrams(n, 48, engine.DEFAULT_H1_CAP, dev)
    counters = _redo(ctx, lambda o: call(o, dist_t=d2, corr_t=c2), out, flagged, ctx.RETRY_LAST_RUNG, None)
    got = _check(out, ref, flagged, counters, 2, True, (source, pattern))
    d2, c2 = d2.cpu().numpy(), c2.cpu().numpy()
    assert np.array_equal(d2[f], od[f]) and np.array_equal(c2[f], oc[f])
    assert (d2[~flagged] == POISON).all() and (c2[~flagged] == POISON).all()
    for w in _sample(f):
        _equals_oracle(got, w, port.rips_dm(od[w]), (source, pattern))


# ------------------------------------------------------------------ h. the rungs reached because the windows need them
def _natural(ctx, wt, words, h1_cap, grid, exact):
    """The fused kernel under plain RETRY_AUTO behind a first pass of `words` class words, against the two-kernel path row
    for row.  Returns (diagrams, indices of the windows the first pass flags, counter)."""
    import torch
    dev = wt.device
    n = wt.shape[0]
    dist = engine.corr_dist_dev(wt, ctx=ctx)
    two = engine.rips_dm_dev(dist, h1_cap=h1_cap, ctx=ctx)
    ctr = torch.zeros(4, dtype=torch.int64, device=dev)
    try:
        ctx.set_class_words(words, 1)
        ctx.set_retry_policy(ctx.RETRY_FIRST_PASS)
        first = engine.eeg_window_dev(wt, h1_cap=h1_cap, ctx=ctx)
        torch.cuda.synchronize()
        need = torch.nonzero(first.status & OVERFLOW).flatten().cpu().numpy()
        print(f"class words {words}: the first pass flags {len(need)} of {n} windows (grid {grid})")
        assert len(need) > 2 * grid, "the test needs a workgroup of the widening pass to make three trips"
        ctx.set_retry_policy(ctx.RETRY_AUTO)
        ctx.set_retry_counter(ctr.data_ptr())
        one = engine.eeg_window_dev(wt, h1_cap=h1_cap, ctx=ctx)
        torch.cuda.synchronize()
    finally:
        ctx.set_retry_counter(None)
        ctx.set_retry_policy(ctx.RETRY_AUTO)
        ctx.set_class_words(2, 1)
    ctr = ctr.cpu().numpy()
    assert int(one.status.max()) == 0 and int(two.status.max()) == 0
    assert torch.equal(one.c0, two.c0) and torch.equal(one.c1, two.c1)
    m0 = torch.arange(one.h0.shape[1], device=dev)[None, :] < two.c0[:, None]
    m1 = torch.arange(h1_cap, device=dev)[None, :] < two.c1[:, None]
    assert torch.equal(one.h0[m0], two.h0[m0]) and torch.equal(one.h1[m1], two.h1[m1])
    assert (ctr[0] == len(need) if exact else ctr[0] >= len(need)) and ctr[1] == 0, (ctr, len(need))
    return one, need, ctr


@gpu
def test_white_noise_takes_the_128_bit_rung_three_trips(ctx):
    """White-noise windows, 64 class bits in the first pass: the windows with more classes alive at once (about 9 %) are
    more than 2 RETRY_GRID, and eeg_window_kernel<3, RES, 2, RETRY> redoes them (the few it flags again go on to 512 bits:
    counter >=)."""
    import torch
    dev = torch.device("cuda", ctx.device)
    g, _, _ = _grids()
    n = WHITE_BATCHES * _three_trips(g)
    gen = torch.Generator(device=dev)
    gen.manual_seed(20261)
    wt = torch.randn((n, 47, 250), generator=gen, dtype=torch.float64, device=dev)
    one, need, _ = _natural(ctx, wt, 1, 512, g, False)
    idx = _sample(need)
    got = tuple(t[torch.from_numpy(idx).to(dev)].cpu().numpy() for t in (one.h0, one.h1, one.c0, one.c1))
    wins = wt[torch.from_numpy(idx).to(dev)].cpu().numpy()
    for i in range(len(idx)):
        _equals_oracle(got, i, port.rips_dm(port.corr_dist(wins[i])[1]), int(idx[i]))


@gpu
def test_bipartite_windows_take_the_512_bit_rung_three_trips(ctx):
    """2 RETRY_GRID_WIDE + 1 windows with 506 classes alive at once, 128 class bits in the first pass: every one needs
    eeg_window_kernel<3, RES, 8, RETRY>, the only rung behind that first pass (counter ==)."""
    import torch
    from test_gpu_parity import _bipartite_windows
    dev = torch.device("cuda", ctx.device)
    _, gw, _ = _grids()
    n = _three_trips(gw)
    W = _bipartite_windows(n, seed=7)
    one, need, _ = _natural(ctx, torch.from_numpy(W).to(dev), 2, 1024, gw, True)
    assert len(need) == n
    got = (one.h0.cpu().numpy(), one.h1.cpu().numpy(), one.c0.cpu().numpy(), one.c1.cpu().numpy())
    assert got[3].min() >= 400                          # hundreds of classes born before the first death
    for w in _sample(need):
        _equals_oracle(got, w, port.rips_dm(port.corr_dist(W[w])[1]), int(w))
