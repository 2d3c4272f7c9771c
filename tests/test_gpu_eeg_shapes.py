"""The EEG window kernels off the reference's 47 x 250 windows: cd_window_products
(csrc/corr_dist_dev.h) as corr_dist_kernel<NB 1..4, resident | streaming>, its sliding form, and the fused
eeg_window kernels (csrc/rips.hip; NB = 3, 33..48 channels, 2..256 samples) behind their three window sources, on the
seeded cases of tests/eeg_shape_cases.py.  The reference is the CPU oracle, bit for bit; tests/test_eeg_shapes_model.py
holds the oracle itself on the same cases.  The RES = true family of the fused kernel (TDA_EEG_RESIDENT=1) runs in a
child process: tests/eeg_resident_child.py."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import eeg_shape_cases as sc
from oracle import brute, port
from tda_eeg_audio_amd import engine
from tda_eeg_audio_amd._lib import TdaError, ptr

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def _same_multiset(a, b):
    return np.array_equal(brute.sort_rows(a), brute.sort_rows(b))


def _dev(ctx):
    import torch
    return torch.device("cuda", ctx.device)


_bytes_equal, _same_diagrams = sc.bytes_equal, sc.same_diagrams


def _two_kernels(ctx, wt, h1_cap=engine.DEFAULT_H1_CAP):
    """corr_dist_dev + rips_dm_dev: (dist, corr, diagrams)."""
    import torch
    dist = torch.empty((wt.shape[0], wt.shape[1], wt.shape[1]), dtype=torch.float64, device=wt.device)
    corr = torch.empty_like(dist)
    engine.corr_dist_dev(wt, dist, corr, ctx=ctx)
    return dist, corr, engine.rips_dm_dev(dist, h1_cap=h1_cap, ctx=ctx)


# ------------------------------------------------------------------ corr_dist_kernel<NB, RES>
@pytest.mark.parametrize("nb", (1, 2, 3, 4))
def test_corr_dist_kernel_every_block_count_resident_and_streaming(ctx, nb):
    """corr_dist_kernel<NB, true> (n_t <= 256) and <NB, false> at 15/16/17, 31/32/33, 47/48/49, 63/64 channels (and 1, 2)
    and at lengths beside every tile boundary (31/32/33, 255/256/257, 287/288/289) and double-trip boundary inside a tile
    (n_t mod 32 in 1..8, 9..16, 17..24, 25..32): dist and corr equal the oracle's bit for bit, and the matrices written
    without corr are the same bytes."""
    bad = []
    for n_ch in sc.channels_of_nb(nb):
        for n_t in sc.RES_LENGTHS + sc.STREAM_LENGTHS:
            W = sc.windows(n_ch, n_t)
            oc, od = sc.oracle_corr_dist(n_ch, n_t)
            corr, dist = engine.corr_dist_batch(W, ctx=ctx)
            only = engine.corr_dist_batch(W, want_corr=False, ctx=ctx)
            if not (np.array_equal(dist, od) and np.array_equal(corr, oc) and only.tobytes() == dist.tobytes()):
                bad.append((n_ch, n_t, int((dist != od).sum()), int((corr != oc).sum())))
            if n_ch == 1:
                assert dist.shape == (sc.N_WIN, 1, 1) and not dist.any()
    assert not bad, f"{len(bad)} shapes differ from the oracle (n_ch, n_t, dist entries, corr entries): {bad[:12]}"


@pytest.mark.parametrize("n_ch", sc.SLIDING_CH)
def test_corr_dist_sliding_other_lengths_steps_and_strides(ctx, n_ch):
    """Windows read in place from a recording: win_len 2, 33, 256 and 300 (streaming), step 1, 7 and larger than the window
    (the samples in the gaps are NaN then), an odd row stride, exactly one window, and no window at all -- the host and
    the device entry against the oracle on the stacked windows."""
    import torch
    bad = []
    for c, win_len, step, n_s in (k for k in sc.sliding_cases() if k[0] == n_ch):
        sig = sc.sliding_signal(1, n_ch, n_s, win_len, step, seed=win_len * 31 + step)[0]
        n_win = sc.n_windows(n_s, win_len, step)
        assert n_win in ((0,) if n_s < win_len else (1,) if n_s == win_len else (4, 5))
        corr, dist = engine.corr_dist_sliding(sig, win_len, step, want_corr=True, ctx=ctx)
        st = torch.from_numpy(np.ascontiguousarray(sig)).to(_dev(ctx))
        ct = torch.full((n_win, n_ch, n_ch), -7.0, dtype=torch.float64, device=st.device)
        dt = engine.corr_dist_sliding_dev(st, win_len, step, corr_t=ct, ctx=ctx)
        assert dist.shape == corr.shape == tuple(dt.shape) == (n_win, n_ch, n_ch)
        assert engine.corr_dist_sliding(sig, win_len, step, ctx=ctx).tobytes() == dist.tobytes()       # corr = NULL
        if n_win:
            oc, od = port.corr_dist_batch(sc.stack_of(sig[None], win_len, step))
            ok = np.array_equal(dist, od) and np.array_equal(corr, oc)
            ok = ok and np.array_equal(dt.cpu().numpy(), od) and np.array_equal(ct.cpu().numpy(), oc)
            if not ok:
                bad.append((win_len, step, n_s))
    assert not bad, f"(win_len, step, n_samples) that differ from the oracle: {bad}"


# ------------------------------------------------------------------ the fused kernel: stacked windows
@pytest.mark.parametrize("n_ch", sc.FUSED_CH)
def test_fused_kernel_every_resident_length(ctx, n_ch):
    """eeg_window_dev at 33 (one live row in the last block) .. 48 channels (no padded row) and 2 .. 256 samples -- short
    double trips, rank-deficient correlations (n_t < n_ch), three-valued distances (n_t = 2) -- with and without the
    matrices: rows, counts and status equal corr_dist_dev + rips_dm_dev, the matrices are the same bytes, and every window
    equals the oracle as a sorted multiset."""
    import torch
    bad = []
    for n_t in sc.RES_LENGTHS:
        W = sc.windows(n_ch, n_t)
        wt = sc.to_device(W, _dev(ctx))
        dist, corr, two = _two_kernels(ctx, wt)
        d2 = torch.full_like(dist, -7.0)
        c2 = torch.full_like(dist, -7.0)
        d3 = torch.full_like(dist, -7.0)
        one = engine.eeg_window_dev(wt, dist_t=d2, corr_t=c2, ctx=ctx)
        nocorr = engine.eeg_window_dev(wt, dist_t=d3, ctx=ctx)
        bare = engine.eeg_window_dev(wt, ctx=ctx)
        torch.cuda.synchronize()
        ok = _bytes_equal(d2, dist) and _bytes_equal(c2, corr) and _bytes_equal(d3, dist)
        ok = ok and np.array_equal(dist.cpu().numpy(), sc.oracle_corr_dist(n_ch, n_t)[1])
        ok = ok and int(two.status.max()) == 0 and all(_same_diagrams(g, two) for g in (one, nocorr, bare))
        e0, e1 = bare.to_lists()
        for w in range(sc.N_WIN):
            o = sc.oracle_diagrams(n_ch, n_t, w)
            ok = ok and _same_multiset(e0[w], o[0]) and _same_multiset(e1[w], o[1])
        if not ok:
            bad.append(n_t)
    assert not bad, f"n_ch {n_ch}: lengths at which the fused kernel differs: {bad}"


# ------------------------------------------------------------------ the fused kernel: windows read in place
FUSED_SLIDING = [(33, 9, 4), (47, 33, 40), (48, 256, 5), (40, 2, 3), (46, 65, 1), (34, 224, 230)]     # (n_ch, win_len, step)


def _sel_of(n, seed):
    """A window list that is shuffled, leaves some windows out and repeats two."""
    p = np.random.default_rng(seed).permutation(n)[:max(2, (2 * n) // 3)]
    return np.concatenate([p, p[:2]]).astype(np.int32)


@pytest.mark.parametrize("n_ch,win_len,step", FUSED_SLIDING)
def test_fused_kernel_sliding_source_and_selection(ctx, n_ch, win_len, step):
    """eeg_window_sliding_dev over three recordings at other win_len / step than 250 / 62 (NaN in the gaps where step >
    win_len), all windows and a shuffled selection with repeats and omissions: row for row what the stacked call gives."""
    import torch
    n_s = win_len + 3 * step
    n_s += 1 - (n_s & 1)
    sig = sc.sliding_signal(3, n_ch, n_s, win_len, step, seed=n_ch * 1000 + win_len)
    stack = sc.stack_of(sig, win_len, step)
    per = sc.n_windows(n_s, win_len, step)
    assert len(stack) == 3 * per and per >= 4 and np.isfinite(stack).all() and np.isnan(sig).any() == (step > win_len)
    dev = _dev(ctx)
    sig_t = torch.from_numpy(sig).to(dev)
    for sel in (None, _sel_of(3 * per, seed=win_len)):
        sub = stack if sel is None else stack[sel]
        sel_t = None if sel is None else torch.from_numpy(sel).to(dev)
        wt = torch.from_numpy(np.ascontiguousarray(sub)).to(dev)
        ref_d = torch.full((len(sub), n_ch, n_ch), -7.0, dtype=torch.float64, device=dev)
        ref_c = torch.full_like(ref_d, -7.0)
        ref = engine.eeg_window_dev(wt, dist_t=ref_d, corr_t=ref_c, ctx=ctx)
        d2, c2 = torch.full_like(ref_d, -7.0), torch.full_like(ref_d, -7.0)
        got, per_rec = engine.eeg_window_sliding_dev(sig_t, win_len, step, sel_t=sel_t, dist_t=d2, corr_t=c2, ctx=ctx)
        bare, _ = engine.eeg_window_sliding_dev(sig_t, win_len, step, sel_t=sel_t, ctx=ctx)
        torch.cuda.synchronize()
        assert per_rec == per
        assert int(ref.status.max()) == 0 and _same_diagrams(got, ref) and _same_diagrams(bare, ref)
        assert _bytes_equal(d2, ref_d) and _bytes_equal(c2, ref_c)
        od = port.corr_dist_batch(sub)[1]
        assert np.array_equal(d2.cpu().numpy(), od)
        e0, e1 = got.to_lists()
        for w in (0, len(sub) - 1):
            o = port.rips_dm(od[w])
            assert _same_multiset(e0[w], o[0]) and _same_multiset(e1[w], o[1])


@pytest.mark.parametrize("n_ch,win_len,step", [(33, 33, 7), (48, 250, 62), (48, 9, 11), (33, 256, 100)])
def test_fused_kernel_window_table(ctx, n_ch, win_len, step):
    """eeg_window_ragged_dev: three recordings of different (odd) lengths packed back to back, the table in shuffled order:
    row for row what the stacked call gives on the same windows."""
    import torch
    rng = np.random.default_rng(n_ch + win_len)
    lens = [win_len + 2 * step + 1, win_len + 5 * step + 3, win_len + 7]
    lens = [L + 1 - (L & 1) for L in lens]                                   # odd row strides
    assert len(set(lens)) == 3
    recs = [rng.standard_normal((n_ch, L)) + 0.4 * rng.standard_normal((1, L)) for L in lens]
    packed = np.concatenate([r.ravel() for r in recs])
    off = np.concatenate([[0], np.cumsum(lens)])
    table = [(r, k) for r, L in enumerate(lens) for k in range(sc.n_windows(L, win_len, step))]
    table = [table[i] for i in rng.permutation(len(table))]
    start = np.array([n_ch * off[r] + k * step for r, k in table], np.int64)
    ld = np.array([lens[r] for r, _ in table], np.int64)
    stack = np.stack([recs[r][:, k * step:k * step + win_len] for r, k in table])
    dev = _dev(ctx)
    wt = torch.from_numpy(np.ascontiguousarray(stack)).to(dev)
    ref_d = torch.full((len(table), n_ch, n_ch), -7.0, dtype=torch.float64, device=dev)
    ref_c = torch.full_like(ref_d, -7.0)
    ref = engine.eeg_window_dev(wt, dist_t=ref_d, corr_t=ref_c, ctx=ctx)
    d2, c2 = torch.full_like(ref_d, -7.0), torch.full_like(ref_d, -7.0)
    args = (torch.from_numpy(packed).to(dev), torch.from_numpy(start).to(dev), torch.from_numpy(ld).to(dev), win_len)
    got = engine.eeg_window_ragged_dev(*args, dist_t=d2, corr_t=c2, n_ch=n_ch, ctx=ctx)
    bare = engine.eeg_window_ragged_dev(*args, n_ch=n_ch, ctx=ctx)
    torch.cuda.synchronize()
    assert len(table) >= 5 and int(ref.status.max()) == 0
    assert _same_diagrams(got, ref) and _same_diagrams(bare, ref)
    assert _bytes_equal(d2, ref_d) and _bytes_equal(c2, ref_c)
    assert np.array_equal(d2.cpu().numpy(), port.corr_dist_batch(stack)[1])


# ------------------------------------------------------------------ class widths and retry
@pytest.mark.parametrize("n_ch", (33, 48))
def test_fused_kernel_first_pass_widths_agree(ctx, n_ch):
    """32, 64 and 128 class bits in the first pass (set_class_words(0 | 1 | 2, 1)): identical results, equal to the
    two-kernel path."""
    import torch
    for n_t in (5, 33, 225, 256):
        wt = sc.to_device(sc.windows(n_ch, n_t), _dev(ctx))
        _, _, two = _two_kernels(ctx, wt)
        got = []
        try:
            for words in (0, 1, 2):
                ctx.set_class_words(words, 1)
                got.append(engine.eeg_window_dev(wt, ctx=ctx))
        finally:
            ctx.set_class_words(2, 1)
        torch.cuda.synchronize()
        assert int(two.status.max()) == 0
        assert all(_same_diagrams(g, two) for g in got), (n_ch, n_t)


def _overflowing(bits):
    """Shapes of the fused grid with windows that have more than `bits` H1 rows alive at once, by the oracle."""
    out = []
    for n_ch in (46, 47, 48):
        for n_t in (224, 225, 249, 255, 256):
            over = [w for w in range(sc.N_WIN) if sc.max_alive(sc.oracle_diagrams(n_ch, n_t, w)[1]) > bits]
            if over:
                out.append((n_ch, n_t, over))
    return out


@pytest.mark.parametrize("words,bits", [(0, 32), (1, 64)])
def test_fused_kernel_narrow_first_pass_overflows_and_the_ladder_repairs(ctx, words, bits):
    """The windows whose diagram has more than 32 (64) rows alive at once cannot fit a first pass of 32 (64) class bits:
    under RETRY_FIRST_PASS they carry TDA_WIN_CLASS_OVERFLOW (status bit 2); under RETRY_AUTO the ladder leaves every
    window clean and equal to the two-kernel path."""
    import torch
    shapes = _overflowing(bits)
    assert shapes, "tests/test_eeg_shapes_model.py::test_fused_grid_input_conditions holds this"
    for n_ch, n_t, over in shapes[::5]:                         # (one length per channel count where all 15 shapes qualify)
        wt = sc.to_device(sc.windows(n_ch, n_t), _dev(ctx))
        _, _, two = _two_kernels(ctx, wt)
        ctx.set_class_words(words, 1)
        try:
            ctx.set_retry_policy(ctx.RETRY_FIRST_PASS)
            first = engine.eeg_window_dev(wt, ctx=ctx)
            torch.cuda.synchronize()
            ctx.set_retry_policy(ctx.RETRY_AUTO)
            full = engine.eeg_window_dev(wt, ctx=ctx)
            torch.cuda.synchronize()
        finally:
            ctx.set_retry_policy(ctx.RETRY_AUTO)
            ctx.set_class_words(2, 1)
        st = first.status.cpu().numpy()
        assert np.all(st[over] & 2), (n_ch, n_t, over, st)
        assert int(full.status.max()) == 0 and _same_diagrams(full, two), (n_ch, n_t)


# ------------------------------------------------------------------ refusals
def _poisoned(n_win, h0_cap, dev):
    out = engine.DeviceDiagrams(n_win, h0_cap, 16, dev)
    for t in (out.h0, out.h1, out.c0, out.c1, out.status):
        t.fill_(-7)
    return out


def _still_poisoned(*ts):
    import torch
    torch.cuda.synchronize()
    return all(bool((t == -7).all()) for t in ts)


def test_refusals_leave_the_outputs_alone(ctx):
    """What the entries refuse, each with its own message and without touching the outputs: 32 and 49 channels, 1 and 257
    samples and h0_cap < n_ch at the fused kernel (three sources); 0 and 65 channels at corr_dist; win_len 1 and step 0 at
    the sliding entries.  The entries still work afterwards."""
    import torch
    dev = _dev(ctx)
    f64 = dict(dtype=torch.float64, device=dev)
    i64 = dict(dtype=torch.int64, device=dev)

    def fused(n_ch, n_t, h0_cap, match):
        out = _poisoned(2, h0_cap, dev)
        d = torch.full((2, n_ch, n_ch), -7.0, **f64)
        with pytest.raises(TdaError, match=match):
            engine.eeg_window_dev(torch.ones((2, n_ch, n_t), **f64), out, dist_t=d, ctx=ctx)
        with pytest.raises(TdaError, match=match):
            engine.eeg_window_sliding_dev(torch.ones((2, n_ch, n_t), **f64), n_t, 1, out=out, dist_t=d, ctx=ctx)
        with pytest.raises(TdaError, match=match):
            engine.eeg_window_ragged_dev(torch.ones(2 * n_ch * n_t, **f64), torch.tensor([0, n_ch * n_t], **i64),
                                         torch.tensor([n_t, n_t], **i64), n_t, out=out, dist_t=d, n_ch=n_ch, ctx=ctx)
        assert _still_poisoned(out.h0, out.h1, out.c0, out.c1, out.status, d)

    fused(32, 64, 32, "33..48 channels")
    fused(49, 64, 49, "33..48 channels")
    fused(40, 257, 40, "2..256 samples")
    fused(40, 64, 39, "h0_cap must be >= n_ch")
    # one sample: the stacked entry names the range, the entries that take a win_len refuse that first
    out = _poisoned(2, 40, dev)
    with pytest.raises(TdaError, match="2..256 samples"):
        engine.eeg_window_dev(torch.ones((2, 40, 1), **f64), out, ctx=ctx)
    with pytest.raises(TdaError, match="win_len must be >= 2 and step >= 1"):
        engine.eeg_window_sliding_dev(torch.ones((2, 40, 1), **f64), 1, 1, out=out, ctx=ctx)
    with pytest.raises(TdaError, match="win_len must be >= 2"):
        engine.eeg_window_ragged_dev(torch.ones(640, **f64), torch.tensor([0, 320], **i64), torch.tensor([8, 8], **i64), 1,
                                     out=out, n_ch=40, ctx=ctx)
    # step 0 (engine's own window count would divide by it: straight to the C entries)
    sig = torch.ones((1, 40, 64), **f64)
    d = torch.full((4, 40, 40), -7.0, **f64)
    tp = lambda t: C.c_void_p(t.data_ptr())
    with pytest.raises(TdaError, match="win_len must be >= 2 and step >= 1"):
        ctx.check(ctx.lib.tda_eeg_window_sliding_dev(ctx.h, tp(sig), 1, 40, 64, 16, 0, None, 0, 2.0, tp(d), None, tp(out.h0),
                                                     out.h0_cap, tp(out.c0), tp(out.h1), out.h1_cap, tp(out.c1),
                                                     tp(out.status), None, None))
    for win_len, step in ((1, 1), (16, 0)):
        with pytest.raises(TdaError, match="win_len must be >= 2 and step >= 1"):
            ctx.check(ctx.lib.tda_corr_dist_sliding_dev(ctx.h, tp(sig), 40, 64, win_len, step, tp(d), None, None, None))
        host = np.full((4, 40, 40), -7.0)
        with pytest.raises(TdaError, match="bad window geometry"):          # (the host entry's own words for it)
            ctx.check(ctx.lib.tda_corr_dist_sliding(ctx.h, ptr(np.ones((40, 64))), 40, 64, win_len, step, ptr(host), None, None))
        assert (host == -7.0).all()
    assert _still_poisoned(out.h0, out.h1, out.c0, out.c1, out.status, d)
    # corr_dist: 0 and 65 channels, one sample
    d65 = torch.full((2, 65, 65), -7.0, **f64)
    w65 = torch.ones((2, 65, 10), **f64)
    for n_ch in (0, 65):                                    # (the buffers of 65 channels for both: none is touched)
        with pytest.raises(TdaError, match=r"n_ch must be in \[1,64\]"):
            ctx.check(ctx.lib.tda_corr_dist_batch_dev(ctx.h, tp(w65), 2, n_ch, 10, tp(d65), None, None))
        with pytest.raises(TdaError, match=r"n_ch must be in \[1,64\]"):
            ctx.check(ctx.lib.tda_corr_dist_sliding_dev(ctx.h, tp(w65), n_ch, 10, 4, 2, tp(d65), None, None, None))
    host = np.full((2, 65, 65), -7.0)
    with pytest.raises(TdaError, match=r"n_ch must be in \[1,64\]"):
        ctx.check(ctx.lib.tda_corr_dist_batch(ctx.h, ptr(np.ones((2, 65, 10))), 2, 65, 10, ptr(host), None))
    with pytest.raises(TdaError, match=r"n_ch must be in \[1,64\]"):
        ctx.check(ctx.lib.tda_corr_dist_sliding(ctx.h, ptr(np.ones((65, 10))), 65, 10, 4, 2, ptr(host), None, None))
    with pytest.raises(TdaError, match="null pointer|n_ch must be in|bad window geometry"):
        engine.corr_dist_batch(np.ones((2, 0, 10)), ctx=ctx)            # (no bytes to stage: refused one step earlier)
    assert (host == -7.0).all()
    with pytest.raises(TdaError, match="n_t must be >= 2"):
        engine.corr_dist_dev(torch.ones((2, 40, 1), **f64), d[:2], ctx=ctx)
    assert _still_poisoned(d65, d)
    # the context stays usable
    W = sc.windows(40, 64)
    got = engine.eeg_window_dev(sc.to_device(W, dev), ctx=ctx)
    e0, e1 = got.to_lists()
    o = sc.oracle_diagrams(40, 64, 0)
    assert int(got.status.max()) == 0 and _same_multiset(e0[0], o[0]) and _same_multiset(e1[0], o[1])


# ------------------------------------------------------------------ 48 channels, more than 512 classes alive at once
def test_fused_kernel_48_channels_more_than_512_classes(ctx):
    """K(24,24) and K(23,25) on 48 channels have 529 and 528 H1 classes alive at once
    (tests/test_eeg_shapes_model.py), more than the 512 class bits of the widest LDS pass: the fused ladder ends in the
    pass with the class vectors in HBM, as the two-kernel path does.  Through all three window sources: status 0
    everywhere, rows and counts equal the two-kernel path and the oracle, the ordinary windows of the batch untouched
    by it, and a second call gives the same."""
    import torch
    dev = _dev(ctx)
    W, bip = sc.batch_48()
    n = len(W)
    wt = sc.to_device(W, dev)
    dist, _, two = _two_kernels(ctx, wt, h1_cap=1024)
    sig, packed, start, ld, order = sc.as_recordings(W)
    sig_t, packed_t = torch.from_numpy(sig).to(dev), torch.from_numpy(packed).to(dev)
    start_t, ld_t = torch.from_numpy(start).to(dev), torch.from_numpy(ld).to(dev)
    runs = []
    for _ in range(2):
        runs.append(("stacked", engine.eeg_window_dev(wt, h1_cap=1024, ctx=ctx), None))
        runs.append(("sliding", engine.eeg_window_sliding_dev(sig_t, 250, 250, h1_cap=1024, ctx=ctx)[0], None))
        runs.append(("table", engine.eeg_window_ragged_dev(packed_t, start_t, ld_t, 250, h1_cap=1024, n_ch=48, ctx=ctx), order))
    torch.cuda.synchronize()
    assert int(two.status.max()) == 0
    b0, b1 = two.to_lists()
    d = dist.cpu().numpy()
    oracle = [port.rips_dm(d[w]) for w in range(n)]
    for w in range(n):
        assert _same_multiset(b0[w], oracle[w][0]) and _same_multiset(b1[w], oracle[w][1])
        assert (sc.max_alive(oracle[w][1]) > 512) == (w in bip)
    for name, got, perm in runs:
        st = got.status.cpu().numpy()
        a0, a1 = got.to_lists()
        idx = np.arange(n) if perm is None else perm
        print(name, "status", st.tolist(), "h1 rows", [len(x) for x in a1])
        assert not st.any(), (name, st)
        for k, w in enumerate(idx):
            assert np.array_equal(a0[k], b0[w]) and np.array_equal(a1[k], b1[w]), (name, k, w)
            assert _same_multiset(a1[k], oracle[w][1]), (name, k, w)


# ------------------------------------------------------------------ TDA_EEG_RESIDENT=1
def test_resident_family_in_a_child_process():
    """eeg_window_kernel<3, true, ...> and eeg_window_ragged_kernel<3, true, ...> (the window kept in registers between
    the two passes: TDA_EEG_RESIDENT=1, read once per process): tests/eeg_resident_child.py in a fresh child."""
    assert "TDA_EEG_RESIDENT" not in os.environ                 # this process runs the streaming family
    env = {k: v for k, v in os.environ.items() if k != "TDA_EEG_RESIDENT"}
    env["TDA_EEG_RESIDENT"] = "1"
    r = subprocess.run([sys.executable, os.path.join(HERE, "eeg_resident_child.py")], env=env, capture_output=True, text=True,
                       timeout=240)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:] + r.stderr[-2000:])
    n_cases = len(sc.RESIDENT_CH) * len(sc.RESIDENT_LENGTHS) * 3 * 3 + 3
    assert f"RESIDENT OK cases {n_cases}" in r.stdout, r.stdout[-2000:]
