"""
The entry into the coverage scan of the Rips sweep on the GPU: inputs whose busy chunks end with no class alive, so that
the scan starts right behind them -- in the middle of a filtration with a birth still to come (the lull clouds), behind
the last busy chunk of a window (the EEG windows), at or behind the end of the filtration (the ring clouds) -- and the
class-bit ladders, whose cut chunks must not scan.  tests/test_scan_entry_model.py proves on the CPU that these inputs
do that; here every kernel that shares the sweep runs them.

Bar: H0 and H1 rows bit-equal to the oracle as sorted multisets, status words 0.
"""
import numpy as np
import pytest

import chunk_cut_model as C
import quiet_tail_model as Q
import scan_entry_model as S
from oracle import brute, port
from tda_eeg_audio_amd import engine, synth

pytestmark = pytest.mark.gpu

WIDTHS = ((2, 1), (2, 2))            # first pass of the point-cloud kernel: narrow (32 class bits), wide (64)


def _same(a, b):
    return np.array_equal(brute.sort_rows(a), brute.sort_rows(b))


def _oracle(pcs, n_pts=None):
    return [port.rips_f32(port.cloud_dm(pc if n_pts is None else pc[:int(n_pts[w])]).astype(np.float32), thresh=S.CLOUD_THRESH)
            for w, pc in enumerate(pcs)]


@pytest.fixture(scope="module")
def lulls():
    """{name: (clouds (8, n, 3), oracle diagrams)}"""
    return {name: (pcs, _oracle(pcs)) for name, pcs in ((nm, S.lull_clouds(nm)) for nm in S.LULLS)}


@pytest.fixture(scope="module")
def ladders():
    out = {}
    for name in C.LADDERS:
        pcs = C.ladder_clouds(name)
        out[name] = (pcs, _oracle(pcs))
    return out


@pytest.fixture(scope="module")
def rings():
    """(clouds, n_pts, oracle diagrams): eight copies of each ring cloud whose last class dies in the last chunk"""
    picked = S.ring_windows_ending_in_the_last_chunk()
    sets = Q.explicit_clouds()
    pcs, n_pts = [], []
    for name in ("ring60", "ring124"):
        ws = [w for nm, w in picked if nm == name][:8]
        assert len(ws) == 8
        clouds, npt = sets[name]
        pad = np.zeros((8, 124, 3))
        pad[:, :clouds.shape[1]] = clouds[ws]
        pcs.append(pad); n_pts.append(npt[ws])
    pcs, n_pts = np.concatenate(pcs), np.concatenate(n_pts).astype(np.int32)
    return pcs, n_pts, _oracle(pcs, n_pts)


def _first_pass_both_widths(ctx, pcs, ref, n_pts=None):
    try:
        for words in WIDTHS:
            ctx.set_class_words(*words)
            h0, h1, st = engine.cloud_rips_batch(pcs, n_pts=n_pts, normalise=False, thresh=S.CLOUD_THRESH, ctx=ctx)
            assert not st.any(), (words, st)
            for w in range(len(pcs)):
                assert _same(h0[w], ref[w][0]) and _same(h1[w], ref[w][1]), (words, w)
    finally:
        ctx.set_class_words(2, 1)


def _widening_passes_alone(ctx, pcs, ref, n_pts=None):
    """Every window flagged by hand and redone by the widening passes alone (TDA_RETRY_ONLY)."""
    import torch
    dev = torch.device("cuda", ctx.device)
    n_win, p_cap, dim = pcs.shape
    if n_pts is None:
        n_pts = np.full(n_win, p_cap, np.int32)
    out = engine.DeviceDiagrams(n_win, p_cap, engine.DEFAULT_H1_CAP, dev)
    out.status.fill_(2); out.c0.fill_(-5); out.c1.fill_(-5)
    pt = torch.from_numpy(np.ascontiguousarray(pcs)).to(dev)
    nt = torch.from_numpy(n_pts).to(dev)
    ctx.set_retry_policy(ctx.RETRY_ONLY)
    try:
        ctx.check(ctx.lib.tda_cloud_rips_batch_dev(ctx.h, engine._tp(pt), engine._tp(nt), n_win, p_cap, dim, 0, S.CLOUD_THRESH,
                                                   engine._tp(out.h0), out.h0_cap, engine._tp(out.c0), engine._tp(out.h1),
                                                   out.h1_cap, engine._tp(out.c1), engine._tp(out.status), engine._stream()))
    finally:
        ctx.set_retry_policy(ctx.RETRY_AUTO)
    torch.cuda.synchronize()
    assert int(out.status.max()) == 0 and int(out.status.min()) == 0
    a0, a1 = out.to_lists()
    for w in range(n_win):
        assert _same(a0[w], ref[w][0]) and _same(a1[w], ref[w][1]), w


def _distance_matrices(ctx, pcs, words=None):
    """rips_dm_kernel: chunks of 256 edges"""
    dms = np.stack([port.cloud_dm(pc) for pc in pcs])
    try:
        if words:
            ctx.set_class_words(*words)
        h0, h1, st = engine.rips_dm_batch(dms, thresh=S.CLOUD_THRESH, ctx=ctx)
    finally:
        ctx.set_class_words(2, 1)
    assert not st.any(), st
    for w in range(len(dms)):
        o = port.rips_dm(dms[w], thresh=S.CLOUD_THRESH)
        assert _same(h0[w], o[0]) and _same(h1[w], o[1]), w


@pytest.mark.parametrize("name", sorted(S.LULLS))
def test_lull_clouds_both_first_pass_widths(ctx, lulls, name):
    _first_pass_both_widths(ctx, *lulls[name])


@pytest.mark.parametrize("name", sorted(S.LULLS))
def test_lull_clouds_widening_passes_alone(ctx, lulls, name):
    _widening_passes_alone(ctx, *lulls[name])


@pytest.mark.parametrize("name", ["lull45", "lull60"])
@pytest.mark.parametrize("words", [(2, 1), (1, 1)])
def test_lull_distance_matrices(ctx, lulls, name, words):
    """45 points: one vertex word, 60: two; the default class words of the kernel and one 64-bit word."""
    _distance_matrices(ctx, lulls[name][0], words)


def test_fused_eeg_kernel_32_and_64_class_bits(ctx):
    """Every one of these windows ends its last busy chunk calm (test_scan_entry_model.py): all of them take the new path."""
    import torch
    dev = torch.device("cuda", ctx.device)
    W = synth.eeg_windows(64, seed=5)
    ref = [port.rips_dm(port.corr_dist(W[w])[1]) for w in range(64)]
    wt = torch.from_numpy(W).to(dev)
    try:
        for words in ((0, 1), (1, 1)):
            ctx.set_class_words(*words)
            out = engine.eeg_window_dev(wt, ctx=ctx)
            torch.cuda.synchronize()
            assert int(out.status.max()) == 0 and int(out.status.min()) == 0, words
            a0, a1 = out.to_lists()
            for w in range(64):
                assert _same(a0[w], ref[w][0]) and _same(a1[w], ref[w][1]), (words, w)
    finally:
        ctx.set_class_words(2, 1)


@pytest.mark.parametrize("name", sorted(C.LADDERS))
def test_ladders_first_passes_and_widening_passes(ctx, ladders, name):
    """Chunks cut at 32 and at 64 class bits: a cut chunk does not scan, the full chunk behind the last cut does."""
    _first_pass_both_widths(ctx, *ladders[name])
    _widening_passes_alone(ctx, *ladders[name])


@pytest.mark.parametrize("name", sorted(C.LADDERS))
def test_ladder_distance_matrices(ctx, ladders, name):
    _distance_matrices(ctx, ladders[name][0], (1, 1))
    _distance_matrices(ctx, ladders[name][0], (2, 1))


def test_ring_clouds_whose_scan_starts_at_the_end_of_the_filtration(ctx, rings):
    pcs, n_pts, ref = rings
    _first_pass_both_widths(ctx, pcs, ref, n_pts)
    _widening_passes_alone(ctx, pcs, ref, n_pts)
    _distance_matrices(ctx, [pcs[w][:int(n_pts[w])] for w in range(8)])          # the eight 60-point copies
