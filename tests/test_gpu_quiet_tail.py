"""
The quiet tail of the Rips sweep on the GPU: inputs on which the coverage scan raises false alarms (edges without a
common neighbour in the stale adjacency rows that the skipped edges cover at their own time) and, behind them, true late
candidates.  tests/test_quiet_tail_model.py proves on the CPU that these inputs do that; here every kernel that shares
the sweep runs them.

Bar: H0 and H1 rows bit-equal to the oracle as sorted multisets, status words 0.
"""
import numpy as np
import pytest

import quiet_tail_model as M
from oracle import brute, port
from tda_eeg_audio_amd import engine, synth

pytestmark = pytest.mark.gpu

WIDTHS = ((2, 1), (2, 2))            # first pass of the point-cloud kernel: narrow (32 class bits), wide (64)


def _same(a, b):
    return np.array_equal(brute.sort_rows(a), brute.sort_rows(b))


@pytest.fixture(scope="module")
def audio():
    """{band: (windows, tau, oracle diagrams)}"""
    out = {}
    for band, (wins, tau) in M.audio_sample().items():
        out[band] = (wins, tau, [port.audio_persistence(w, tau)[0] for w in wins])
    return out


@pytest.fixture(scope="module")
def clouds():
    """{name: (clouds, n_pts, oracle diagrams)}: the far-point and ring clouds, and the control"""
    out = {}
    sets = dict(M.explicit_clouds())
    sets["control"] = (M.control_cloud()[None], np.array([40], np.int32))
    for name, (pcs, n_pts) in sets.items():
        ref = [port.rips_f32(port.cloud_dm(M.cloud_points(pcs, n_pts, w)).astype(np.float32), thresh=M.CLOUD_THRESH)
               for w in range(len(pcs))]
        out[name] = (pcs, n_pts, ref)
    return out


@pytest.mark.parametrize("band", M.AUDIO_BANDS)
def test_audio_windows_both_first_pass_widths(ctx, audio, band):
    import torch
    dev = torch.device("cuda", ctx.device)
    wins, tau, ref = audio[band]
    wt = torch.from_numpy(wins).to(dev)
    tt = torch.full((len(wins),), tau, dtype=torch.int32, device=dev)
    try:
        for words in WIDTHS:
            ctx.set_class_words(*words)
            out = engine.takens_rips_dev(wt, tt, ctx=ctx)
            torch.cuda.synchronize()
            assert int(out.status.max()) == 0 and int(out.status.min()) == 0, (band, words)
            a0, a1 = out.to_lists()
            for w in range(len(wins)):
                assert _same(a0[w], ref[w][0]) and _same(a1[w], ref[w][1]), (band, words, w)
    finally:
        ctx.set_class_words(2, 1)


@pytest.mark.parametrize("name", ["far60", "far124", "ring60", "ring124", "control"])
def test_explicit_clouds_both_first_pass_widths(ctx, clouds, name):
    pcs, n_pts, ref = clouds[name]
    try:
        for words in WIDTHS:
            ctx.set_class_words(*words)
            h0, h1, st = engine.cloud_rips_batch(pcs, n_pts=n_pts, normalise=False, thresh=M.CLOUD_THRESH, ctx=ctx)
            assert not st.any(), (name, words, st)
            for w in range(len(pcs)):
                assert _same(h0[w], ref[w][0]) and _same(h1[w], ref[w][1]), (name, words, w)
    finally:
        ctx.set_class_words(2, 1)


@pytest.mark.parametrize("n", [47, 70])
def test_distance_matrices_of_the_clouds(ctx, n):
    """rips_dm_kernel (chunks of 256 edges; one vertex word at 47 points, two at 70)."""
    import torch
    dev = torch.device("cuda", ctx.device)
    pcs = np.concatenate([M.jittered(M.blob_far(n, 11), 8, 5), M.jittered(M.blob_ring(n, 12), 8, 6)])
    dms = np.stack([port.cloud_dm(pc) for pc in pcs])
    out = engine.rips_dm_dev(torch.from_numpy(dms).to(dev), thresh=M.CLOUD_THRESH, ctx=ctx)
    torch.cuda.synchronize()
    assert int(out.status.max()) == 0 and int(out.status.min()) == 0
    a0, a1 = out.to_lists()
    for w in range(len(dms)):
        o = port.rips_dm(dms[w], thresh=M.CLOUD_THRESH)
        assert _same(a0[w], o[0]) and _same(a1[w], o[1]), (n, w)


def test_fused_eeg_kernel(ctx):
    import torch
    dev = torch.device("cuda", ctx.device)
    W = synth.eeg_windows(64, seed=5)
    out = engine.eeg_window_dev(torch.from_numpy(W).to(dev), ctx=ctx)
    torch.cuda.synchronize()
    assert int(out.status.max()) == 0 and int(out.status.min()) == 0
    a0, a1 = out.to_lists()
    for w in range(64):
        o = port.rips_dm(port.corr_dist(W[w])[1])
        assert _same(a0[w], o[0]) and _same(a1[w], o[1]), w


@pytest.mark.parametrize("name", ["ring60", "ring124"])
def test_widening_passes_on_the_ring_clouds(ctx, clouds, name):
    """Every window flagged by hand and redone by the widening passes alone (TDA_RETRY_ONLY)."""
    import torch
    dev = torch.device("cuda", ctx.device)
    pcs, n_pts, ref = clouds[name]
    n_win, p_cap, dim = pcs.shape
    out = engine.DeviceDiagrams(n_win, p_cap, engine.DEFAULT_H1_CAP, dev)
    out.status.fill_(2); out.c0.fill_(-5); out.c1.fill_(-5)
    pt = torch.from_numpy(np.ascontiguousarray(pcs)).to(dev)
    nt = torch.from_numpy(n_pts).to(dev)
    ctx.set_retry_policy(ctx.RETRY_ONLY)
    try:
        ctx.check(ctx.lib.tda_cloud_rips_batch_dev(ctx.h, engine._tp(pt), engine._tp(nt), n_win, p_cap, dim, 0, M.CLOUD_THRESH,
                                                   engine._tp(out.h0), out.h0_cap, engine._tp(out.c0), engine._tp(out.h1),
                                                   out.h1_cap, engine._tp(out.c1), engine._tp(out.status), engine._stream()))
    finally:
        ctx.set_retry_policy(ctx.RETRY_AUTO)
    torch.cuda.synchronize()
    assert int(out.status.max()) == 0 and int(out.status.min()) == 0
    a0, a1 = out.to_lists()
    for w in range(n_win):
        assert _same(a0[w], ref[w][0]) and _same(a1[w], ref[w][1]), (name, w)
