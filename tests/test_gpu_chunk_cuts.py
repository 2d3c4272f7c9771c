"""
Chunks cut short for class bits, on the GPU: inputs whose births do not fit the free class bits of a chunk, so that the
chunk closes at the first birth that does not fit and the sweep goes on from there with the bits its kills have freed.
tests/test_chunk_cut_model.py proves on the CPU where these inputs cut (first chunk, later chunk, twice in one stretch,
a chunk behind a cut with no other candidate, not at all); here every kernel that shares the sweep runs them.

The audio windows are the theta windows of quiet_tail_model.audio_sample(), the band that cuts most (all five bands go
through both first-pass widths in tests/test_gpu_quiet_tail.py); the ladders cut at 32 bits and, with four rails, at 64.

Bar: H0 and H1 rows bit-equal to the oracle as sorted multisets, status words 0.
"""
import numpy as np
import pytest

import chunk_cut_model as M
import quiet_tail_model as Q
from oracle import brute, port
from tda_eeg_audio_amd import engine, synth

pytestmark = pytest.mark.gpu

WIDTHS = ((2, 1), (2, 2))            # first pass of the point-cloud kernel: narrow (32 class bits), wide (64)


def _same(a, b):
    return np.array_equal(brute.sort_rows(a), brute.sort_rows(b))


@pytest.fixture(scope="module")
def ladders():
    """{name: (clouds, oracle diagrams)}"""
    out = {}
    for name in M.LADDERS:
        pcs = M.ladder_clouds(name)
        out[name] = (pcs, [port.rips_f32(port.cloud_dm(pc).astype(np.float32), thresh=M.CLOUD_THRESH) for pc in pcs])
    return out


def test_theta_windows_that_cut_both_first_pass_widths(ctx):
    import torch
    dev = torch.device("cuda", ctx.device)
    wins, tau = Q.audio_sample()["theta"]
    cs = M.audio_cases(32, bands=("theta",))["theta"]
    assert any("double" in c for c in cs) and any("lonely" in c for c in cs) and any(c == {"none"} for c in cs)
    ref = [port.audio_persistence(w, tau)[0] for w in wins]
    wt = torch.from_numpy(wins).to(dev)
    tt = torch.full((len(wins),), tau, dtype=torch.int32, device=dev)
    try:
        for words in WIDTHS:
            ctx.set_class_words(*words)
            out = engine.takens_rips_dev(wt, tt, ctx=ctx)
            torch.cuda.synchronize()
            assert int(out.status.max()) == 0 and int(out.status.min()) == 0, words
            a0, a1 = out.to_lists()
            for w in range(len(wins)):
                assert _same(a0[w], ref[w][0]) and _same(a1[w], ref[w][1]), (words, w, cs[w])
    finally:
        ctx.set_class_words(2, 1)


@pytest.mark.parametrize("name", sorted(M.LADDERS))
def test_ladders_both_first_pass_widths(ctx, ladders, name):
    pcs, ref = ladders[name]
    try:
        for words in WIDTHS:
            ctx.set_class_words(*words)
            h0, h1, st = engine.cloud_rips_batch(pcs, normalise=False, thresh=M.CLOUD_THRESH, ctx=ctx)
            assert not st.any(), (name, words, st)
            for w in range(len(pcs)):
                assert _same(h0[w], ref[w][0]) and _same(h1[w], ref[w][1]), (name, words, w)
    finally:
        ctx.set_class_words(2, 1)


@pytest.mark.parametrize("name", sorted(M.LADDERS))
def test_ladder_distance_matrices_one_class_word(ctx, ladders, name):
    """rips_dm_kernel with one 64-bit class word and chunks of 256 edges: the four-rail ladders cut in the second chunk."""
    pcs, _ = ladders[name]
    dms = np.stack([port.cloud_dm(pc) for pc in pcs])
    try:
        ctx.set_class_words(1, 1)
        h0, h1, st = engine.rips_dm_batch(dms, thresh=M.CLOUD_THRESH, ctx=ctx)
    finally:
        ctx.set_class_words(2, 1)
    assert not st.any(), (name, st)
    for w in range(len(dms)):
        o = port.rips_dm(dms[w], thresh=M.CLOUD_THRESH)
        assert _same(h0[w], o[0]) and _same(h1[w], o[1]), (name, w)


def test_fused_eeg_kernel_32_and_64_class_bits(ctx):
    """The fused kernel takes windows, not matrices, so no matrix can be built for it: synthetic windows through its
    32-bit and its 64-bit first pass (class words 0 and 1), where the narrower one runs out of bits first."""
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
