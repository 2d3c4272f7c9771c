"""
Triangle lists of phase d that do not fit (csrc/rips.hip, LCAP): the entries that were stored -- the first LCAP of the
list in (owner, v) order -- are reduced, the table is rewritten and the chunk is listed again, until the list fits.
The inputs (tests/list_capacity_cases.py): the audio windows of the two bands that overflow least and most often, and
ball-and-circle clouds whose lists were measured -- longer than twice the capacity, longer than it, and between the
capacity of 255 entries that one class word had before and the 416 it has now.

Every flavour of the list goes through them: one 32-bit and one 64-bit class word (wave 0 takes the list block by
block: both first-pass widths of the cloud kernel and its widening pass), and two and four 64-bit words (all blocks in
registers, capacities 166 and 92: the distance-matrix kernels, which list chunks of 256 edges).

Bar: H0 and H1 rows bit-equal to the oracle as sorted multisets, status words 0.
"""
import numpy as np
import pytest

import list_capacity_cases as L
from oracle import brute, port
from tda_eeg_audio_amd import engine, synth

pytestmark = pytest.mark.gpu

WIDTHS = ((2, 1), (2, 2))            # first pass of the point-cloud kernel: narrow (32 class bits), wide (64)
THRESH = 100.0                       # explicit clouds: the enclosing radius is the only cut
N_DM = 32                            # audio windows that also go through the distance-matrix kernel


def _same(a, b):
    return np.array_equal(brute.sort_rows(a), brute.sort_rows(b))


@pytest.fixture(scope="module")
def audio():
    """{band: (windows, tau, oracle diagrams)}"""
    out = {}
    for band in ("alpha", "delta"):
        wins = synth.audio_windows(256, band, seed=1)
        tau = port.compute_tau(wins[0], 125)
        out[band] = (wins, tau, [port.audio_persistence(w, tau)[0] for w in wins])
    return out


@pytest.fixture(scope="module")
def clouds():
    """{name: (clouds, oracle diagrams)}"""
    out = {}
    for name in L.CASES:
        pcs = L.clouds(name)
        out[name] = (pcs, [port.rips_f32(port.cloud_dm(pc).astype(np.float32), thresh=THRESH) for pc in pcs])
    return out


def _takens(ctx, wins, tau, ref, out=None):
    import torch
    dev = torch.device("cuda", ctx.device)
    wt = torch.from_numpy(wins).to(dev)
    tt = torch.full((len(wins),), tau, dtype=torch.int32, device=dev)
    out = engine.takens_rips_dev(wt, tt, out=out, ctx=ctx)
    torch.cuda.synchronize()
    assert int(out.status.max()) == 0 and int(out.status.min()) == 0
    a0, a1 = out.to_lists()
    for w in range(len(wins)):
        assert _same(a0[w], ref[w][0]) and _same(a1[w], ref[w][1]), w


@pytest.mark.parametrize("band", ["alpha", "delta"])
def test_audio_windows_both_first_pass_widths(ctx, audio, band):
    wins, tau, ref = audio[band]
    try:
        for words in WIDTHS:
            ctx.set_class_words(*words)
            _takens(ctx, wins, tau, ref)
    finally:
        ctx.set_class_words(2, 1)


@pytest.mark.parametrize("band", ["alpha", "delta"])
def test_audio_windows_widening_pass(ctx, audio, band):
    """Every window flagged by hand and redone by the widening passes alone (TDA_RETRY_ONLY)."""
    import torch
    wins, tau, ref = audio[band]
    out = engine.DeviceDiagrams(len(wins), engine._lib.MAX_POINTS, engine.DEFAULT_H1_CAP, torch.device("cuda", ctx.device))
    out.status.fill_(2); out.c0.fill_(-5); out.c1.fill_(-5)
    ctx.set_retry_policy(ctx.RETRY_ONLY)
    try:
        _takens(ctx, wins, tau, ref, out=out)
    finally:
        ctx.set_retry_policy(ctx.RETRY_AUTO)


@pytest.mark.parametrize("words", [1, 2])
def test_audio_distance_matrices(ctx, audio, words):
    """rips_dm_kernel on the clouds of the alpha windows, 124 points: one class word (block by block) and two."""
    wins, tau, _ = audio["alpha"]
    dms = np.stack([port.cloud_dm(port.minmax_normalise(port.takens(w, 3, tau, 2))) for w in wins[:N_DM]])
    try:
        ctx.set_class_words(words, 1)
        h0, h1, st = engine.rips_dm_batch(dms, ctx=ctx)
    finally:
        ctx.set_class_words(2, 1)
    assert not st.any(), st
    for w in range(N_DM):
        o = port.rips_dm(dms[w])
        assert _same(h0[w], o[0]) and _same(h1[w], o[1]), (words, w)


@pytest.mark.parametrize("name", sorted(L.CASES))
def test_ball_and_circle_both_first_pass_widths(ctx, clouds, name):
    pcs, ref = clouds[name]
    try:
        for words in WIDTHS:
            ctx.set_class_words(*words)
            h0, h1, st = engine.cloud_rips_batch(pcs, normalise=False, thresh=THRESH, ctx=ctx)
            assert not st.any(), (name, words, st)
            for w in range(len(pcs)):
                assert _same(h0[w], ref[w][0]) and _same(h1[w], ref[w][1]), (name, words, w)
    finally:
        ctx.set_class_words(2, 1)


@pytest.mark.parametrize("name,words", [("twice60", 1), ("twice60", 2), ("twice60", 4), ("once60", 4),
                                        ("twice124", 1), ("twice124", 2), ("between124", 2)])
def test_ball_and_circle_distance_matrices(ctx, clouds, name, words):
    """rips_dm_kernel with one, two and four 64-bit class words (four: up to 64 points)."""
    pcs, _ = clouds[name]
    dms = np.stack([port.cloud_dm(pc) for pc in pcs])
    try:
        ctx.set_class_words(words, 1)
        h0, h1, st = engine.rips_dm_batch(dms, thresh=THRESH, ctx=ctx)
    finally:
        ctx.set_class_words(2, 1)
    assert not st.any(), (name, words, st)
    for w in range(len(dms)):
        o = port.rips_dm(dms[w], thresh=THRESH)
        assert _same(h0[w], o[0]) and _same(h1[w], o[1]), (name, words, w)
