"""
landscapes=(grid, levels) through the step and the recording passes: the rows stay what they are; ws.land is the reference
(tests/landscape_ref.py) applied to the step's own diagrams; land_h (n_rec, n_bands, 3, levels + 1, n_grid) holds, per
recording, the bytes the same recording gives when it runs alone through a pass of its own; NaN for a recording without a
window.
"""
import numpy as np
import pytest

import landscape_ref as lr
from test_gpu_ragged import FIX, _env, _raw
from tda_eeg_audio_amd import _lib, pipeline, preprocess, recordings, synth

pytestmark = pytest.mark.gpu

# four recordings with three distinct lengths and one too short for a window, in two shards
LENGTHS = [FIX[0], FIX[3], 200, FIX[0], FIX[2]]
BUDGET = FIX[0] + FIX[3] + 200
K, R = 5, 48
GRID = np.linspace(0.0, 2.0, R)
SKIP = _lib.TDA_WIN_DEGENERATE | _lib.TDA_WIN_TOO_LARGE


def test_ragged_pass_landscapes(ctx):
    import torch
    dev = torch.device("cuda", ctx.device)
    rng = np.random.default_rng(41)
    raws = [_raw(rng, L) for L in LENGTHS]
    envs = [_env(rng, L) for L in LENGTHS]
    xh, _ = preprocess.pack_recordings(raws)
    eh, _ = preprocess.pack_recordings(envs)
    plain = recordings.RaggedRecordingPass(LENGTHS, None, dev, shard_samples=BUDGET, n_sets=2, ctx=ctx)
    assert plain.plan.shards == [(0, 3), (3, 5)] and plain.empty.tolist() == [2]
    rows = plain.run(xh, eh).numpy().copy()
    assert plain.land_h is None
    rp = recordings.RaggedRecordingPass(LENGTHS, None, dev, shard_samples=BUDGET, n_sets=2, ctx=ctx, landscapes=(GRID, K))
    got = rp.run(xh, eh).numpy().copy()
    land = rp.land_h.numpy().copy()
    assert got.tobytes() == rows.tobytes()
    assert land.shape == (5, 5, 3, K + 1, R)
    assert np.isnan(land[2]).all()
    alone = {}                                                      # one pass per length
    for r, L in enumerate(LENGTHS):
        if r == 2:
            continue
        if L not in alone:
            alone[L] = recordings.RaggedRecordingPass([L], None, dev, n_sets=1, ctx=ctx, landscapes=(GRID, K))
        one = alone[L]
        x1, _ = preprocess.pack_recordings(raws[r:r + 1])
        e1, _ = preprocess.pack_recordings(envs[r:r + 1])
        rows1 = one.run(x1, e1).numpy()
        assert np.array_equal(rows1[0], rows[r], equal_nan=True)
        assert np.isfinite(one.land_h.numpy()).all()
        assert one.land_h.numpy()[0].tobytes() == land[r].tobytes(), r
    live = [0, 1, 3, 4]
    lam, beta = land[live][:, :, :, :K], land[live][:, :, :, K]
    assert (lam[:, :, :, :-1] >= lam[:, :, :, 1:]).all() and (lam >= 0).all() and lam.any()
    assert (beta >= 0).all() and (beta[:, :, 0, 0] >= 1).all()      # EEG H0 at t = 0: every birth is 0


def test_run_step_with_landscapes(ctx):
    import torch
    dev = torch.device("cuda", ctx.device)
    seg_off = np.array([0, 3, 6], np.int32)                         # two groups of three windows
    n_win = 6
    eeg = torch.from_numpy(synth.eeg_windows(n_win, seed=3, windows_per_recording=3)).to(dev)
    aud = torch.from_numpy(synth.audio_windows(n_win, "alpha", seed=4)).to(dev)
    plain = pipeline.Workspace(n_win, seg_off, dev)
    want = pipeline.run_step(eeg, aud, plain, ctx=ctx).cpu().numpy().copy()
    assert plain.land is None
    ws = pipeline.Workspace(n_win, seg_off, dev, landscapes=(GRID, K))
    got = pipeline.run_step(eeg, aud, ws, ctx=ctx).cpu().numpy().copy()
    torch.cuda.synchronize()
    assert got.tobytes() == want.tobytes()
    land = ws.land.cpu().numpy().copy()
    assert land.shape == (2, 3, K + 1, R)
    e0, e1 = ws.eeg.to_lists()
    _, a1 = ws.aud.to_lists()
    st = ws.aud.status.cpu().numpy()
    assert np.array_equal(land[:, 0], lr.lists_mean(e0, GRID, K, seg_off), equal_nan=True)
    assert np.array_equal(land[:, 1], lr.lists_mean(e1, GRID, K, seg_off), equal_nan=True)
    assert np.array_equal(land[:, 2], lr.lists_mean(a1, GRID, K, seg_off, status=st, skip_mask=SKIP), equal_nan=True)
    assert np.isfinite(land[:, :2]).all() and land[:, :, :K].any()
    # a view over the first group, and the EEG half alone
    v = ws.view(seg_off[:2])
    pipeline.run_step(eeg[:3], aud[:3], v, ctx=ctx)
    assert v.land.shape == (1, 3, K + 1, R) and np.array_equal(v.land.cpu().numpy(), land[:1], equal_nan=True)
    fs = pipeline.Workspace(n_win, seg_off, dev, landscapes=(GRID, K))
    pipeline.run_features_step(eeg, fs, ctx=ctx)
    assert np.array_equal(fs.land.cpu().numpy()[:, :2], land[:, :2])
    # through the lanes: captured once, replayed once; the same bytes
    lanes = pipeline.Lanes(1, n_win, seg_off, dev, graph=True, landscapes=(GRID, K))
    for rnd in range(2):
        b = lanes.submit(eeg, aud, ctx=ctx, post=lambda r: r.clone())
        lanes.drain()
        torch.cuda.synchronize()
        assert b.result().cpu().numpy().tobytes() == want.tobytes(), rnd
        assert lanes.ws[0].land.cpu().numpy().tobytes() == land.tobytes(), rnd
        lanes.ws[0].land.fill_(-7.0)                                # the replay has to write it again
    assert len(lanes.graphs) == 1
