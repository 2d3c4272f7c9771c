"""
sliced=dirs through the step and the recording passes: `result` and the rows stay what they are; ws.s0 / ws.s1 are the
sliced Wasserstein distances of the step's own diagram pairs (tests/sliced_ref.py, within the contract's bound), ws.slc
their per-group nanmean under the rule of ws.bott; slc_h (n_rec, n_bands, 2) holds, per recording, the values the same
recording gives when it runs alone through a pass of its own, NaN for a recording without a window.
"""
import numpy as np
import pytest

import sliced_ref as sr
from test_gpu_ragged import FIX, _env, _raw
from tda_eeg_audio_amd import _lib, pipeline, preprocess, recordings, synth, utils

pytestmark = pytest.mark.gpu

DIRS = utils.default_directions(16)
# four recordings with three distinct lengths and one too short for a window, in two shards
LENGTHS = [FIX[0], FIX[3], 200, FIX[0], FIX[2]]
BUDGET = FIX[0] + FIX[3] + 200


def _long_tau_window():
    """An audio window whose autocorrelation stays positive up to lag 123 and is negative at 124 (a slow downward ramp,
    one large spike up at 0 and one down at 124): tau = 124 leaves a Takens cloud of one point, TDA_WIN_DEGENERATE."""
    x = -0.001 * np.arange(250.0)
    x[0] += 1000.0
    x[124] -= 1000.0
    return x


def test_run_step_with_sliced(ctx):
    """20 windows in six groups; group 1 is ONE window and it is degenerate (tau is decided per group, so a degenerate
    window takes its whole group along: the group's means are NaN, those of the other groups run over all their windows)."""
    import torch
    dev = torch.device("cuda", ctx.device)
    n_win = 20
    seg_off = np.array([0, 4, 5, 8, 12, 16, 20], np.int32)
    eeg = torch.from_numpy(synth.eeg_windows(n_win, seed=3, windows_per_recording=4)).to(dev)
    aud_h = synth.audio_windows_all_bands(n_win // 5, seed=4)[0].copy()
    aud_h[4] = _long_tau_window()
    aud = torch.from_numpy(aud_h).to(dev)
    plain = pipeline.Workspace(n_win, seg_off, dev)
    want = pipeline.run_step(eeg, aud, plain, ctx=ctx).cpu().numpy().copy()
    assert plain.slc is None and plain.s0 is None
    ws = pipeline.Workspace(n_win, seg_off, dev, sliced=DIRS)
    got = pipeline.run_step(eeg, aud, ws, ctx=ctx).cpu().numpy()
    torch.cuda.synchronize()
    assert got.tobytes() == want.tobytes()
    status = ws.aud.status.cpu().numpy()
    keep = (status & (_lib.TDA_WIN_DEGENERATE | _lib.TDA_WIN_TOO_LARGE)) == 0
    assert status[4] & _lib.TDA_WIN_DEGENERATE and not keep[4] and keep.sum() >= 15
    e0, e1 = ws.eeg.to_lists()
    a0, a1 = ws.aud.to_lists()
    s0, s1 = ws.s0.cpu().numpy(), ws.s1.cpu().numpy()
    assert (ws.ss0.cpu().numpy() == 0).all() and (ws.ss1.cpu().numpy() == 0).all()
    for s, ea, au in ((s0, e0, a0), (s1, e1, a1)):
        ref = np.array([sr.sliced_wasserstein(a, b, DIRS) for a, b in zip(ea, au)])
        N = np.array([sr.n_points(a, b) for a, b in zip(ea, au)])
        err, tol = np.abs(s - ref), sr.tolerance(N, len(DIRS), ref)
        print("largest error / bound:", float(np.max(err / np.maximum(tol, 1e-300))), "N up to", int(N.max()))
        assert (err <= tol).all() and (ref[keep] > 0).all()
    slc = ws.slc.cpu().numpy()
    assert slc.shape == (6, pipeline.SLC_COLS)
    assert np.isnan(slc[1]).all() and np.isfinite(slc[[0, 2, 3, 4, 5]]).any()
    for g in range(6):
        sl = slice(seg_off[g], seg_off[g + 1])
        if not keep[sl].any():
            assert np.isnan(slc[g]).all()
        else:
            assert slc[g, 0] == np.nanmean(s0[sl][keep[sl]]) and slc[g, 1] == np.nanmean(s1[sl][keep[sl]])
    # a view over the first groups computes the same values
    v = ws.view(seg_off[:4])
    pipeline.run_step(eeg[:8], aud[:8], v, ctx=ctx)
    torch.cuda.synchronize()
    assert np.array_equal(v.slc.cpu().numpy(), slc[:3], equal_nan=True) and v.s0.shape[0] == 8
    with pytest.raises(_lib.TdaError):
        pipeline.Workspace(n_win, seg_off, dev, sliced=np.zeros((2, 3)))
    with pytest.raises(_lib.TdaError):
        pipeline.Workspace(n_win, seg_off, dev, sliced=[[np.nan, 1.0]])


def test_ragged_pass_sliced(ctx):
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
    assert plain.slc_h is None
    rp = recordings.RaggedRecordingPass(LENGTHS, None, dev, shard_samples=BUDGET, n_sets=2, ctx=ctx, sliced=DIRS)
    got = rp.run(xh, eh).numpy().copy()
    slc = rp.slc_h.numpy().copy()
    assert got.tobytes() == rows.tobytes()
    assert slc.shape == (5, 5, 2)
    assert np.isnan(slc[2]).all()
    alone = {}                                                      # one pass per length
    for r, L in enumerate(LENGTHS):
        if r == 2:
            continue
        if L not in alone:
            alone[L] = recordings.RaggedRecordingPass([L], None, dev, n_sets=1, ctx=ctx, sliced=DIRS)
        one = alone[L]
        x1, _ = preprocess.pack_recordings(raws[r:r + 1])
        e1, _ = preprocess.pack_recordings(envs[r:r + 1])
        rows1 = one.run(x1, e1).numpy()
        assert np.array_equal(rows1[0], rows[r], equal_nan=True)
        assert np.isfinite(one.slc_h.numpy()).all()
        assert one.slc_h.numpy()[0].tobytes() == slc[r].tobytes(), r
    # Every projection onto a unit direction is 1-Lipschitz, and an optimal Wasserstein matching induces a matching of A'
    # and B' (a matched pair and the pair of its images cost at most twice the pair, a point sent to the diagonal meets
    # its own image at the same cost): every L_k, their mean, and the means over the same windows are at most twice the
    # Wasserstein means of the rows.  default_directions has unit rows to rounding.
    live = [0, 1, 3, 4]
    assert (slc[live] > 0).all() and (slc[live] <= 2 * rows[live][:, :, :2] * (1 + 1e-9)).all()


def test_recording_pass_sliced(ctx):
    import torch
    dev = torch.device("cuda", ctx.device)
    rng = np.random.default_rng(42)
    n_rec, L = 2, 1500
    raw = rng.standard_normal((n_rec, 47, L)) + 0.5 * rng.standard_normal((n_rec, 1, L))
    env = np.abs(rng.standard_normal((n_rec, L))).cumsum(axis=1) * 0.01 + np.abs(rng.standard_normal((n_rec, L)))
    raw_h, env_h = torch.from_numpy(raw).pin_memory(), torch.from_numpy(env).pin_memory()
    rows = recordings.RecordingPass(L, 2, dev, ctx=ctx).run(raw_h, env_h).numpy().copy()
    rp = recordings.RecordingPass(L, 2, dev, ctx=ctx, sliced=DIRS)
    got = rp.run(raw_h, env_h).numpy().copy()
    slc = rp.slc_h.numpy().copy()
    assert got.tobytes() == rows.tobytes() and slc.shape == (2, 5, 2) and np.isfinite(slc).all()
    assert (slc > 0).all() and (slc <= 2 * rows[:, :, :2] * (1 + 1e-9)).all()
    one = recordings.RecordingPass(L, 1, dev, ctx=ctx, sliced=DIRS)
    for r in range(n_rec):
        rows1 = one.run(raw_h[r:r + 1], env_h[r:r + 1]).numpy()
        assert rows1[0].tobytes() == rows[r].tobytes()
        assert one.slc_h.numpy()[0].tobytes() == slc[r].tobytes(), r
