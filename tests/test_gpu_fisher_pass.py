"""
fisher=sigma through the step and the recording passes: `result` and the rows stay what they are; ws.f0 / ws.f1 are the
persistence Fisher distances of the step's own diagram pairs, ws.pf their per-group nanmean under the rule of ws.bott;
pf_h (n_rec, n_bands, 2) holds, per recording, the values the same recording gives when it runs alone through a pass of
its own, NaN for a recording without a window.
"""
import numpy as np
import pytest

import fisher_ref as pf
from test_gpu_ragged import FIX, _env, _raw
from test_gpu_sliced_pass import _long_tau_window
from tda_eeg_audio_amd import _lib, engine, pipeline, preprocess, recordings, synth

pytestmark = pytest.mark.gpu

SIGMA = 0.1
LENGTHS = [FIX[0], FIX[3], 200, FIX[0], FIX[2]]
BUDGET = FIX[0] + FIX[3] + 200


def test_run_step_with_fisher(ctx):
    """20 windows in six groups; group 1 is ONE window and it is degenerate, so its means are NaN."""
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
    assert plain.pf is None and plain.f0 is None and plain.fisher is None
    ws = pipeline.Workspace(n_win, seg_off, dev, fisher=SIGMA)
    got = pipeline.run_step(eeg, aud, ws, ctx=ctx).cpu().numpy()
    torch.cuda.synchronize()
    assert got.tobytes() == want.tobytes()                              # `result`: the same bytes with the option on and off
    assert [o.name for o in ws.outputs] == ["pf"] and ws.fisher == SIGMA
    status = ws.aud.status.cpu().numpy()
    keep = (status & (_lib.TDA_WIN_DEGENERATE | _lib.TDA_WIN_TOO_LARGE)) == 0
    assert status[4] & _lib.TDA_WIN_DEGENERATE and not keep[4] and keep.sum() >= 15
    e0, e1 = ws.eeg.to_lists()
    a0, a1 = ws.aud.to_lists()
    f0, f1 = ws.f0.cpu().numpy(), ws.f1.cpu().numpy()
    assert (ws.fs0.cpu().numpy() == 0).all() and (ws.fs1.cpu().numpy() == 0).all()
    ninv = pf.args(SIGMA)
    for f, ea, au in ((f0, e0, a0), (f1, e1, a1)):
        ref = np.array([pf.distance_fsum(a, b, ninv) for a, b in zip(ea, au)])
        N = np.array([pf.n_points(a, b) for a, b in zip(ea, au)])
        err = np.abs(f - ref)
        print("q step pairs:", float(err.max() / pf.U), "N up to", int(N.max()))
        assert (err <= pf.tolerance(N)).all()
        assert (f[keep] > 0).all() and (f <= np.pi / 2).all()
    pfm = ws.pf.cpu().numpy()
    assert pfm.shape == (6, pipeline.PF_COLS)
    assert np.isnan(pfm[1]).all() and np.isfinite(pfm[[0, 2, 3, 4, 5]]).all()
    for g in range(6):
        sl = slice(seg_off[g], seg_off[g + 1])
        if not keep[sl].any():
            assert np.isnan(pfm[g]).all()
        else:
            assert pfm[g, 0] == np.nanmean(f0[sl][keep[sl]]) and pfm[g, 1] == np.nanmean(f1[sl][keep[sl]])
    # a view over the first groups computes the same values
    v = ws.view(seg_off[:4])
    pipeline.run_step(eeg[:8], aud[:8], v, ctx=ctx)
    torch.cuda.synchronize()
    assert np.array_equal(v.pf.cpu().numpy(), pfm[:3], equal_nan=True) and v.f0.shape[0] == 8 and v.fs1.shape[0] == 8
    with pytest.raises(ValueError):
        pipeline.Workspace(n_win, seg_off, dev, fisher=0.0)
    # through the lanes: captured once, replayed once; the same bytes
    lanes = pipeline.Lanes(1, n_win, seg_off, dev, graph=True, fisher=SIGMA)
    for rnd in range(2):
        b = lanes.submit(eeg, aud, ctx=ctx, post=lambda r: r.clone())
        lanes.drain()
        torch.cuda.synchronize()
        assert b.result().cpu().numpy().tobytes() == want.tobytes(), rnd
        assert lanes.ws[0].pf.cpu().numpy().tobytes() == pfm.tobytes(), rnd
        assert lanes.ws[0].f0.cpu().numpy().tobytes() == f0.tobytes(), rnd
        lanes.ws[0].pf.fill_(-7.0)                                  # the replay has to write it again
        lanes.ws[0].f0.fill_(-7.0)
    assert len(lanes.graphs) == 1


def test_ragged_pass_fisher(ctx):
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
    assert plain.pf_h is None
    rp = recordings.RaggedRecordingPass(LENGTHS, None, dev, shard_samples=BUDGET, n_sets=2, ctx=ctx, fisher=SIGMA)
    got = rp.run(xh, eh).numpy().copy()
    pfh = rp.pf_h.numpy().copy()
    assert got.tobytes() == rows.tobytes()
    assert pfh.shape == (5, 5, 2) and np.isnan(pfh[2]).all()                # the recording without a window
    live = [0, 1, 3, 4]
    assert np.isfinite(pfh[live]).all() and (pfh[live] > 0).all() and (pfh[live] <= np.pi / 2).all()
    # every recording alone through a pass of its own (one pass per length): the same bytes as inside the pass
    alone = {}
    for r in live:
        L = LENGTHS[r]
        if L not in alone:
            alone[L] = recordings.RaggedRecordingPass([L], None, dev, n_sets=1, ctx=ctx, fisher=SIGMA)
        one = alone[L]
        x1, _ = preprocess.pack_recordings(raws[r:r + 1])
        e1, _ = preprocess.pack_recordings(envs[r:r + 1])
        rows1 = one.run(x1, e1).numpy()
        assert np.array_equal(rows1[0], rows[r], equal_nan=True)
        assert one.pf_h.numpy()[0].tobytes() == pfh[r].tobytes(), r


def test_recording_pass_fisher(ctx):
    import torch
    dev = torch.device("cuda", ctx.device)
    rng = np.random.default_rng(42)
    n_rec, L = 2, 1500
    raw = rng.standard_normal((n_rec, 47, L)) + 0.5 * rng.standard_normal((n_rec, 1, L))
    env = np.abs(rng.standard_normal((n_rec, L))).cumsum(axis=1) * 0.01 + np.abs(rng.standard_normal((n_rec, L)))
    raw_h, env_h = torch.from_numpy(raw).pin_memory(), torch.from_numpy(env).pin_memory()
    plain = recordings.RecordingPass(L, 2, dev, ctx=ctx)
    rows = plain.run(raw_h, env_h).numpy().copy()
    assert plain.pf_h is None
    rp = recordings.RecordingPass(L, 2, dev, ctx=ctx, fisher=SIGMA)
    got = rp.run(raw_h, env_h).numpy().copy()
    pfh = rp.pf_h.numpy().copy()
    assert got.tobytes() == rows.tobytes() and pfh.shape == (2, 5, 2) and np.isfinite(pfh).all() and (pfh > 0).all()
    one = recordings.RecordingPass(L, 1, dev, ctx=ctx, fisher=SIGMA)
    for r in range(n_rec):
        rows1 = one.run(raw_h[r:r + 1], env_h[r:r + 1]).numpy()
        assert rows1[0].tobytes() == rows[r].tobytes()
        assert one.pf_h.numpy()[0].tobytes() == pfh[r].tobytes(), r
