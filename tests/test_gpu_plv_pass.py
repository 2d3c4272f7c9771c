"""
phase_locking=method through the step in its three EEG input modes, the lanes with a captured graph and the recording
passes.  ws.pl is compared, as bytes, with the same 24 numbers composed from the separate engine calls (plv_dist_dev ->
rips_dm_dev with its whole ladder and rows ordered in the call -> features_dev, wasserstein_dev against the step's audio
diagrams -> segment_nanmean_dev); `result` and every other output are the same bytes with the option on and off.
"""
import numpy as np
import pytest

from test_gpu_ragged import FIX, _env, _raw
from test_gpu_sliced_pass import _long_tau_window
from test_gpu_sublevel_pass import _inputs
from tda_eeg_audio_amd import _lib, engine, pipeline, preprocess, recordings

pytestmark = pytest.mark.gpu

N_CH, N_T, STEP = 47, 250, 62
LENGTHS = [FIX[0], FIX[3], 200, FIX[0], FIX[2]]
BUDGET = FIX[0] + FIX[3] + 200
SKIP = _lib.TDA_WIN_DEGENERATE | _lib.TDA_WIN_TOO_LARGE


def _compose(ws, eeg_t, method, ctx):
    """The 24 numbers of every group from the separate engine calls, and the per-window pieces."""
    import torch
    dist, _, st = engine.plv_dist_dev(eeg_t, method=method, ctx=ctx)
    dg = engine.rips_dm_dev(dist, ctx=ctx)
    f0, f1 = engine.features_dev(dg.h0, dg.c0, ctx=ctx), engine.features_dev(dg.h1, dg.c1, ctx=ctx)
    w0, s0 = engine.wasserstein_dev(dg.h0, dg.c0, ws.aud.h0, ws.aud.c0, ctx=ctx)
    w1, s1 = engine.wasserstein_dev(dg.h1, dg.c1, ws.aud.h1, ws.aud.c1, ctx=ctx)
    assert not st.any() and not dg.status.any()
    nan = torch.full((), float("nan"), dtype=torch.float64, device=eeg_t.device)
    out = (ws.aud.status & SKIP) != 0
    cols = [f0[:, k].contiguous() for k in range(11)] + [f1[:, k].contiguous() for k in range(11)]
    cols += [torch.where(out | (s0 != 0), nan, w0), torch.where(out | (s1 != 0), nan, w1)]
    pl = torch.stack([engine.segment_nanmean_dev(c, ws.seg_off, ctx=ctx) for c in cols], dim=1)
    torch.cuda.synchronize()
    return pl.cpu().numpy(), dict(dist=dist, dg=dg, f0=f0, f1=f1, w0=w0, w1=w1)


@pytest.mark.parametrize("method", [True, "standard"])
def test_step_fills_pl_in_three_input_modes(ctx, method):
    import torch
    dev = torch.device("cuda", ctx.device)
    rec, sel, seg_off, eeg, aud, start, ld = _inputs()
    aud = aud.copy()
    aud[4] = _long_tau_window()                                     # group 1 (one window): its audio cloud is degenerate
    n_win = len(sel)
    eeg_t, aud_t, rec_t = (torch.from_numpy(a).to(dev) for a in (eeg, aud, rec))
    modes = {"stacked": {}, "sliding": dict(eeg_sliding=(rec_t, N_T, STEP, torch.from_numpy(sel).to(dev))),
             "table": dict(eeg_table=(rec_t.view(-1), torch.from_numpy(start).to(dev), torch.from_numpy(ld).to(dev), N_T))}
    plain = pipeline.Workspace(n_win, seg_off, dev, bottleneck=True, sublevel=True)
    res0 = pipeline.run_step(eeg_t, aud_t, plain, ctx=ctx).cpu().numpy().copy()
    bott0, sl0 = plain.bott.cpu().numpy().copy(), plain.sl.cpu().numpy().copy()
    assert plain.pl is None and plain.pl_dist is None and plain.pl_dgm is None and plain.phase_locking is None
    assert [o.name for o in plain.outputs] == ["bott", "sl"]
    name_of = "euclidean" if method is True else method
    first = None
    for name, kw in modes.items():
        ws = pipeline.Workspace(n_win, seg_off, dev, bottleneck=True, sublevel=True, phase_locking=method)
        assert [o.name for o in ws.outputs] == ["bott", "sl", "pl"] and ws.pl.shape == (3, pipeline.PL_COLS)
        res = pipeline.run_step(eeg_t, aud_t, ws, ctx=ctx, **kw).cpu().numpy()
        torch.cuda.synchronize()
        assert res.tobytes() == res0.tobytes() and ws.bott.cpu().numpy().tobytes() == bott0.tobytes(), name
        assert ws.sl.cpu().numpy().tobytes() == sl0.tobytes(), name
        got = ws.pl.cpu().numpy()
        want, parts = _compose(ws, eeg_t, name_of, ctx)
        assert got.tobytes() == want.tobytes(), (name, np.abs(got - want).max())
        # the per-window pieces the workspace keeps: the same bytes as the separate calls'
        assert ws.pl_dist.cpu().numpy().tobytes() == parts["dist"].cpu().numpy().tobytes()
        assert (ws.pl_dgm.c1 == parts["dg"].c1).all() and (ws.pl_dgm.c0 == parts["dg"].c0).all()
        c1 = ws.pl_dgm.c1.cpu().numpy()
        a, b = ws.pl_dgm.h1.cpu().numpy(), parts["dg"].h1.cpu().numpy()
        assert all(a[w, :c1[w]].tobytes() == b[w, :c1[w]].tobytes() for w in range(n_win))      # ripser's H1 order
        assert ws.pl_f1.cpu().numpy().tobytes() == parts["f1"].cpu().numpy().tobytes()
        assert ws.pl_w1.cpu().numpy().tobytes() == parts["w1"].cpu().numpy().tobytes()
        assert not ws.pl_st.any() and not ws.pl_dgm.status.any() and (c1 > 0).all()
        # a degenerate audio group has NaN in columns 22 and 23 only
        status = ws.aud.status.cpu().numpy()
        assert (status[4] & _lib.TDA_WIN_DEGENERATE) and not (status[[0, 1, 2, 3, 5, 6, 7]] & SKIP).any()
        assert np.isnan(got[1, 22:]).all() and np.isfinite(got[1, :22]).all() and np.isfinite(got[[0, 2]]).all()
        # ... and the numpy statement of the means
        f0 = ws.pl_f0.cpu().numpy()
        for g in range(3):
            sl = slice(seg_off[g], seg_off[g + 1])
            assert np.allclose(got[g, :11], np.nanmean(f0[sl], axis=0), rtol=1e-13, atol=0)
        first = got if first is None else first
        assert got.tobytes() == first.tobytes(), name               # the three modes read the same samples
        if name == "stacked":
            v = ws.view(seg_off[:3])                                 # a view over the first two groups
            pipeline.run_step(eeg_t[:5], aud_t[:5], v, ctx=ctx)
            torch.cuda.synchronize()
            assert v.pl.cpu().numpy().tobytes() == got[:2].tobytes() and v.pl_dist.shape[0] == 5 and v.pl_dgm.n_win == 5
    # through the lanes: first passes only in the step (the stage's own Rips call keeps its ladder), captured once, replayed
    lanes = pipeline.Lanes(1, n_win, seg_off, dev, graph=True, bottleneck=True, sublevel=True, phase_locking=method)
    for rnd in range(3):
        b = lanes.submit(eeg_t, aud_t, ctx=ctx, post=lambda r: r.clone())
        lanes.drain()
        torch.cuda.synchronize()
        assert b.result().cpu().numpy().tobytes() == res0.tobytes(), rnd
        assert lanes.ws[0].pl.cpu().numpy().tobytes() == first.tobytes(), rnd
        assert lanes.ws[0].bott.cpu().numpy().tobytes() == bott0.tobytes(), rnd
        lanes.ws[0].pl.fill_(-7.0)                                  # the replay has to write it again
        lanes.ws[0].pl_dist.fill_(-7.0)
    assert len(lanes.graphs) == 1


def test_stage_counts_a_flagged_window_as_nan(ctx):
    """The stage alone after a clean step: window 6 gets an inf in one channel.  Its block goes to Rips as points on a line,
    the window leaves the means of group 2, the other groups keep their bytes."""
    import torch
    dev = torch.device("cuda", ctx.device)
    _, _, seg_off, eeg, aud, _, _ = _inputs()
    eeg_t, aud_t = torch.from_numpy(eeg).to(dev), torch.from_numpy(aud).to(dev)
    ws = pipeline.Workspace(len(aud), seg_off, dev, phase_locking="abs")
    pipeline.run_step(eeg_t, aud_t, ws, ctx=ctx)
    clean = ws.pl.cpu().numpy().copy()
    f0, w0 = ws.pl_f0.cpu().numpy().copy(), ws.pl_w0.cpu().numpy().copy()
    bad = eeg.copy()
    bad[6, 11, 249] = np.inf
    with ctx.deferred():
        pipeline._phase_locking_stage(ws, ctx, torch.from_numpy(bad).to(dev), None, None)
    torch.cuda.synchronize()
    got = ws.pl.cpu().numpy()
    assert ws.pl_st.cpu().numpy().tolist() == [0, 0, 0, 0, 0, 0, _lib.TDA_WIN_NOT_FINITE, 0]
    assert got[:2].tobytes() == clean[:2].tobytes() and np.isfinite(got).all()
    assert np.allclose(got[2, :11], np.nanmean(f0[[5, 7]], axis=0), rtol=1e-13, atol=0)
    assert np.isclose(got[2, 22], np.mean(w0[[5, 7]]), rtol=1e-13, atol=0)
    assert torch.equal(ws.pl_dist[6], ws.pl_line) and not torch.isnan(ws.pl_dist).any()


def test_recording_pass_phase_locking(ctx):
    import torch
    dev = torch.device("cuda", ctx.device)
    rng = np.random.default_rng(72)
    n_rec, L = 2, 1500
    raw = rng.standard_normal((n_rec, 47, L)) + 0.5 * rng.standard_normal((n_rec, 1, L))
    env = np.abs(rng.standard_normal((n_rec, L))).cumsum(axis=1) * 0.01 + np.abs(rng.standard_normal((n_rec, L)))
    raw_h, env_h = torch.from_numpy(raw).pin_memory(), torch.from_numpy(env).pin_memory()
    plain = recordings.RecordingPass(L, 2, dev, ctx=ctx)
    rows = plain.run(raw_h, env_h).numpy().copy()
    assert plain.pl_h is None and plain.phase_locking is None
    rp = recordings.RecordingPass(L, 2, dev, ctx=ctx, phase_locking=True)
    got = rp.run(raw_h, env_h).numpy().copy()
    plh = rp.pl_h.numpy().copy()
    assert rp.phase_locking == "euclidean" and got.tobytes() == rows.tobytes() and plh.shape == (2, 5, 24)
    assert np.isfinite(plh[..., :22]).all()
    # column 1 / 12: one essential H0 class, none in H1; column 0: 46 finite H0 rows; distances are not negative
    assert (plh[..., 0] == 46.0).all() and (plh[..., 1] == 1.0).all() and (plh[..., 12] == 0.0).all()
    assert (plh[..., 22:][np.isfinite(plh[..., 22:])] >= 0).all() and np.isfinite(plh[..., 22:]).any()
    one = recordings.RecordingPass(L, 1, dev, ctx=ctx, phase_locking="euclidean")
    for r in range(n_rec):
        rows1 = one.run(raw_h[r:r + 1], env_h[r:r + 1]).numpy()
        assert rows1[0].tobytes() == rows[r].tobytes()
        assert one.pl_h.numpy()[0].tobytes() == plh[r].tobytes(), r
    with pytest.raises(ValueError):
        recordings.RecordingPass(L, 1, dev, ctx=ctx, phase_locking="coherence")


def test_ragged_pass_phase_locking(ctx):
    import torch
    dev = torch.device("cuda", ctx.device)
    rng = np.random.default_rng(73)
    raws = [_raw(rng, L) for L in LENGTHS]
    envs = [_env(rng, L) for L in LENGTHS]
    xh, _ = preprocess.pack_recordings(raws)
    eh, _ = preprocess.pack_recordings(envs)
    plain = recordings.RaggedRecordingPass(LENGTHS, None, dev, shard_samples=BUDGET, n_sets=2, ctx=ctx)
    assert plain.plan.shards == [(0, 3), (3, 5)] and plain.empty.tolist() == [2]
    rows = plain.run(xh, eh).numpy().copy()
    assert plain.pl_h is None
    rp = recordings.RaggedRecordingPass(LENGTHS, None, dev, shard_samples=BUDGET, n_sets=2, ctx=ctx, phase_locking="sqrt")
    got = rp.run(xh, eh).numpy().copy()
    plh = rp.pl_h.numpy().copy()
    assert got.tobytes() == rows.tobytes()
    assert plh.shape == (5, 5, 24) and np.isnan(plh[2]).all()               # the recording without a window
    live = [0, 1, 3, 4]
    assert np.isfinite(plh[live][..., :22]).all() and (plh[live][..., 0] == 46.0).all()
    alone = {}
    for r in live:                                                          # alone through a pass of its own: the same bytes
        L = LENGTHS[r]
        if L not in alone:
            alone[L] = recordings.RaggedRecordingPass([L], None, dev, n_sets=1, ctx=ctx, phase_locking="sqrt")
        one = alone[L]
        x1, _ = preprocess.pack_recordings(raws[r:r + 1])
        e1, _ = preprocess.pack_recordings(envs[r:r + 1])
        rows1 = one.run(x1, e1).numpy()
        assert np.array_equal(rows1[0], rows[r], equal_nan=True)
        assert one.pl_h.numpy()[0].tobytes() == plh[r].tobytes(), r
