"""
takens=(dim, subsample, n_perm) through the step, the lanes and RecordingPass: the audio stage runs on greedy landmarks
and everything downstream takes its diagrams as it takes any others.  Checked as bytes against the engine calls composed
by hand; the default Workspace beside it keeps calling takens_rips_dev as before.  Last, the stability bound on the GPU.
"""
import numpy as np
import pytest

from tda_eeg_audio_amd import _lib, engine, pipeline, recordings, synth

pytestmark = pytest.mark.gpu

TAKENS = (3, 1, 128)


def _slow_window(seed):
    """A slow sinusoid with a little noise: tau = 76 (oracle.port.compute_tau), so the whole cloud has 98 points."""
    return np.sin(2 * np.pi * np.arange(250) / 300) + 0.05 * np.random.default_rng(300 + seed).standard_normal(250)


def _by_hand(aud, tau_win, ctx, takens=TAKENS):
    """The audio stage composed from the two engine calls: landmarks, then the cloud Rips on them, H1 in ripser's order."""
    import torch
    dim, sub, n_perm = takens
    lm = engine.takens_landmarks_dev(aud, tau_win, dim=dim, subsample=sub, n_perm=n_perm, ctx=ctx)
    n = aud.shape[0]
    out = engine.DeviceDiagrams(n, _lib.MAX_POINTS, engine.DEFAULT_H1_CAP, aud.device)
    ctx.check(ctx.lib.tda_cloud_rips_batch_dev(ctx.h, engine._tp(lm.lm), engine._tp(lm.n_lm), n, n_perm, dim, 0,
                                               float(engine.MAX_EDGE_LENGTH), engine._tp(out.h0), out.h0_cap, engine._tp(out.c0),
                                               engine._tp(out.h1), out.h1_cap, engine._tp(out.c1), engine._tp(out.status),
                                               engine._stream()))
    torch.cuda.synchronize()
    return out, lm


def _same_diagrams(a, b):
    for name in ("c0", "c1", "status"):
        assert np.array_equal(getattr(a, name).cpu().numpy(), getattr(b, name).cpu().numpy()), name
    c0, c1 = a.c0.cpu().numpy(), a.c1.cpu().numpy()
    h0a, h0b, h1a, h1b = (t.cpu().numpy() for t in (a.h0, b.h0, a.h1, b.h1))
    for w in range(len(c0)):
        assert h0a[w, :c0[w]].tobytes() == h0b[w, :c0[w]].tobytes(), w
        assert h1a[w, :min(c1[w], a.h1_cap)].tobytes() == h1b[w, :min(c1[w], a.h1_cap)].tobytes(), w


def _check_ws(ws, eeg_diagrams, aud, ctx):
    import torch
    torch.cuda.synchronize()
    want, lm = _by_hand(aud, ws.tau_win, ctx)
    _same_diagrams(ws.aud, want)
    assert np.array_equal(ws.aud.n_points.cpu().numpy(), lm.n_lm.cpu().numpy())
    for name in ("lm", "idx", "lam", "r_cover", "n_lm", "n_full"):
        assert getattr(ws.lm, name).cpu().numpy().tobytes() == getattr(lm, name).cpu().numpy().tobytes(), name
    e = eeg_diagrams
    w0, _ = engine.wasserstein_dev(e.h0, e.c0, want.h0, want.c0, ctx=ctx)
    w1, _ = engine.wasserstein_dev(e.h1, e.c1, want.h1, want.c1, ctx=ctx)
    torch.cuda.synchronize()
    assert ws.w0.cpu().numpy().tobytes() == w0.cpu().numpy().tobytes()
    assert ws.w1.cpu().numpy().tobytes() == w1.cpu().numpy().tobytes()
    return lm


def test_run_step_and_lanes_with_landmarks(ctx):
    """15 windows in five groups: a slow sinusoid (tau 76: 98 points, the identity case), then one band per group with
    tau from 11 down to 2 (228 to 246 points), in one batch."""
    import torch
    dev = torch.device("cuda", ctx.device)
    n_win = 15
    seg_off = np.array([0, 3, 6, 9, 12, 15], np.int32)
    eeg = torch.from_numpy(synth.eeg_windows(n_win, seed=5, windows_per_recording=3)).to(dev)
    aud_h = synth.audio_windows_all_bands(3, seed=6)[0].copy()
    aud_h[:3] = [_slow_window(k) for k in range(3)]
    aud = torch.from_numpy(aud_h).to(dev)
    # the default Workspace: the audio stage is takens_rips_dev as it always was
    plain = pipeline.Workspace(n_win, seg_off, dev)
    assert plain.lm is None and plain.takens is None
    res_plain = pipeline.run_step(eeg, aud, plain, ctx=ctx).cpu().numpy().copy()
    torch.cuda.synchronize()
    old = engine.takens_rips_dev(aud, plain.tau_win, ctx=ctx)
    torch.cuda.synchronize()
    _same_diagrams(plain.aud, old)
    assert np.array_equal(plain.aud.n_points.cpu().numpy(), old.n_points.cpu().numpy())
    # the landmark Workspace, eager
    ws = pipeline.Workspace(n_win, seg_off, dev, takens=TAKENS)
    assert ws.takens == TAKENS and ws.lm.lm.shape == (n_win, 128, 3)
    res = pipeline.run_step(eeg, aud, ws, ctx=ctx).cpu().numpy().copy()
    lm = _check_ws(ws, ws.eeg, aud, ctx)
    n_full, n_lm, rc = (t.cpu().numpy() for t in (lm.n_full, lm.n_lm, lm.r_cover))
    tau = ws.tau_win.cpu().numpy()
    assert np.array_equal(n_full, 250 - 2 * tau) and np.array_equal(n_lm, np.minimum(n_full, 128))
    assert (n_full > 128).any() and (n_full <= 128).any() and (rc[n_full > 128] > 0).all() and not rc[n_full <= 128].any()
    assert (ws.aud.status.cpu().numpy() == 0).all()
    # tau, n_windows and the EEG features of `result` do not depend on the audio stage
    assert np.array_equal(res[:, 2:], res_plain[:, 2:]) and np.isfinite(res[:, :2]).all()
    _same_diagrams(ws.eeg, plain.eeg)
    # a view over the first groups
    v = ws.view(seg_off[:3])
    pipeline.run_step(eeg[:6], aud[:6], v, ctx=ctx)
    torch.cuda.synchronize()
    assert v.lm.n_win == 6 and np.array_equal(v.result.cpu().numpy(), res[:2])
    # the same step captured in a graph through the lanes, replayed once
    lanes = pipeline.Lanes(1, n_win, seg_off, dev, graph=True, takens=TAKENS)
    for rnd in range(2):
        b = lanes.submit(eeg, aud, ctx=ctx, post=lambda r: r.clone())
        lanes.drain()
        torch.cuda.synchronize()
        assert b.result().cpu().numpy().tobytes() == res.tobytes(), rnd
        _check_ws(lanes.ws[0], ws.eeg, aud, ctx)
        lanes.ws[0].lm.r_cover.fill_(-7.0)                          # the replay has to write them again
        lanes.ws[0].w1.fill_(-7.0)
    assert len(lanes.graphs) == 1
    with pytest.raises(_lib.TdaError):
        pipeline.Workspace(n_win, seg_off, dev, takens=(3, 1, 129))


def test_recording_pass_with_landmarks(ctx):
    import torch
    dev = torch.device("cuda", ctx.device)
    rng = np.random.default_rng(42)
    n_rec, L = 2, 1500
    raw = rng.standard_normal((n_rec, 47, L)) + 0.5 * rng.standard_normal((n_rec, 1, L))
    env = np.abs(rng.standard_normal((n_rec, L))).cumsum(axis=1) * 0.01 + np.abs(rng.standard_normal((n_rec, L)))
    raw_h, env_h = torch.from_numpy(raw).pin_memory(), torch.from_numpy(env).pin_memory()
    rows_plain = recordings.RecordingPass(L, 2, dev, ctx=ctx).run(raw_h, env_h).numpy().copy()
    rp = recordings.RecordingPass(L, 2, dev, ctx=ctx, takens=TAKENS)
    rows = rp.run(raw_h, env_h).numpy().copy()
    assert rows.shape == rows_plain.shape and np.array_equal(rows[..., 2:], rows_plain[..., 2:]) and np.isfinite(rows).all()
    # one shard: its windows and its Workspace are still in the first buffer set
    st = rp.set[0]
    ws = st["ws"]
    lm = _check_ws(ws, ws.eeg, st["aw"], ctx)
    assert (lm.n_full.cpu().numpy() > 128).any()
    res = ws.result.cpu().numpy()
    assert np.array_equal(rows, res.reshape(5, 2, -1).transpose(1, 0, 2))
    # every recording alone: the same rows
    one = recordings.RecordingPass(L, 1, dev, ctx=ctx, takens=TAKENS)
    for r in range(n_rec):
        assert one.run(raw_h[r:r + 1], env_h[r:r + 1]).numpy()[0].tobytes() == rows[r].tobytes()


def test_ragged_pass_with_landmarks(ctx):
    """Recordings of different lengths, one of them without a window, in two shards (views of one Workspace)."""
    import torch
    from test_gpu_ragged import FIX, _env, _raw
    from tda_eeg_audio_amd import preprocess
    dev = torch.device("cuda", ctx.device)
    lengths = [FIX[0], 200, FIX[0]]
    rng = np.random.default_rng(44)
    raws = [_raw(rng, L) for L in lengths]
    envs = [_env(rng, L) for L in lengths]
    xh, _ = preprocess.pack_recordings(raws)
    eh, _ = preprocess.pack_recordings(envs)
    kw = dict(shard_samples=FIX[0] + 200, n_sets=2, ctx=ctx)
    rows_plain = recordings.RaggedRecordingPass(lengths, None, dev, **kw).run(xh, eh).numpy().copy()
    rp = recordings.RaggedRecordingPass(lengths, None, dev, takens=TAKENS, **kw)
    assert rp.plan.shards == [(0, 2), (2, 3)] and rp.empty.tolist() == [1]
    rows = rp.run(xh, eh).numpy().copy()
    assert np.array_equal(rows[..., 2:], rows_plain[..., 2:], equal_nan=True)
    assert np.isnan(rows[1, :, :2]).all() and np.isfinite(rows[[0, 2]]).all()
    # the last shard is still in its buffer set: its view against the composition by hand
    st = rp.set[1]
    v = st["views"][1]
    lm = _check_ws(v, v.eeg, st["aw"][:v.n_win], ctx)
    assert (lm.n_full.cpu().numpy() > 128).any()
    # a recording alone: the same rows
    one = recordings.RaggedRecordingPass([FIX[0]], None, dev, n_sets=1, ctx=ctx, takens=TAKENS)
    for r in (0, 2):
        x1, _ = preprocess.pack_recordings(raws[r:r + 1])
        e1, _ = preprocess.pack_recordings(envs[r:r + 1])
        assert one.run(x1, e1).numpy()[0].tobytes() == rows[r].tobytes(), r


def test_stability_bound_on_the_gpu(ctx):
    """Whole clouds of at most 124 points (subsample 2) against 32 landmarks: for H0 and H1 the bottleneck distance
    (engine.bottleneck_batch) is at most 2 * r_cover; 1e-6 covers the float32 rounding of diagram values up to 2."""
    import torch
    dev = torch.device("cuda", ctx.device)
    wins = synth.audio_windows_all_bands(4, seed=12)[0]
    aud = torch.from_numpy(wins.copy()).to(dev)
    tau = engine.tau_dev(aud, 125, ctx=ctx)
    tau[0] = 100                                                    # 25 points: fewer than the landmarks asked for
    full = engine.takens_rips_dev(aud, tau, subsample=2, ctx=ctx)
    land, lm = engine.takens_rips_landmarks_dev(aud, tau, subsample=2, n_perm=32, ctx=ctx)
    torch.cuda.synchronize()
    n_full, rc = lm.n_full.cpu().numpy(), lm.r_cover.cpu().numpy()
    assert np.array_equal(n_full, full.n_points.cpu().numpy()) and (n_full <= 128).all() and (n_full > 32).sum() == 19
    assert (full.status.cpu().numpy() == 0).all() and (land.status.cpu().numpy() == 0).all()
    for k, (ra, ca, rb, cb) in enumerate(((land.h0, land.c0, full.h0, full.c0), (land.h1, land.c1, full.h1, full.c1))):
        B, st = engine.bottleneck_batch(ra.cpu().numpy(), ca.cpu().numpy(), rb.cpu().numpy(), cb.cpu().numpy(), ctx=ctx,
                                        want_status=True)
        print(f"H{k}: B / (2 r_cover) up to", float(np.nanmax(B[rc > 0] / (2 * rc[rc > 0]))))
        assert (st == 0).all() and (B <= 2 * rc + 1e-6).all()
        assert n_full[0] == 25 and B[0] == 0                        # the identity case: the same diagram
