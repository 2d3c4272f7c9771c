"""
frechet=(cap, max_iter) through the step and the recording passes: the rows stay what they are; ws.fm is
engine.frechet_mean_dev applied to the step's own diagrams and masks, packed as (3, cap + 2, 2) per group -- the mean with
NaN beyond its count, [count, variance], [iterations, status]; fm_h holds, per recording, the group's block, NaN for a
recording without a window.
"""
import numpy as np
import pytest

from tda_eeg_audio_amd import _lib, engine, pipeline, preprocess, recordings, synth

pytestmark = pytest.mark.gpu

CAP, ITERS = 256, 24
SKIP = _lib.TDA_WIN_DEGENERATE | _lib.TDA_WIN_TOO_LARGE


def _block(ws, rows, cnt, status, mask, ctx):
    """The (n_seg, CAP + 2, 2) block of one diagram set from engine.frechet_mean_dev."""
    import torch
    mean, mc, var, it, st = (t.cpu().numpy() for t in engine.frechet_mean_dev(rows, cnt, seg_off_t=ws.seg_off, status_t=status,
                                                                           skip_mask=mask, max_iter=ITERS, cap_out=CAP, ctx=ctx))
    torch.cuda.synchronize()
    mean[np.arange(CAP)[None, :] >= mc[:, None]] = np.nan
    tail = np.stack([np.stack([mc, var], 1), np.stack([it, st], 1)], 1).astype(np.float64)
    return np.concatenate([mean, tail], 1)


def test_run_step_with_frechet(ctx):
    import torch
    dev = torch.device("cuda", ctx.device)
    seg_off = np.array([0, 3, 6, 7], np.int32)                      # groups of three, three and one window
    n_win = 7
    eeg = torch.from_numpy(synth.eeg_windows(n_win, seed=3, windows_per_recording=3)).to(dev)
    aud = torch.from_numpy(synth.audio_windows(n_win, "alpha", seed=4)).to(dev)
    plain = pipeline.Workspace(n_win, seg_off, dev)
    want = pipeline.run_step(eeg, aud, plain, ctx=ctx).cpu().numpy().copy()
    flags = plain.seg_flags.cpu().numpy().copy()
    assert plain.fm is None
    ws = pipeline.Workspace(n_win, seg_off, dev, frechet=(CAP, ITERS))
    assert [o.name for o in ws.outputs] == ["fm"]
    got = pipeline.run_step(eeg, aud, ws, ctx=ctx).cpu().numpy().copy()
    torch.cuda.synchronize()
    assert got.tobytes() == want.tobytes() and np.array_equal(ws.seg_flags.cpu().numpy(), flags)
    fm = ws.fm.cpu().numpy().copy()
    assert fm.shape == (3, 3, CAP + 2, 2)
    sets = [(ws.eeg.h0, ws.eeg.c0, None, 0), (ws.eeg.h1, ws.eeg.c1, None, 0), (ws.aud.h1, ws.aud.c1, ws.aud.status, SKIP)]
    for s, (rows, cnt, status, mask) in enumerate(sets):
        assert np.array_equal(fm[:, s], _block(ws, rows, cnt, status, mask, ctx), equal_nan=True), s
    count, var, iters, status = fm[:, :, CAP, 0], fm[:, :, CAP, 1], fm[:, :, CAP + 1, 0], fm[:, :, CAP + 1, 1]
    assert (status[:, :2] == 0).all() and (count[:, 0] == 46).all()             # EEG H0: 46 finite rows in every window
    assert (var[:2, :2] > 0).all() and (iters[:2, :2] >= 2).all()
    assert (var[2, :2] == 0).all() and (iters[2, :2] == 1).all()                # a group of one window is that window
    e0, _ = ws.eeg.to_lists()
    d = np.asarray(e0[6], dtype=np.float64)
    assert np.array_equal(fm[2, 0, :46], d[np.isfinite(d).all(axis=1)])
    # a view over the first group, and the EEG half alone
    v = ws.view(seg_off[:2])
    pipeline.run_step(eeg[:3], aud[:3], v, ctx=ctx)
    assert v.fm.shape == (1, 3, CAP + 2, 2) and np.array_equal(v.fm.cpu().numpy(), fm[:1], equal_nan=True)
    fs = pipeline.Workspace(n_win, seg_off, dev, frechet=(CAP, ITERS))
    pipeline.run_features_step(eeg, fs, ctx=ctx)
    assert np.array_equal(fs.fm.cpu().numpy()[:, :2], fm[:, :2], equal_nan=True)


def test_recording_pass_frechet(ctx):
    import torch
    dev = torch.device("cuda", ctx.device)
    rng = np.random.default_rng(52)
    n_rec, L = 2, 1500
    raw = rng.standard_normal((n_rec, 47, L)) + 0.5 * rng.standard_normal((n_rec, 1, L))
    env = np.abs(rng.standard_normal((n_rec, L))).cumsum(axis=1) * 0.01 + np.abs(rng.standard_normal((n_rec, L)))
    raw_h, env_h = torch.from_numpy(raw).pin_memory(), torch.from_numpy(env).pin_memory()
    plain = recordings.RecordingPass(L, 2, dev, ctx=ctx)
    rows = plain.run(raw_h, env_h).numpy().copy()
    assert plain.fm_h is None
    rp = recordings.RecordingPass(L, 2, dev, ctx=ctx, frechet=(CAP, ITERS))
    got = rp.run(raw_h, env_h).numpy().copy()
    fmh = rp.fm_h.numpy().copy()
    assert got.tobytes() == rows.tobytes() and fmh.shape == (2, 5, 3, CAP + 2, 2)
    assert (fmh[:, :, :2, CAP + 1, 1] == 0).all() and (fmh[:, :, 0, CAP, 0] == 46).all()
    assert np.isfinite(fmh[:, :, :2, CAP]).all() and (fmh[:, :, :2, CAP, 1] > 0).all()
    one = recordings.RecordingPass(L, 1, dev, ctx=ctx, frechet=(CAP, ITERS))
    for r in range(n_rec):                                          # the group in front: a recording alone gives its block
        rows1 = one.run(raw_h[r:r + 1], env_h[r:r + 1]).numpy()
        assert rows1[0].tobytes() == rows[r].tobytes()
        assert one.fm_h.numpy()[0].tobytes() == fmh[r].tobytes(), r


def test_ragged_pass_frechet(ctx):
    import torch
    from test_gpu_ragged import _env, _raw
    dev = torch.device("cuda", ctx.device)
    rng = np.random.default_rng(53)
    lengths = [1500, 200, 1200]                                     # the middle one too short for a window
    raws, envs = [_raw(rng, L) for L in lengths], [_env(rng, L) for L in lengths]
    xh, _ = preprocess.pack_recordings(raws)
    eh, _ = preprocess.pack_recordings(envs)
    rows = recordings.RaggedRecordingPass(lengths, None, dev, shard_samples=1700, n_sets=2, ctx=ctx).run(xh, eh).numpy().copy()
    rp = recordings.RaggedRecordingPass(lengths, None, dev, shard_samples=1700, n_sets=2, ctx=ctx, frechet=(CAP, ITERS))
    got = rp.run(xh, eh).numpy().copy()
    fmh = rp.fm_h.numpy().copy()
    assert np.array_equal(got, rows, equal_nan=True) and fmh.shape == (3, 5, 3, CAP + 2, 2)
    assert np.isnan(fmh[1]).all()
    assert (fmh[[0, 2]][:, :, 0, CAP, 0] == 46).all() and (fmh[[0, 2]][:, :, :2, CAP + 1, 1] == 0).all()
    one = recordings.RaggedRecordingPass([1200], None, dev, n_sets=1, ctx=ctx, frechet=(CAP, ITERS))
    x1, _ = preprocess.pack_recordings(raws[2:])
    e1, _ = preprocess.pack_recordings(envs[2:])
    one.run(x1, e1)
    assert one.fm_h.numpy()[0].tobytes() == fmh[2].tobytes()
