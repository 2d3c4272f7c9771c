"""
sublevel=True through engine.sublevel_features_dev, the step, the lanes and the recording passes.

The features of a sublevel-set diagram are compared with oracle.port.features of the reference diagram
(tests/sublevel_ref.py) at the project's feature bar, rtol 1e-12.  ws.sl is compared with the numpy
composition of those reference features: np.nanmean over the group's windows (columns 0..10, audio) and np.nanmean over
the windows of np.mean over the channels (columns 11..21, EEG).  Its tolerance is 2e-12 * M per entry, M the same
composition of the ABSOLUTE reference values: every term carries at most 1e-12 of its magnitude, the at most 47 + k
additions of a mean add (47 + k) * 2^-53 < 1e-14 of M, and mean_birth / mean_death of a zero-mean signal cancel, so the
bound cannot be relative to the mean itself.  `result` and every other output are the same bytes with the option on and off.
"""
import numpy as np
import pytest

import sublevel_ref as ref
from oracle import port
from test_gpu_ragged import FIX, _env, _raw
from tda_eeg_audio_amd import _lib, engine, pipeline, preprocess, recordings

pytestmark = pytest.mark.gpu

N_CH, N_T, STEP = 47, 250, 62
LENGTHS = [FIX[0], FIX[3], 200, FIX[0], FIX[2]]
BUDGET = FIX[0] + FIX[3] + 200


def _ref_features(sigs):
    """(n_sig, 11) reference features of the sublevel-set diagrams; NaN rows for signals with a non-finite sample."""
    out = np.full((sigs.shape[0], 11), np.nan)
    for s, x in enumerate(sigs):
        if np.isfinite(x).all():
            out[s] = port.features(ref.sublevel_union_find(x)[0])
    return out


def _assert_features(got, want):
    assert got.shape == want.shape
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    assert np.allclose(got[ok], want[ok], rtol=1e-12, atol=0), float(np.abs(got[ok] / want[ok] - 1)[want[ok] != 0].max())


@pytest.mark.parametrize("max_bytes, chunks", [(3 * 3 * 125 * 16, [3, 3, 1]), (1, [1] * 7), (engine.SL_SCRATCH_BYTES, [7])])
def test_features_over_chunks(ctx, max_bytes, chunks):
    """7 windows of 3 channels: a bound of three windows gives two full chunks and a last one that is not."""
    import torch
    dev = torch.device("cuda", ctx.device)
    rng = np.random.default_rng(70)
    sig = np.round(rng.standard_normal((7, 3, N_T)).cumsum(axis=2), 2)
    sig[2, 1, 17] = np.nan                                          # flagged: NaN features, its neighbours untouched
    sig[6, 2, 0] = -np.inf                                          # ... in the last, short chunk
    want = _ref_features(sig.reshape(21, N_T)).reshape(7, 3, 11)
    sc = engine.SublevelScratch(3, N_T, dev, max_bytes, n_win=7)
    assert [min(sc.chunk_windows, 7 - w) for w in range(0, 7, sc.chunk_windows)] == chunks and sc.n_chunks(7) == len(chunks)
    assert sc.dgm.shape == (sc.chunk_windows * 3, 125, 2)
    st = torch.full((7, 3), -5, dtype=torch.int32, device=dev)
    got = engine.sublevel_features_dev(torch.from_numpy(sig).to(dev), status_t=st, scratch=sc, ctx=ctx)
    torch.cuda.synchronize()
    _assert_features(got.cpu().numpy(), want)
    flags = np.zeros((7, 3), np.int32); flags[2, 1] = flags[6, 2] = _lib.TDA_WIN_NOT_FINITE
    assert np.array_equal(st.cpu().numpy(), flags)
    # the same windows read in place through tables, and without a scratch of the caller's
    flat = torch.from_numpy(sig.reshape(-1)).to(dev)
    start = torch.arange(7, device=dev) * (3 * N_T)
    ld = torch.full((7,), N_T, dtype=torch.int64, device=dev)
    tab = engine.sublevel_features_dev(flat, N_T, start, ld, 3, max_bytes=max_bytes, ctx=ctx)
    assert tab.cpu().numpy().tobytes() == got.cpu().numpy().tobytes()


def _inputs():
    """Three recordings of 600 samples, eight selected windows in three groups of 4, 1 and 3 windows.  Every sample is
    finite: these inputs also go through the Rips stages of the step."""
    rng = np.random.default_rng(71)
    n_rec, L = 3, 600
    rec = np.round(rng.standard_normal((n_rec, N_CH, L)).cumsum(axis=2) * 0.1, 3)
    per_rec = (L - N_T) // STEP + 1
    sel = np.array([0, 1, 2, 3, per_rec + 1, 2 * per_rec, 2 * per_rec + 2, 2 * per_rec + 5], np.int32)
    seg_off = np.array([0, 4, 5, 8], np.int32)
    r, k = sel // per_rec, sel % per_rec
    eeg = np.stack([rec[a, :, b * STEP:b * STEP + N_T] for a, b in zip(r, k)])
    aud = rng.standard_normal((len(sel), N_T)).cumsum(axis=1)
    start = (r.astype(np.int64) * N_CH * L + k * STEP)
    return rec, sel, seg_off, eeg, aud, start, np.full(len(sel), L, np.int64)


def _ref_sl(eeg, aud, seg_off):
    """(sl, tol): the numpy composition of the reference features, and 2e-12 * the same composition of their magnitudes."""
    fa = _ref_features(aud)
    fe = _ref_features(eeg.reshape(-1, N_T)).reshape(eeg.shape[0], N_CH, 11)
    out, tol = np.empty((len(seg_off) - 1, 22)), np.empty((len(seg_off) - 1, 22))
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)              # nanmean of a group whose only window is flagged
        for g in range(len(seg_off) - 1):
            sl = slice(seg_off[g], seg_off[g + 1])
            out[g, :11], out[g, 11:] = np.nanmean(fa[sl], axis=0), np.nanmean(np.mean(fe[sl], axis=1), axis=0)
            tol[g, :11] = 2e-12 * np.nanmean(np.abs(fa[sl]), axis=0)
            tol[g, 11:] = 2e-12 * np.nanmean(np.mean(np.abs(fe[sl]), axis=1), axis=0)
    return out, tol


def _assert_sl(got, want, tol):
    assert got.shape == want.shape and np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    err = np.abs(got[ok] - want[ok])
    print("sl: largest error / tolerance", float((err / np.maximum(tol[ok], 1e-300)).max()))
    assert (err <= tol[ok]).all()


def test_step_fills_sl_in_three_input_modes(ctx):
    import torch
    dev = torch.device("cuda", ctx.device)
    rec, sel, seg_off, eeg, aud, start, ld = _inputs()
    n_win = len(sel)
    want, tol = _ref_sl(eeg, aud, seg_off)
    assert np.isfinite(want).all()
    eeg_t, aud_t, rec_t = (torch.from_numpy(a).to(dev) for a in (eeg, aud, rec))
    modes = {"stacked": {}, "sliding": dict(eeg_sliding=(rec_t, N_T, STEP, torch.from_numpy(sel).to(dev))),
             "table": dict(eeg_table=(rec_t.view(-1), torch.from_numpy(start).to(dev), torch.from_numpy(ld).to(dev), N_T))}
    # the option off: no buffer, no output; with another output on, its bytes are the yardstick
    plain = pipeline.Workspace(n_win, seg_off, dev, bottleneck=True)
    res0 = pipeline.run_step(eeg_t, aud_t, plain, ctx=ctx).cpu().numpy().copy()
    bott0 = plain.bott.cpu().numpy().copy()
    assert plain.sl is None and plain.sl_fe is None and plain.sl_scratch is None and not plain.sublevel
    assert [o.name for o in plain.outputs] == ["bott"]
    first = None
    for name, kw in modes.items():
        # a bound of three windows of 47 channels: chunks of 3, 3 and 2 windows for the EEG
        ws = pipeline.Workspace(n_win, seg_off, dev, bottleneck=True, sublevel=True, sublevel_bytes=3 * N_CH * 125 * 16)
        assert [o.name for o in ws.outputs] == ["bott", "sl"] and ws.sl.shape == (3, pipeline.SL_COLS)
        res = pipeline.run_step(eeg_t, aud_t, ws, ctx=ctx, **kw).cpu().numpy()
        torch.cuda.synchronize()
        assert res.tobytes() == res0.tobytes() and ws.bott.cpu().numpy().tobytes() == bott0.tobytes(), name
        assert ws.sl_scratch[(N_CH, N_T)].n_chunks(n_win) == 3 and ws.sl_scratch[(1, N_T)].n_chunks(n_win) == 1
        got = ws.sl.cpu().numpy()
        _assert_sl(got, want, tol)
        assert not ws.sl_se.any() and not ws.sl_sa.any()
        _assert_features(ws.sl_fa.cpu().numpy().reshape(n_win, 11), _ref_features(aud))
        first = got if first is None else first
        assert got.tobytes() == first.tobytes(), name               # the three modes read the same samples
        if name == "stacked":
            v = ws.view(seg_off[:3])                                 # a view over the first two groups
            pipeline.run_step(eeg_t[:5], aud_t[:5], v, ctx=ctx)
            torch.cuda.synchronize()
            assert v.sl.cpu().numpy().tobytes() == got[:2].tobytes() and v.sl_fe.shape[0] == 5
    # through the lanes: captured once, replayed once; the same bytes
    lanes = pipeline.Lanes(1, n_win, seg_off, dev, graph=True, bottleneck=True, sublevel=True,
                           sublevel_bytes=3 * N_CH * 125 * 16)
    for rnd in range(2):
        b = lanes.submit(eeg_t, aud_t, ctx=ctx, post=lambda r: r.clone())
        lanes.drain()
        torch.cuda.synchronize()
        assert b.result().cpu().numpy().tobytes() == res0.tobytes(), rnd
        assert lanes.ws[0].sl.cpu().numpy().tobytes() == first.tobytes(), rnd
        assert lanes.ws[0].bott.cpu().numpy().tobytes() == bott0.tobytes(), rnd
        lanes.ws[0].sl.fill_(-7.0)                                  # the replay has to write it again
        lanes.ws[0].sl_fe.fill_(-7.0)
    assert len(lanes.graphs) == 1


def test_stage_counts_flagged_signals_as_nan(ctx):
    """The sublevel stage alone (no Rips kernel sees these samples): window 4, alone in its group, has a NaN in the audio,
    window 6 an inf in one EEG channel.  The audio columns of group 1 are NaN, window 6 leaves the EEG mean of group 2."""
    import torch
    dev = torch.device("cuda", ctx.device)
    _, _, seg_off, eeg, aud, _, _ = _inputs()
    aud[4, 100] = np.nan
    eeg[6, 11, 249] = np.inf
    want, tol = _ref_sl(eeg, aud, seg_off)
    assert np.isnan(want[1, :11]).all() and np.isfinite(want[1, 11:]).all() and np.isfinite(want[[0, 2]]).all()
    ws = pipeline.Workspace(len(aud), seg_off, dev, sublevel=True, sublevel_bytes=3 * N_CH * 125 * 16)
    pipeline._sublevel_stage(ws, ctx, torch.from_numpy(eeg).to(dev), torch.from_numpy(aud).to(dev), None, None)
    torch.cuda.synchronize()
    _assert_sl(ws.sl.cpu().numpy(), want, tol)
    se = ws.sl_se.cpu().numpy()
    assert se[6, 11] == _lib.TDA_WIN_NOT_FINITE and np.count_nonzero(se) == 1
    assert ws.sl_sa.cpu().numpy().reshape(-1).tolist() == [0, 0, 0, 0, _lib.TDA_WIN_NOT_FINITE, 0, 0, 0]
    clean, _ = _ref_sl(np.delete(eeg, 6, axis=0), np.delete(aud, 6, axis=0), np.array([0, 4, 5, 7], np.int32))
    assert np.array_equal(want[2, 11:], clean[2, 11:])             # the reference itself: the flagged window is left out


def test_recording_pass_sublevel(ctx):
    import torch
    dev = torch.device("cuda", ctx.device)
    rng = np.random.default_rng(72)
    n_rec, L = 2, 1500
    raw = rng.standard_normal((n_rec, 47, L)) + 0.5 * rng.standard_normal((n_rec, 1, L))
    env = np.abs(rng.standard_normal((n_rec, L))).cumsum(axis=1) * 0.01 + np.abs(rng.standard_normal((n_rec, L)))
    raw_h, env_h = torch.from_numpy(raw).pin_memory(), torch.from_numpy(env).pin_memory()
    plain = recordings.RecordingPass(L, 2, dev, ctx=ctx)
    rows = plain.run(raw_h, env_h).numpy().copy()
    assert plain.sl_h is None
    rp = recordings.RecordingPass(L, 2, dev, ctx=ctx, sublevel=True)
    got = rp.run(raw_h, env_h).numpy().copy()
    slh = rp.sl_h.numpy().copy()
    assert got.tobytes() == rows.tobytes() and slh.shape == (2, 5, 22) and np.isfinite(slh).all()
    # one essential class per diagram (audio column 1, EEG column 12); the gamma band has finite rows and persistence
    assert (slh[..., [1, 12]] == 1.0).all() and (slh[:, 4][:, [0, 11]] >= 1.0).all() and (slh[:, 4][:, [9, 20]] > 0).all()
    # slow bands have fewer extrema than fast ones: delta against gamma, audio and EEG
    assert (slh[:, 0, 0] < slh[:, 4, 0]).all() and (slh[:, 0, 11] < slh[:, 4, 11]).all()
    one = recordings.RecordingPass(L, 1, dev, ctx=ctx, sublevel=True)
    for r in range(n_rec):
        rows1 = one.run(raw_h[r:r + 1], env_h[r:r + 1]).numpy()
        assert rows1[0].tobytes() == rows[r].tobytes()
        assert one.sl_h.numpy()[0].tobytes() == slh[r].tobytes(), r


def test_ragged_pass_sublevel(ctx):
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
    assert plain.sl_h is None
    rp = recordings.RaggedRecordingPass(LENGTHS, None, dev, shard_samples=BUDGET, n_sets=2, ctx=ctx, sublevel=True)
    got = rp.run(xh, eh).numpy().copy()
    slh = rp.sl_h.numpy().copy()
    assert got.tobytes() == rows.tobytes()
    assert slh.shape == (5, 5, 22) and np.isnan(slh[2]).all()               # the recording without a window
    live = [0, 1, 3, 4]
    assert np.isfinite(slh[live]).all() and (slh[live][..., [1, 12]] == 1.0).all()
    alone = {}
    for r in live:                                                          # alone through a pass of its own: the same bytes
        L = LENGTHS[r]
        if L not in alone:
            alone[L] = recordings.RaggedRecordingPass([L], None, dev, n_sets=1, ctx=ctx, sublevel=True)
        one = alone[L]
        x1, _ = preprocess.pack_recordings(raws[r:r + 1])
        e1, _ = preprocess.pack_recordings(envs[r:r + 1])
        rows1 = one.run(x1, e1).numpy()
        assert np.array_equal(rows1[0], rows[r], equal_nan=True)
        assert one.sl_h.numpy()[0].tobytes() == slh[r].tobytes(), r
