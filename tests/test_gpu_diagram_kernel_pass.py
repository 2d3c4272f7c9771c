"""
kernel_distance=kernel through the step and the recording passes: `result` and the rows stay what they are; ws.k0 / ws.k1
are the kernel-induced distances of the step's own diagram pairs, ws.kd their per-group nanmean under the rule of ws.bott;
kd_h (n_rec, n_bands, 2) holds, per recording, the values the same recording gives when it runs alone through a pass of
its own, NaN for a recording without a window.
"""
import numpy as np
import pytest

import diagram_kernel_ref as dk
from test_gpu_ragged import FIX, _env, _raw
from test_gpu_sliced_pass import _long_tau_window
from tda_eeg_audio_amd import _lib, engine, pipeline, preprocess, recordings, synth

pytestmark = pytest.mark.gpu

KERNEL = ("pss", 0.05)
LENGTHS = [FIX[0], FIX[3], 200, FIX[0], FIX[2]]
BUDGET = FIX[0] + FIX[3] + 200


def test_run_step_with_kernel_distance(ctx):
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
    assert plain.kd is None and plain.k0 is None and plain.kernel_distance is None
    ws = pipeline.Workspace(n_win, seg_off, dev, kernel_distance=KERNEL)
    got = pipeline.run_step(eeg, aud, ws, ctx=ctx).cpu().numpy()
    torch.cuda.synchronize()
    assert got.tobytes() == want.tobytes()                              # `result`: the same bytes with the option on and off
    assert [o.name for o in ws.outputs] == ["kd"] and ws.kernel_distance == KERNEL
    status = ws.aud.status.cpu().numpy()
    keep = (status & (_lib.TDA_WIN_DEGENERATE | _lib.TDA_WIN_TOO_LARGE)) == 0
    assert status[4] & _lib.TDA_WIN_DEGENERATE and not keep[4] and keep.sum() >= 15
    e0, e1 = ws.eeg.to_lists()
    a0, a1 = ws.aud.to_lists()
    k0, k1 = ws.k0.cpu().numpy(), ws.k1.cpu().numpy()
    assert (ws.ks0.cpu().numpy() == 0).all() and (ws.ks1.cpu().numpy() == 0).all()
    par = dk.named(KERNEL)
    legs = ((k0, e0, a0, ws.eeg.h0, ws.eeg.c0, ws.aud.h0, ws.aud.c0), (k1, e1, a1, ws.eeg.h1, ws.eeg.c1, ws.aud.h1, ws.aud.c1))
    for k, ea, au, ra, ca, rb, cb in legs:
        # the kernel values of the step's own pairs against the reference; the distance is theirs bit for bit
        kv = torch.empty((n_win, 3), dtype=torch.float64, device=dev)
        again, _ = engine.diagram_kernel_dev(ra, ca, rb, cb, KERNEL, kvals_t=kv, ctx=ctx)
        kv = kv.cpu().numpy()
        ref = [dk.pair(a, b, par) for a, b in zip(ea, au)]
        R, A, N = (np.array([r[i] for r in ref]) for i in range(3))
        err, tol = np.abs(kv - R), dk.tolerance(A, N, R, par[2], 1.0)
        print("largest error / bound:", float(np.max(err / np.maximum(tol, 1e-300))), "terms up to", int(N.max()))
        assert (err <= tol).all()
        assert again.cpu().numpy().tobytes() == k.tobytes() == dk.distance(kv).tobytes()
        assert (k[keep] > 0).all()
    kd = ws.kd.cpu().numpy()
    assert kd.shape == (6, pipeline.KD_COLS)
    assert np.isnan(kd[1]).all() and np.isfinite(kd[[0, 2, 3, 4, 5]]).all()
    for g in range(6):
        sl = slice(seg_off[g], seg_off[g + 1])
        if not keep[sl].any():
            assert np.isnan(kd[g]).all()
        else:
            assert kd[g, 0] == np.nanmean(k0[sl][keep[sl]]) and kd[g, 1] == np.nanmean(k1[sl][keep[sl]])
    # a view over the first groups computes the same values
    v = ws.view(seg_off[:4])
    pipeline.run_step(eeg[:8], aud[:8], v, ctx=ctx)
    torch.cuda.synchronize()
    assert np.array_equal(v.kd.cpu().numpy(), kd[:3], equal_nan=True) and v.k0.shape[0] == 8 and v.ks1.shape[0] == 8
    with pytest.raises(ValueError):
        pipeline.Workspace(n_win, seg_off, dev, kernel_distance=("pss", 0.0))
    # through the lanes: captured once, replayed once; the same bytes
    lanes = pipeline.Lanes(1, n_win, seg_off, dev, graph=True, kernel_distance=KERNEL)
    for rnd in range(2):
        b = lanes.submit(eeg, aud, ctx=ctx, post=lambda r: r.clone())
        lanes.drain()
        torch.cuda.synchronize()
        assert b.result().cpu().numpy().tobytes() == want.tobytes(), rnd
        assert lanes.ws[0].kd.cpu().numpy().tobytes() == kd.tobytes(), rnd
        assert lanes.ws[0].k0.cpu().numpy().tobytes() == k0.tobytes(), rnd
        lanes.ws[0].kd.fill_(-7.0)                                  # the replay has to write it again
        lanes.ws[0].k0.fill_(-7.0)
    assert len(lanes.graphs) == 1


def test_gram_from_distances(ctx):
    """drivers.diagram_kernel_gram_from_distances: four recordings of 3, 1, 0 and 5 windows of 12 points each."""
    from tda_eeg_audio_amd import drivers
    rng = np.random.default_rng(43)
    dist_list = []
    for k in (3, 1, 0, 5):
        pts = rng.uniform(0, 0.9, (k, 12, 3))
        dist_list.append(np.sqrt(((pts[:, :, None] - pts[:, None, :]) ** 2).sum(-1)))
    allw = np.concatenate([d for d in dist_list if len(d)])
    h0, h1, st = engine.rips_dm_batch(allw, ctx=ctx)
    assert (st == 0).all()
    off = np.cumsum([0, 3, 1, 0, 5])
    for kernel in (("pss", 0.1), ("pwg", 0.1, 2.0)):
        par = dk.named(kernel)
        G = drivers.diagram_kernel_gram_from_distances(dist_list, kernel)
        assert G.shape == (2, 4, 4)
        for s, dgms in enumerate((h0, h1)):
            groups = [list(dgms[off[g]:off[g + 1]]) for g in range(4)]
            R, A, N = dk.gram(groups, groups, par)
            assert G[s].tobytes() == G[s].T.copy().tobytes()
            assert np.isnan(G[s][2]).all() and np.isnan(G[s][:, 2]).all()
            live = np.ix_([0, 1, 3], [0, 1, 3])
            err, tol = np.abs(G[s][live] - R[live]), dk.tolerance(A[live], N[live], R[live], par[2], dk.wmax(list(dgms), par))
            assert (err <= tol).all() and (s == 1 or (G[s][live] > 0).all())
    with pytest.raises(_lib.TdaError):
        drivers.diagram_kernel_gram_from_distances(dist_list, ("pss", -1.0))


def test_ragged_pass_kernel_distance(ctx):
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
    assert plain.kd_h is None
    rp = recordings.RaggedRecordingPass(LENGTHS, None, dev, shard_samples=BUDGET, n_sets=2, ctx=ctx, kernel_distance=("pwg", 0.1, 2.0))
    got = rp.run(xh, eh).numpy().copy()
    kd = rp.kd_h.numpy().copy()
    assert got.tobytes() == rows.tobytes()
    assert kd.shape == (5, 5, 2) and np.isnan(kd[2]).all()
    live = [0, 1, 3, 4]
    assert np.isfinite(kd[live]).all() and (kd[live] > 0).all()
    # one shard of one recording: the same bytes as inside the pass
    one = recordings.RaggedRecordingPass([LENGTHS[1]], None, dev, n_sets=1, ctx=ctx, kernel_distance=("pwg", 0.1, 2.0))
    x1, _ = preprocess.pack_recordings(raws[1:2])
    e1, _ = preprocess.pack_recordings(envs[1:2])
    rows1 = one.run(x1, e1).numpy()
    assert np.array_equal(rows1[0], rows[1], equal_nan=True)
    assert one.kd_h.numpy()[0].tobytes() == kd[1].tobytes()
