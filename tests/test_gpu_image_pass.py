"""
images=(xe, ye, sigma, power) through the step and the recording passes: the rows stay what they are; ws.img is within the
tolerance of the reference (tests/image_ref.py) applied to the step's own diagrams; img_h (n_rec, n_bands, 3, n_y, n_x)
holds, per recording, the bytes the same recording gives when it runs alone through a pass of its own; NaN for a recording
without a window.
"""
import numpy as np
import pytest

import image_ref as ir
from test_gpu_ragged import FIX, _env, _raw
from tda_eeg_audio_amd import _lib, pipeline, preprocess, recordings, synth

pytestmark = pytest.mark.gpu

# four recordings with three distinct lengths and one too short for a window, in two shards
LENGTHS = [FIX[0], FIX[3], 200, FIX[0], FIX[2]]
BUDGET = FIX[0] + FIX[3] + 200
N_X, N_Y, SIGMA, POWER = 12, 9, 0.05, 1
XE, YE = np.linspace(0.0, 2.0, N_X + 1), np.linspace(0.0, 1.0, N_Y + 1)
IMAGES = (XE, YE, SIGMA, POWER)
SKIP = _lib.TDA_WIN_DEGENERATE | _lib.TDA_WIN_TOO_LARGE


def _close(got, ref, what):
    mean, W, N = ref
    nan = np.isnan(mean)
    assert got.shape == mean.shape and np.array_equal(np.isnan(got), nan), what
    err = np.where(nan, 0.0, np.abs(got - mean))
    live = W > 0
    if live.any():
        print(f"q = {(err[live].reshape(live.sum(), -1).max(axis=1) / (ir.EPS * W[live])).max():.3f}   [{what}]")
    assert (err <= np.where(nan, 0.0, ir.tolerance(np.where(nan, 0.0, mean), W, N, ir.C))).all(), what


def test_ragged_pass_images(ctx):
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
    assert plain.img_h is None
    rp = recordings.RaggedRecordingPass(LENGTHS, None, dev, shard_samples=BUDGET, n_sets=2, ctx=ctx, images=IMAGES)
    got = rp.run(xh, eh).numpy().copy()
    img = rp.img_h.numpy().copy()
    assert got.tobytes() == rows.tobytes()
    assert img.shape == (5, 5, 3, N_Y, N_X)
    assert np.isnan(img[2]).all()
    alone = {}                                                      # one pass per length
    for r, L in enumerate(LENGTHS):
        if r == 2:
            continue
        if L not in alone:
            alone[L] = recordings.RaggedRecordingPass([L], None, dev, n_sets=1, ctx=ctx, images=IMAGES)
        one = alone[L]
        x1, _ = preprocess.pack_recordings(raws[r:r + 1])
        e1, _ = preprocess.pack_recordings(envs[r:r + 1])
        rows1 = one.run(x1, e1).numpy()
        assert np.array_equal(rows1[0], rows[r], equal_nan=True)
        assert np.isfinite(one.img_h.numpy()).all()
        assert one.img_h.numpy()[0].tobytes() == img[r].tobytes(), r
    live = img[[0, 1, 3, 4]]
    assert (live >= 0).all() and (live > 0).any()
    assert (live[:, :, 0] > 0).any() and (live[:, :, 1] > 0).any() and (live[:, :, 2] > 0).any()


def test_run_step_with_images(ctx):
    import torch
    dev = torch.device("cuda", ctx.device)
    seg_off = np.array([0, 3, 6], np.int32)                         # two groups of three windows
    n_win = 6
    eeg = torch.from_numpy(synth.eeg_windows(n_win, seed=3, windows_per_recording=3)).to(dev)
    aud = torch.from_numpy(synth.audio_windows(n_win, "alpha", seed=4)).to(dev)
    plain = pipeline.Workspace(n_win, seg_off, dev)
    want = pipeline.run_step(eeg, aud, plain, ctx=ctx).cpu().numpy().copy()
    assert plain.img is None
    ws = pipeline.Workspace(n_win, seg_off, dev, images=IMAGES)
    got = pipeline.run_step(eeg, aud, ws, ctx=ctx).cpu().numpy().copy()
    torch.cuda.synchronize()
    assert got.tobytes() == want.tobytes()
    img = ws.img.cpu().numpy().copy()
    assert img.shape == (2, 3, N_Y, N_X)
    assert ws.img_sets.is_contiguous() and ws.img_sets.data_ptr() == ws.img.data_ptr()
    e0, e1 = ws.eeg.to_lists()
    _, a1 = ws.aud.to_lists()
    st = ws.aud.status.cpu().numpy()
    _close(img[:, 0], ir.lists_mean(e0, XE, YE, SIGMA, POWER, seg_off), "step EEG H0")
    _close(img[:, 1], ir.lists_mean(e1, XE, YE, SIGMA, POWER, seg_off), "step EEG H1")
    _close(img[:, 2], ir.lists_mean(a1, XE, YE, SIGMA, POWER, seg_off, status=st, skip_mask=SKIP), "step audio H1")
    assert np.isfinite(img[:, :2]).all() and img[:, 0].any() and img[:, 1].any()
    # a view over the first group, and the EEG half alone
    v = ws.view(seg_off[:2])
    pipeline.run_step(eeg[:3], aud[:3], v, ctx=ctx)
    assert v.img.shape == (1, 3, N_Y, N_X) and np.array_equal(v.img.cpu().numpy(), img[:1], equal_nan=True)
    fs = pipeline.Workspace(n_win, seg_off, dev, images=IMAGES)
    pipeline.run_features_step(eeg, fs, ctx=ctx)
    assert np.array_equal(fs.img.cpu().numpy()[:, :2], img[:, :2])
    # through the lanes: captured once, replayed once; the same bytes
    lanes = pipeline.Lanes(1, n_win, seg_off, dev, graph=True, images=IMAGES)
    for rnd in range(2):
        b = lanes.submit(eeg, aud, ctx=ctx, post=lambda r: r.clone())
        lanes.drain()
        torch.cuda.synchronize()
        assert b.result().cpu().numpy().tobytes() == want.tobytes(), rnd
        assert lanes.ws[0].img.cpu().numpy().tobytes() == img.tobytes(), rnd
        lanes.ws[0].img.fill_(-7.0)                                 # the replay has to write it again
    assert len(lanes.graphs) == 1
