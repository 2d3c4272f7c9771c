"""
bottleneck=True through the recording passes: the rows stay what they are, and bott_h (n_rec, n_bands, 2) holds, per
recording, the values the same recording gives when it runs alone through a pass of its own; NaN for a recording without
a window.
"""
import numpy as np
import pytest

from test_gpu_ragged import FIX, _env, _raw
from tda_eeg_audio_amd import preprocess, recordings

pytestmark = pytest.mark.gpu

# four recordings with three distinct lengths and one too short for a window, in two shards
LENGTHS = [FIX[0], FIX[3], 200, FIX[0], FIX[2]]
BUDGET = FIX[0] + FIX[3] + 200


def test_ragged_pass_bottleneck(ctx):
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
    assert plain.bott_h is None
    rp = recordings.RaggedRecordingPass(LENGTHS, None, dev, shard_samples=BUDGET, n_sets=2, ctx=ctx, bottleneck=True)
    got = rp.run(xh, eh).numpy().copy()
    bott = rp.bott_h.numpy().copy()
    assert got.tobytes() == rows.tobytes()
    assert bott.shape == (5, 5, 2)
    assert np.isnan(bott[2]).all()
    alone = {}                                                      # one pass per length
    for r, L in enumerate(LENGTHS):
        if r == 2:
            continue
        if L not in alone:
            alone[L] = recordings.RaggedRecordingPass([L], None, dev, n_sets=1, ctx=ctx, bottleneck=True)
        one = alone[L]
        x1, _ = preprocess.pack_recordings(raws[r:r + 1])
        e1, _ = preprocess.pack_recordings(envs[r:r + 1])
        rows1 = one.run(x1, e1).numpy()
        assert np.array_equal(rows1[0], rows[r], equal_nan=True)
        assert np.isfinite(one.bott_h.numpy()).all()
        assert one.bott_h.numpy()[0].tobytes() == bott[r].tobytes(), r
    # the bottleneck distance is the largest matched cost, the Wasserstein distance their sum
    live = [0, 1, 3, 4]
    assert (bott[live] > 0).all() and (bott[live] <= rows[live][:, :, :2] + 1e-12).all()


def test_recording_pass_bottleneck(ctx):
    import torch
    dev = torch.device("cuda", ctx.device)
    rng = np.random.default_rng(42)
    n_rec, L = 2, 1500
    raw = rng.standard_normal((n_rec, 47, L)) + 0.5 * rng.standard_normal((n_rec, 1, L))
    env = np.abs(rng.standard_normal((n_rec, L))).cumsum(axis=1) * 0.01 + np.abs(rng.standard_normal((n_rec, L)))
    raw_h, env_h = torch.from_numpy(raw).pin_memory(), torch.from_numpy(env).pin_memory()
    rows = recordings.RecordingPass(L, 2, dev, ctx=ctx).run(raw_h, env_h).numpy().copy()
    rp = recordings.RecordingPass(L, 2, dev, ctx=ctx, bottleneck=True)
    got = rp.run(raw_h, env_h).numpy().copy()
    bott = rp.bott_h.numpy().copy()
    assert got.tobytes() == rows.tobytes() and bott.shape == (2, 5, 2) and np.isfinite(bott).all()
    one = recordings.RecordingPass(L, 1, dev, ctx=ctx, bottleneck=True)
    for r in range(n_rec):
        rows1 = one.run(raw_h[r:r + 1], env_h[r:r + 1]).numpy()
        assert rows1[0].tobytes() == rows[r].tobytes()
        assert one.bott_h.numpy()[0].tobytes() == bott[r].tobytes(), r
