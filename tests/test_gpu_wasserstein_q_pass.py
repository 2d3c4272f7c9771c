"""
wasserstein_q=(2, "l2") through the recording passes: the rows stay what they are, and wq_h (n_rec, n_bands, 2) holds, per
recording, the values the same recording gives when it runs alone through a pass of its own; NaN for a recording without
a window.  Then all six optional outputs at once (the small parameter sets of test_gpu_shard_verify.py): every output is
the bytes of a pass with that option alone, and the repair branch of the shard driver reproduces all of them.
"""
import numpy as np
import pytest

from test_gpu_ragged import FIX, _env, _raw
from test_gpu_shard_verify import HOST, OUTPUTS, _flagging, _inputs
from tda_eeg_audio_amd import preprocess, recordings

pytestmark = pytest.mark.gpu

# four recordings with three distinct lengths and one too short for a window, in two shards
LENGTHS = [FIX[0], FIX[3], 200, FIX[0], FIX[2]]
BUDGET = FIX[0] + FIX[3] + 200
WQ = (2, "l2")
ALL = dict(OUTPUTS, wasserstein_q=(1, "linf"))
ALL_HOST = dict(HOST, wasserstein_q="wq_h")


def test_ragged_pass_wasserstein_q(ctx):
    import torch
    dev = torch.device("cuda", ctx.device)
    rng = np.random.default_rng(51)
    raws = [_raw(rng, L) for L in LENGTHS]
    envs = [_env(rng, L) for L in LENGTHS]
    xh, _ = preprocess.pack_recordings(raws)
    eh, _ = preprocess.pack_recordings(envs)
    plain = recordings.RaggedRecordingPass(LENGTHS, None, dev, shard_samples=BUDGET, n_sets=2, ctx=ctx)
    assert plain.plan.shards == [(0, 3), (3, 5)] and plain.empty.tolist() == [2]
    rows = plain.run(xh, eh).numpy().copy()
    assert plain.wq_h is None
    rp = recordings.RaggedRecordingPass(LENGTHS, None, dev, shard_samples=BUDGET, n_sets=2, ctx=ctx, wasserstein_q=WQ)
    got = rp.run(xh, eh).numpy().copy()
    wqh = rp.wq_h.numpy().copy()
    assert got.tobytes() == rows.tobytes()
    assert wqh.shape == (5, 5, 2)
    assert np.isnan(wqh[2]).all()
    alone = {}                                                      # one pass per length
    for r, L in enumerate(LENGTHS):
        if r == 2:
            continue
        if L not in alone:
            alone[L] = recordings.RaggedRecordingPass([L], None, dev, n_sets=1, ctx=ctx, wasserstein_q=WQ)
        one = alone[L]
        x1, _ = preprocess.pack_recordings(raws[r:r + 1])
        e1, _ = preprocess.pack_recordings(envs[r:r + 1])
        rows1 = one.run(x1, e1).numpy()
        assert np.array_equal(rows1[0], rows[r], equal_nan=True)
        assert np.isfinite(one.wq_h.numpy()).all()
        assert one.wq_h.numpy()[0].tobytes() == wqh[r].tobytes(), r
    # the root of a sum of squares is at most the sum: W2(l2) <= W1(l2), the rows' own distance (1e-6: the two entries
    # round their point costs differently, include/tdaeeg.h)
    live = [0, 1, 3, 4]
    assert (wqh[live] > 0).all() and (wqh[live] <= rows[live][:, :, :2] + 1e-6).all()


def test_recording_pass_wasserstein_q(ctx):
    import torch
    dev = torch.device("cuda", ctx.device)
    rng = np.random.default_rng(52)
    n_rec, L = 2, 1500
    raw = rng.standard_normal((n_rec, 47, L)) + 0.5 * rng.standard_normal((n_rec, 1, L))
    env = np.abs(rng.standard_normal((n_rec, L))).cumsum(axis=1) * 0.01 + np.abs(rng.standard_normal((n_rec, L)))
    raw_h, env_h = torch.from_numpy(raw).pin_memory(), torch.from_numpy(env).pin_memory()
    plain = recordings.RecordingPass(L, 2, dev, ctx=ctx)
    rows = plain.run(raw_h, env_h).numpy().copy()
    assert plain.wq_h is None
    rp = recordings.RecordingPass(L, 2, dev, ctx=ctx, wasserstein_q=WQ)
    got = rp.run(raw_h, env_h).numpy().copy()
    wqh = rp.wq_h.numpy().copy()
    assert got.tobytes() == rows.tobytes() and wqh.shape == (2, 5, 2) and np.isfinite(wqh).all()
    one = recordings.RecordingPass(L, 1, dev, ctx=ctx, wasserstein_q=WQ)
    for r in range(n_rec):
        rows1 = one.run(raw_h[r:r + 1], env_h[r:r + 1]).numpy()
        assert rows1[0].tobytes() == rows[r].tobytes()
        assert one.wq_h.numpy()[0].tobytes() == wqh[r].tobytes(), r


@pytest.fixture(scope="module")
def ragged_six(ctx):
    import torch
    dev = torch.device("cuda", ctx.device)
    rp = recordings.RaggedRecordingPass([1500, 200, 1500], None, dev, shard_samples=1600, n_sets=2, ctx=ctx, **ALL)
    xh, eh = _inputs([1500, 200, 1500], 61)
    rows = rp.run(xh, eh).numpy().copy()
    return dict(p=rp, xh=xh, eh=eh, rows=rows, out={h: getattr(rp, h).numpy().copy() for h in ALL_HOST.values()})


def test_all_six_outputs_at_once_equal_each_alone(ragged_six, ctx):
    """Three shards, the middle one without a window, the third reusing buffer set 0."""
    import torch
    dev = torch.device("cuda", ctx.device)
    rp, rows, out = ragged_six["p"], ragged_six["rows"], ragged_six["out"]
    assert rp.plan.shards == [(0, 1), (1, 2), (2, 3)] and rp.n_sets == 2
    assert [o.name for o in rp.outputs] == ["corr", "bott", "land", "img", "slc", "wq"]
    assert out["wq_h"].shape == (3, 5, 2)
    for option, host in ALL_HOST.items():
        one = recordings.RaggedRecordingPass([1500, 200, 1500], None, dev, shard_samples=1600, n_sets=2, ctx=ctx,
                                             **{option: ALL[option]})
        assert np.array_equal(one.run(ragged_six["xh"], ragged_six["eh"]).numpy(), rows, equal_nan=True), option
        assert np.array_equal(getattr(one, host).numpy(), out[host], equal_nan=True), option
        assert [getattr(one, h) is None for h in ALL_HOST.values()] == [h != host for h in ALL_HOST.values()]
        del one
    for host in ALL_HOST.values():
        assert np.isnan(out[host][1]).all(), host                       # the recording without a window
        assert np.isfinite(out[host][[0, 2]]).any(), host
    # the same family of metrics: bottleneck <= W1(linf), per (recording, band) mean as per pair
    assert (out["bott_h"][[0, 2]] <= out["wq_h"][[0, 2]] + 1e-9).all()


def test_repair_reproduces_all_six_outputs(ragged_six, monkeypatch):
    """The repair branch of _verify with all six outputs on."""
    rp = ragged_six["p"]
    before = rp.repairs
    monkeypatch.setattr(rp, "_rips_step", _flagging(rp))
    got = rp.run(ragged_six["xh"], ragged_six["eh"]).numpy()
    assert np.array_equal(got, ragged_six["rows"], equal_nan=True)
    for host, want in ragged_six["out"].items():
        assert np.array_equal(getattr(rp, host).numpy(), want, equal_nan=True), host
    assert rp.repairs - before == 2
