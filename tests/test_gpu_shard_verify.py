"""
The repair and withhold branches of the shard driver's verify-then-publish (recordings._ShardedPass._verify), once
through each subclass.  The kernels are not made to overflow: the pass' _rips_step is wrapped so that a step left the
class-overflow bit (2) in the first word of the shard's seg_flags and in its pinned copy, as run_step leaves it.  The
rerun with retry="auto" assigns seg_flags again (recording_rows_dev), so the bit is gone and the rows are the ones of an
unpatched run.  One pass per class (module fixtures): the Rips retry lists are keyed by stream.
The optional outputs (pipeline.step_outputs) take the path of the rows: with all five on, every one equals the output of a
pass with that option alone, and the repair reproduces all of them.
"""
import numpy as np
import pytest

from tda_eeg_audio_amd import recordings, utils
from tda_eeg_audio_amd._lib import TdaError

pytestmark = pytest.mark.gpu

# every optional output, small: a grid of 16 points with 2 levels, 4 x 4 images, 4 directions
OUTPUTS = dict(correlations=True, bottleneck=True, landscapes=(np.linspace(0.0, 2.0, 16), 2),
               images=(np.linspace(0.0, 2.0, 5), np.linspace(0.0, 1.0, 5), 0.1, 1), sliced=utils.default_directions(4))
HOST = dict(correlations="corr_h", bottleneck="bott_h", landscapes="land_h", images="img_h", sliced="slc_h")


def _inputs(lengths, seed):
    import torch
    rng = np.random.default_rng(seed)
    raw = np.concatenate([(rng.standard_normal((47, L)) + 0.5 * rng.standard_normal((1, L))).ravel() for L in lengths])
    env = np.concatenate([np.abs(rng.standard_normal(L)).cumsum() * 0.01 + np.abs(rng.standard_normal(L)) for L in lengths])
    return torch.from_numpy(raw).pin_memory(), torch.from_numpy(env).pin_memory()


def _flagging(p, after_auto=False):
    """p._rips_step, leaving bit 2 behind after a call with retry != "auto" (after_auto: after every call)."""
    inner = p._rips_step

    def step(st, i, retry):
        res = inner(st, i, retry)
        if retry != "auto" or after_auto:
            ws = p._flags_ws(st, i)
            ws.seg_flags[:1].bitwise_or_(2)
            ws.flags_host.copy_(ws.seg_flags, non_blocking=True)
        return res
    return step


@pytest.fixture(scope="module")
def ragged(ctx):
    import torch
    dev = torch.device("cuda", ctx.device)
    rp = recordings.RaggedRecordingPass([1500, 200, 1500], None, dev, shard_samples=1600, n_sets=2, ctx=ctx, correlations=True)
    xh, eh = _inputs([1500, 200, 1500], 61)
    rows = rp.run(xh, eh).numpy().copy()
    return dict(p=rp, xh=xh, eh=eh, rows=rows, corr=rp.corr_h.numpy().copy())


@pytest.fixture(scope="module")
def equal(ctx):
    import torch
    dev = torch.device("cuda", ctx.device)
    rp = recordings.RecordingPass(1500, 2, dev, ctx=ctx)
    xh, eh = _inputs([1500] * 3, 62)
    xh, eh = xh.view(3, 47, 1500), eh.view(3, 1500)
    return dict(p=rp, xh=xh, eh=eh, rows=rp.run(xh, eh).numpy().copy())


def _outputs(p):
    return {name: getattr(p, name).numpy().copy() for name in HOST.values()}


@pytest.fixture(scope="module")
def ragged_all(ctx):
    import torch
    dev = torch.device("cuda", ctx.device)
    rp = recordings.RaggedRecordingPass([1500, 200, 1500], None, dev, shard_samples=1600, n_sets=2, ctx=ctx, **OUTPUTS)
    xh, eh = _inputs([1500, 200, 1500], 61)
    rows = rp.run(xh, eh).numpy().copy()
    return dict(p=rp, xh=xh, eh=eh, rows=rows, out=_outputs(rp))


@pytest.fixture(scope="module")
def equal_all(ctx):
    import torch
    dev = torch.device("cuda", ctx.device)
    rp = recordings.RecordingPass(1500, 2, dev, ctx=ctx, **OUTPUTS)
    xh, eh = _inputs([1500] * 3, 62)
    xh, eh = xh.view(3, 47, 1500), eh.view(3, 1500)
    rows = rp.run(xh, eh).numpy().copy()
    return dict(p=rp, xh=xh, eh=eh, rows=rows, out=_outputs(rp))


def test_all_outputs_at_once_equal_each_alone(ragged_all, ctx):
    """Three shards, the middle one without a window, the third reusing buffer set 0: the rows and every output of the pass
    with all five on are the bytes of a pass with that option alone."""
    import torch
    dev = torch.device("cuda", ctx.device)
    rp, rows, out = ragged_all["p"], ragged_all["rows"], ragged_all["out"]
    assert rp.plan.shards == [(0, 1), (1, 2), (2, 3)] and rp.plan.k.tolist() == [15, 0, 15] and rp.n_sets == 2
    assert [o.name for o in rp.outputs] == ["corr", "bott", "land", "img", "slc"]
    assert out["land_h"].shape == (3, 5, 3, 3, 16) and out["img_h"].shape == (3, 5, 3, 4, 4)
    for option, host in HOST.items():
        one = recordings.RaggedRecordingPass([1500, 200, 1500], None, dev, shard_samples=1600, n_sets=2, ctx=ctx,
                                             **{option: OUTPUTS[option]})
        assert np.array_equal(one.run(ragged_all["xh"], ragged_all["eh"]).numpy(), rows, equal_nan=True), option
        assert np.array_equal(getattr(one, host).numpy(), out[host], equal_nan=True), option
        assert [getattr(one, h) is None for h in HOST.values()] == [h != host for h in HOST.values()]
        del one
    for host in HOST.values():
        assert np.isnan(out[host][1]).all(), host                       # the recording without a window
        assert np.isfinite(out[host][[0, 2]]).any(), host


@pytest.mark.parametrize("which", ["ragged_all", "equal_all"])
def test_repair_reproduces_every_output(which, request, monkeypatch):
    """The repair branch of _verify with all five outputs on: the ragged pass above, and equal lengths in shards of 2 and
    1 (the last one padded)."""
    f = request.getfixturevalue(which)
    rp = f["p"]
    before = rp.repairs
    monkeypatch.setattr(rp, "_rips_step", _flagging(rp))
    got = rp.run(f["xh"], f["eh"]).numpy()
    assert np.array_equal(got, f["rows"], equal_nan=True)
    for host, want in f["out"].items():
        assert np.array_equal(getattr(rp, host).numpy(), want, equal_nan=True), host
    assert rp.repairs - before == 2


def test_ragged_pass_repairs_flagged_shards(ragged, monkeypatch):
    rp, rows, corr = ragged["p"], ragged["rows"], ragged["corr"]
    # the middle shard has no window (nothing to verify); the third one reuses buffer set 0
    assert rp.plan.shards == [(0, 1), (1, 2), (2, 3)] and rp.plan.k.tolist() == [15, 0, 15] and rp.n_sets == 2
    assert (rows[[0, 2]][:, :, 3] == 15).all() and np.isfinite(rows[[0, 2]][:, :, 4:]).all() and np.isfinite(corr[[0, 2]]).any()
    before = rp.repairs
    monkeypatch.setattr(rp, "_rips_step", _flagging(rp))
    got = rp.run(ragged["xh"], ragged["eh"]).numpy()
    assert np.array_equal(got, rows, equal_nan=True)
    assert np.array_equal(rp.corr_h.numpy(), corr, equal_nan=True)
    assert rp.repairs - before == 2
    assert np.isnan(got[1][:, [0, 1, 2]]).all() and np.isnan(got[1][:, 4:]).all() and (got[1][:, 3] == 0).all()
    assert np.isnan(rp.corr_h.numpy()[1]).all()


def test_recording_pass_repairs_flagged_shards(equal, monkeypatch):
    rp, rows = equal["p"], equal["rows"]
    assert rp.S == 2 and rows.shape[0] == 3 and (rows[:, :, 3] == 15).all()          # shards of 2 and 1: the last one is padded
    before = rp.repairs
    monkeypatch.setattr(rp, "_rips_step", _flagging(rp))
    got = rp.run(equal["xh"], equal["eh"]).numpy()
    assert np.array_equal(got, rows, equal_nan=True)
    assert rp.repairs - before == 2


def test_status_bit_left_after_the_repair_withholds_the_rows(equal, monkeypatch):
    rp, rows = equal["p"], equal["rows"]
    with monkeypatch.context() as m:
        m.setattr(rp, "_rips_step", _flagging(rp, after_auto=True))
        with pytest.raises(TdaError, match=r"status bits 0x2 left in shard 0"):
            rp.run(equal["xh"], equal["eh"])
    # the driver leaves no state behind
    before = rp.repairs
    assert np.array_equal(rp.run(equal["xh"], equal["eh"]).numpy(), rows, equal_nan=True)
    assert rp.repairs == before
