"""
All eleven optional outputs of pipeline.step_outputs on at once, through the step, a view, the lanes with a captured graph,
the stage timers and RecordingPass.  Every other test turns on one output, or a few; here `result` keeps the bytes of the
plain Workspace, every output the bytes of a Workspace with that output alone, and the per-window and per-group buffers a
view slices are taken from the table (pipeline.OUTPUTS), so a buffer that a record does not declare fails here.
The file also runs, unchanged, on the commit before that table existed (BY_HAND stands in for it there): it is a
characterisation test, and every comparison in it was byte-equal on that commit too.
The inputs are those of test_gpu_fisher_pass.py::test_run_step_with_fisher: 20 windows in six groups, group 1 ONE window
whose audio cloud is degenerate, so the means that follow the rule of `bott` are NaN there; bytes compare NaN too.
"""
import collections

import numpy as np
import pytest

from test_gpu_sliced_pass import _long_tau_window
from tda_eeg_audio_amd import engine, pipeline, recordings, synth, utils

pytestmark = pytest.mark.gpu

N_WIN, N_CH = 20, 47
SEG_OFF = np.array([0, 4, 5, 8, 12, 16, 20], np.int32)
ALL = dict(correlations=True, bottleneck=True, landscapes=(np.linspace(0.0, 1.5, 16), 2),
           images=(np.linspace(0.0, 1.0, 5), np.linspace(0.0, 1.0, 6), 0.1, 1), sliced=utils.default_directions(4),
           wasserstein_q=(2, "l2"), frechet=(8, 4), kernel_distance=("pss", 0.1), fisher=0.1, sublevel=True,
           phase_locking="euclidean")
WS_KW = dict(sublevel_bytes=3 * N_CH * 125 * 16)           # a bound of three windows of 47 channels: chunks of the EEG
NAMES = ["corr", "bott", "land", "img", "slc", "wq", "fm", "kd", "pf", "sl", "pl"]
# the stages of a step with everything on, in launch order (the fused EEG path: neither corr_dist nor rips_eeg)
LAUNCH = ["eeg_window", "tau", "rips_audio", "finish", "temporal_corr", "landscape", "image", "wasserstein_h0", "wasserstein_h1",
          "bottleneck_h0", "bottleneck_h1", "sliced_h0", "sliced_h1", "wasserstein_q_h0", "wasserstein_q_h1",
          "kernel_distance_h0", "kernel_distance_h1", "fisher_h0", "fisher_h1", "frechet", "sublevel", "phase_locking", "reduce"]


# the table as the code kept it by hand before pipeline.OUTPUTS: (name, keyword, per-window buffers, per-group buffers)
_Rec = collections.namedtuple("_Rec", "name keyword per_window per_group")
_QUAD = lambda p: (p + "0", p + "1", p + "s0", p + "s1")      # noqa: E731
BY_HAND = [_Rec("corr", "correlations", (), ()), _Rec("bott", "bottleneck", _QUAD("b"), ()), _Rec("land", "landscapes", (), ()),
           _Rec("img", "images", (), ()), _Rec("slc", "sliced", _QUAD("s"), ()), _Rec("wq", "wasserstein_q", _QUAD("q"), ()),
           _Rec("fm", "frechet", (), ("fm_out",)), _Rec("kd", "kernel_distance", _QUAD("k"), ()), _Rec("pf", "fisher", _QUAD("f"), ()),
           _Rec("sl", "sublevel", ("sl_fa", "sl_fe", "sl_sa", "sl_se"), ()),
           _Rec("pl", "phase_locking", ("pl_dist", "pl_st", "pl_dgm", "pl_f0", "pl_f1", "pl_w0", "pl_w1", "pl_ws0", "pl_ws1"), ())]
TABLE = getattr(pipeline, "OUTPUTS", BY_HAND)


def _host(t):
    return t.cpu().numpy().copy()


@pytest.fixture(scope="module")
def full(ctx):
    """The inputs on the device, `result` of the plain Workspace, every output of a Workspace with it alone, and the
    Workspace with all eleven after one step, with host copies of its result and outputs."""
    import torch
    dev = torch.device("cuda", ctx.device)
    eeg = torch.from_numpy(synth.eeg_windows(N_WIN, seed=3, windows_per_recording=4)).to(dev)
    aud_h = synth.audio_windows_all_bands(N_WIN // 5, seed=4)[0].copy()
    aud_h[4] = _long_tau_window()
    aud = torch.from_numpy(aud_h).to(dev)
    want = _host(pipeline.run_step(eeg, aud, pipeline.Workspace(N_WIN, SEG_OFF, dev), ctx=ctx))
    alone = {}
    for rec in TABLE:
        one = pipeline.Workspace(N_WIN, SEG_OFF, dev, **{rec.keyword: ALL[rec.keyword]}, **WS_KW)
        assert [o.name for o in one.outputs] == [rec.name]
        assert _host(pipeline.run_step(eeg, aud, one, ctx=ctx)).tobytes() == want.tobytes(), rec.name
        alone[rec.name] = _host(getattr(one, rec.name))
    ws = pipeline.Workspace(N_WIN, SEG_OFF, dev, **ALL, **WS_KW)
    got = _host(pipeline.run_step(eeg, aud, ws, ctx=ctx))
    torch.cuda.synchronize()
    return dict(dev=dev, eeg=eeg, aud=aud, want=want, alone=alone, ws=ws, got=got,
                outs={n: _host(getattr(ws, n)) for n in NAMES})


def test_table_and_shapes(full):
    ws = full["ws"]
    assert [rec.name for rec in TABLE] == NAMES == [o.name for o in ws.outputs]
    assert [rec.keyword for rec in TABLE] == list(ALL)
    # the table declares the buffers the code used to list by hand, no fewer
    assert [(tuple(rec.per_window), tuple(rec.per_group)) for rec in TABLE] == [(r.per_window, r.per_group) for r in BY_HAND]
    for o in ws.outputs:
        assert full["outs"][o.name].shape == (6,) + o.shape, o.name


def test_all_on_equals_each_alone(full):
    assert full["got"].tobytes() == full["want"].tobytes()               # `result`: the bytes of the plain Workspace
    for n in NAMES:
        assert full["outs"][n].shape == full["alone"][n].shape, n
        assert full["outs"][n].tobytes() == full["alone"][n].tobytes(), n
    # NaN by contract: the group of the degenerate window has no distance, every other group has all of them
    for n in ("bott", "slc", "wq", "kd", "pf"):
        assert np.isnan(full["outs"][n][1]).all() and np.isfinite(full["outs"][n][[0, 2, 3, 4, 5]]).all(), n
    assert np.isfinite(full["outs"]["sl"]).all() and np.isfinite(full["outs"]["pl"][:, :22]).all()
    assert np.isnan(full["outs"]["pl"][1, 22:]).all()


def test_view_over_the_first_groups(full, ctx):
    import torch
    ws = full["ws"]
    v = ws.view(SEG_OFF[:4])
    res = _host(pipeline.run_step(full["eeg"][:8], full["aud"][:8], v, ctx=ctx))
    torch.cuda.synchronize()
    assert res.tobytes() == full["want"][:3].tobytes()
    for n in NAMES:
        assert _host(getattr(v, n)).tobytes() == full["outs"][n][:3].tobytes(), n
    for rec in TABLE:
        assert rec.per_window or rec.name in ("corr", "land", "img", "fm"), rec.name
        for attr in rec.per_window:
            buf = getattr(v, attr)
            assert (buf.n_win if isinstance(buf, engine.DeviceDiagrams) else buf.shape[0]) == 8, attr
        for attr in rec.per_group:
            assert all(t.shape[0] == 3 for t in getattr(v, attr)), attr
    assert v.pl_dgm.n_win == 8
    # the view wrote into the buffers of `ws`: the full step puts them back for the tests after this one
    assert _host(pipeline.run_step(full["eeg"], full["aud"], ws, ctx=ctx)).tobytes() == full["want"].tobytes()
    torch.cuda.synchronize()


def test_lanes_capture_once_and_replay(full, ctx):
    import torch
    lanes = pipeline.Lanes(1, N_WIN, SEG_OFF, full["dev"], graph=True, **ALL, **WS_KW)
    for rnd in range(2):
        b = lanes.submit(full["eeg"], full["aud"], ctx=ctx, post=lambda r: r.clone())
        lanes.drain()
        torch.cuda.synchronize()
        assert b.result().cpu().numpy().tobytes() == full["want"].tobytes(), rnd
        for n in NAMES:
            assert _host(getattr(lanes.ws[0], n)).tobytes() == full["outs"][n].tobytes(), (n, rnd)
            getattr(lanes.ws[0], n).fill_(-7.0)                          # the replay has to write it again
    assert len(lanes.graphs) == 1


def test_stage_timers_pin_names_and_order(full, ctx):
    import torch
    assert set(pipeline.STAGES) - {"corr_dist", "rips_eeg"} <= set(LAUNCH)
    timers = {name: (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for name in LAUNCH}
    res = _host(pipeline.run_step(full["eeg"], full["aud"], full["ws"], ctx=ctx, timers=timers))
    torch.cuda.synchronize()
    assert res.tobytes() == full["want"].tobytes()
    for name in LAUNCH:                                                  # elapsed_time raises for an event never recorded
        assert timers[name][0].elapsed_time(timers[name][1]) >= 0, name
    for a, b in zip(LAUNCH, LAUNCH[1:]):
        assert timers[a][0].elapsed_time(timers[b][0]) >= 0, (a, b)


def test_recording_pass_all_outputs(ctx):
    import torch
    dev = torch.device("cuda", ctx.device)
    rng = np.random.default_rng(42)
    n_rec, L = 2, 1500
    raw = rng.standard_normal((n_rec, 47, L)) + 0.5 * rng.standard_normal((n_rec, 1, L))
    env = np.abs(rng.standard_normal((n_rec, L))).cumsum(axis=1) * 0.01 + np.abs(rng.standard_normal((n_rec, L)))
    raw_h, env_h = torch.from_numpy(raw).pin_memory(), torch.from_numpy(env).pin_memory()
    rows = recordings.RecordingPass(L, 2, dev, ctx=ctx).run(raw_h, env_h).numpy().copy()
    rp = recordings.RecordingPass(L, 2, dev, ctx=ctx, **ALL)
    got = rp.run(raw_h, env_h).numpy().copy()
    assert got.tobytes() == rows.tobytes()
    assert [o.name for o in rp.outputs] == NAMES
    for o in rp.outputs:
        assert getattr(rp, o.name + "_h").shape == (2, 5) + o.shape, o.name
