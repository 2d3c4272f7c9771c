"""
GPU: the delay and dimension selection kernels (csrc/embedding.hip) against the CPU statement (tests/embedding_ref.py) at
the shapes of tests/embedding_cases.py.  The joint counts, status words and every output of the false nearest neighbours
are compared as bytes; the mutual information to embedding_ref.AMI_BAR, eight times the error of the numpy statement
against 50 digits, measured in tests/test_embedding_model.py and never against the kernel; tau as bytes against the
first-minimum rule applied to the row the kernel returned, and against the reference's value on the four named signals.
"""
import ctypes as C

import numpy as np
import pytest

import embedding_cases as ec
import embedding_ref as er

pytestmark = pytest.mark.gpu
SENT = -12345


def _dev(a):
    import torch
    return torch.from_numpy(np.array(a, order="C")).to(torch.device("cuda", 0))


def _bytes_equal(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), what


def _check_ami(got, ref, what):
    ami, tau, joint, st = got
    _bytes_equal(st, ref["status"], (what, "status"))
    if joint is not None:
        _bytes_equal(joint, ref["joint"], (what, "joint"))
    assert ami.shape == ref["ami"].shape and tau.dtype == np.int32
    for w in range(len(st)):
        if st[w] == er.TDA_WIN_NOT_FINITE:
            assert np.isnan(ami[w]).all() and tau[w] == 0, (what, w)
            continue
        err = np.abs(ami[w] - ref["ami"][w]).max()
        print(f"{what} window {w}: largest |kernel - numpy statement| = {err:.3e} (bar {er.AMI_BAR:.3e})")
        assert err <= er.AMI_BAR, (what, w, err)
        assert tau[w] == er.first_minimum(ami[w]), (what, w)              # a byte-exact function of the returned row
        if st[w] == er.TDA_WIN_DEGENERATE:
            assert ami[w].tobytes() == np.zeros_like(ami[w]).tobytes() and tau[w] == 0


@pytest.mark.parametrize("name", [c[0] for c in ec.ami_cases()])
def test_ami_parity(ctx, name):
    from tda_eeg_audio_amd import engine
    _, wins, max_lag, n_bins = next(c for c in ec.ami_cases() if c[0] == name)
    ref = ec.reference("ami", name)
    full = engine.ami_batch(wins, max_lag, n_bins, joint=True, ctx=ctx)
    _check_ami(full, ref, name)
    # a NULL joint changes no other byte
    lean = engine.ami_batch(wins, max_lag, n_bins, ctx=ctx)
    assert lean[2] is None
    for k in (0, 1, 3):
        _bytes_equal(lean[k], full[k], (name, "joint NULL", k))
    # a window alone and inside the batch: the same bytes
    for w in range(len(wins)):
        one = engine.ami_batch(wins[w:w + 1], max_lag, n_bins, joint=True, ctx=ctx)
        for k in range(4):
            _bytes_equal(one[k][0], full[k][w], (name, "alone", w, k))
    # the device form, twice
    for _ in range(2):
        out = engine.ami_dev(_dev(wins), max_lag, n_bins, joint=True, ctx=ctx).to_host()
        for k, key in enumerate(("ami", "tau", "joint", "ami_status")):
            _bytes_equal(out[key], full[k], (name, "dev", key))


def test_ami_named_signals(ctx):
    from tda_eeg_audio_amd import engine
    for name, (x, tau, _) in ec.named().items():
        ami, got, _, st = engine.ami_batch(x[None], ctx=ctx)
        assert st[0] == 0 and got[0] == tau == er.ami_np(x)["tau"], (name, got[0])
        assert ami.shape == (1, len(x) // 4 + 1)


def test_ami_segments(ctx):
    """Groups: an empty one, one whose first window has no minimum (a ramp on two bins up to lag 5: the fallback), one whose
    first window is refused, and plain ones; tau_win carries the group's value to every window."""
    import torch
    from tda_eeg_audio_amd import engine
    nm = ec.named()
    wins = np.stack([nm["sine"][0], nm["henon"][0], nm["white_noise"][0], np.arange(250.0), nm["sine"][0],
                     np.full(250, 3.0), nm["henon"][0], nm["white_noise"][0]])
    seg = np.array([0, 2, 2, 3, 5, 7, 8], np.int32)
    first = [0, None, 2, 3, 5, 7]
    for max_lag, n_bins in ((None, 16), (40, 16), (5, 2)):
        lag = er.resolve_max_lag(250, max_lag)
        each = engine.ami_batch(wins, max_lag, n_bins, ctx=ctx)[1]
        want = np.array([0 if f is None else (each[f] if each[f] else max(lag // 10, 1)) for f in first], np.int32)
        tau_win = torch.full((8,), SENT, dtype=torch.int32, device="cuda:0")
        tau_seg = engine.ami_segments_dev(_dev(wins), _dev(seg), max_lag, n_bins, None, tau_win, ctx=ctx).cpu().numpy()
        _bytes_equal(tau_seg, want, ("tau_seg", max_lag))
        _bytes_equal(tau_win.cpu().numpy(), np.repeat(want, np.diff(seg)), ("tau_win", max_lag))
        assert engine.ami_segments_dev(_dev(wins), _dev(seg), max_lag, n_bins, ctx=ctx).cpu().numpy().tobytes() == want.tobytes()
    assert each[3] == 0 and each[5] == 0                               # (5, 2): the ramp and the constant window have no minimum


@pytest.mark.parametrize("name", [c[0] for c in ec.fnn_cases()])
def test_fnn_parity(ctx, name):
    from tda_eeg_audio_amd import engine
    _, wins, taus, d_max, theiler = next(c for c in ec.fnn_cases() if c[0] == name)
    ref = ec.reference("fnn", name)
    keys = ("counts", "frac", "dim", "nn", "status")
    full = engine.fnn_batch(wins, taus, d_max, theiler, nn=True, ctx=ctx)
    for k, key in enumerate(keys):
        _bytes_equal(full[k], ref[key], (name, key))
    lean = engine.fnn_batch(wins, taus, d_max, theiler, ctx=ctx)
    assert lean[3] is None
    for k in (0, 1, 2, 4):
        _bytes_equal(lean[k], full[k], (name, "nn NULL", keys[k]))
    tau_arr = np.broadcast_to(np.asarray(taus, np.int32), (len(wins),))
    out = engine.fnn_dev(_dev(wins), _dev(tau_arr), d_max, theiler, nn=True, ctx=ctx).to_host()
    for k, key in enumerate(("counts", "frac", "dim", "nn", "fnn_status")):
        _bytes_equal(out[key], full[k], (name, "dev", key))
    w = len(wins) - 1
    one = engine.fnn_batch(wins[w:], tau_arr[w:], d_max, theiler, nn=True, ctx=ctx)
    for k in range(5):
        _bytes_equal(one[k][0], full[k][w], (name, "alone", keys[k]))


def test_fnn_tolerances_and_named(ctx):
    from tda_eeg_audio_amd import engine
    x = ec.sine()
    cnt, frac, dim, _, st = engine.fnn_batch(x[None], 7, 5, 1, ctx=ctx)
    assert st[0] == 0 and tuple(cnt[0, :3, 3]) == ec.SINE_EITHER and tuple(cnt[0, :3, 0]) == ec.SINE_VALID and dim[0] == 2
    lor = ec.lorenz()
    for theiler in (1, 6):
        got = engine.fnn_batch(lor[None], 6, 5, theiler, nn=True, ctx=ctx)
        ref = er.fnn_np(lor, 6, 5, theiler)
        assert got[2][0] == 3
        for k, key in enumerate(("counts", "frac", "dim", "nn", "status")):
            _bytes_equal(got[k][0], np.asarray(ref[key], got[k].dtype), ("lorenz", theiler, key))
    # other tolerances: the criteria and the dimension rule, not the neighbours
    for r_tol, a_tol, frac_tol in ((2.0, 0.5, 0.0), (15.0, 1e6, 1.0), (1e-3, 2.0, 0.3)):
        got = engine.fnn_batch(x[None], 7, 4, 2, r_tol, a_tol, frac_tol, nn=True, ctx=ctx)
        ref = er.fnn_np(x, 7, 4, 2, r_tol, a_tol, frac_tol)
        for k, key in enumerate(("counts", "frac", "dim", "nn", "status")):
            _bytes_equal(got[k][0], np.asarray(ref[key], got[k].dtype), ("tolerances", r_tol, key))


def _msg(ctx):
    buf = C.create_string_buffer(512)
    ctx.lib.tda_last_error(ctx.h, buf, 512)
    return buf.value.decode()


def test_refusals(ctx):
    """Every refusal of the header: TDA_ERR_INVALID with a message, nothing launched or written."""
    import torch
    from tda_eeg_audio_amd import engine
    dev = torch.device("cuda", 0)
    p = engine._tp
    win = torch.zeros((2, 9000), dtype=torch.float64, device=dev)
    ami = torch.full((2 * 9000,), -7.0, dtype=torch.float64, device=dev)
    frac = torch.full((2 * 8,), -7.0, dtype=torch.float64, device=dev)
    ints = [torch.full((2 * 9000,), SENT, dtype=torch.int32, device=dev) for _ in range(5)]
    tau, joint, st, cnt, dim = ints
    seg = torch.tensor([0, 1, 2], dtype=torch.int32, device=dev)
    lib, h = ctx.lib, ctx.h
    tol = (10.0, 2.0, 0.05)
    nan = float("nan")
    calls = [
        lambda: lib.tda_ami_batch_dev(h, p(win), 2, 3, -1, 16, p(ami), p(tau), p(joint), p(st), None),               # n_t
        lambda: lib.tda_ami_batch_dev(h, p(win), 2, 8193, -1, 16, p(ami), p(tau), None, p(st), None),
        lambda: lib.tda_ami_batch_dev(h, p(win), 2, 250, -1, 1, p(ami), p(tau), None, p(st), None),                  # n_bins
        lambda: lib.tda_ami_batch_dev(h, p(win), 2, 250, -1, 33, p(ami), p(tau), None, p(st), None),
        lambda: lib.tda_ami_batch_dev(h, p(win), -1, 250, -1, 16, p(ami), p(tau), None, p(st), None),                # n_win
        lambda: lib.tda_ami_batch_dev(h, None, 2, 250, -1, 16, p(ami), p(tau), None, p(st), None),                   # pointers
        lambda: lib.tda_ami_batch_dev(h, p(win), 2, 250, -1, 16, None, p(tau), None, p(st), None),
        lambda: lib.tda_ami_batch_dev(h, p(win), 2, 250, -1, 16, p(ami), None, None, p(st), None),
        lambda: lib.tda_ami_batch_dev(h, p(win), 2, 250, -1, 16, p(ami), p(tau), None, None, None),
        lambda: lib.tda_ami_segments_dev(h, p(win), p(seg), 2, 3, -1, 16, p(tau), p(st), None),
        lambda: lib.tda_ami_segments_dev(h, p(win), p(seg), 2, 250, -1, 0, p(tau), p(st), None),
        lambda: lib.tda_ami_segments_dev(h, p(win), None, 2, 250, -1, 16, p(tau), p(st), None),
        lambda: lib.tda_ami_segments_dev(h, p(win), p(seg), 2, 250, -1, 16, None, p(st), None),
        lambda: lib.tda_fnn_batch_dev(h, p(win), p(seg), 2, 3, 5, 1, *tol, p(cnt), p(frac), p(dim), None, p(st), None),     # n_t
        lambda: lib.tda_fnn_batch_dev(h, p(win), p(seg), 2, 2049, 5, 1, *tol, p(cnt), p(frac), p(dim), None, p(st), None),
        lambda: lib.tda_fnn_batch_dev(h, p(win), p(seg), 2, 250, 0, 1, *tol, p(cnt), p(frac), p(dim), None, p(st), None),   # d_max
        lambda: lib.tda_fnn_batch_dev(h, p(win), p(seg), 2, 250, 9, 1, *tol, p(cnt), p(frac), p(dim), None, p(st), None),
        lambda: lib.tda_fnn_batch_dev(h, p(win), p(seg), 2, 250, 5, 0, *tol, p(cnt), p(frac), p(dim), None, p(st), None),   # theiler
        lambda: lib.tda_fnn_batch_dev(h, p(win), p(seg), 2, 250, 5, 251, *tol, p(cnt), p(frac), p(dim), None, p(st), None),
        lambda: lib.tda_fnn_batch_dev(h, p(win), p(seg), 2, 250, 5, 1, 0.0, 2.0, 0.05, p(cnt), p(frac), p(dim), None, p(st), None),
        lambda: lib.tda_fnn_batch_dev(h, p(win), p(seg), 2, 250, 5, 1, nan, 2.0, 0.05, p(cnt), p(frac), p(dim), None, p(st), None),
        lambda: lib.tda_fnn_batch_dev(h, p(win), p(seg), 2, 250, 5, 1, 10.0, -2.0, 0.05, p(cnt), p(frac), p(dim), None, p(st), None),
        lambda: lib.tda_fnn_batch_dev(h, p(win), p(seg), 2, 250, 5, 1, 10.0, nan, 0.05, p(cnt), p(frac), p(dim), None, p(st), None),
        lambda: lib.tda_fnn_batch_dev(h, p(win), p(seg), 2, 250, 5, 1, 10.0, 2.0, -0.01, p(cnt), p(frac), p(dim), None, p(st), None),
        lambda: lib.tda_fnn_batch_dev(h, p(win), p(seg), 2, 250, 5, 1, 10.0, 2.0, 1.01, p(cnt), p(frac), p(dim), None, p(st), None),
        lambda: lib.tda_fnn_batch_dev(h, p(win), p(seg), 2, 250, 5, 1, 10.0, 2.0, nan, p(cnt), p(frac), p(dim), None, p(st), None),
        lambda: lib.tda_fnn_batch_dev(h, p(win), None, 2, 250, 5, 1, *tol, p(cnt), p(frac), p(dim), None, p(st), None),     # pointers
        lambda: lib.tda_fnn_batch_dev(h, p(win), p(seg), 2, 250, 5, 1, *tol, None, p(frac), p(dim), None, p(st), None),
        lambda: lib.tda_fnn_batch_dev(h, p(win), p(seg), 2, 250, 5, 1, *tol, p(cnt), None, p(dim), None, p(st), None),
        lambda: lib.tda_fnn_batch_dev(h, p(win), p(seg), 2, 250, 5, 1, *tol, p(cnt), p(frac), None, None, p(st), None),
        lambda: lib.tda_fnn_batch_dev(h, p(win), p(seg), 2, 250, 5, 1, *tol, p(cnt), p(frac), p(dim), None, None, None),
    ]
    for k, call in enumerate(calls):
        assert call() == 1, k                                      # TDA_ERR_INVALID
        assert _msg(ctx), k
    torch.cuda.synchronize()
    assert (ami == -7.0).all() and (frac == -7.0).all() and all((t == SENT).all() for t in ints)
    # the host forms refuse before anything is staged or written
    hp = lambda a: a.ctypes.data_as(C.c_void_p)                   # noqa: E731
    wh, ah, fh = np.zeros((2, 250)), np.full((2, 63), -7.0), np.full((2, 5), -7.0)
    ih = [np.full(2 * 5 * 250, SENT, np.int32) for _ in range(4)]
    assert lib.tda_ami_batch(h, hp(wh), 2, 3, -1, 16, hp(ah), hp(ih[0]), None, hp(ih[1])) == 1 and _msg(ctx)
    assert lib.tda_ami_batch(h, hp(wh), 2, 250, -1, 64, hp(ah), hp(ih[0]), None, hp(ih[1])) == 1
    assert lib.tda_ami_batch(h, hp(wh), 2, 250, -1, 16, hp(ah), None, None, hp(ih[1])) == 1
    assert lib.tda_fnn_batch(h, hp(wh), hp(ih[3]), 2, 250, 9, 1, *tol, hp(ih[0]), hp(fh), hp(ih[1]), None, hp(ih[2])) == 1
    assert lib.tda_fnn_batch(h, hp(wh), hp(ih[3]), 2, 250, 5, 300, *tol, hp(ih[0]), hp(fh), hp(ih[1]), None, hp(ih[2])) == 1
    assert lib.tda_fnn_batch(h, hp(wh), hp(ih[3]), 2, 250, 5, 1, 10.0, 2.0, 1.5, hp(ih[0]), hp(fh), hp(ih[1]), None, hp(ih[2])) == 1
    assert (ah == -7.0).all() and (fh == -7.0).all() and all((a == SENT).all() for a in ih)
    # an empty batch is no error and touches nothing
    assert lib.tda_ami_batch_dev(h, None, 0, 250, -1, 16, None, None, None, None, None) == 0
    assert lib.tda_ami_segments_dev(h, None, None, 0, 250, -1, 16, None, None, None) == 0
    assert lib.tda_fnn_batch_dev(h, None, None, 0, 250, 5, 1, *tol, None, None, None, None, None, None) == 0
    assert lib.tda_ami_batch(h, None, 0, 250, -1, 16, None, None, None, None) == 0
    assert engine.ami_batch(np.zeros((0, 250)), ctx=ctx)[0].shape == (0, 63)
    assert engine.fnn_batch(np.zeros((0, 250)), 3, ctx=ctx)[0].shape == (0, 5, 4)
