"""
The phase-locking value kernel against the 40-digit evaluation of its contract (tests/plv_ref.py; include/tdaeeg.h,
"Phase-locking value").

Bars (tests/plv_ref.py): |plv_kernel - plv_exact| <= PLV_BAR = 8 * PLV_E_REF, PLV_E_REF the measured
difference of the numpy definition from the 40-digit one on these same inputs; for the distances the bar that follows from
it, dist_bar(method): sqrt(2 e) for "euclidean" and "sqrt", e for "abs" and "standard".  Diagrams are compared bit for bit
with tda_rips_dm_batch on the kernel's own distance bytes, never with numpy's.
"""
import numpy as np
import pytest

import plv_ref as ref
from tda_eeg_audio_amd import _lib, engine, utils

pytestmark = pytest.mark.gpu

FILL = -7.25


def _dev(ctx):
    import torch
    return torch.device("cuda", ctx.device)


def _run(x, ctx, method="euclidean", want_plv=True, tables=None):
    """(dist, plv or None, status) of plv_dist_dev into pre-filled buffers; x stacked (n_win, n_ch, n_t), or flat with
    tables = (start, ld, n_ch, n_t)."""
    import torch
    dev = _dev(ctx)
    x_t = torch.from_numpy(np.array(x)).to(dev)
    kw = {}
    if tables is not None:
        start, ld, n_ch, n_t = tables
        n_win = len(start)
        kw = dict(n_t=n_t, win_start_t=torch.from_numpy(start).to(dev), win_ld_t=torch.from_numpy(ld).to(dev), n_ch=n_ch)
    else:
        n_win, n_ch, _ = x.shape
    out = torch.full((n_win, n_ch, n_ch), FILL, dtype=torch.float64, device=dev)
    plv = torch.full((n_win, n_ch, n_ch), FILL, dtype=torch.float64, device=dev) if want_plv else None
    st = torch.full((n_win,), -5, dtype=torch.int32, device=dev)
    engine.plv_dist_dev(x_t, method=method, out=out, plv_t=plv, status_t=st, ctx=ctx, **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy(), None if plv is None else plv.cpu().numpy(), st.cpu().numpy()


def _same(a, b):
    return all((p is None and q is None) or p.tobytes() == q.tobytes() for p, q in zip(a, b))


def _assert_shape_of_result(dist, plv):
    for w in range(dist.shape[0]):
        assert plv[w].tobytes() == plv[w].T.copy().tobytes() and dist[w].tobytes() == dist[w].T.copy().tobytes()
        assert (np.diagonal(plv[w]) == 1.0).all() and (np.diagonal(dist[w]) == 0.0).all()
        assert not np.signbit(np.diagonal(dist[w])).any()
    assert (plv >= 0).all() and (plv <= 1 + ref.PLV_BAR).all() and (dist >= 0).all()


@pytest.mark.parametrize("name", list(ref.cases()))
def test_plv_and_distances_against_exact(ctx, name):
    """Every shape of plv_ref.SHAPES (n_ch 2, 3, 16, 17, 47, 48, 56, 61, 64; n_t 2, 3, 63, 64, 65, 249, 250, 256: the three
    time-block sizes, even and odd lengths, up to 272 pair tiles) and the special channels, the four methods."""
    x = ref.cases()[name]
    ex = ref.exact(name)
    dist0 = None
    for m, method in enumerate(ref.METHODS):
        dist, plv, st = _run(x, ctx, method)
        assert (st == 0).all()
        _assert_shape_of_result(dist, plv)
        e_p = float(np.abs(plv - ex).max())
        want = np.stack([ref.dist_of(p, m) for p in ex])
        e_d = float(np.abs(dist - want).max())
        print(f"{name} {method}: plv error {e_p:.3e} (bar {ref.PLV_BAR:.3e}), dist error {e_d:.3e} (bar {ref.dist_bar(m):.3e})")
        assert e_p <= ref.PLV_BAR and e_d <= ref.dist_bar(m)
        # the kernel's distance is correlation_to_distance of the kernel's own plv, to the rounding of the formula
        own = np.stack([ref.dist_of(p, m) for p in plv])
        assert np.abs(dist - own).max() <= 2.0 ** -50
        if m == 0:
            dist0, plv0 = dist, plv
        else:
            assert plv.tobytes() == plv0.tobytes()                  # the method changes the distance only
    assert dist0 is not None


def test_special_channels(ctx):
    """special_8x250: channel 3 duplicates channel 1, 4 is zero, 5 constant, 6 three times channel 2."""
    x = ref.cases()["special_8x250"]
    dist, plv, st = _run(x, ctx)
    bar = ref.PLV_BAR
    assert st[0] == 0
    assert abs(plv[0, 1, 3] - 1) <= bar and abs(plv[0, 2, 6] - 1) <= bar and abs(plv[0, 4, 5] - 1) <= bar
    # the square root near p = 1 turns the bar into sqrt(2 * bar) = 1.1e-7
    assert max(dist[0, 1, 3], dist[0, 2, 6], dist[0, 4, 5]) <= ref.dist_bar(0)
    for k in (0, 2, 7):                                             # a duplicate has its original's row
        assert abs(plv[0, 1, k] - plv[0, 3, k]) <= bar
    y = x.copy()
    y[0, 5] = -2.5                                                  # a negative constant: phase pi against the zero channel's 0
    assert abs(_run(y, ctx)[1][0, 4, 5] - 1) <= bar


def test_alone_and_in_a_batch_of_300(ctx):
    x = ref._rng_windows(300, 5, 33, 21)
    batch = _run(x, ctx)
    assert (batch[2] == 0).all()
    for w in (0, 137, 299):
        assert _same(_run(x[w:w + 1], ctx), [b[w:w + 1] for b in batch])
    p = ref.plv_numpy(x[299])
    assert np.abs(batch[1][299] - p).max() <= ref.PLV_BAR + ref.PLV_E_REF


@pytest.mark.parametrize("n_ch, L", [(3, 700), (47, 520)])
def test_table_addressing_reads_windows_in_place(ctx, n_ch, L):
    """Overlapping windows (step 62) of packed recordings of two lengths, rows win_ld = L_r != n_t apart, against the same
    windows stacked; the host twin on the same tables."""
    rng = np.random.default_rng(62)
    n_t, step, lens = 250, 62, [L, L + 131]
    recs = [rng.standard_normal((n_ch, l)) for l in lens]
    flat = np.concatenate([r.reshape(-1) for r in recs])
    off = np.concatenate([[0], np.cumsum([n_ch * l for l in lens])])
    start, ld, stacked = [], [], []
    for r, l in enumerate(lens):
        for k in range((l - n_t) // step + 1):
            start.append(off[r] + k * step); ld.append(l)
            stacked.append(recs[r][:, k * step:k * step + n_t])
    start, ld, stacked = np.array(start, np.int64), np.array(ld, np.int64), np.stack(stacked)
    in_place = _run(flat, ctx, "abs", tables=(start, ld, n_ch, n_t))
    assert _same(in_place, _run(stacked, ctx, "abs"))
    host = engine.plv_dist_batch(flat, n_t=n_t, win_start=start, win_ld=ld, n_ch=n_ch, method="abs", ctx=ctx)
    assert _same(host, in_place)


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_non_finite_sample_flags_its_window_only(ctx, bad):
    x = ref._rng_windows(5, 6, 250, 31)
    clean = _run(x, ctx)
    y = x.copy()
    y[2, 5, 249] = bad                                              # the last sample of the last row
    dist, plv, st = _run(y, ctx)
    assert st.tolist() == [0, 0, _lib.TDA_WIN_NOT_FINITE, 0, 0]
    assert np.isnan(dist[2]).all() and np.isnan(plv[2]).all()
    for w in (0, 1, 3, 4):
        assert dist[w].tobytes() == clean[0][w].tobytes() and plv[w].tobytes() == clean[1][w].tobytes()
    d2, none, st2 = _run(y, ctx, want_plv=False)                    # ... and without a plv buffer
    assert none is None and d2.tobytes() == dist.tobytes() and st2.tobytes() == st.tobytes()


def test_plv_buffer_is_optional(ctx):
    """plv NULL: the distances are the same bytes, and a buffer the caller keeps beside them is not touched."""
    import torch
    x = ref.cases()["rand_17x64"]
    dist, plv, st = _run(x, ctx, "sqrt")
    d2, none, st2 = _run(x, ctx, "sqrt", want_plv=False)
    assert none is None and d2.tobytes() == dist.tobytes() and (st2 == 0).all()
    dev = _dev(ctx)
    both = torch.full((2,) + dist.shape, FILL, dtype=torch.float64, device=dev)     # [0]: dist, [1]: the caller's fill
    engine.plv_dist_dev(torch.from_numpy(np.array(x)).to(dev), method="sqrt", out=both[0], ctx=ctx)
    torch.cuda.synchronize()
    assert both[0].cpu().numpy().tobytes() == dist.tobytes() and (both[1] == FILL).all()


def test_refusals_launch_nothing(ctx):
    import torch
    dev = _dev(ctx)

    def refused(sig, method="euclidean"):
        n_win, n_ch = sig.shape[0], max(sig.shape[1], 1)
        out = torch.full((n_win, n_ch, n_ch), FILL, dtype=torch.float64, device=dev)
        plv = torch.full((n_win, n_ch, n_ch), FILL, dtype=torch.float64, device=dev)
        st = torch.full((n_win,), -5, dtype=torch.int32, device=dev)
        with pytest.raises(_lib.TdaError):
            ctx.check(ctx.lib.tda_plv_dist_batch_dev(ctx.h, engine._tp(torch.from_numpy(sig).to(dev)), None, None, sig.shape[0],
                                                     sig.shape[1], sig.shape[2], engine._tp(engine.plv_g_table(8, dev)),
                                                     method if isinstance(method, int) else engine.DIST_METHODS[method],
                                                     engine._tp(out), engine._tp(plv), engine._tp(st), engine._stream()))
        torch.cuda.synchronize()
        assert (out == FILL).all() and (plv == FILL).all() and (st == -5).all()
        if not isinstance(method, int):
            with pytest.raises(_lib.TdaError):
                engine.plv_dist_batch(sig, method=method, ctx=ctx)
            with pytest.raises(_lib.TdaError):
                engine.plv_dist_dev(torch.from_numpy(sig).to(dev), method=method, ctx=ctx)

    refused(np.zeros((2, 1, 8)))                                    # n_ch < 2
    refused(np.zeros((2, _lib.PLV_MAX_CHANNELS + 1, 8)))            # n_ch > TDA_PLV_MAX_CHANNELS
    refused(np.zeros((2, 3, 1)))                                    # n_t < 2
    refused(np.zeros((1, 3, _lib.PLV_MAX_SAMPLES + 1)))             # n_t > TDA_PLV_MAX_SAMPLES
    refused(np.zeros((2, 3, 8)), method=4)                          # an unknown method number
    refused(np.zeros((2, 3, 8)), method=-1)
    flat, tab = torch.zeros(64, dtype=torch.float64, device=dev), torch.zeros(2, dtype=torch.int64, device=dev)
    g8 = engine.plv_g_table(8, dev)
    for a, b in ((tab, None), (None, tab)):                         # one table without the other
        st = torch.full((2,), -5, dtype=torch.int32, device=dev)
        with pytest.raises(_lib.TdaError):
            ctx.check(ctx.lib.tda_plv_dist_batch_dev(ctx.h, engine._tp(flat), engine._tp(a), engine._tp(b), 2, 2, 8, engine._tp(g8),
                                                     0, engine._tp(flat), None, engine._tp(st), None))
        torch.cuda.synchronize()
        assert (st == -5).all() and (flat == 0).all()
    with pytest.raises(_lib.TdaError):
        engine.plv_dist_dev(flat, n_t=_lib.PLV_MAX_SAMPLES + 1, win_start_t=tab, win_ld_t=tab, n_ch=3, ctx=ctx)
    for bad in ("plv", 0, None):
        with pytest.raises(ValueError):
            engine.plv_dist_batch(np.zeros((1, 3, 8)), method=bad, ctx=ctx)
    # the limits themselves are accepted; no window is no launch and no error
    d, p, st = _run(np.ones((1, 2, 2)), ctx)
    assert st[0] == 0 and p[0].tolist() == [[1, 1], [1, 1]] and d[0].tolist() == [[0, 0], [0, 0]]
    assert engine.plv_dist_batch(np.zeros((0, 3, 8)), ctx=ctx)[0].shape == (0, 3, 3)


@pytest.mark.parametrize("name, method", [("rand_3x65", "euclidean"), ("rand_47x250", "standard"), ("rand_64x256", "sqrt")])
def test_host_twin_equals_dev_form(ctx, name, method):
    x = ref.cases()[name].copy()
    if x.shape[0] > 1:
        x[1, 0, 0] = np.nan
    host = engine.plv_dist_batch(x, method=method, ctx=ctx)
    assert _same(host, _run(x, ctx, method))
    no_plv = engine.plv_dist_batch(x, method=method, want_plv=False, ctx=ctx)
    assert no_plv[1] is None and no_plv[0].tobytes() == host[0].tobytes()


def test_utils_matrix_and_persistence(ctx):
    x = ref.cases()["rand_47x250"][1]
    p = utils.compute_plv_matrix(x)
    assert p.shape == (47, 47) and np.abs(p - ref.exact("rand_47x250")[1]).max() <= ref.PLV_BAR
    for method in ("euclidean", "abs"):
        dist, _, st = engine.plv_dist_batch(x, method=method, ctx=ctx)
        assert st[0] == 0
        h0, h1, rst = engine.rips_dm_batch(dist, h1_cap=utils._h1_cap(47), ctx=ctx)
        got = utils.compute_plv_persistence(x, method=method)
        assert rst[0] == 0 and len(got) == 2 and len(h1[0]) > 0
        assert got[0].tobytes() == h0[0].tobytes() and got[1].tobytes() == h1[0].tobytes()
        assert got[0].shape == (47, 2) and np.isinf(got[0][-1, 1])
    with pytest.raises(ValueError):
        utils.compute_plv_persistence(x, method="pearson")
    with pytest.raises(ValueError):
        utils.compute_plv_matrix(np.zeros(250))
    y = x.copy()
    y[3, 7] = np.inf
    with pytest.raises(ValueError):
        utils.compute_plv_matrix(y)
    with pytest.raises(ValueError):
        utils.compute_plv_persistence(y)
    with pytest.raises(_lib.TdaError):
        utils.compute_plv_matrix(np.zeros((2, _lib.PLV_MAX_SAMPLES + 1)))
