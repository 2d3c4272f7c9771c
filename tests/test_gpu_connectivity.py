"""
The analytic-signal connectivity kernel (wpli, imcoh, coh, aec) against the 40-digit evaluation of its contract
(tests/connectivity_ref.py; include/tdaeeg.h, "Analytic-signal connectivity").

Bars (tests/connectivity_ref.py): |value_kernel - value_exact| <= BAR[m] = 8 * E_REF[m], E_REF[m] the measured
difference of the numpy definition from the 40-digit one on these same inputs; for the distances the bar that follows from
it, plv_ref.dist_bar(method, BAR[m]).  Diagrams are compared bit for bit with tda_rips_dm_batch on the kernel's own distance
bytes, never with numpy's.
"""
import numpy as np
import pytest

import connectivity_ref as ref
import plv_ref
from tda_eeg_audio_amd import _lib, engine, utils

pytestmark = pytest.mark.gpu

FILL = -7.25
MEASURES = ref.MEASURES


def _dev(ctx):
    import torch
    return torch.device("cuda", ctx.device)


def _run(x, ctx, measure, method="euclidean", want_value=True, tables=None):
    """(dist, value or None, status) of connectivity_dist_dev into pre-filled buffers; x stacked (n_win, n_ch, n_t), or flat
    with tables = (start, ld, n_ch, n_t)."""
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
    val = torch.full((n_win, n_ch, n_ch), FILL, dtype=torch.float64, device=dev) if want_value else None
    st = torch.full((n_win,), -5, dtype=torch.int32, device=dev)
    engine.connectivity_dist_dev(x_t, measure=measure, method=method, out=out, value_t=val, status_t=st, ctx=ctx, **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy(), None if val is None else val.cpu().numpy(), st.cpu().numpy()


def _same(a, b):
    return all((p is None and q is None) or p.tobytes() == q.tobytes() for p, q in zip(a, b))


def _assert_shape_of_result(dist, val, measure):
    for w in range(dist.shape[0]):
        assert val[w].tobytes() == val[w].T.copy().tobytes() and dist[w].tobytes() == dist[w].T.copy().tobytes()
        assert (np.diagonal(val[w]) == 1.0).all() and (np.diagonal(dist[w]) == 0.0).all()
        assert not np.signbit(np.diagonal(dist[w])).any()
    lo = -1.0 if measure == "aec" else 0.0
    assert (val >= lo - ref.BAR[measure]).all() and (val <= 1 + ref.BAR[measure]).all() and (dist >= 0).all()


@pytest.mark.parametrize("measure", MEASURES)
@pytest.mark.parametrize("name", list(plv_ref.cases()))
def test_values_and_distances_against_exact(ctx, name, measure):
    """Every shape of plv_ref.SHAPES (n_ch 2, 3, 16, 17, 47, 48, 56, 58, 61, 64; n_t 2, 3, 63, 64, 65, 213, 249, 250, 256: the
    three time-block sizes and the static-LDS edge, even and odd lengths, up to 272 pair tiles) and the special channels,
    the four methods; every pair of every window."""
    x = plv_ref.cases()[name]
    ex = ref.exact(name)[measure]
    bar = ref.BAR[measure]
    val0 = None
    for m, method in enumerate(plv_ref.METHODS):
        dist, val, st = _run(x, ctx, measure, method)
        assert (st == 0).all()
        _assert_shape_of_result(dist, val, measure)
        e_v = float(np.abs(val - ex).max())
        want = np.stack([plv_ref.dist_of(p, m) for p in ex])
        e_d = float(np.abs(dist - want).max())
        print(f"{name} {measure} {method}: value error {e_v:.3e} (bar {bar:.3e}), dist error {e_d:.3e} "
              f"(bar {plv_ref.dist_bar(m, bar):.3e})")
        assert e_v <= bar and e_d <= plv_ref.dist_bar(m, bar)
        # the kernel's distance is correlation_to_distance of the kernel's own value, to the rounding of the formula
        own = np.stack([plv_ref.dist_of(p, m) for p in val])
        assert np.abs(dist - own).max() <= 2.0 ** -50
        if m == 0:
            val0 = val
        else:
            assert val.tobytes() == val0.tobytes()                  # the method changes the distance only
    assert val0 is not None


def test_degenerate_pairs_are_exact(ctx):
    """special_8x250: channel 3 duplicates channel 1, 4 is zero, 5 constant, 6 three times channel 2.  Where a rule of the
    definition decides the value it is that value exactly, and the distance the exact distance of it."""
    x = plv_ref.cases()["special_8x250"]
    zero = {"wpli": [(1, 3), (2, 6)] + [(4, k) for k in range(8) if k != 4],
            "imcoh": [(1, 3)] + [(4, k) for k in range(8) if k != 4],
            "coh": [(4, k) for k in range(8) if k != 4],
            "aec": [(4, k) for k in range(8) if k != 4] + [(5, k) for k in range(8) if k != 5]}
    one = {"wpli": [], "imcoh": [], "coh": [(1, 3)], "aec": [(1, 3)]}
    d_of_zero = (np.sqrt(2.0), 1.0, 1.0, 1.0)                        # correlation_to_distance(0.0, method)
    for measure in MEASURES:
        ex = ref.exact("special_8x250")[measure][0]
        for m, method in enumerate(plv_ref.METHODS):
            dist, val, st = _run(x, ctx, measure, method)
            assert st[0] == 0
            for i, j in zero[measure]:
                assert ex[i, j] == 0.0
                assert val[0, i, j] == 0.0 and val[0, j, i] == 0.0 and not np.signbit(val[0, i, j]), (measure, i, j)
                assert dist[0, i, j] == d_of_zero[m] and dist[0, j, i] == d_of_zero[m], (measure, method, i, j)
            for i, j in one[measure]:
                assert ex[i, j] == 1.0
                assert val[0, i, j] == 1.0 and dist[0, i, j] == 0.0, (measure, method, i, j)
    # the rescaled channel: coh and aec 1 to the bar, imcoh 0 to the bar
    assert abs(_run(x, ctx, "coh")[1][0, 2, 6] - 1.0) <= ref.BAR["coh"]
    assert abs(_run(x, ctx, "aec")[1][0, 2, 6] - 1.0) <= ref.BAR["aec"]
    assert _run(x, ctx, "imcoh")[1][0, 2, 6] <= ref.BAR["imcoh"]
    # n_t = 2: h = 0, so wpli and imcoh are exactly 0
    y = np.array([[[1.0, 2.0], [3.0, -1.0]], [[1.0, -2.0], [0.5, 0.25]]])
    for measure in ("wpli", "imcoh"):
        assert (_run(y, ctx, measure)[1][:, 0, 1] == 0.0).all()


@pytest.mark.parametrize("measure", MEASURES)
def test_alone_in_a_batch_and_through_a_table(ctx, measure):
    """The same bytes for a window alone, inside a batch of 300, and read in place through a window table whose row stride
    is not n_t (overlapping windows of packed recordings of two lengths); the host twin on the same tables."""
    x = plv_ref._rng_windows(300, 5, 33, 21)
    batch = _run(x, ctx, measure)
    assert (batch[2] == 0).all()
    for w in (0, 137, 299):
        assert _same(_run(x[w:w + 1], ctx, measure), [b[w:w + 1] for b in batch])
    rng = np.random.default_rng(62)
    n_ch, n_t, step, lens = 47, 250, 62, [520, 651]
    recs = [rng.standard_normal((n_ch, l)) for l in lens]
    flat = np.concatenate([r.reshape(-1) for r in recs])
    off = np.concatenate([[0], np.cumsum([n_ch * l for l in lens])])
    start, ld, stacked = [], [], []
    for r, l in enumerate(lens):
        for k in range((l - n_t) // step + 1):
            start.append(off[r] + k * step); ld.append(l)
            stacked.append(recs[r][:, k * step:k * step + n_t])
    start, ld, stacked = np.array(start, np.int64), np.array(ld, np.int64), np.stack(stacked)
    in_place = _run(flat, ctx, measure, "abs", tables=(start, ld, n_ch, n_t))
    assert (in_place[2] == 0).all() and _same(in_place, _run(stacked, ctx, measure, "abs"))
    host = engine.connectivity_dist_batch(flat, n_t=n_t, win_start=start, win_ld=ld, n_ch=n_ch, measure=measure, method="abs",
                                          ctx=ctx)
    assert _same(host, in_place)


@pytest.mark.parametrize("measure", MEASURES)
def test_non_finite_sample_flags_its_window_only(ctx, measure):
    x = plv_ref._rng_windows(5, 6, 250, 31)
    clean = _run(x, ctx, measure)
    for bad in (np.nan, np.inf, -np.inf):
        y = x.copy()
        y[2, 5, 249] = bad                                          # the last sample of the last row
        dist, val, st = _run(y, ctx, measure)
        assert st.tolist() == [0, 0, _lib.TDA_WIN_NOT_FINITE, 0, 0]
        assert np.isnan(dist[2]).all() and np.isnan(val[2]).all()
        for w in (0, 1, 3, 4):
            assert dist[w].tobytes() == clean[0][w].tobytes() and val[w].tobytes() == clean[1][w].tobytes()
        d2, none, st2 = _run(y, ctx, measure, want_value=False)      # ... and without a value buffer
        assert none is None and d2.tobytes() == dist.tobytes() and st2.tobytes() == st.tobytes()


@pytest.mark.parametrize("measure", MEASURES)
def test_value_buffer_is_optional(ctx, measure):
    """value NULL: the distances are the same bytes, and a buffer the caller keeps beside them is not touched."""
    import torch
    x = plv_ref.cases()["rand_17x64"]
    dist, val, st = _run(x, ctx, measure, "sqrt")
    d2, none, st2 = _run(x, ctx, measure, "sqrt", want_value=False)
    assert none is None and d2.tobytes() == dist.tobytes() and (st2 == 0).all()
    dev = _dev(ctx)
    both = torch.full((2,) + dist.shape, FILL, dtype=torch.float64, device=dev)     # [0]: dist, [1]: the caller's fill
    engine.connectivity_dist_dev(torch.from_numpy(np.array(x)).to(dev), measure=measure, method="sqrt", out=both[0], ctx=ctx)
    torch.cuda.synchronize()
    assert both[0].cpu().numpy().tobytes() == dist.tobytes() and (both[1] == FILL).all()


def test_refusals_launch_nothing(ctx):
    import torch
    dev = _dev(ctx)
    g8 = engine.plv_g_table(8, dev)

    def refused(sig, measure=0, method=0):
        n_win, n_ch = sig.shape[0], max(sig.shape[1], 1)
        out = torch.full((n_win, n_ch, n_ch), FILL, dtype=torch.float64, device=dev)
        val = torch.full((n_win, n_ch, n_ch), FILL, dtype=torch.float64, device=dev)
        st = torch.full((n_win,), -5, dtype=torch.int32, device=dev)
        with pytest.raises(_lib.TdaError):
            ctx.check(ctx.lib.tda_connectivity_dist_batch_dev(ctx.h, engine._tp(torch.from_numpy(sig).to(dev)), None, None,
                                                              sig.shape[0], sig.shape[1], sig.shape[2], engine._tp(g8), measure,
                                                              method, engine._tp(out), engine._tp(val), engine._tp(st),
                                                              engine._stream()))
        torch.cuda.synchronize()
        assert (out == FILL).all() and (val == FILL).all() and (st == -5).all()
        dist = np.full((n_win, n_ch, n_ch), FILL)
        status = np.full(n_win, -5, np.int32)
        g_host = np.zeros(max(sig.shape[2], 8))
        with pytest.raises(_lib.TdaError):                           # the host twin refuses before it stages anything
            ctx.check(ctx.lib.tda_connectivity_dist_batch(ctx.h, engine.ptr(sig), None, None, sig.shape[0], sig.shape[1],
                                                          sig.shape[2], engine.ptr(g_host), measure, method,
                                                          engine.ptr(dist), None, engine.ptr(status)))
        assert (dist == FILL).all() and (status == -5).all()

    refused(np.zeros((2, 1, 8)))                                    # n_ch < 2
    refused(np.zeros((2, _lib.PLV_MAX_CHANNELS + 1, 8)))            # n_ch > TDA_PLV_MAX_CHANNELS
    refused(np.zeros((2, 3, 1)))                                    # n_t < 2
    refused(np.zeros((1, 3, _lib.PLV_MAX_SAMPLES + 1)))             # n_t > TDA_PLV_MAX_SAMPLES
    refused(np.zeros((2, 3, 8)), measure=4)                         # an unknown measure number
    refused(np.zeros((2, 3, 8)), measure=-1)
    refused(np.zeros((2, 3, 8)), method=4)                          # an unknown method number
    refused(np.zeros((2, 3, 8)), method=-1)
    flat, tab = torch.zeros(64, dtype=torch.float64, device=dev), torch.zeros(2, dtype=torch.int64, device=dev)
    for a, b in ((tab, None), (None, tab)):                         # one table without the other
        st = torch.full((2,), -5, dtype=torch.int32, device=dev)
        with pytest.raises(_lib.TdaError):
            ctx.check(ctx.lib.tda_connectivity_dist_batch_dev(ctx.h, engine._tp(flat), engine._tp(a), engine._tp(b), 2, 2, 8,
                                                              engine._tp(g8), 0, 0, engine._tp(flat), None, engine._tp(st), None))
        torch.cuda.synchronize()
        assert (st == -5).all() and (flat == 0).all()
    for measure in MEASURES:
        with pytest.raises(_lib.TdaError):
            engine.connectivity_dist_batch(np.zeros((1, 3, _lib.PLV_MAX_SAMPLES + 1)), measure=measure, ctx=ctx)
        with pytest.raises(_lib.TdaError):
            engine.connectivity_dist_dev(flat, n_t=_lib.PLV_MAX_SAMPLES + 1, win_start_t=tab, win_ld_t=tab, n_ch=3,
                                         measure=measure, ctx=ctx)
        # the limits themselves are accepted; no window is no launch and no error
        d, v, st = _run(np.ones((1, 2, 2)), ctx, measure)
        assert st[0] == 0 and v[0, 0, 0] == v[0, 1, 1] == 1.0 and d[0, 0, 0] == d[0, 1, 1] == 0.0
        assert engine.connectivity_dist_batch(np.zeros((0, 3, 8)), measure=measure, ctx=ctx)[0].shape == (0, 3, 3)
    with pytest.raises(ValueError):
        engine.connectivity_dist_dev(flat.view(1, 2, 32), measure="plv", ctx=ctx)


@pytest.mark.parametrize("measure", MEASURES)
@pytest.mark.parametrize("name, method", [("rand_3x65", "euclidean"), ("rand_47x250", "standard"), ("rand_64x256", "sqrt")])
def test_host_twin_equals_dev_form(ctx, name, method, measure):
    x = plv_ref.cases()[name].copy()
    if x.shape[0] > 1:
        x[1, 0, 0] = np.nan
    host = engine.connectivity_dist_batch(x, measure=measure, method=method, ctx=ctx)
    assert _same(host, _run(x, ctx, measure, method))
    no_val = engine.connectivity_dist_batch(x, measure=measure, method=method, want_value=False, ctx=ctx)
    assert no_val[1] is None and no_val[0].tobytes() == host[0].tobytes()


@pytest.mark.parametrize("measure", MEASURES)
def test_utils_matrix_and_persistence(ctx, measure):
    x = plv_ref.cases()["rand_47x250"][1]
    v = utils.compute_connectivity_matrix(x, measure)
    assert v.shape == (47, 47) and np.abs(v - ref.exact("rand_47x250")[measure][1]).max() <= ref.BAR[measure]
    for method in ("euclidean", "abs"):
        dist, _, st = engine.connectivity_dist_batch(x, measure=measure, method=method, ctx=ctx)
        assert st[0] == 0
        h0, h1, rst = engine.rips_dm_batch(dist, h1_cap=utils._h1_cap(47), ctx=ctx)
        got = utils.compute_connectivity_persistence(x, measure, method=method)
        assert rst[0] == 0 and len(got) == 2 and len(h1[0]) > 0
        assert got[0].tobytes() == h0[0].tobytes() and got[1].tobytes() == h1[0].tobytes()
        assert got[0].shape == (47, 2) and np.isinf(got[0][-1, 1])
    y = x.copy()
    y[3, 7] = np.inf
    with pytest.raises(ValueError):
        utils.compute_connectivity_matrix(y, measure)
    with pytest.raises(ValueError):
        utils.compute_connectivity_persistence(y, measure)
    with pytest.raises(_lib.TdaError):
        utils.compute_connectivity_matrix(np.zeros((2, _lib.PLV_MAX_SAMPLES + 1)), measure)
