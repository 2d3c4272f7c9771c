"""
GPU tests of the network curves (csrc/network.hip; include/tdaeeg.h, "Network curves"): bytes against tests/network_ref.py
for counts, measures and nodal.  The shapes are the smallest that can break the kernel: the mask word boundary and the last
bit of each word (63, 64, 65, 127, 128), the one- and two-word templates, fewer and more grid points than waves, sparse
scales with many components and long paths beside dense ones, graphs with known answers, the key rules, the three input
forms with their status words, batches, means and the refusals.
"""
import ctypes as C

import numpy as np
import pytest

import euler_ref as er
import network_cases as nc
import network_ref as nr

pytestmark = pytest.mark.gpu

SENT = -7


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda", 0))


def _sym_random(n_win, n, seed, hi=2.2):
    rng = np.random.default_rng(seed)
    d = rng.random((n_win, n, n)) * hi
    return (d + d.transpose(0, 2, 1)) / 2


def _grid(n_grid, seed):
    """[1.1] and then unsorted scales in [0.05, 0.9]: many components and long paths at the small ones, one component
    at the large ones."""
    rng = np.random.default_rng(seed)
    return np.concatenate([[1.1], rng.random(n_grid - 1) * 0.85 + 0.05])[:n_grid]


def _ref_dm(dms, grid, thresh=2.0, symmetrise=True):
    return nr.stack([nr.block_dm(d, grid, thresh, symmetrise) for d in dms])


def _net_dm(dms, grid, thresh=2.0, symmetrise=True, nodal=True, ctx=None):
    from tda_eeg_audio_amd import engine
    net = engine.network_dm_dev(_dev(dms), _dev(np.asarray(grid, dtype=np.float64)), nodal, thresh, symmetrise, ctx=ctx)
    return net.to_host()


def _same(out, ref, what=""):
    cnt, mea, nod = ref
    assert out["counts"].dtype == np.int32 and out["counts"].shape == cnt.shape, what
    assert out["counts"].tobytes() == cnt.tobytes(), (what, np.argwhere(out["counts"] != cnt)[:5])
    assert out["measures"].dtype == np.float64 and out["measures"].shape == mea.shape, what
    assert out["measures"].tobytes() == mea.tobytes(), (what, np.argwhere(out["measures"] != mea)[:5])
    if "nodal" in out:
        assert out["nodal"].dtype == np.int32 and out["nodal"].shape == nod.shape, what
        assert out["nodal"].tobytes() == nod.tobytes(), (what, np.argwhere(out["nodal"] != nod)[:5])


# (n, n_grid, windows)
DM_CASES = [(1, 1, 3), (2, 3, 3), (3, 5, 3), (47, 7, 3), (63, 3, 2), (64, 5, 2), (65, 5, 2), (127, 3, 1), (128, 5, 1), (9, 256, 2)]


@pytest.mark.parametrize("n,n_grid,n_win", DM_CASES)
def test_distance_matrices(ctx, n, n_grid, n_win):
    dms = _sym_random(n_win, n, 1000 + n)
    grid = _grid(n_grid, 200 + n_grid)             # (seeds at which the 5- and 7-point grids hold a scale in 0.1 .. 0.3)
    out = _net_dm(dms, grid, ctx=ctx)
    ref = _ref_dm(dms, grid)
    _same(out, ref, (n, n_grid))
    assert (out["status"] == 0).all()
    if n in (47, 65, 128):
        comps, diam = ref[0][:, 5], ref[0][:, 9]
        assert comps.max() > 1 and comps.min() == 1 and diam.max() >= 4          # both regimes, and a search of some depth


@pytest.mark.parametrize("name", sorted(nc.known()))
def test_known_answers(ctx, name):
    A, cnt, mea = nc.known()[name]
    d = nc.dm_of_graph(A)[None]
    # the graph at SCALE between an empty and a complete one, all on one wave's grid points (0, 4, 8) and on others
    grid = np.array([nc.SCALE, 0.1, 2.0, 0.1, 0.1, nc.SCALE, 2.0, 2.0, nc.SCALE])
    out = _net_dm(d, grid, ctx=ctx)
    for g in (0, 5, 8):
        assert out["counts"][0, :, g].tolist() == cnt, (name, g)
        assert out["measures"][0, :, g].tobytes() == np.array(mea, np.float64).tobytes(), (name, g, out["measures"][0, :, g])
    _same(out, _ref_dm(d, grid), name)


def test_key_rules(ctx):
    n = 13
    rng = np.random.default_rng(11)
    # grid points equal to keys and one ulp (of the double) below them
    d = _sym_random(2, n, 12)
    keys = er.keys_dm(d[0])
    picks = np.sort(keys[np.tril_indices(n, -1)].astype(np.float64))[[3, 20, 40, 70]]
    grid = np.concatenate([picks, np.nextafter(picks, -np.inf)])
    out = _net_dm(d, grid, ctx=ctx)
    _same(out, _ref_dm(d, grid), "key and one ulp below")
    assert (out["counts"][0, 0, :4] - out["counts"][0, 0, 4:] >= 1).all()
    # thresh cutting the filtration: (float)thresh is what the keys are compared with
    for thresh in (0.9, float(picks[2]), float(np.nextafter(picks[2], -np.inf))):
        _same(_net_dm(d, grid, thresh=thresh, ctx=ctx), _ref_dm(d, grid, thresh=thresh), thresh)
    # symmetrise 0 and 1 on a matrix that is not symmetric and has negative entries
    raw = rng.random((2, n, n)) * 2.4 - 0.4
    g5 = _grid(5, 13)
    o1, o0 = _net_dm(raw, g5, symmetrise=True, ctx=ctx), _net_dm(raw, g5, symmetrise=False, ctx=ctx)
    _same(o1, _ref_dm(raw, g5, symmetrise=True), "symmetrise 1")
    _same(o0, _ref_dm(raw, g5, symmetrise=False), "symmetrise 0")
    assert o0["counts"].tobytes() != o1["counts"].tobytes()
    # a NaN entry, and a NaN in a descending grid
    d = _sym_random(1, n, 14)
    d[0, 7, 3] = d[0, 3, 7] = np.nan
    grid = np.array([2.5, 1.4, np.nan, 0.9, 0.3])
    out = _net_dm(d, grid, thresh=3.0, ctx=ctx)
    _same(out, _ref_dm(d, grid, thresh=3.0), "NaN")
    assert out["counts"][0, :, 2].tolist() == [0, n, 0, 0, 0, n, 1, 0, 0, 0] and out["counts"][0, 0, 0] == n * (n - 1) // 2 - 1
    assert out["counts"][0, 9, 0] == 2                              # the missing edge is two hops


@pytest.mark.parametrize("n", [13, 70])
def test_repeated_and_saturated_scales(ctx, n):
    """A wave keeps the results of its previous grid point (g - 4) when the edge count has not changed: scales that repeat,
    scales past the largest key, scales below the smallest, a NaN after an empty graph, and neighbours that differ."""
    d = _sym_random(2, n, 15, hi=1.5)
    grid = np.array([3.0, 0.001, 0.6, np.nan, 2.5, 0.0005, 0.6, -1.0, 1.6, 0.9, 0.61, np.nan, 0.3, 0.9, 0.6, 0.0, 9.0])
    out = _net_dm(d, grid, ctx=ctx)
    _same(out, _ref_dm(d, grid), n)
    assert (out["counts"][:, :, 0] == out["counts"][:, :, 4]).all() and (out["nodal"][:, :, 0] == out["nodal"][:, :, 8]).all()
    assert not out["counts"][:, 0, [1, 5, 3, 7, 11, 15]].any()


def test_agreement_with_euler(ctx):
    from tda_eeg_audio_amd import engine
    for n in (47, 70):
        dm_t, grid_t = _dev(_sym_random(3, n, 70 + n)), _dev(_grid(7, 71))
        net = engine.network_dm_dev(dm_t, grid_t, ctx=ctx)
        f, _, _ = engine.euler_dm_dev(dm_t, grid_t, 2, ctx=ctx)
        assert (net.counts[:, 0] == f[:, 1]).all() and (net.counts[:, 4] == f[:, 2]).all() and int(f[:, 2].max()) > 0
        assert net.nodal is None


# ---------------------------------------------------------------- cloud forms
CLOUD_P = [2, 3, 64, 65, 128, 129]


def _clouds(dim, seed, p_cap=129):
    rng = np.random.default_rng(seed)
    pc = rng.random((len(CLOUD_P) + 1, p_cap, dim)) * 3.0 - 1.0
    n_pts = np.array(CLOUD_P + [40], np.int32)
    pc[-1, :, 0] = 0.25                                           # a constant column: range 0 -> 1
    return pc, n_pts


@pytest.mark.parametrize("dim,normalise", [(3, True), (2, False)])
def test_clouds(ctx, dim, normalise):
    from tda_eeg_audio_amd import engine
    pc, n_pts = _clouds(dim, 20 + dim)
    grid = np.array([0.12, 0.3, 0.2]) if normalise else np.array([0.4, 0.9, 0.6])
    out = engine.network_cloud_dev(_dev(pc), _dev(n_pts), _dev(grid), True, normalise, ctx=ctx).to_host()
    st = out["status"]
    for w, P in enumerate(n_pts):
        ref, rst = nr.block_cloud(pc[w], int(P), grid, 2.0, normalise)
        assert st[w] == rst, (w, P)
        _same({k: out[k][w] for k in ("counts", "measures", "nodal")}, ref, (w, P))
    assert st.tolist() == [4, 0, 0, 0, 0, 16, 0]
    assert out["nodal"].shape == (7, 5, 3, 129) and not out["nodal"][6, :, :, 40:].any()
    for w in (0, 5):
        assert not out["counts"][w].any() and not out["nodal"][w].any()
        assert out["measures"][w].tobytes() == np.zeros((4, 3)).tobytes()
    # the one-word template on the same clouds: p_cap = 64
    sub, n_sub = np.ascontiguousarray(pc[[1, 2, 6], :64]), np.array([3, 64, 40], np.int32)
    o64 = engine.network_cloud_dev(_dev(sub), _dev(n_sub), _dev(grid), True, normalise, ctx=ctx).to_host()
    assert o64["counts"].tobytes() == out["counts"][[1, 2, 6]].tobytes() and not o64["status"].any()
    assert o64["measures"].tobytes() == out["measures"][[1, 2, 6]].tobytes()
    assert o64["nodal"].tobytes() == np.ascontiguousarray(out["nodal"][[1, 2, 6], :, :, :64]).tobytes()
    # the host form
    ch, mh, nh, sh = engine.network_cloud_batch(pc, grid, True, n_pts=n_pts, normalise=normalise, ctx=ctx)
    assert ch.tobytes() == out["counts"].tobytes() and mh.tobytes() == out["measures"].tobytes()
    assert nh.tobytes() == out["nodal"].tobytes() and sh.tobytes() == st.tobytes()


def test_takens_windows(ctx):
    import torch
    from tda_eeg_audio_amd import engine, synth
    taus = np.array([102, 2, 0, 125, 124, 40, -3], np.int32)        # P = 23, 123, refused, 0, 1, 85, refused
    sig = synth.audio_windows(len(taus), "alpha", seed=3)
    grid = np.array([0.1, 0.35, 0.2, 0.6])
    npts_t = torch.full((len(taus),), SENT, dtype=torch.int32, device="cuda:0")
    out = engine.network_takens_dev(_dev(sig), _dev(taus), _dev(grid), True, n_points_t=npts_t, ctx=ctx).to_host()
    st, npts = out["status"], npts_t.cpu().numpy()
    for w, tau in enumerate(taus):
        ref, rst = nr.block_takens(sig[w], int(tau), grid)
        assert st[w] == rst, (w, tau)
        _same({k: out[k][w] for k in ("counts", "measures", "nodal")}, ref, (w, tau))
    assert st.tolist() == [0, 0, 16, 4, 4, 0, 16] and out["nodal"].shape == (7, 5, 4, 128)
    assert npts[:2].tolist() == [23, 123] and npts[3:6].tolist() == [0, 1, 85]          # as the Euler form
    for w in (2, 3, 4, 6):
        assert not out["counts"][w].any() and not out["nodal"][w].any() and not out["measures"][w].any()
    # the host form, with and without n_points
    ch, mh, nh, ph, sh = engine.network_takens_batch(sig, taus, grid, True, ctx=ctx)
    assert ch.tobytes() == out["counts"].tobytes() and mh.tobytes() == out["measures"].tobytes()
    assert nh.tobytes() == out["nodal"].tobytes() and sh.tobytes() == st.tobytes() and ph.tolist() == npts.tolist()
    p = engine.ptr
    w, tau, c2, m2, s2 = engine.f64(sig), engine.i32(taus), np.zeros_like(ch), np.ones_like(mh), np.zeros_like(sh)
    ctx.check(ctx.lib.tda_network_takens_batch(ctx.h, p(w), p(tau), len(taus), sig.shape[1], 3, 2, 2.0, p(grid), len(grid),
                                               p(c2), p(m2), None, None, p(s2)))
    assert c2.tobytes() == ch.tobytes() and m2.tobytes() == mh.tobytes() and s2.tobytes() == st.tobytes()


# ---------------------------------------------------------------- batches, nodal, host forms
def test_batch_and_nodal(ctx):
    import torch
    from tda_eeg_audio_amd import engine
    dms = _sym_random(20, 47, 40)
    grid = _grid(5, 41)
    dm_t, grid_t = _dev(dms), _dev(grid)
    # an oversized out pre-filled with a sentinel: the batch is fully overwritten, the tail is not touched
    big = engine.DeviceNetworkCurves(23, 5, 47, dm_t.device, nodal=True)
    for t in (big.counts, big.nodal, big.status):
        t.fill_(SENT)
    big.measures.fill_(float(SENT))
    engine.network_dm_dev(dm_t, grid_t, True, out=big, ctx=ctx)
    out = big.to_host()
    for k in ("counts", "measures", "nodal", "status"):
        assert (out[k][20:] == SENT).all(), k
    assert not out["status"][:20].any()
    _same({k: out[k][[3, 19]] for k in ("counts", "measures", "nodal")}, _ref_dm(dms[[3, 19]], grid), "batch")
    ref_all = {k: out[k][:20] for k in ("counts", "measures", "nodal")}
    assert (ref_all["counts"][:, 5] >= 1).all() and (ref_all["counts"][:, 6] >= 1).all()      # no sentinel left behind
    # a window alone and inside the batch
    for w in (0, 7, 19):
        alone = _net_dm(dms[w:w + 1], grid, ctx=ctx)
        for k in ("counts", "measures", "nodal"):
            assert alone[k][0].tobytes() == out[k][w].tobytes(), (w, k)
    # nodal absent changes no other byte
    plain = engine.DeviceNetworkCurves(20, 5, 47, dm_t.device)
    plain.counts.fill_(SENT); plain.measures.fill_(float(SENT)); plain.status.fill_(SENT)
    engine.network_dm_dev(dm_t, grid_t, False, out=plain, ctx=ctx)
    ph = plain.to_host()
    assert "nodal" not in ph and ph["counts"].tobytes() == out["counts"][:20].tobytes()
    assert ph["measures"].tobytes() == out["measures"][:20].tobytes() and not ph["status"].any()
    # the host form
    ch, mh, nh, sh = engine.network_dm_batch(dms, grid, True, ctx=ctx)
    assert ch.tobytes() == ph["counts"].tobytes() and mh.tobytes() == ph["measures"].tobytes() and not sh.any()
    assert nh.tobytes() == out["nodal"][:20].tobytes()
    ch2, mh2, nh2, _ = engine.network_dm_batch(dms, grid, ctx=ctx)
    assert nh2 is None and ch2.tobytes() == ch.tobytes() and mh2.tobytes() == mh.tobytes()
    torch.cuda.synchronize()


# ---------------------------------------------------------------- means and refusals
def test_group_means(ctx):
    from tda_eeg_audio_amd import engine
    pc, n_pts = _clouds(3, 50)                                     # statuses 4, 0, 0, 0, 0, 16, 0
    grid = np.array([0.12, 0.3, 0.2])
    grid_t = _dev(grid)
    seg = np.array([0, 0, 1, 6, 7], np.int32)                       # sizes 0, 1 (degenerate alone), 5, 1
    net = engine.network_cloud_dev(_dev(pc), _dev(n_pts), grid_t, True, seg_off_t=_dev(seg), skip_mask=4 | 16, ctx=ctx)
    out = net.to_host()
    st = out["status"]
    assert out["mean_counts"].shape == (4, 10, 3) and out["mean_measures"].shape == (4, 4, 3)
    assert out["mean_nodal"].shape == (4, 5, 3, 129)
    assert out["mean_counts"].tobytes() == nr.mean_exact(out["counts"], seg, st, 4 | 16).tobytes()
    assert out["mean_nodal"].tobytes() == nr.mean_exact(out["nodal"], seg, st, 4 | 16).tobytes()
    assert out["mean_measures"].tobytes() == nr.mean_seq(out["measures"], seg, st, 4 | 16).tobytes()
    for k in ("mean_counts", "mean_measures", "mean_nodal"):
        assert np.isnan(out[k][0]).all() and np.isnan(out[k][1]).all() and not np.isnan(out[k][2:]).any(), k
    # nothing skipped: the flagged windows' zeros are members; counts alone
    mc, mm, mn = engine.network_mean_dev(net.counts, None, None, 7, 3, 129, seg_off_t=_dev(seg), ctx=ctx)
    assert mm is None and mn is None and mc.cpu().numpy().tobytes() == nr.mean_exact(out["counts"], seg).tobytes()
    # seg_off = NULL: every window its own group
    mc, mm, mn = engine.network_mean_dev(net.counts, net.measures, net.nodal, 7, 3, 129, ctx=ctx)
    assert mc.cpu().numpy().tobytes() == out["counts"].astype(np.float64).tobytes()
    assert mm.cpu().numpy().tobytes() == (0.0 + out["measures"]).tobytes()
    assert mn.cpu().numpy().tobytes() == out["nodal"].astype(np.float64).tobytes()
    own = engine.network_cloud_dev(_dev(pc), _dev(n_pts), grid_t, mean=True, ctx=ctx)
    assert own.mean_nodal is None and own.mean_measures.cpu().numpy().tobytes() == mm.cpu().numpy().tobytes()
    # the host form
    hp = lambda a: a.ctypes.data_as(C.c_void_p)                    # noqa: E731
    hc, hm, hn = np.full((4, 10, 3), -1.0), np.full((4, 4, 3), -1.0), np.full((4, 5, 3, 129), -1.0)
    ctx.check(ctx.lib.tda_network_mean(ctx.h, hp(out["counts"]), hp(out["measures"]), hp(out["nodal"]), 7, 3, 129, hp(seg), 4,
                                       hp(st), 4 | 16, hp(hc), hp(hm), hp(hn)))
    assert hc.tobytes() == out["mean_counts"].tobytes() and hm.tobytes() == out["mean_measures"].tobytes()
    assert hn.tobytes() == out["mean_nodal"].tobytes()
    h7 = np.full((7, 4, 3), -1.0)
    ctx.check(ctx.lib.tda_network_mean(ctx.h, None, hp(out["measures"]), None, 7, 3, 0, None, 7, None, 0, None, hp(h7), None))
    assert h7.tobytes() == (0.0 + out["measures"]).tobytes()


def _msg(ctx):
    buf = C.create_string_buffer(512)
    ctx.lib.tda_last_error(ctx.h, buf, 512)
    return buf.value.decode()


def test_refusals(ctx):
    import torch
    from tda_eeg_audio_amd import _lib, engine
    dev = torch.device("cuda", 0)
    p = engine._tp
    dm = torch.zeros((2, 129, 129), dtype=torch.float64, device=dev)
    grid = torch.zeros(_lib.MAX_GRID + 1, dtype=torch.float64, device=dev)
    cnt = torch.full((2 * 10 * (_lib.MAX_GRID + 1),), SENT, dtype=torch.int32, device=dev)
    mea = torch.full((2 * 4 * (_lib.MAX_GRID + 1),), -7.0, dtype=torch.float64, device=dev)
    nod = torch.full((2 * 5 * 4 * 129,), SENT, dtype=torch.int32, device=dev)
    st = torch.full((2,), SENT, dtype=torch.int32, device=dev)
    mean = torch.full((2 * 10 * 4,), -7.0, dtype=torch.float64, device=dev)
    tau = torch.ones(2, dtype=torch.int32, device=dev)
    lib, h = ctx.lib, ctx.h
    outs = (p(cnt), p(mea), p(nod))
    calls = [
        lambda: lib.tda_network_dm_batch_dev(h, p(dm), 2, 129, 2.0, 1, p(grid), 4, *outs, p(st), None),        # n
        lambda: lib.tda_network_dm_batch_dev(h, p(dm), 2, 0, 2.0, 1, p(grid), 4, *outs, p(st), None),
        lambda: lib.tda_network_dm_batch_dev(h, p(dm), 2, 9, 2.0, 1, p(grid), 0, *outs, p(st), None),          # n_grid
        lambda: lib.tda_network_dm_batch_dev(h, p(dm), 2, 9, 2.0, 1, p(grid), _lib.MAX_GRID + 1, *outs, p(st), None),
        lambda: lib.tda_network_cloud_batch_dev(h, p(dm), p(tau), 2, 8, 5, 1, 2.0, p(grid), 4, *outs, p(st), None),   # dim
        lambda: lib.tda_network_cloud_batch_dev(h, p(dm), p(tau), 2, 8, 0, 1, 2.0, p(grid), 4, *outs, p(st), None),
        lambda: lib.tda_network_cloud_batch_dev(h, p(dm), p(tau), 2, 0, 3, 1, 2.0, p(grid), 4, *outs, p(st), None),   # p_cap
        lambda: lib.tda_network_takens_batch_dev(h, p(dm), p(tau), 2, 250, 5, 2, 2.0, p(grid), 4, *outs, None, p(st), None),
        lambda: lib.tda_network_takens_batch_dev(h, p(dm), p(tau), 2, 0, 3, 2, 2.0, p(grid), 4, *outs, None, p(st), None),
        lambda: lib.tda_network_mean_dev(h, p(cnt), None, None, 2, 4, 9, None, 1, None, 0, p(mean), None, None, None),  # n_seg
        lambda: lib.tda_network_mean_dev(h, p(cnt), None, None, 2, 0, 9, None, 2, None, 0, p(mean), None, None, None),  # n_grid
        lambda: lib.tda_network_mean_dev(h, p(cnt), None, None, 2, 4, 9, None, 2, None, 0, None, p(mean), None, None),  # pairs
        lambda: lib.tda_network_mean_dev(h, None, None, p(nod), 2, 4, 0, None, 2, None, 0, None, None, p(mean), None),  # n_node
    ]
    for k, call in enumerate(calls):
        assert call() == 1, k                                      # TDA_ERR_INVALID
        assert _msg(ctx), k
    torch.cuda.synchronize()
    assert (cnt == SENT).all() and (mea == -7.0).all() and (nod == SENT).all() and (st == SENT).all() and (mean == -7.0).all()
    # the host forms refuse before anything is staged or written
    hp = lambda a: a.ctypes.data_as(C.c_void_p)                   # noqa: E731
    ch, mh, sh = np.full((2, 10, 4), SENT, np.int32), np.full((2, 4, 4), -7.0), np.full(2, SENT, np.int32)
    dmh, gh = np.zeros((2, 9, 9)), np.zeros(4)
    assert lib.tda_network_dm_batch(h, hp(dmh), 2, 9, 2.0, 1, hp(gh), 0, hp(ch), hp(mh), None, hp(sh)) == 1
    assert lib.tda_network_dm_batch(h, hp(dmh), 2, 129, 2.0, 1, hp(gh), 4, hp(ch), hp(mh), None, hp(sh)) == 1
    assert lib.tda_network_mean(h, hp(ch), None, None, 2, 4, 9, None, 1, None, 0, hp(np.zeros(80)), None, None) == 1
    assert (ch == SENT).all() and (mh == -7.0).all() and (sh == SENT).all()
    # the Python front end refuses with ValueError before any call
    with pytest.raises(ValueError):
        engine.network_dm_dev(dm[:, :9, :9].contiguous(), grid, ctx=ctx)
    with pytest.raises(ValueError):
        engine.network_dm_batch(np.zeros((1, 9, 9)), [], ctx=ctx)
    # an empty batch is no error and touches nothing
    assert lib.tda_network_dm_batch_dev(h, None, 0, 9, 2.0, 1, None, 4, None, None, None, None, None) == 0


# ---------------------------------------------------------------- composition with the EEG route
def test_eeg_windows(ctx):
    from oracle import port
    from tda_eeg_audio_amd import engine, synth
    win = synth.eeg_windows(4, seed=60, windows_per_recording=4)
    grid = np.linspace(0.0, 2.0, 9)
    net = engine.network_eeg_windows_dev(_dev(win), _dev(grid), True, ctx=ctx).to_host()
    ref = nr.stack([nr.curves(er.keys_dm(port.corr_dist(w)[1]), grid) for w in win])
    _same(net, ref, "eeg windows")
    assert not net["status"].any() and net["counts"][:, 4].max() > 0
