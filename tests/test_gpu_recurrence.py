"""
GPU tests of the recurrence curves (csrc/recurrence.hip; include/tdaeeg.h, "Recurrence curves"): bytes against
tests/recurrence_ref.py for counts, hist and the five ratio measures; the two entropies to recurrence_ref.ENTROPY_BAR, and
as bytes where the histogram has a single bin.  The shapes are the smallest that can break the kernel: the mask word
boundary and the last bit of each word (63, 64, 65, 127, 128), the one- and two-word templates, fewer and more grid points
than waves, every Theiler band that meets a word boundary or the window's size, plots with known answers, the key rules, the
three input forms with their status words, batches, means and the refusals.
"""
import ctypes as C

import numpy as np
import pytest

import euler_ref as er
import recurrence_cases as rc
import recurrence_ref as rr

pytestmark = pytest.mark.gpu

SENT = -7


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda", 0))


def _ref_dm(dms, grid, par=(1, 2, 2), thresh=2.0, symmetrise=True):
    return rr.stack([rr.block_dm(d, grid, *par, thresh, symmetrise) for d in dms])


def _rq_dm(dms, grid, par=(1, 2, 2), thresh=2.0, symmetrise=True, hist=True, ctx=None):
    from tda_eeg_audio_amd import engine
    out = engine.recurrence_dm_dev(_dev(dms), _dev(np.asarray(grid, dtype=np.float64)), *par, hist, thresh, symmetrise, ctx=ctx)
    return out.to_host()


def _same(out, ref, what=""):
    """counts, hist and the ratio rows as bytes; the entropy rows to the bar, and exactly 0.0 (bytes) where the reference
    histogram has at most one bin at or above the minimum length (the reference's own value there is 0.0)."""
    cnt, mea, his = ref
    assert out["counts"].dtype == np.int32 and out["counts"].shape == cnt.shape, what
    assert out["counts"].tobytes() == cnt.tobytes(), (what, np.argwhere(out["counts"] != cnt)[:5])
    got = out["measures"]
    assert got.dtype == np.float64 and got.shape == mea.shape, what
    ratio, ent = list(rr.RATIO_ROWS), list(rr.ENTROPY_ROWS)
    assert np.ascontiguousarray(got[..., ratio, :]).tobytes() == np.ascontiguousarray(mea[..., ratio, :]).tobytes(), \
        (what, np.argwhere(got[..., ratio, :] != mea[..., ratio, :])[:5])
    err = np.abs(got[..., ent, :] - mea[..., ent, :])
    print(f"{what}: entropy |kernel - numpy statement| max {err.max(initial=0.0):.3e}, bar {rr.ENTROPY_BAR:.3e}")
    assert (err <= rr.ENTROPY_BAR).all(), (what, err.max())
    zero = mea[..., ent, :] == 0.0
    assert np.ascontiguousarray(got[..., ent, :][zero]).tobytes() == np.zeros(int(zero.sum())).tobytes(), what
    if "hist" in out:
        assert out["hist"].dtype == np.int32 and out["hist"].shape == his.shape, what
        assert out["hist"].tobytes() == his.tobytes(), (what, np.argwhere(out["hist"] != his)[:5])


@pytest.mark.parametrize("case", rc.DM_CASES, ids=lambda c: "n%d_g%d_w%d_th%d_l%d_v%d_%d" % c)
def test_distance_matrices(ctx, case):
    n, n_grid, n_win, theiler, l_min, v_min, _ = case
    dms, grid = rc.dm_case(case)
    par = (theiler, l_min, v_min)
    out = _rq_dm(dms, grid, par, ctx=ctx)
    ref = _ref_dm(dms, grid, par)
    _same(out, ref, case)
    assert (out["status"] == 0).all()
    if n >= 47 and theiler <= 2:
        assert ref[0][:, 3].max() >= 10 and ref[0][:, 6].max() >= 3 and ref[1][:, 3].max() > 0.5      # lines, a broad histogram


@pytest.mark.parametrize("name", sorted(rc.known()))
def test_known_answers(ctx, name):
    d, par, cnt, mea = rc.known()[name]
    d = d[None]
    # the plot at SCALE between empty ones and full ones, all on one wave's grid points (0, 4, 8) and on others
    grid = np.array([rc.SCALE, -1.0, 2.0, -1.0, -1.0, rc.SCALE, 2.0, 2.0, rc.SCALE])
    out = _rq_dm(d, grid, par, ctx=ctx)
    mea = np.array(mea, np.float64)
    ratio, ent = list(rr.RATIO_ROWS), list(rr.ENTROPY_ROWS)
    for g in (0, 5, 8):
        assert out["counts"][0, :, g].tolist() == cnt, (name, g)
        assert out["measures"][0, ratio, g].tobytes() == mea[ratio].tobytes(), (name, g, out["measures"][0, :, g])
        assert (np.abs(out["measures"][0, ent, g] - mea[ent]) <= rr.ENTROPY_BAR).all(), (name, g)
        for q in ent:                                              # no line or a single bin: 0.0 as bytes
            if mea[q] == 0.0:
                assert out["measures"][0, q, g].tobytes() == np.float64(0.0).tobytes(), (name, g, q)
    _same(out, _ref_dm(d, grid, par), name)


def test_single_bin_entropy_is_zero_bytes(ctx):
    """One non-zero bin: p = 1.0, log(1.0) = 0.0, S = 0.0 - 1.0 * 0.0."""
    # two far-apart pairs of identical points: four recurrences, two diagonal lines and four vertical lines of length 1
    n = 70
    R = np.zeros((n, n), bool)
    for a, b in ((3, 40), (66, 20)):
        R[a, b] = R[b, a] = True
    out = _rq_dm(rc.dm_of_plot(R)[None], [rc.SCALE], (1, 1, 1), ctx=ctx)
    assert out["counts"][0, :, 0].tolist() == [4, 4, 4, 1, 4, 4, 1]
    assert out["hist"][0, :, 0, 0].tolist() == [4, 4] and not out["hist"][0, :, 0, 1:].any()
    assert out["measures"][0, [3, 6], 0].tobytes() == np.zeros(2).tobytes()
    assert out["measures"][0, [1, 2, 4, 5], 0].tolist() == [1.0, 1.0, 1.0, 1.0]
    # the periodic plot with l_min at its longest line: one bin of two lines
    d, _, _, _ = rc.known()["periodic_128"]
    out = _rq_dm(d[None], [rc.SCALE], (1, 121, 1), ctx=ctx)
    assert out["counts"][0, 1:4, 0].tolist() == [2, 242, 121]
    assert out["measures"][0, [3, 6], 0].tobytes() == np.zeros(2).tobytes()


def test_key_rules(ctx):
    n = 13
    rng = np.random.default_rng(11)
    # grid points equal to keys and one ulp (of the double) below them
    d = rc.trajectory_dm(2, n, 12)
    keys = er.keys_dm(d[0])
    picks = np.sort(keys[np.tril_indices(n, -1)].astype(np.float64))[[3, 20, 40, 70]]
    grid = np.concatenate([picks, np.nextafter(picks, -np.inf)])
    out = _rq_dm(d, grid, ctx=ctx)
    _same(out, _ref_dm(d, grid), "key and one ulp below")
    assert (out["counts"][0, 0, :4] - out["counts"][0, 0, 4:] >= 2).all()
    # thresh cutting the filtration: (float)thresh is what the keys are compared with; a key above thresh is absent at
    # every scale
    for thresh in (0.9, float(picks[2]), float(np.nextafter(picks[2], -np.inf))):
        o = _rq_dm(d, np.append(grid, 9.0), thresh=thresh, ctx=ctx)
        _same(o, _ref_dm(d, np.append(grid, 9.0), thresh=thresh), thresh)
        assert o["counts"][0, 0, -1] == 2 * int((keys[np.tril_indices(n, -1)] <= np.float32(thresh)).sum())
    # symmetrise 0 and 1 on a matrix that is not symmetric and has negative entries
    raw = rng.random((2, n, n)) * 2.4 - 0.4
    g5 = rc.grid_of(5, 13)
    o1, o0 = _rq_dm(raw, g5, symmetrise=True, ctx=ctx), _rq_dm(raw, g5, symmetrise=False, ctx=ctx)
    _same(o1, _ref_dm(raw, g5, symmetrise=True), "symmetrise 1")
    _same(o0, _ref_dm(raw, g5, symmetrise=False), "symmetrise 0")
    assert o0["counts"].tobytes() != o1["counts"].tobytes()
    # a NaN entry, and a NaN in a descending grid
    d = rc.trajectory_dm(1, n, 14)
    d[0, 7, 3] = d[0, 3, 7] = np.nan
    grid = np.array([3.5, 1.4, np.nan, 0.9, 0.3])
    out = _rq_dm(d, grid, thresh=4.0, ctx=ctx)
    _same(out, _ref_dm(d, grid, thresh=4.0), "NaN")
    assert not out["counts"][0, :, 2].any() and out["counts"][0, 0, 0] == n * (n - 1) - 2


@pytest.mark.parametrize("n", [13, 70])
def test_repeated_and_unsorted_scales(ctx, n):
    """A wave keeps the results of its previous grid point (g - 4) when the recurrence count has not changed: scales that
    repeat, scales past the largest key, scales below the smallest, a NaN after an empty plot, and neighbours that differ."""
    d = rc.trajectory_dm(2, n, 15, ties=True)
    grid = np.array([3.0, 0.001, 0.6, np.nan, 2.5, 0.0005, 0.6, -1.0, 1.6, 0.9, 0.61, np.nan, 0.3, 0.9, 0.6, 0.0, 9.0])
    out = _rq_dm(d, grid, (2, 2, 2), ctx=ctx)
    _same(out, _ref_dm(d, grid, (2, 2, 2)), n)
    assert (out["counts"][:, :, 0] == out["counts"][:, :, 4]).all() and (out["hist"][:, :, 0] == out["hist"][:, :, 16]).all()
    assert not out["counts"][:, 0, [1, 5, 3, 7, 11]].any()


def test_recurrences_are_twice_the_edges(ctx):
    from tda_eeg_audio_amd import engine
    for n in (47, 70):
        dm_t, grid_t = _dev(rc.trajectory_dm(3, n, 70 + n)), _dev(rc.grid_of(7, 71))
        rq = engine.recurrence_dm_dev(dm_t, grid_t, ctx=ctx)
        net = engine.network_dm_dev(dm_t, grid_t, ctx=ctx)
        assert (rq.counts[:, 0] == 2 * net.counts[:, 0]).all() and int(rq.counts[:, 0].max()) > 0
        assert rq.hist is None


# ---------------------------------------------------------------- cloud forms
CLOUD_P = [2, 3, 64, 65, 128, 129]


def _clouds(dim, seed, p_cap=129):
    """Noisy closed curves in time order, p_cap rows each; the last one has a constant column (range 0 -> 1)."""
    rng = np.random.default_rng(seed)
    i = np.arange(p_cap)
    pc = np.zeros((len(CLOUD_P) + 1, p_cap, dim))
    for w in range(len(pc)):
        ph = 2 * np.pi * rng.uniform(0.03, 0.09) * i
        pc[w] = np.stack([np.cos(ph), np.sin(ph), np.sin(2 * ph)][:dim], axis=1) * 1.5 + rng.normal(0, 0.05, (p_cap, dim))
    n_pts = np.array(CLOUD_P + [40], np.int32)
    pc[-1, :, 0] = 0.25
    return pc, n_pts


@pytest.mark.parametrize("dim,normalise", [(3, True), (2, False)])
def test_clouds(ctx, dim, normalise):
    from tda_eeg_audio_amd import engine
    pc, n_pts = _clouds(dim, 20 + dim)
    grid = np.array([0.12, 0.3, 0.2]) if normalise else np.array([0.4, 0.9, 0.6])
    par = (2, 2, 1)
    out = engine.recurrence_cloud_dev(_dev(pc), _dev(n_pts), _dev(grid), *par, True, normalise, ctx=ctx).to_host()
    st = out["status"]
    for w, P in enumerate(n_pts):
        ref, rst = rr.block_cloud(pc[w], int(P), grid, *par, 2.0, normalise)
        assert st[w] == rst, (w, P)
        _same({k: out[k][w] for k in ("counts", "measures", "hist")}, ref, (w, P))
    assert st.tolist() == [4, 0, 0, 0, 0, 16, 0]
    assert out["hist"].shape == (7, 2, 3, 129) and not out["hist"][6, :, :, 40:].any() and out["counts"][4, 3].max() >= 5
    for w in (0, 5):
        assert not out["counts"][w].any() and not out["hist"][w].any()
        assert out["measures"][w].tobytes() == np.zeros((7, 3)).tobytes()
    # the one-word template on the same clouds: p_cap = 64
    sub, n_sub = np.ascontiguousarray(pc[[1, 2, 6], :64]), np.array([3, 64, 40], np.int32)
    o64 = engine.recurrence_cloud_dev(_dev(sub), _dev(n_sub), _dev(grid), *par, True, normalise, ctx=ctx).to_host()
    assert o64["counts"].tobytes() == out["counts"][[1, 2, 6]].tobytes() and not o64["status"].any()
    assert o64["measures"].tobytes() == out["measures"][[1, 2, 6]].tobytes()
    assert o64["hist"].tobytes() == np.ascontiguousarray(out["hist"][[1, 2, 6], :, :, :64]).tobytes()
    # the host form
    ch, mh, hh, sh = engine.recurrence_cloud_batch(pc, grid, *par, True, n_pts=n_pts, normalise=normalise, ctx=ctx)
    assert ch.tobytes() == out["counts"].tobytes() and mh.tobytes() == out["measures"].tobytes()
    assert hh.tobytes() == out["hist"].tobytes() and sh.tobytes() == st.tobytes()


def test_takens_windows(ctx):
    import torch
    from tda_eeg_audio_amd import engine, synth
    taus = np.array([102, 2, 0, 125, 124, 40, -3], np.int32)        # P = 23, 123, refused, 0, 1, 85, refused
    sig = synth.audio_windows(len(taus), "alpha", seed=3)
    grid = np.array([0.1, 0.35, 0.2, 0.6])
    par = (1, 2, 2)
    npts_t = torch.full((len(taus),), SENT, dtype=torch.int32, device="cuda:0")
    out = engine.recurrence_takens_dev(_dev(sig), _dev(taus), _dev(grid), *par, True, n_points_t=npts_t, ctx=ctx).to_host()
    st, npts = out["status"], npts_t.cpu().numpy()
    for w, tau in enumerate(taus):
        ref, rst = rr.block_takens(sig[w], int(tau), grid, *par)
        assert st[w] == rst, (w, tau)
        _same({k: out[k][w] for k in ("counts", "measures", "hist")}, ref, (w, tau))
    assert st.tolist() == [0, 0, 16, 4, 4, 0, 16] and out["hist"].shape == (7, 2, 4, 128)
    assert npts[:2].tolist() == [23, 123] and npts[3:6].tolist() == [0, 1, 85]          # as the Euler form
    for w in (2, 3, 4, 6):
        assert not out["counts"][w].any() and not out["hist"][w].any() and not out["measures"][w].any()
    # the host form, with and without n_points and hist
    ch, mh, hh, ph, sh = engine.recurrence_takens_batch(sig, taus, grid, *par, True, ctx=ctx)
    assert ch.tobytes() == out["counts"].tobytes() and mh.tobytes() == out["measures"].tobytes()
    assert hh.tobytes() == out["hist"].tobytes() and sh.tobytes() == st.tobytes() and ph.tolist() == npts.tolist()
    p = engine.ptr
    w, tau, c2, m2, s2 = engine.f64(sig), engine.i32(taus), np.zeros_like(ch), np.ones_like(mh), np.zeros_like(sh)
    ctx.check(ctx.lib.tda_recurrence_takens_batch(ctx.h, p(w), p(tau), len(taus), sig.shape[1], 3, 2, 2.0, p(grid), len(grid),
                                                  1, 2, 2, p(c2), p(m2), None, None, p(s2)))
    assert c2.tobytes() == ch.tobytes() and m2.tobytes() == mh.tobytes() and s2.tobytes() == st.tobytes()


# ---------------------------------------------------------------- batches, hist, host forms
def test_batch_and_hist(ctx):
    import torch
    from tda_eeg_audio_amd import engine
    dms = rc.trajectory_dm(20, 47, 40)
    grid = rc.grid_of(5, 41)
    dm_t, grid_t = _dev(dms), _dev(grid)
    par = (1, 2, 2)
    # an oversized out pre-filled with a sentinel: the batch is fully overwritten, the tail is not touched
    big = engine.DeviceRecurrenceCurves(23, 5, 47, dm_t.device, hist=True)
    for t in (big.counts, big.hist, big.status):
        t.fill_(SENT)
    big.measures.fill_(float(SENT))
    engine.recurrence_dm_dev(dm_t, grid_t, *par, True, out=big, ctx=ctx)
    out = big.to_host()
    for k in ("counts", "measures", "hist", "status"):
        assert (out[k][20:] == SENT).all(), k
    assert not out["status"][:20].any()
    _same({k: out[k][[3, 19]] for k in ("counts", "measures", "hist")}, _ref_dm(dms[[3, 19]], grid, par), "batch")
    assert (out["counts"][:20] >= 0).all() and (out["hist"][:20] >= 0).all() and (out["measures"][:20] >= 0).all()   # no sentinel
    # a window alone and inside the batch
    for w in (0, 7, 19):
        alone = _rq_dm(dms[w:w + 1], grid, par, ctx=ctx)
        for k in ("counts", "measures", "hist"):
            assert alone[k][0].tobytes() == out[k][w].tobytes(), (w, k)
    # hist absent changes no other byte
    plain = engine.DeviceRecurrenceCurves(20, 5, 47, dm_t.device)
    plain.counts.fill_(SENT); plain.measures.fill_(float(SENT)); plain.status.fill_(SENT)
    engine.recurrence_dm_dev(dm_t, grid_t, *par, False, out=plain, ctx=ctx)
    ph = plain.to_host()
    assert "hist" not in ph and ph["counts"].tobytes() == out["counts"][:20].tobytes()
    assert ph["measures"].tobytes() == out["measures"][:20].tobytes() and not ph["status"].any()
    # the host form
    ch, mh, hh, sh = engine.recurrence_dm_batch(dms, grid, *par, True, ctx=ctx)
    assert ch.tobytes() == ph["counts"].tobytes() and mh.tobytes() == ph["measures"].tobytes() and not sh.any()
    assert hh.tobytes() == out["hist"][:20].tobytes()
    ch2, mh2, hh2, _ = engine.recurrence_dm_batch(dms, grid, ctx=ctx)
    assert hh2 is None and ch2.tobytes() == ch.tobytes() and mh2.tobytes() == mh.tobytes()
    torch.cuda.synchronize()


# ---------------------------------------------------------------- means and refusals
def test_group_means(ctx):
    from tda_eeg_audio_amd import engine
    pc, n_pts = _clouds(3, 50)                                     # statuses 4, 0, 0, 0, 0, 16, 0
    grid = np.array([0.12, 0.3, 0.2])
    grid_t = _dev(grid)
    seg = np.array([0, 0, 1, 6, 7], np.int32)                       # sizes 0, 1 (degenerate alone), 5, 1
    rq = engine.recurrence_cloud_dev(_dev(pc), _dev(n_pts), grid_t, hist=True, seg_off_t=_dev(seg), skip_mask=4 | 16, ctx=ctx)
    out = rq.to_host()
    st = out["status"]
    assert out["mean_counts"].shape == (4, 7, 3) and out["mean_measures"].shape == (4, 7, 3)
    assert out["mean_hist"].shape == (4, 2, 3, 129)
    assert out["mean_counts"].tobytes() == rr.mean_exact(out["counts"], seg, st, 4 | 16).tobytes()
    assert out["mean_hist"].tobytes() == rr.mean_exact(out["hist"], seg, st, 4 | 16).tobytes()
    assert out["mean_measures"].tobytes() == rr.mean_seq(out["measures"], seg, st, 4 | 16).tobytes()
    for k in ("mean_counts", "mean_measures", "mean_hist"):
        assert np.isnan(out[k][0]).all() and np.isnan(out[k][1]).all() and not np.isnan(out[k][2:]).any(), k
    # nothing skipped: the flagged windows' zeros are members; counts alone
    mc, mm, mh = engine.recurrence_mean_dev(rq.counts, None, None, 7, 3, 129, seg_off_t=_dev(seg), ctx=ctx)
    assert mm is None and mh is None and mc.cpu().numpy().tobytes() == rr.mean_exact(out["counts"], seg).tobytes()
    # seg_off = NULL: every window its own group
    mc, mm, mh = engine.recurrence_mean_dev(rq.counts, rq.measures, rq.hist, 7, 3, 129, ctx=ctx)
    assert mc.cpu().numpy().tobytes() == out["counts"].astype(np.float64).tobytes()
    assert mm.cpu().numpy().tobytes() == (0.0 + out["measures"]).tobytes()
    assert mh.cpu().numpy().tobytes() == out["hist"].astype(np.float64).tobytes()
    own = engine.recurrence_cloud_dev(_dev(pc), _dev(n_pts), grid_t, mean=True, ctx=ctx)
    assert own.mean_hist is None and own.mean_measures.cpu().numpy().tobytes() == mm.cpu().numpy().tobytes()
    # the host form
    hp = lambda a: a.ctypes.data_as(C.c_void_p)                    # noqa: E731
    hc, hm, hn = np.full((4, 7, 3), -1.0), np.full((4, 7, 3), -1.0), np.full((4, 2, 3, 129), -1.0)
    ctx.check(ctx.lib.tda_recurrence_mean(ctx.h, hp(out["counts"]), hp(out["measures"]), hp(out["hist"]), 7, 3, 129, hp(seg), 4,
                                          hp(st), 4 | 16, hp(hc), hp(hm), hp(hn)))
    assert hc.tobytes() == out["mean_counts"].tobytes() and hm.tobytes() == out["mean_measures"].tobytes()
    assert hn.tobytes() == out["mean_hist"].tobytes()
    h7 = np.full((7, 7, 3), -1.0)
    ctx.check(ctx.lib.tda_recurrence_mean(ctx.h, None, hp(out["measures"]), None, 7, 3, 0, None, 7, None, 0, None, hp(h7), None))
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
    cnt = torch.full((2 * 7 * (_lib.MAX_GRID + 1),), SENT, dtype=torch.int32, device=dev)
    mea = torch.full((2 * 7 * (_lib.MAX_GRID + 1),), -7.0, dtype=torch.float64, device=dev)
    his = torch.full((2 * 2 * 4 * 129,), SENT, dtype=torch.int32, device=dev)
    st = torch.full((2,), SENT, dtype=torch.int32, device=dev)
    mean = torch.full((2 * 7 * 4,), -7.0, dtype=torch.float64, device=dev)
    tau = torch.ones(2, dtype=torch.int32, device=dev)
    lib, h = ctx.lib, ctx.h
    outs = (p(cnt), p(mea), p(his))
    ok = (1, 2, 2)
    calls = [
        lambda: lib.tda_recurrence_dm_batch_dev(h, p(dm), 2, 129, 2.0, 1, p(grid), 4, *ok, *outs, p(st), None),        # n
        lambda: lib.tda_recurrence_dm_batch_dev(h, p(dm), 2, 0, 2.0, 1, p(grid), 4, *ok, *outs, p(st), None),
        lambda: lib.tda_recurrence_dm_batch_dev(h, p(dm), 2, 9, 2.0, 1, p(grid), 0, *ok, *outs, p(st), None),          # n_grid
        lambda: lib.tda_recurrence_dm_batch_dev(h, p(dm), 2, 9, 2.0, 1, p(grid), _lib.MAX_GRID + 1, *ok, *outs, p(st), None),
        lambda: lib.tda_recurrence_dm_batch_dev(h, p(dm), 2, 9, 2.0, 1, p(grid), 4, 0, 2, 2, *outs, p(st), None),      # theiler
        lambda: lib.tda_recurrence_dm_batch_dev(h, p(dm), 2, 9, 2.0, 1, p(grid), 4, 129, 2, 2, *outs, p(st), None),
        lambda: lib.tda_recurrence_dm_batch_dev(h, p(dm), 2, 9, 2.0, 1, p(grid), 4, 1, 0, 2, *outs, p(st), None),      # l_min
        lambda: lib.tda_recurrence_dm_batch_dev(h, p(dm), 2, 9, 2.0, 1, p(grid), 4, 1, 129, 2, *outs, p(st), None),
        lambda: lib.tda_recurrence_dm_batch_dev(h, p(dm), 2, 9, 2.0, 1, p(grid), 4, 1, 2, -1, *outs, p(st), None),     # v_min
        lambda: lib.tda_recurrence_dm_batch_dev(h, p(dm), 2, 9, 2.0, 1, p(grid), 4, 1, 2, 129, *outs, p(st), None),
        lambda: lib.tda_recurrence_cloud_batch_dev(h, p(dm), p(tau), 2, 8, 5, 1, 2.0, p(grid), 4, *ok, *outs, p(st), None),   # dim
        lambda: lib.tda_recurrence_cloud_batch_dev(h, p(dm), p(tau), 2, 8, 0, 1, 2.0, p(grid), 4, *ok, *outs, p(st), None),
        lambda: lib.tda_recurrence_cloud_batch_dev(h, p(dm), p(tau), 2, 0, 3, 1, 2.0, p(grid), 4, *ok, *outs, p(st), None),   # p_cap
        lambda: lib.tda_recurrence_cloud_batch_dev(h, p(dm), p(tau), 2, 8, 3, 1, 2.0, p(grid), 4, 1, 2, 0, *outs, p(st), None),
        lambda: lib.tda_recurrence_takens_batch_dev(h, p(dm), p(tau), 2, 250, 5, 2, 2.0, p(grid), 4, *ok, *outs, None, p(st), None),
        lambda: lib.tda_recurrence_takens_batch_dev(h, p(dm), p(tau), 2, 0, 3, 2, 2.0, p(grid), 4, *ok, *outs, None, p(st), None),
        lambda: lib.tda_recurrence_takens_batch_dev(h, p(dm), p(tau), 2, 250, 3, 2, 2.0, p(grid), 4, 200, 2, 2, *outs, None, p(st), None),
        lambda: lib.tda_recurrence_mean_dev(h, p(cnt), None, None, 2, 4, 9, None, 1, None, 0, p(mean), None, None, None),  # n_seg
        lambda: lib.tda_recurrence_mean_dev(h, p(cnt), None, None, 2, 0, 9, None, 2, None, 0, p(mean), None, None, None),  # n_grid
        lambda: lib.tda_recurrence_mean_dev(h, p(cnt), None, None, 2, 4, 9, None, 2, None, 0, None, p(mean), None, None),  # pairs
        lambda: lib.tda_recurrence_mean_dev(h, None, None, p(his), 2, 4, 0, None, 2, None, 0, None, None, p(mean), None),  # n_hist
    ]
    for k, call in enumerate(calls):
        assert call() == 1, k                                      # TDA_ERR_INVALID
        assert _msg(ctx), k
    torch.cuda.synchronize()
    assert (cnt == SENT).all() and (mea == -7.0).all() and (his == SENT).all() and (st == SENT).all() and (mean == -7.0).all()
    # the host forms refuse before anything is staged or written
    hp = lambda a: a.ctypes.data_as(C.c_void_p)                   # noqa: E731
    ch, mh, sh = np.full((2, 7, 4), SENT, np.int32), np.full((2, 7, 4), -7.0), np.full(2, SENT, np.int32)
    dmh, gh = np.zeros((2, 9, 9)), np.zeros(4)
    assert lib.tda_recurrence_dm_batch(h, hp(dmh), 2, 9, 2.0, 1, hp(gh), 0, 1, 2, 2, hp(ch), hp(mh), None, hp(sh)) == 1
    assert lib.tda_recurrence_dm_batch(h, hp(dmh), 2, 129, 2.0, 1, hp(gh), 4, 1, 2, 2, hp(ch), hp(mh), None, hp(sh)) == 1
    assert lib.tda_recurrence_dm_batch(h, hp(dmh), 2, 9, 2.0, 1, hp(gh), 4, 0, 2, 2, hp(ch), hp(mh), None, hp(sh)) == 1
    assert lib.tda_recurrence_dm_batch(h, hp(dmh), 2, 9, 2.0, 1, hp(gh), 4, 1, 2, 129, hp(ch), hp(mh), None, hp(sh)) == 1
    assert lib.tda_recurrence_mean(h, hp(ch), None, None, 2, 4, 9, None, 1, None, 0, hp(np.zeros(56)), None, None) == 1
    assert (ch == SENT).all() and (mh == -7.0).all() and (sh == SENT).all()
    # the Python front end refuses with ValueError before any call
    with pytest.raises(ValueError):
        engine.recurrence_dm_dev(dm[:, :9, :9].contiguous(), grid, ctx=ctx)
    with pytest.raises(ValueError):
        engine.recurrence_dm_dev(dm[:, :9, :9].contiguous(), grid[:4].contiguous(), theiler=0, ctx=ctx)
    with pytest.raises(ValueError):
        engine.recurrence_dm_batch(np.zeros((1, 9, 9)), [], ctx=ctx)
    # an empty batch is no error and touches nothing
    assert lib.tda_recurrence_dm_batch_dev(h, None, 0, 9, 2.0, 1, None, 4, 1, 2, 2, None, None, None, None, None) == 0
