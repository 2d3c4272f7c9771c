"""
The landmark kernel (greedy permutation, n_perm) and the composed landmark Rips call against tests/landmark_ref.py.

lm_idx, n_lm and n_full are compared as integers; lm, lm_lambda and r_cover as BYTES: every operation of the selection is
one the oracle states and the cloud Rips kernel already reproduces bit for bit.  The diagrams of the composed call are,
as bytes, those of engine.cloud_rips_batch on the landmark rows with normalise=False, and as sorted multisets the oracle's.
"""
import numpy as np
import pytest

import landmark_ref as ref
from oracle import brute
from tda_eeg_audio_amd import _lib, engine

pytestmark = pytest.mark.gpu

H1_CAP = 1024
SENTINEL = -7.0


def _dev(ctx):
    import torch
    return torch.device("cuda", ctx.device)


def _fresh(n_win, n_perm, dim, dev):
    """Landmark buffers filled with a sentinel: whatever the kernel must leave untouched still holds it afterwards."""
    lm = engine.DeviceLandmarks(n_win, n_perm, dim, dev)
    for t in (lm.lm, lm.lam, lm.r_cover):
        t.fill_(SENTINEL)
    for t in (lm.idx, lm.n_lm, lm.n_full):
        t.fill_(int(SENTINEL))
    return lm


def _host(lm):
    return {k: getattr(lm, k).cpu().numpy() for k in ("lm", "idx", "lam", "r_cover", "n_lm", "n_full")}


def _check_window(got, w, X, n_perm, tau_ok=True):
    """Window w of the landmark outputs against the reference on its (normalised) cloud X."""
    want = ref.landmarks(X, n_perm) if tau_ok else None
    lm, idx, lam = got["lm"][w], got["idx"][w], got["lam"][w]
    if want is None:                                            # refused: a count no landmark set has, nothing written
        assert got["n_lm"][w] == _lib.MAX_POINTS + 1 and np.isnan(got["r_cover"][w])
        assert (lm == SENTINEL).all() and (idx == int(SENTINEL)).all() and (lam == SENTINEL).all()
        return None
    rows, ridx, rlam, rc, n_lm, n_full = want
    assert got["n_lm"][w] == n_lm and got["n_full"][w] == n_full
    assert np.array_equal(idx[:n_lm], ridx)
    assert lm[:n_lm].tobytes() == rows.tobytes()
    assert lam[:n_lm].tobytes() == rlam.tobytes()
    assert got["r_cover"][w].tobytes() == np.float64(rc).tobytes()
    assert (lm[n_lm:] == SENTINEL).all() and (idx[n_lm:] == int(SENTINEL)).all() and (lam[n_lm:] == SENTINEL).all()
    return rows


def _check_diagrams(out, got, w, rows, ctx):
    """The diagrams of window w of the composed call: the cloud path on the landmark rows, and the oracle's."""
    h0, c0, h1, c1, st = (t.cpu().numpy() for t in (out.h0, out.c0, out.h1, out.c1, out.status))
    assert out.n_points.cpu().numpy()[w] == got["n_lm"][w]
    if rows is None:
        assert st[w] == _lib.TDA_WIN_TOO_LARGE and c0[w] == 0 and c1[w] == 0
        return
    g0, gc0, g1, gc1, gst = engine.cloud_rips_batch(got["lm"][w:w + 1], n_pts=got["n_lm"][w:w + 1], normalise=False,
                                                    h1_cap=H1_CAP, ctx=ctx, raw=True)
    assert (c0[w], c1[w], st[w]) == (gc0[0], gc1[0], gst[0])
    assert h0[w, :c0[w]].tobytes() == g0[0, :c0[w]].tobytes() and h1[w, :c1[w]].tobytes() == g1[0, :c1[w]].tobytes()
    if len(rows) < 3:
        assert st[w] == _lib.TDA_WIN_DEGENERATE and c0[w] == 1 and c1[w] == 1 and not h0[w, 0].any() and not h1[w, 0].any()
        return
    assert st[w] == 0
    o = ref.diagrams(rows)
    assert np.array_equal(brute.sort_rows(h0[w, :c0[w]]), brute.sort_rows(o[0]))
    assert np.array_equal(brute.sort_rows(h1[w, :c1[w]]), brute.sort_rows(o[1]))


def _run_takens(ctx, wins, taus, dim, sub, n_perm):
    import torch
    dev = _dev(ctx)
    wins = np.ascontiguousarray(wins, dtype=np.float64)
    lm = _fresh(len(wins), n_perm, dim, dev)
    out = engine.DeviceDiagrams(len(wins), _lib.MAX_POINTS, H1_CAP, dev)
    engine.takens_rips_landmarks_dev(torch.from_numpy(wins).to(dev), torch.tensor(taus, dtype=torch.int32, device=dev),
                                     out, lm, dim=dim, subsample=sub, ctx=ctx)
    torch.cuda.synchronize()
    return out, _host(lm)


# (n_t, dim, subsample, n_perm, taus): the cloud sizes P of the windows are in the comments
TAKENS_CASES = [
    (131, 3, 1, 128, [1]),                  # 129: one point more than the landmarks
    (250, 3, 1, 128, [2, 1, 6]),            # 246, 248, 238: one point per thread, not every thread
    (259, 3, 1, 64, [1]),                   # 257: the second point of thread 0 only
    (600, 3, 1, 128, [5]),                  # 590: three points per thread
    (1026, 3, 1, 128, [1]),                 # 1024: every slot of every thread
    (1027, 3, 1, 17, [1, 2]),               # 1025: refused; 1023
    (300, 1, 1, 3, [1, 9]),                 # dim 1 (tau plays no part), the smallest n_perm
    (300, 2, 2, 17, [3, 50]),               # dim 2, subsample 2: 149, 125
    (400, 4, 1, 64, [7, 30]),               # dim 4: 379, 310
    (130, 3, 1, 64, [33, 34, 20]),          # 64 = n_perm: identity; 62 < n_perm: identity; 90
    (250, 3, 1, 64, [124, 125, 0, -3, 3]),  # P = 2 and P = 0: degenerate; tau < 1: refused; 244
]


@pytest.mark.parametrize("n_t,dim,sub,n_perm,taus", TAKENS_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_takens_landmarks_and_diagrams(ctx, n_t, dim, sub, n_perm, taus):
    rng = np.random.default_rng(n_t * 131 + dim * 17 + n_perm)
    wins = rng.standard_normal((len(taus), n_t))
    if n_t == 250 and n_perm == 128:
        wins[2] = ref.band_window(250, 7)                       # a band-limited window: a curve, not a ball
    out, got = _run_takens(ctx, wins, taus, dim, sub, n_perm)
    for w, tau in enumerate(taus):
        X = ref.cloud_of(wins[w], tau, dim, sub) if tau >= 1 else np.zeros((0, dim))
        if tau >= 1:
            assert got["n_full"][w] == len(X) == ref.n_takens(n_t, dim, tau, sub)
        rows = _check_window(got, w, X, n_perm, tau_ok=tau >= 1)
        _check_diagrams(out, got, w, rows, ctx)
    if (n_t, dim, sub, n_perm) == (300, 2, 2, 17):
        _check_host_takens_rips_landmarks(ctx, wins, taus, dim, sub, n_perm, out, got)


def _check_host_takens_rips_landmarks(ctx, wins, taus, dim, sub, n_perm, out, got):
    """The host forms tda_takens_rips_landmarks and tda_takens_landmarks on numpy buffers: the bytes of the _dev form, with
    and without the optional outputs (lm_lambda, n_points); rows from n_lm on keep the caller's zeros; h0_cap < n_perm is
    refused."""
    p = engine.ptr
    n_win, n_t = wins.shape
    w_h, tau_h = engine.f64(wins), engine.i32(taus)
    dev = {k: getattr(out, k).cpu().numpy() for k in ("h0", "c0", "h1", "c1", "status", "n_points")}

    def call(optional, rips=True, h0_cap=_lib.MAX_POINTS):
        lm, idx, lam, rc, n_lm, n_full = engine._landmark_out(n_win, n_perm, dim)
        h0, h1 = np.zeros((n_win, _lib.MAX_POINTS, 2)), np.zeros((n_win, H1_CAP, 2))
        c0, c1, n_points, st = (np.zeros(n_win, np.int32) for _ in range(4))
        lms = (p(lm), p(idx), p(lam) if optional else None, p(rc), p(n_lm), p(n_full))
        if rips:
            rc_ = ctx.lib.tda_takens_rips_landmarks(ctx.h, p(w_h), p(tau_h), n_win, n_t, dim, sub, n_perm, engine.MAX_EDGE_LENGTH,
                                                    *lms, p(h0), h0_cap, p(c0), p(h1), H1_CAP, p(c1),
                                                    p(n_points) if optional else None, p(st))
        else:
            rc_ = ctx.lib.tda_takens_landmarks(ctx.h, p(w_h), p(tau_h), n_win, n_t, dim, sub, n_perm, *lms)
        return rc_, dict(lm=lm, idx=idx, lam=lam, r_cover=rc, n_lm=n_lm, n_full=n_full, h0=h0, c0=c0, h1=h1, c1=c1,
                         n_points=n_points, status=st)

    for optional, rips in ((True, True), (False, True), (True, False), (False, False)):
        rc_, h = call(optional, rips)
        assert rc_ == 0
        for name in ("r_cover", "n_lm", "n_full"):
            assert h[name].tobytes() == got[name].tobytes(), (optional, rips, name)
        for w in range(n_win):
            k = got["n_lm"][w]
            assert 0 < k <= n_perm
            for name in ("lm", "idx") + (("lam",) if optional else ()):
                assert h[name][w, :k].tobytes() == got[name][w, :k].tobytes(), (optional, rips, name, w)
                assert not h[name][w, k:].any(), (optional, rips, name, w)
            assert optional or not h["lam"][w].any()
        if not rips:
            continue
        for name in ("c0", "c1", "status"):
            assert h[name].tobytes() == dev[name].tobytes(), (optional, name)
        assert h["n_points"].tobytes() == (dev["n_points"] if optional else np.zeros(n_win, np.int32)).tobytes()
        for w in range(n_win):
            c0, c1 = dev["c0"][w], dev["c1"][w]
            assert h["h0"][w, :c0].tobytes() == dev["h0"][w, :c0].tobytes()
            assert h["h1"][w, :c1].tobytes() == dev["h1"][w, :c1].tobytes()
    assert call(True, h0_cap=n_perm - 1)[0] == 1


@pytest.mark.parametrize("n_t,sub,n_perm,taus,n_lm", [
    (250, 2, 128, [2, 10, 60, 124], [123, 115, 65, 1]),         # P < n_perm, down to a degenerate window
    (130, 1, 64, [33, 34, 1], [64, 62, 64]),                    # P = n_perm, P < n_perm; 128 points: selected, not identity
])
def test_identity_case_is_takens_rips(ctx, n_t, sub, n_perm, taus, n_lm):
    """P <= n_perm: the landmark route and takens_rips_dev on the same windows give the same bytes."""
    import torch
    dev = _dev(ctx)
    n = len(taus)
    wins = np.random.default_rng(77).standard_normal((n, n_t))
    out, got = _run_takens(ctx, wins, taus, 3, sub, n_perm)
    plain = engine.takens_rips_dev(torch.from_numpy(wins).to(dev), torch.tensor(taus, dtype=torch.int32, device=dev),
                                   engine.DeviceDiagrams(n, _lib.MAX_POINTS, H1_CAP, dev), subsample=sub, ctx=ctx)
    torch.cuda.synchronize()
    assert got["n_lm"].tolist() == n_lm
    same = got["n_full"] <= n_perm
    assert same.sum() >= 2 and not got["r_cover"][same].any() and (got["r_cover"][~same] > 0).all()
    c0, c1 = plain.c0.cpu().numpy(), plain.c1.cpu().numpy()
    for w in np.flatnonzero(same):
        for name in ("c0", "c1", "status", "n_points"):
            assert getattr(out, name)[w].item() == getattr(plain, name)[w].item(), (w, name)
        assert out.h0[w, :c0[w]].cpu().numpy().tobytes() == plain.h0[w, :c0[w]].cpu().numpy().tobytes()
        assert out.h1[w, :c1[w]].cpu().numpy().tobytes() == plain.h1[w, :c1[w]].cpu().numpy().tobytes()


@pytest.mark.parametrize("normalise", [True, False])
def test_cloud_landmarks(ctx, normalise):
    import torch
    dev = _dev(ctx)
    rng = np.random.default_rng(5 + normalise)
    p_cap, dim, n_perm = 300, 2, 64
    n_pts = [300, 200, 129, 64, 2, 0, 301]                      # 301 > p_cap: refused, whatever TDA_LM_MAX_POINTS is
    pc = rng.random((len(n_pts), p_cap, dim)) * np.array([3.0, 0.5]) - 0.25
    lm = _fresh(len(n_pts), n_perm, dim, dev)
    engine.cloud_landmarks_dev(torch.from_numpy(pc).to(dev), torch.tensor(n_pts, dtype=torch.int32, device=dev), lm,
                               normalise=normalise, ctx=ctx)
    torch.cuda.synchronize()
    got = _host(lm)
    from oracle import port
    for w, P in enumerate(n_pts):
        X = pc[w, :min(P, p_cap)]
        X = port.minmax_normalise(X) if normalise and len(X) else X.copy()
        _check_window(got, w, X, n_perm, tau_ok=P <= p_cap)
    # the host form on the same clouds: the same bytes, and what the kernel leaves alone is left alone on the host too
    h = engine.cloud_landmarks_batch(pc, n_perm, n_pts=n_pts, normalise=normalise, ctx=ctx)
    for name, arr in zip(("lm", "idx", "lam", "r_cover", "n_lm", "n_full"), h):
        keep = got[name] != (SENTINEL if arr.dtype == np.float64 else int(SENTINEL))
        assert np.array_equal(arr[keep], got[name][keep], equal_nan=True) and not arr[~keep].any(), name
    if normalise:                                               # ... and without lm_lambda: the other outputs' bytes
        p, pc_h, n_h = engine.ptr, engine.f64(pc), engine.i32(n_pts)
        lm2, idx2, lam2, rc2, n_lm2, n_full2 = engine._landmark_out(len(n_pts), n_perm, dim)
        assert ctx.lib.tda_cloud_landmarks(ctx.h, p(pc_h), p(n_h), len(n_pts), p_cap, dim, 1, n_perm, p(lm2), p(idx2), None, p(rc2),
                                           p(n_lm2), p(n_full2)) == 0
        for a, b in zip((lm2, idx2, rc2, n_lm2, n_full2), (h[0], h[1], h[3], h[4], h[5])):
            assert a.tobytes() == b.tobytes()
        assert not lam2.any()


def test_batch_of_300_and_single_windows(ctx):
    rng = np.random.default_rng(300)
    wins = rng.standard_normal((300, 250))
    taus = rng.integers(1, 61, 300).tolist()
    out, got = _run_takens(ctx, wins, taus, 3, 1, 64)
    assert (got["n_lm"] == 64).all() and (out.status.cpu().numpy() == 0).all()
    c0, c1 = out.c0.cpu().numpy(), out.c1.cpu().numpy()
    for w in (0, 63, 64, 217, 299):                             # also past the first wave of workgroups
        rows = _check_window(got, w, ref.cloud_of(wins[w], taus[w]), 64)
        _check_diagrams(out, got, w, rows, ctx)
        one_out, one = _run_takens(ctx, wins[w:w + 1], taus[w:w + 1], 3, 1, 64)
        for name in got:
            assert one[name][0].tobytes() == got[name][w].tobytes(), (w, name)
        assert (one_out.c0.item(), one_out.c1.item()) == (c0[w], c1[w])
        assert one_out.h0[0, :c0[w]].cpu().numpy().tobytes() == out.h0[w, :c0[w]].cpu().numpy().tobytes()
        assert one_out.h1[0, :c1[w]].cpu().numpy().tobytes() == out.h1[w, :c1[w]].cpu().numpy().tobytes()


def test_ties_and_exhausted_landmarks(ctx):
    """An integer signal with values 0..4: the arg-max ties at a positive distance (n_perm 64), and the landmarks run out
    of distinct points so that index 0 repeats (n_perm 128)."""
    s = np.random.default_rng(3).integers(0, 5, 250).astype(np.float64)
    X = ref.cloud_of(s, 1)
    distinct = len(np.unique(X, axis=0))
    assert distinct < 128
    for n_perm in (64, 128):
        out, got = _run_takens(ctx, s[None], [1], 3, 1, n_perm)
        rows = _check_window(got, 0, X, n_perm)
        _check_diagrams(out, got, 0, rows, ctx)
    assert got["r_cover"][0] == 0.0 and (got["idx"][0, distinct:] == 0).all()


def test_refusals_leave_the_buffers_untouched(ctx):
    import torch
    dev = _dev(ctx)
    n_win, n_t, p_cap = 2, 250, 300
    win = torch.zeros((n_win, n_t), dtype=torch.float64, device=dev)
    pc = torch.zeros((n_win, p_cap, 3), dtype=torch.float64, device=dev)
    aux = torch.ones(n_win, dtype=torch.int32, device=dev)
    lm = _fresh(n_win, 128, 4, dev)                             # large enough for every n_perm and dim tried
    out = engine.DeviceDiagrams(n_win, _lib.MAX_POINTS, 16, dev)
    for t in (out.h0, out.h1):
        t.fill_(SENTINEL)
    for t in (out.c0, out.c1, out.status, out.n_points):
        t.fill_(int(SENTINEL))
    p = engine._tp
    bufs = [p(lm.lm), p(lm.idx), p(lm.lam), p(lm.r_cover), p(lm.n_lm), p(lm.n_full)]
    dgm = [p(out.h0), out.h0_cap, p(out.c0), p(out.h1), out.h1_cap, p(out.c1), p(out.n_points), p(out.status)]
    ok = dict(n_t=n_t, dim=3, sub=1, n_perm=64)
    bad = [dict(n_perm=2), dict(n_perm=129), dict(dim=0), dict(dim=5), dict(sub=0), dict(n_t=4097), dict(n_t=0)]
    for change in bad:
        a = dict(ok, **change)
        rc = ctx.lib.tda_takens_landmarks_dev(ctx.h, p(win), p(aux), n_win, a["n_t"], a["dim"], a["sub"], a["n_perm"], *bufs, None)
        assert rc == 1, change
        rc = ctx.lib.tda_takens_rips_landmarks_dev(ctx.h, p(win), p(aux), n_win, a["n_t"], a["dim"], a["sub"], a["n_perm"], 2.0,
                                                   *bufs, *dgm, None)
        assert rc == 1, change
    for a in (dict(p_cap=1025), dict(p_cap=0), dict(n_perm=2), dict(dim=5)):
        a = dict(dict(p_cap=p_cap, dim=3, n_perm=64), **a)
        rc = ctx.lib.tda_cloud_landmarks_dev(ctx.h, p(pc), p(aux), n_win, a["p_cap"], a["dim"], 1, a["n_perm"], *bufs, None)
        assert rc == 1, a
    # the second stage's own demand, h0_cap >= n_perm, is refused before the first stage is launched
    dgm_small = [p(out.h0), 63] + dgm[2:]
    assert ctx.lib.tda_takens_rips_landmarks_dev(ctx.h, p(win), p(aux), n_win, n_t, 3, 1, 64, 2.0, *bufs, *dgm_small, None) == 1
    torch.cuda.synchronize()
    for t in (lm.lm, lm.lam, lm.r_cover, out.h0, out.h1):
        assert bool((t == SENTINEL).all())
    for t in (lm.idx, lm.n_lm, lm.n_full, out.c0, out.c1, out.status, out.n_points):
        assert bool((t == int(SENTINEL)).all())
    with pytest.raises(_lib.TdaError):
        engine.DeviceLandmarks(1, 129, 3, dev)
    with pytest.raises(_lib.TdaError):
        engine.takens_landmarks_batch(np.zeros((1, 250)), [1], n_perm=2, ctx=ctx)


def test_utils_n_perm(ctx):
    """compute_audio_persistence(n_perm=...) and greedy_landmarks on one cloud of 246 points; without n_perm the wall
    stays where it is."""
    from tda_eeg_audio_amd import utils
    win = np.random.default_rng(9).standard_normal(250)
    pc = utils.takens_embedding(win, 3, 2, 1)
    assert len(pc) == 246
    with pytest.raises(_lib.TdaError):
        utils.compute_audio_persistence(pc)
    X = ref.cloud_of(win, 2)
    rows, ridx, rlam, rc, _, _ = ref.landmarks(X, 64)
    idx, lam, r_cover = utils.greedy_landmarks(pc, 64)
    assert np.array_equal(idx, ridx) and lam.tobytes() == rlam.tobytes() and r_cover == rc
    h0, h1 = utils.compute_audio_persistence(pc, n_perm=64)
    o = ref.diagrams(rows)
    assert np.array_equal(brute.sort_rows(h0), brute.sort_rows(o[0])) and np.array_equal(brute.sort_rows(h1), brute.sort_rows(o[1]))
    assert utils.compute_audio_persistence(pc[:2], n_perm=64)[0].tolist() == [[0, 0]]
    with utils.batch():
        with pytest.raises(NotImplementedError, match="takens_rips_landmarks_dev"):
            utils.compute_audio_persistence(pc, n_perm=64)
        with pytest.raises(NotImplementedError, match="cloud_landmarks_batch"):
            utils.greedy_landmarks(pc, 64)
    with pytest.raises(_lib.TdaError):
        utils.compute_audio_persistence(np.zeros((1025, 3)), n_perm=64)
