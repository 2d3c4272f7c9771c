"""
The kernels on diagrams on the GPU against tests/diagram_kernel_ref.py: pair values and distances, group Gram matrices.
The pair kernel stages 64 rows at a time and the Gram kernel 256, so the finite-row counts sit on both sides of those
edges: 0, 1, T - 1, T, T + 1, 2 T + 1.  Every comparison prints q = |gpu - ref| / (2^-53 A), the figure C is made of
(diagram_kernel_ref.C).
"""
import numpy as np
import pytest

import diagram_kernel_ref as dk
from tda_eeg_audio_amd import _lib, engine

pytestmark = pytest.mark.gpu

NO_PAIR = _lib.TDA_WIN_NO_PAIR
KERNELS = {"pss": ("pss", 0.1), "pwg": ("pwg", 0.1, 2.0), "pers": (-3.0, 0, 0.75, dk.KW_PERS, 0.0)}
PT, GT = 64, 256                      # rows staged at a time by the pair kernel and by the Gram kernel


def _par(name):
    k = KERNELS[name]
    return k if len(k) == 5 else dk.named(k)


def _diagram(rng, n_finite, junk=True):
    """n_finite rows with d > b, with a (0, inf) row and a NaN row worked in between them."""
    b = rng.uniform(0, 1, n_finite)
    rows = np.stack([b, b + rng.uniform(0, 0.8, n_finite)], axis=1)
    if junk:
        extra = np.array([[0.0, np.inf], [np.nan, 0.5], [0.25, np.nan]])
        at = np.sort(rng.integers(0, n_finite + 1, len(extra)))
        rows = np.insert(rows, at, extra, axis=0)
    return rows


def _pack(dgms, cap=None):
    rows, cnt = engine.pack_diagrams(dgms, cap=cap)
    return rows, cnt


def _dev(ctx, *arrays):
    import torch
    dev = torch.device("cuda", ctx.device)
    return [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays]


def _hold(what, got, ref, A, N, par, w_max):
    """Print q of the comparison, then hold it against the tolerance."""
    got, ref, A, N = (np.asarray(x) for x in (got, ref, A, N))
    err = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(A > 0, err / (dk.U * A), 0.0)
    k = int(np.argmax(q)) if q.size else 0
    print(f"q {what}: {float(q.max()) if q.size else 0.0:.3f} (entry {k}, N_t {int(N.ravel()[k]) if q.size else 0})")
    tol = dk.tolerance(A, N, ref, par[2], w_max)
    assert np.isfinite(got).all() and (err <= tol).all(), (what, float((err / np.maximum(tol, 1e-300)).max()))


@pytest.fixture(scope="module")
def pair_case():
    """Six diagrams a side and a seventh in A with cnt > cap, every one of A against every one of B, and the reference of
    the 42 pairs under the three kernels."""
    rng = np.random.default_rng(11)
    sizes = [0, 1, PT - 1, PT, PT + 1, 2 * PT + 1]
    da = [_diagram(rng, n) for n in sizes]
    db = [_diagram(rng, n) for n in sizes]
    ra, ca = _pack(da)
    rb, cb = _pack(db, cap=2 * PT + 1 + 9)
    # cnt > cap: the diagram is its first cap rows (every row of the buffer is a real one)
    full = _diagram(rng, ra.shape[1], junk=False)
    da.append(full); ra = np.concatenate([ra, full[None]]); ca = np.concatenate([ca, [ra.shape[1] + 40]]).astype(np.int32)
    ia, ib = (x.ravel().astype(np.int32) for x in np.meshgrid(np.arange(len(da)), np.arange(len(db)), indexing="ij"))
    ref = {name: [dk.pair(da[i], db[j], _par(name)) for i, j in zip(ia, ib)] for name in KERNELS}
    return da, db, ra, ca, rb, cb, ia, ib, ref


@pytest.mark.parametrize("name", list(KERNELS))
def test_pair_values_and_distance(ctx, pair_case, name):
    import torch
    da, db, ra, ca, rb, cb, ia, ib, ref = pair_case
    par = _par(name)
    t = _dev(ctx, ra, ca, rb, cb, ia, ib)
    kv_t = torch.full((len(ia), 3), float("nan"), dtype=torch.float64, device=t[0].device)
    out_t, st_t = engine.diagram_kernel_dev(t[0], t[1], t[2], t[3], KERNELS[name], idx_a=t[4], idx_b=t[5], kvals_t=kv_t, ctx=ctx)
    torch.cuda.synchronize()
    out, st, kv = out_t.cpu().numpy(), st_t.cpu().numpy(), kv_t.cpu().numpy()
    assert (st == 0).all()
    R = np.array([r[0] for r in ref[name]]); A = np.array([r[1] for r in ref[name]]); N = np.array([r[2] for r in ref[name]])
    _hold(f"pairs {name}", kv, R, A, N, par, dk.wmax(da + db, par))
    # the distance is its own kvals' bit for bit
    assert out.tobytes() == dk.distance(kv).tobytes()
    # an empty diagram is the zero measure: k_ab = 0, k_aa = 0 and the distance is sqrt(k_bb)
    e = np.flatnonzero((ia == 0) & (ib == 4))[0]
    assert kv[e, 0] == 0.0 and kv[e, 1] == 0.0 and kv[e, 2] > 0 and out[e] == np.sqrt(kv[e, 2])
    both = np.flatnonzero((ia == 0) & (ib == 0))[0]
    assert (kv[both] == 0.0).all() and out[both] == 0.0
    # the host twin gives the same bytes; without kvals the distances do not change
    out_h, kv_h, st_h = engine.diagram_kernel_batch(ra, ca, rb, cb, KERNELS[name], idx_a=ia, idx_b=ib, ctx=ctx, want_status=True)
    assert out_h.tobytes() == out.tobytes() and kv_h.tobytes() == kv.tobytes() and (st_h == 0).all()
    p, out_n, st_n = engine.ptr, np.empty(len(ia)), np.empty(len(ia), np.int32)
    ha, hca, hb, hcb, hia, hib = engine.f64(ra), engine.i32(ca), engine.f64(rb), engine.i32(cb), engine.i32(ia), engine.i32(ib)
    ctx.check(ctx.lib.tda_diagram_kernel_pairs(ctx.h, p(ha), p(hca), len(ca), ra.shape[1], p(hb), p(hcb), len(cb), rb.shape[1], p(hia),
                                               p(hib), len(ia), *engine._kernel_params(KERNELS[name]), p(out_n), None, p(st_n)))
    assert out_n.tobytes() == out.tobytes() and (st_n == 0).all()
    out2, _ = engine.diagram_kernel_dev(t[0], t[1], t[2], t[3], KERNELS[name], idx_a=t[4], idx_b=t[5], ctx=ctx)
    assert out2.cpu().numpy().tobytes() == out.tobytes()


def test_pair_indices(ctx, pair_case):
    import torch
    da, db, ra, ca, rb, cb, _, _, ref = pair_case
    t = _dev(ctx, ra, ca, rb, cb)
    n_a, n_b = len(ca), len(cb)
    # identity pairs need equal counts: the first six of A against B
    out_t, st_t = engine.diagram_kernel_dev(t[0][:n_b], t[1][:n_b], t[2], t[3], KERNELS["pss"], ctx=ctx)
    ident = out_t.cpu().numpy()
    assert (st_t.cpu().numpy() == 0).all()
    # idx_a alone, idx_b alone, and indices outside their sets
    ia = np.array([5, 4, 3, 2, 1, 0], np.int32)
    (ia_t,) = _dev(ctx, ia)
    kv_t = torch.empty((6, 3), dtype=torch.float64, device=ia_t.device)
    w_max = dk.wmax(da + db, _par("pss"))
    engine.diagram_kernel_dev(t[0], t[1], t[2], t[3], KERNELS["pss"], idx_a=ia_t, kvals_t=kv_t, ctx=ctx)
    want = [dk.pair(da[i], db[j], _par("pss")) for j, i in enumerate(ia)]
    _hold("pairs idx_a", kv_t.cpu().numpy(), [w[0] for w in want], [w[1] for w in want], [w[2] for w in want], _par("pss"), w_max)
    engine.diagram_kernel_dev(t[0][:n_b], t[1][:n_b], t[2], t[3], KERNELS["pss"], idx_b=ia_t, kvals_t=kv_t, ctx=ctx)
    want = [dk.pair(da[j], db[i], _par("pss")) for j, i in enumerate(ia)]
    _hold("pairs idx_b", kv_t.cpu().numpy(), [w[0] for w in want], [w[1] for w in want], [w[2] for w in want], _par("pss"), w_max)
    ia = np.array([2, -1, 3, n_a, 4, 2 ** 30, 5], np.int32)
    ib = np.array([2, 1, n_b, 3, -7, 4, 5], np.int32)
    ia_t, ib_t = _dev(ctx, ia, ib)
    kv_t = torch.zeros((7, 3), dtype=torch.float64, device=ia_t.device)
    out_t, st_t = engine.diagram_kernel_dev(t[0], t[1], t[2], t[3], KERNELS["pss"], idx_a=ia_t, idx_b=ib_t, kvals_t=kv_t, ctx=ctx)
    out, st, kv = out_t.cpu().numpy(), st_t.cpu().numpy(), kv_t.cpu().numpy()
    bad = np.array([1, 2, 3, 4, 5])
    assert st[bad].tolist() == [NO_PAIR] * 5 and np.isnan(out[bad]).all() and np.isnan(kv[bad]).all()
    assert st[[0, 6]].tolist() == [0, 0] and out[0] == ident[2] and out[6] == ident[5]
    # a pair alone gives the bytes it gives inside the batch
    for i, j in ((3, 5), (5, 2), (6, 4)):
        one_kv = torch.empty((1, 3), dtype=torch.float64, device=ia_t.device)
        one, _ = engine.diagram_kernel_dev(t[0][i:i + 1], t[1][i:i + 1], t[2][j:j + 1], t[3][j:j + 1], KERNELS["pwg"], kvals_t=one_kv,
                                           ctx=ctx)
        ij = _dev(ctx, np.array([0, i, 1], np.int32), np.array([0, j, 1], np.int32))
        three_kv = torch.empty((3, 3), dtype=torch.float64, device=ia_t.device)
        three, _ = engine.diagram_kernel_dev(t[0], t[1], t[2], t[3], KERNELS["pwg"], idx_a=ij[0], idx_b=ij[1], kvals_t=three_kv, ctx=ctx)
        assert one.cpu().numpy().tobytes() == three.cpu().numpy()[1:2].tobytes()
        assert one_kv.cpu().numpy().tobytes() == three_kv.cpu().numpy()[1:2].tobytes()


# ------------------------------------------------------------------------------------------- Gram matrices
SKIP = _lib.TDA_WIN_DEGENERATE | _lib.TDA_WIN_TOO_LARGE


@pytest.fixture(scope="module")
def gram_case():
    """Seven groups of 1, 5 (+ one masked), 0, 2, 3, 2 (all masked) and 2 diagrams with 255, 256, 0, 257, 513, (90), 1
    finite rows in all.  Returns the packed set, its tables and the kept diagrams per group."""
    rng = np.random.default_rng(12)
    plan = [[GT - 1], [60, 60, -30, 60, 60, 16], [], [200, 57], [300, 200, 13], [-40, -50], [1, 0]]     # < 0: masked
    dgms, status, groups, off = [], [], [], [0]
    for g in plan:
        kept = []
        for n in g:
            d = _diagram(rng, abs(n))
            dgms.append(d); status.append(_lib.TDA_WIN_DEGENERATE if n < 0 else _lib.TDA_WIN_H1_TRUNCATED if n == 57 else 0)
            if n >= 0:
                kept.append(d)
        groups.append(kept); off.append(len(dgms))
    rows, cnt = _pack(dgms)
    return dgms, rows, cnt, np.array(off, np.int32), np.array(status, np.int32), groups


@pytest.mark.parametrize("name", list(KERNELS))
def test_gram_symmetric(ctx, gram_case, name):
    import torch
    dgms, rows, cnt, off, status, groups = gram_case
    par = _par(name)
    t = _dev(ctx, rows, cnt, off, status)
    G = engine.diagram_kernel_gram_dev(t[0], t[1], KERNELS[name], seg_off_a=t[2], status_a=t[3], skip_mask=SKIP, ctx=ctx).cpu().numpy()
    assert G.shape == (7, 7) and G.tobytes() == G.T.copy().tobytes()                 # symmetric as bytes
    R, A, N = dk.gram(groups, groups, par)
    dead = [2, 5]                                                                      # no diagram; every diagram masked
    assert np.isnan(G[dead]).all() and np.isnan(G[:, dead]).all()
    live = np.ix_([0, 1, 3, 4, 6], [0, 1, 3, 4, 6])
    _hold(f"gram {name}", G[live], R[live], A[live], N[live], par, dk.wmax(dgms, par))
    # the host twin: the same bytes
    Gh = engine.diagram_kernel_gram(rows, cnt, KERNELS[name], seg_off_a=off, status_a=status, skip_mask=SKIP, ctx=ctx)
    assert Gh.tobytes() == G.tobytes()
    # the cross route with both sets equal: the same values inside the tolerance (its G[h, g] is a sum in another order)
    X = engine.diagram_kernel_gram_dev(t[0], t[1], KERNELS[name], seg_off_a=t[2], status_a=t[3], rows_b=t[0], cnt_b=t[1], seg_off_b=t[2],
                                       status_b=t[3], skip_mask=SKIP, ctx=ctx).cpu().numpy()
    assert np.isnan(X[dead]).all() and np.isnan(X[:, dead]).all()
    _hold(f"gram cross route {name}", X[live], R[live], A[live], N[live], par, dk.wmax(dgms, par))
    assert X[np.triu_indices(7)].tobytes() == G[np.triu_indices(7)].tobytes()         # the tiles h >= g are the same launch shape
    Xh = engine.diagram_kernel_gram(rows, cnt, KERNELS[name], seg_off_a=off, status_a=status, rows_b=rows, cnt_b=cnt, seg_off_b=off,
                                    status_b=status, skip_mask=SKIP, ctx=ctx)
    assert Xh.tobytes() == X.tobytes()                                                # the host twin with status_b
    # a group alone gives the bytes it gives inside the batch; so does a pair of groups through the cross route
    for g in (1, 4, 6):
        sl = slice(off[g], off[g + 1])
        one = _dev(ctx, rows[sl], cnt[sl], np.array([0, off[g + 1] - off[g]], np.int32), status[sl])
        G1 = engine.diagram_kernel_gram_dev(one[0], one[1], KERNELS[name], seg_off_a=one[2], status_a=one[3], skip_mask=SKIP, ctx=ctx)
        assert G1.shape == (1, 1) and G1.cpu().numpy()[0, 0].tobytes() == G[g, g].tobytes()          # n_seg of 1
        other = _dev(ctx, rows[off[3]:off[4]], cnt[off[3]:off[4]], np.array([0, 2], np.int32))
        X1 = engine.diagram_kernel_gram_dev(one[0], one[1], KERNELS[name], seg_off_a=one[2], status_a=one[3], rows_b=other[0],
                                            cnt_b=other[1], seg_off_b=other[2], skip_mask=SKIP, ctx=ctx).cpu().numpy()
        assert X1.shape == (1, 1) and X1[0, 0].tobytes() == X[g, 3].tobytes()


def test_gram_without_groups_and_rectangular(ctx, gram_case):
    dgms, rows, cnt, off, status, groups = gram_case
    par = _par("pwg")
    # seg_off NULL: every diagram its own group (the first nine diagrams; the masked one is a NaN row and column)
    n = 9
    t = _dev(ctx, rows[:n], cnt[:n], status[:n])
    G = engine.diagram_kernel_gram_dev(t[0], t[1], KERNELS["pwg"], status_a=t[2], skip_mask=SKIP, ctx=ctx).cpu().numpy()
    each = [[d] if s & SKIP == 0 else [] for d, s in zip(dgms[:n], status[:n])]
    R, A, N = dk.gram(each, each, par)
    live = np.flatnonzero([len(e) for e in each])
    assert G.shape == (n, n) and G.tobytes() == G.T.copy().tobytes() and len(live) == n - 1
    assert np.isnan(np.delete(G, live, axis=0)).all() and np.isnan(np.delete(G, live, axis=1)).all()
    ix = np.ix_(live, live)
    _hold("gram per diagram pwg", G[ix], R[ix], A[ix], N[ix], par, dk.wmax(dgms[:n], par))
    # no status array at all: nothing is masked
    G2 = engine.diagram_kernel_gram_dev(t[0], t[1], KERNELS["pwg"], ctx=ctx).cpu().numpy()
    assert np.isfinite(G2).all() and G2[ix].tobytes() == G[ix].tobytes()
    # the host twin without seg_off, symmetric and cross
    assert engine.diagram_kernel_gram(rows[:n], cnt[:n], KERNELS["pwg"], status_a=status[:n], skip_mask=SKIP, ctx=ctx).tobytes() == G.tobytes()
    X2 = engine.diagram_kernel_gram_dev(t[0], t[1], KERNELS["pwg"], rows_b=t[0], cnt_b=t[1], ctx=ctx).cpu().numpy()
    assert engine.diagram_kernel_gram(rows[:n], cnt[:n], KERNELS["pwg"], rows_b=rows[:n], cnt_b=cnt[:n], ctx=ctx).tobytes() == X2.tobytes()
    # a rectangular 3 x 5 cross matrix between two sets with capacities of their own
    rng = np.random.default_rng(13)
    A3 = [[_diagram(rng, 40), _diagram(rng, 7)], [_diagram(rng, GT + 1)], [_diagram(rng, 3) for _ in range(5)]]
    B5 = [[_diagram(rng, 20)], [], [_diagram(rng, GT), _diagram(rng, 30)], [_diagram(rng, 1)], [_diagram(rng, 64), _diagram(rng, 0)]]
    ra, ca = _pack([d for g in A3 for d in g])
    rb, cb = _pack([d for g in B5 for d in g], cap=GT + 20)
    oa = np.cumsum([0] + [len(g) for g in A3]).astype(np.int32)
    ob = np.cumsum([0] + [len(g) for g in B5]).astype(np.int32)
    for name in ("pss", "pers"):
        par = _par(name)
        R, A, N = dk.gram(A3, B5, par)
        X = engine.diagram_kernel_gram(ra, ca, KERNELS[name], seg_off_a=oa, rows_b=rb, cnt_b=cb, seg_off_b=ob, ctx=ctx)
        assert X.shape == (3, 5) and np.isnan(X[:, 1]).all()
        keep = [0, 2, 3, 4]
        _hold(f"gram 3 x 5 {name}", X[:, keep], R[:, keep], A[:, keep], N[:, keep], par,
              dk.wmax([d for g in A3 + B5 for d in g], par))
        XT = engine.diagram_kernel_gram(rb, cb, KERNELS[name], seg_off_a=ob, rows_b=ra, cnt_b=ca, seg_off_b=oa, ctx=ctx)
        assert XT.shape == (5, 3)
        _hold(f"gram 5 x 3 {name}", XT[keep], R.T[keep], A.T[keep], N.T[keep], par, dk.wmax([d for g in A3 + B5 for d in g], par))


def test_refusals_leave_the_outputs_alone(ctx, pair_case):
    import torch
    _, _, ra, ca, rb, cb, _, _, _ = pair_case
    t = _dev(ctx, ra[:6], ca[:6], rb, cb, np.array([0, 2, 6], np.int32))
    nan = float("nan")
    bad = [(0.0, 1, 1.0, 0, 0.0), (0.5, 1, 1.0, 0, 0.0), (nan, 1, 1.0, 0, 0.0), (-np.inf, 1, 1.0, 0, 0.0), (-1.0, 2, 1.0, 0, 0.0),
           (-1.0, -1, 1.0, 0, 0.0), (-1.0, 1, np.inf, 0, 0.0), (-1.0, 1, nan, 0, 0.0), (-1.0, 0, 1.0, 3, 0.0), (-1.0, 0, 1.0, -1, 0.0),
           (-1.0, 0, 1.0, dk.KW_ATAN, nan), (-1.0, 0, 1.0, dk.KW_ATAN, np.inf)]
    out = torch.full((6,), nan, dtype=torch.float64, device=t[0].device)
    kv = torch.full((6, 3), nan, dtype=torch.float64, device=t[0].device)
    st = torch.full((6,), -5, dtype=torch.int32, device=t[0].device)
    G = torch.full((2, 2), nan, dtype=torch.float64, device=t[0].device)
    X = torch.full((2, 6), nan, dtype=torch.float64, device=t[0].device)
    empty = torch.empty((6, 0, 2), dtype=torch.float64, device=t[0].device)
    for par in bad:
        with pytest.raises(_lib.TdaError):
            engine.diagram_kernel_dev(t[0], t[1], t[2], t[3], par, out_t=out, status_t=st, kvals_t=kv, ctx=ctx)
        with pytest.raises(_lib.TdaError):
            engine.diagram_kernel_gram_dev(t[0], t[1], par, seg_off_a=t[4], out_t=G, ctx=ctx)
        with pytest.raises(_lib.TdaError):
            engine.diagram_kernel_gram_dev(t[0], t[1], par, seg_off_a=t[4], rows_b=t[2], cnt_b=t[3], out_t=X, ctx=ctx)
        with pytest.raises(_lib.TdaError):
            engine.diagram_kernel_batch(ra[:6], ca[:6], rb, cb, par, ctx=ctx)
        with pytest.raises(_lib.TdaError):
            engine.diagram_kernel_gram(ra[:6], ca[:6], par, ctx=ctx)
    good = (-1.0, 1, 1.0, 0, 0.0)
    with pytest.raises(_lib.TdaError):                                   # cap < 1
        engine.diagram_kernel_dev(empty, t[1], t[2], t[3], good, out_t=out, status_t=st, kvals_t=kv, ctx=ctx)
    with pytest.raises(_lib.TdaError):
        engine.diagram_kernel_gram_dev(empty, t[1], good, seg_off_a=t[4], out_t=G, ctx=ctx)
    with pytest.raises(_lib.TdaError):                                   # without seg_off every diagram is a group
        ctx.check(ctx.lib.tda_diagram_kernel_gram_dev(ctx.h, engine._tp(t[0]), engine._tp(t[1]), 6, ra.shape[1], None, 2, None, None,
                                                      None, 0, 0, None, 0, None, 0, *good, engine._tp(G), engine._stream()))
    for bad_kernel in (("pss", 0.0), ("pwg", 0.1), "pss"):
        with pytest.raises(_lib.TdaError):
            engine.diagram_kernel_dev(t[0], t[1], t[2], t[3], bad_kernel, out_t=out, status_t=st, kvals_t=kv, ctx=ctx)
    torch.cuda.synchronize()
    assert torch.isnan(out).all() and torch.isnan(kv).all() and (st == -5).all() and torch.isnan(G).all() and torch.isnan(X).all()
    # and the same buffers are filled by a good call
    engine.diagram_kernel_dev(t[0], t[1], t[2], t[3], good, out_t=out, status_t=st, kvals_t=kv, ctx=ctx)
    engine.diagram_kernel_gram_dev(t[0], t[1], good, seg_off_a=t[4], out_t=G, ctx=ctx)
    torch.cuda.synchronize()
    assert torch.isfinite(out).all() and (st == 0).all() and torch.isfinite(G).all()


def test_utils_entry_points(ctx):
    from tda_eeg_audio_amd import utils
    rng = np.random.default_rng(14)
    dgms = [_diagram(rng, n) for n in (5, 0, 70, 33)]
    for kernel in (("pss", 0.1), ("pwg", 0.2, 1.5)):
        par = dk.named(kernel)
        G = utils.diagram_kernel_gram(dgms, kernel=kernel)
        R, A, N = dk.gram([[d] for d in dgms], [[d] for d in dgms], par)
        _hold(f"utils gram {kernel[0]}", G, R, A, N, par, dk.wmax(dgms, par))
        assert G.tobytes() == G.T.copy().tobytes() and (G[1] == 0.0).all()
        # the pair route adds in another order than the Gram route: the same value inside the tolerance, not the same bytes
        k = utils.diagram_kernel(dgms[0], dgms[2], kernel=kernel)
        _hold(f"utils value {kernel[0]}", [k], [R[0, 2]], [A[0, 2]], [N[0, 2]], par, dk.wmax(dgms, par))
        ra, ca = engine.pack_diagrams([dgms[0]])
        rb, cb = engine.pack_diagrams([dgms[2]])
        out, kv = engine.diagram_kernel_batch(ra, ca, rb, cb, kernel, ctx=ctx)
        d = utils.kernel_distance(dgms[0], dgms[2], kernel=kernel)
        assert k == kv[0, 0] and d == out[0] and d > 0
        with utils.batch():
            lazy = [utils.kernel_distance(dgms[0], x, kernel=kernel) for x in dgms]
            broken = utils.kernel_distance(dgms[0], dgms[2], kernel=("pss", -1.0))
        assert float(lazy[2]) == d and float(lazy[0]) == 0.0 and np.isnan(float(broken))
    assert np.isnan(utils.kernel_distance(dgms[0], dgms[2], kernel=("abc", 1.0)))
    with pytest.raises(_lib.TdaError):
        utils.diagram_kernel(dgms[0], dgms[2], kernel=("pss", 0.0))
