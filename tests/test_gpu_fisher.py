"""
The persistence Fisher distance on the GPU against tests/fisher_ref.py.  The kernel walks a diagram 64 rows at a time and
a thread owns the points t, t + T, .. of Theta (2N points), so the finite-row counts 0, 1, 31, 33, 64, 127, 129, 256 on
each side take 2N across 64, 128, 256, 512 and 1,024; N = 512 is the limit.  Every comparison prints
q = max |gpu - ref_fsum| / 2^-53, the figure C is made of (fisher_ref.C).
"""
import numpy as np
import pytest

import fisher_ref as pf
from tda_eeg_audio_amd import _lib, engine

pytestmark = pytest.mark.gpu

NO_PAIR, TOO_LARGE = _lib.TDA_WIN_NO_PAIR, _lib.TDA_WIN_TOO_LARGE
SIZES = [0, 1, 31, 33, 64, 127, 129, 256]
SIGMA = 0.1
JUNK = np.array([[0.0, np.inf], [np.nan, 0.5], [0.25, np.nan]])


def _diagram(rng, n_finite, junk=True):
    """n_finite rows with d > b, with a (0, inf), a (nan, x) and an (x, nan) row worked in between them."""
    b = rng.uniform(0, 1, n_finite)
    rows = np.stack([b, b + rng.uniform(0, 0.8, n_finite)], axis=1)
    if junk:
        at = np.sort(rng.integers(0, n_finite + 1, len(JUNK)))
        rows = np.insert(rows, at, JUNK, axis=0)
    return rows


def _dev(ctx, *arrays):
    import torch
    dev = torch.device("cuda", ctx.device)
    return [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays]


def _hold(what, got, ref_fsum, N):
    """Print q of the comparison, then hold it against the tolerance."""
    got, ref_fsum, N = (np.asarray(x, dtype=np.float64) for x in (got, ref_fsum, N))
    err = np.abs(got - ref_fsum)
    k = int(np.argmax(err)) if err.size else 0
    print(f"q {what}: {float(err.max() / pf.U) if err.size else 0.0:.3f} (entry {k}, N {int(N.ravel()[k]) if err.size else 0})")
    tol = pf.tolerance(N)
    assert np.isfinite(got).all() and (err <= tol).all(), (what, float((err / tol).max()))
    assert (got >= 0.0).all() and (got <= np.pi / 2).all()


@pytest.fixture(scope="module")
def grid():
    """Set A: the eight sizes, 512 and 513 finite rows, and a diagram with cnt < 0.  Set B: the eight sizes, 257 finite
    rows, and a diagram with cnt > cap (every row of its buffer is a real one; it is not the last of the set).  The pairs:
    all 64 of the eight sizes, then the limit and the special diagrams; the references of the valid ones, computed once."""
    rng = np.random.default_rng(21)
    da = [_diagram(rng, n) for n in SIZES] + [_diagram(rng, 512), _diagram(rng, 513), _diagram(rng, 40)]
    db = [_diagram(rng, n) for n in SIZES]
    cap_b = 257 + len(JUNK)
    full = _diagram(rng, cap_b - len(JUNK))
    db += [full, _diagram(rng, 257)]
    ra, ca = engine.pack_diagrams(da)
    rb, cb = engine.pack_diagrams(db, cap=cap_b)
    ca[10] = -3                                   # cnt < 0: empty
    cb[8] = cap_b + 40                            # cnt > cap: its first cap rows
    eff_a = da[:10] + [np.zeros((0, 2))]
    eff_b = db
    pairs = [(i, j) for i in range(8) for j in range(8)]
    pairs += [(8, 0), (10, 5), (10, 0), (1, 8), (6, 8), (7, 8)]                 # (512, 0); cnt < 0; cnt > cap with N = 258, 386, 513
    pairs += [(7, 9), (9, 0), (8, 1)]                                           # (256, 257), (513, 0), (512, 1): too large
    ia, ib = (np.array(x, np.int32) for x in zip(*pairs))
    N = np.array([pf.n_points(eff_a[i], eff_b[j]) for i, j in pairs])
    ninv = pf.args(SIGMA)
    valid = N <= pf.PF_MAX_POINTS
    ref = np.array([pf.distance(eff_a[i], eff_b[j], ninv) if v else np.nan for (i, j), v in zip(pairs, valid)])
    ref_fsum = np.array([pf.distance_fsum(eff_a[i], eff_b[j], ninv) if v else np.nan for (i, j), v in zip(pairs, valid)])
    return dict(da=da, db=db, ra=ra, ca=ca, rb=rb, cb=cb, ia=ia, ib=ib, N=N, valid=valid, ref=ref, ref_fsum=ref_fsum, pairs=pairs)


def test_pair_grid(ctx, grid):
    import torch
    g = grid
    t = _dev(ctx, g["ra"], g["ca"], g["rb"], g["cb"], g["ia"], g["ib"])
    out_t, st_t = engine.persistence_fisher_dev(t[0], t[1], t[2], t[3], SIGMA, idx_a=t[4], idx_b=t[5], ctx=ctx)
    torch.cuda.synchronize()
    out, st = out_t.cpu().numpy(), st_t.cpu().numpy()
    v = g["valid"]
    assert g["N"][v].max() == 512 and (~v).sum() == 4 and sorted(g["N"][~v].tolist()) == [513, 513, 513, 513]
    assert (st[v] == 0).all() and (st[~v] == TOO_LARGE).all() and np.isnan(out[~v]).all()
    _hold("pair grid vs fsum reference", out[v], g["ref_fsum"][v], g["N"][v])
    # the reference with numpy's sums: inside the same tolerance (its own order is part of the 8 N)
    assert (np.abs(out[v] - g["ref"][v]) <= pf.tolerance(g["N"][v])).all()
    # both empty: 0; cnt < 0 counts as empty
    assert out[0] == 0.0 and out[g["pairs"].index((10, 0))] == 0.0
    assert out[g["pairs"].index((10, 5))] > 0
    # the host form: the same bytes
    out_h, st_h = engine.persistence_fisher_batch(g["ra"], g["ca"], g["rb"], g["cb"], SIGMA, idx_a=g["ia"], idx_b=g["ib"], ctx=ctx,
                                                  want_status=True)
    assert out_h.tobytes() == out.tobytes() and st_h.tobytes() == st.tobytes()
    # a pair alone: the same bytes as inside the batch
    for k in (9, 27, 45, 63, 64, 68):
        i, j = g["pairs"][k]
        one, one_st = engine.persistence_fisher_dev(t[0][i:i + 1], t[1][i:i + 1], t[2][j:j + 1], t[3][j:j + 1], SIGMA, ctx=ctx)
        assert one.cpu().numpy().tobytes() == out[k:k + 1].tobytes() and int(one_st.cpu()[0]) == 0, k
    # ... and from buffers of another capacity (the dynamic LDS is only room)
    i, j = g["pairs"][27]
    wide_a = np.zeros((1, 700, 2)); wide_a[0, :g["ra"].shape[1]] = g["ra"][i]
    wide_b = np.zeros((1, 300, 2)); wide_b[0, :g["rb"].shape[1]] = g["rb"][j]
    w = _dev(ctx, wide_a, g["ca"][i:i + 1], wide_b, g["cb"][j:j + 1])
    one, _ = engine.persistence_fisher_dev(w[0], w[1], w[2], w[3], SIGMA, ctx=ctx)
    assert one.cpu().numpy().tobytes() == out[27:28].tobytes()


@pytest.mark.parametrize("sigma", [0.02, 1.0])
def test_other_sigmas(ctx, grid, sigma):
    g = grid
    sel = [9, 20, 36, 42, 55, 63]
    ia, ib = g["ia"][sel], g["ib"][sel]
    out = engine.persistence_fisher_batch(g["ra"], g["ca"], g["rb"], g["cb"], sigma, idx_a=ia, idx_b=ib, ctx=ctx)
    ref = [pf.distance_fsum(g["da"][i], g["db"][j], pf.args(sigma)) for i, j in zip(ia, ib)]
    _hold(f"sigma {sigma}", out, ref, g["N"][sel])


def test_exact_zero_against_a_copy(ctx):
    """Every size against a copy of itself in another buffer, the junk rows elsewhere: 0.0 exactly, status 0."""
    rng = np.random.default_rng(22)
    da, db = [], []
    for n in SIZES:
        d = _diagram(rng, n, junk=False)
        da.append(np.insert(d, np.sort(rng.integers(0, n + 1, 3)), JUNK, axis=0))
        db.append(np.insert(d, np.sort(rng.integers(0, n + 1, 5)), np.concatenate([JUNK[::-1], JUNK[:2]]), axis=0))
    ra, ca = engine.pack_diagrams(da)
    rb, cb = engine.pack_diagrams(db, cap=300)
    for sigma in (0.05, 1.0):
        out, st = engine.persistence_fisher_batch(ra, ca, rb, cb, sigma, ctx=ctx, want_status=True)
        assert (st == 0).all() and out.tobytes() == np.zeros(len(SIZES)).tobytes(), out
    # the limit too: 256 finite rows a side
    assert pf.n_points(da[7], db[7]) == pf.PF_MAX_POINTS


def test_one_point_closed_form(ctx):
    empty = np.zeros((1, 1, 2)); zero = np.zeros(1, np.int32)
    for L, sigma in pf.ONE_POINT_CASES:
        x = np.array([[[0.375, 0.375 + L]]]); one = np.ones(1, np.int32)
        want = pf.one_point_closed_form(L, sigma)
        for a, b in (((x, one), (empty, zero)), ((empty, zero), (x, one))):
            out, st = engine.persistence_fisher_batch(a[0], a[1], b[0], b[1], sigma, ctx=ctx, want_status=True)
            q = abs(out[0] - want) / pf.U
            print(f"q one point L {L} sigma {sigma}: {q:.3f}")
            assert st[0] == 0 and abs(out[0] - want) <= pf.tolerance(1), (L, sigma, q)


def test_refusals(ctx, grid):
    import torch
    g = grid
    t = _dev(ctx, g["ra"], g["ca"], g["rb"], g["cb"])
    n_a, n_b = len(g["ca"]), len(g["cb"])
    ia = np.array([2, -1, 3, n_a, 4, 2 ** 30, 5], np.int32)
    ib = np.array([2, 1, n_b, 3, -7, 4, 5], np.int32)
    ia_t, ib_t = _dev(ctx, ia, ib)
    out_t, st_t = engine.persistence_fisher_dev(t[0], t[1], t[2], t[3], SIGMA, idx_a=ia_t, idx_b=ib_t, ctx=ctx)
    out, st = out_t.cpu().numpy(), st_t.cpu().numpy()
    bad = np.array([1, 2, 3, 4, 5])
    assert st[bad].tolist() == [NO_PAIR] * 5 and np.isnan(out[bad]).all()
    k2, k5 = g["pairs"].index((2, 2)), g["pairs"].index((5, 5))
    assert st[[0, 6]].tolist() == [0, 0]
    ref = [g["ref_fsum"][k2], g["ref_fsum"][k5]]
    _hold("good pairs beside refused ones", out[[0, 6]], ref, g["N"][[k2, k5]])
    # the host form: the same statuses, the same bytes
    out_h, st_h = engine.persistence_fisher_batch(g["ra"], g["ca"], g["rb"], g["cb"], SIGMA, idx_a=ia, idx_b=ib, ctx=ctx,
                                                  want_status=True)
    assert st_h.tobytes() == st.tobytes() and out_h.tobytes() == out.tobytes()
    # a bad ninv or cap: TDA_ERR_INVALID and nothing is written
    nan = float("nan")
    o = torch.full((7,), -7.0, dtype=torch.float64, device=t[0].device)
    s = torch.full((7,), -5, dtype=torch.int32, device=t[0].device)
    empty = torch.empty((n_a, 0, 2), dtype=torch.float64, device=t[0].device)
    args = (engine._tp(t[0]), engine._tp(t[1]), n_a, g["ra"].shape[1], engine._tp(t[2]), engine._tp(t[3]), n_b, g["rb"].shape[1],
            engine._tp(ia_t), engine._tp(ib_t), 7)
    oh, sh = np.full(7, -7.0), np.full(7, -5, np.int32)
    hargs = (engine.ptr(g["ra"]), engine.ptr(g["ca"]), n_a, g["ra"].shape[1], engine.ptr(g["rb"]), engine.ptr(g["cb"]), n_b,
             g["rb"].shape[1], engine.ptr(ia), engine.ptr(ib), 7)
    for ninv in (0.0, 0.5, nan, -np.inf, np.inf):
        assert ctx.lib.tda_persistence_fisher_batch_dev(ctx.h, *args, ninv, engine._tp(o), engine._tp(s), engine._stream()) == 1
        assert ctx.lib.tda_persistence_fisher_batch(ctx.h, *hargs, ninv, engine.ptr(oh), engine.ptr(sh)) == 1
    for sigma in (0.0, -1.0, nan, np.inf, True):
        with pytest.raises(_lib.TdaError):
            engine.persistence_fisher_dev(t[0], t[1], t[2], t[3], sigma, idx_a=ia_t, idx_b=ib_t, out_t=o, status_t=s, ctx=ctx)
        with pytest.raises(_lib.TdaError):
            engine.persistence_fisher_batch(g["ra"], g["ca"], g["rb"], g["cb"], sigma, idx_a=ia, idx_b=ib, ctx=ctx)
    with pytest.raises(_lib.TdaError):                                   # cap < 1
        engine.persistence_fisher_dev(empty, t[1], t[2], t[3], SIGMA, idx_a=ia_t, idx_b=ib_t, out_t=o, status_t=s, ctx=ctx)
    with pytest.raises(_lib.TdaError):
        engine.persistence_fisher_dev(t[0], t[1], empty, t[3], SIGMA, idx_a=ia_t, idx_b=ib_t, out_t=o, status_t=s, ctx=ctx)
    torch.cuda.synchronize()
    assert (o == -7.0).all() and (s == -5).all() and (oh == -7.0).all() and (sh == -5).all()
    # and the same buffers are filled by a good call
    engine.persistence_fisher_dev(t[0], t[1], t[2], t[3], SIGMA, idx_a=ia_t, idx_b=ib_t, out_t=o, status_t=s, ctx=ctx)
    torch.cuda.synchronize()
    assert o.cpu().numpy().tobytes() == out.tobytes() and s.cpu().numpy().tobytes() == st.tobytes()


def test_gram_and_utils(ctx, grid):
    from tda_eeg_audio_amd import utils
    rng = np.random.default_rng(23)
    dgms = [_diagram(rng, n) for n in (5, 0, 70, 33, 1, 129, 64, 12, 200)]
    rows, cnt = engine.pack_diagrams(dgms)
    G = engine.persistence_fisher_gram(rows, cnt, SIGMA, ctx=ctx)
    assert G.shape == (9, 9) and G.tobytes() == G.T.copy().tobytes()                  # symmetric as bytes
    assert np.diag(G).tobytes() == np.zeros(9).tobytes()                              # computed, and exactly 0.0
    iu, ju = np.triu_indices(9)
    pairs = engine.persistence_fisher_batch(rows, cnt, rows, cnt, SIGMA, idx_a=iu, idx_b=ju, ctx=ctx)
    assert G[iu, ju].tobytes() == pairs.tobytes()                                     # the bytes of the pair route
    ref = [pf.distance_fsum(dgms[i], dgms[j], pf.args(SIGMA)) for i, j in zip(iu, ju)]
    _hold("gram", pairs, ref, [pf.n_points(dgms[i], dgms[j]) for i, j in zip(iu, ju)])
    off = iu != ju
    assert (pairs[off] > 0).all()
    t = _dev(ctx, rows, cnt)
    Gd = engine.persistence_fisher_gram_dev(t[0], t[1], SIGMA, ctx=ctx).cpu().numpy()
    assert Gd.tobytes() == G.tobytes()
    # utils: distances, kernel, Gram, inside and outside a batch
    D = utils.persistence_fisher_distances(dgms, sigma=SIGMA)
    assert D.tobytes() == G.tobytes()
    K = utils.persistence_fisher_gram(dgms, sigma=SIGMA, t=2.0)
    assert K.tobytes() == np.exp(-2.0 * G).tobytes() and (np.diag(K) == 1.0).all()
    assert utils.persistence_fisher_distances([], sigma=SIGMA).shape == (0, 0)
    assert utils.persistence_fisher_gram([]).shape == (0, 0)
    d = utils.persistence_fisher_distance(dgms[0], dgms[2], sigma=SIGMA)
    assert d == G[0, 2] and utils.persistence_fisher_kernel(dgms[0], dgms[2], sigma=SIGMA, t=0.5) == np.exp(-0.5 * d)
    assert utils.persistence_fisher_distance(dgms[2], dgms[2].copy(), sigma=SIGMA) == 0.0
    assert np.isnan(utils.persistence_fisher_distance(dgms[0], dgms[2], sigma=0.0))
    assert np.isnan(utils.persistence_fisher_distance(grid["da"][9], dgms[0], sigma=SIGMA))       # 513 finite rows
    with utils.batch():
        lazy = [utils.persistence_fisher_distance(dgms[0], x, sigma=SIGMA) for x in dgms]
        broken = utils.persistence_fisher_distance(dgms[0], dgms[2], sigma=-1.0)
        other = utils.persistence_fisher_distance(dgms[0], dgms[2], sigma=1.0)
    assert [float(v) for v in lazy] == G[0].tolist() and np.isnan(float(broken))
    assert float(other) == utils.persistence_fisher_distance(dgms[0], dgms[2], sigma=1.0) != d
    with pytest.raises(_lib.TdaError):
        utils.persistence_fisher_distances(dgms, sigma=np.nan)
