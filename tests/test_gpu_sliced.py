"""
The sliced Wasserstein kernel (csrc/sliced.hip) against the CPU reference tests/sliced_ref.py.

Bar everywhere: abs(out - ref) <= (N + M + 1) * 2^-52 * ref (the contract's bound on two orders of the same non-negative
terms; exact where ref is 0), status 0 unless the case says otherwise.  A few hundred pairs; the references are computed
once per module.
"""
import numpy as np
import pytest

import sliced_ref as sr
from tda_eeg_audio_amd import _lib, engine, utils

pytestmark = pytest.mark.gpu


def _pack(dgms, cap, fill=7.25):
    """Diagrams in a buffer of `cap` rows with stale rows (fill) behind the count."""
    rows = np.full((len(dgms), cap, 2), fill)
    cnt = np.zeros(len(dgms), np.int32)
    for i, d in enumerate(dgms):
        d = np.asarray(d, float).reshape(-1, 2)
        assert len(d) <= cap
        rows[i, :len(d)] = d
        cnt[i] = len(d)
    return rows, cnt


def _gpu(ctx, A, B, cap_a, cap_b, dirs, **kw):
    ra, ca = _pack(A, cap_a)
    rb, cb = _pack(B, cap_b)
    return engine.sliced_wasserstein_batch(ra, ca, rb, cb, dirs, ctx=ctx, want_status=True, **kw)


def _check(ctx, A, B, cap_a, cap_b, dirs, ref=None):
    ref = np.array([sr.sliced_wasserstein(a, b, dirs) for a, b in zip(A, B)]) if ref is None else ref
    out, st = _gpu(ctx, A, B, cap_a, cap_b, dirs)
    N = np.array([sr.n_points(a, b) for a, b in zip(A, B)])
    err, tol = np.abs(out - ref), sr.tolerance(N, len(dirs), ref)
    print("M", len(dirs), "largest error / bound:", float(np.max(err / np.maximum(tol, 1e-300))))
    bad = np.flatnonzero(~(err <= tol) | (st != 0))
    assert len(bad) == 0, [(int(i), out[i], ref[i], int(st[i]), len(A[i]), len(B[i])) for i in bad[:5]]
    return out, ref


def test_known_answers(ctx):
    A, B = [k[0] for k in sr.KNOWN], [k[1] for k in sr.KNOWN]
    out, st = _gpu(ctx, A, B, 4, 4, sr.XY)
    assert out.tolist() == [k[2] for k in sr.KNOWN] and (st == 0).all()
    out, st = _gpu(ctx, B, A, 4, 4, sr.XY)
    assert out.tolist() == [k[2] for k in sr.KNOWN] and (st == 0).all()


SIZES = [(1, 1), (1, 2), (3, 60), (31, 33), (32, 33), (46, 122), (63, 65), (64, 65), (100, 156), (128, 129), (200, 312), (256, 256)]
MANY_M = [0, 1, 2, 3, 5]                                            # the sizes every direction count runs on


@pytest.fixture(scope="module")
def sized():
    """Random float32-exact diagrams at the sizes where the kernel changes path (1 / 2 / 4 / 8 values per lane, both sides
    of every threshold), every other one with ties."""
    rng = np.random.default_rng(21)
    A = [sr.random_diagram(rng, m, ties=i % 2 == 1) for i, (m, n) in enumerate(SIZES)]
    B = [sr.random_diagram(rng, n, ties=i % 2 == 1) for i, (m, n) in enumerate(SIZES)]
    return A, B


@pytest.mark.parametrize("M", [1, 3, 50, 128])
def test_sizes_both_ways_round(ctx, sized, M):
    A, B = sized
    dirs = utils.default_directions(M)                              # M = 1 and 3 leave waves without a direction
    pick = range(len(SIZES)) if M == 50 else MANY_M
    A, B = [A[i] for i in pick], [B[i] for i in pick]
    ref = np.array([sr.sliced_wasserstein(a, b, dirs) for a, b in zip(A, B)])
    assert (ref > 0).all()
    fwd, _ = _check(ctx, A, B, 512, 512, dirs, ref)
    rev, _ = _check(ctx, B, A, 512, 512, dirs, ref)
    assert fwd.tobytes() == rev.tobytes()
    # the kernel's route restated on the CPU, additions in the kernel's order: the same bits
    route = np.array([sr.kernel_route(a, b, dirs) for a, b in zip(A, B)])
    assert fwd.tobytes() == route.tobytes(), (fwd - route).tolist()
    # buffers of different capacities, the small side first / second; smaller launches compile in smaller networks
    small = [i for i, (a, b) in enumerate(zip(A, B)) if len(a) <= 47 and len(b) <= 128]
    sa, sb = [A[i] for i in small], [B[i] for i in small]
    f2, _ = _check(ctx, sa, sb, 47, 128, dirs, ref[small])
    r2, _ = _check(ctx, sb, sa, 128, 47, dirs, ref[small])
    assert f2.tobytes() == fwd[small].tobytes() == r2.tobytes()
    tiny = [i for i, (a, b) in enumerate(zip(A, B)) if len(a) <= 3 and len(b) <= 60]
    t2, _ = _check(ctx, [A[i] for i in tiny], [B[i] for i in tiny], 3, 61, dirs, ref[tiny])      # cap_a + cap_b = 64
    assert t2.tobytes() == fwd[tiny].tobytes()


def test_pair_above_the_point_limit_is_a_status(ctx):
    rng = np.random.default_rng(22)
    d = lambda n: sr.random_diagram(rng, n)
    A, B = [d(10), d(256), d(256), d(257), d(20)], [d(30), d(257), d(256), d(256), d(5)]
    dirs = utils.default_directions(16)
    out, st = _gpu(ctx, A, B, 300, 300, dirs)
    assert st.tolist() == [0, _lib.TDA_WIN_TOO_LARGE, 0, _lib.TDA_WIN_TOO_LARGE, 0]
    assert np.isnan(out[[1, 3]]).all()
    ok = [0, 2, 4]
    alone, st1 = _gpu(ctx, [A[i] for i in ok], [B[i] for i in ok], 300, 300, dirs)
    assert (st1 == 0).all() and alone.tobytes() == out[ok].tobytes()
    ref = np.array([sr.sliced_wasserstein(A[i], B[i], dirs) for i in ok])
    N = np.array([sr.n_points(A[i], B[i]) for i in ok])
    assert (np.abs(alone - ref) <= sr.tolerance(N, 16, ref)).all()
    # 520 rows of which 8 are essential: 512 points in all with the other side's one
    fin = np.vstack([d(511), [[0.0, np.inf]] * 9])
    one = d(1)
    out, st = _gpu(ctx, [fin], [one], 600, 600, dirs)
    ref = sr.sliced_wasserstein(fin, one, dirs)
    assert st[0] == 0 and abs(out[0] - ref) <= sr.tolerance(512, 16, ref)


def test_buffer_hygiene(ctx):
    rng = np.random.default_rng(23)
    d = lambda n: sr.random_diagram(rng, n)
    inf_mid = np.insert(d(20), 7, [0.25, np.inf], axis=0)
    nan_mid = np.insert(d(9), 3, [np.nan, 0.5], axis=0)
    both = np.insert(np.insert(d(70), 66, [0.5, np.inf], axis=0), 2, [np.nan, np.nan], axis=0)      # behind lane 63 too
    all_inf = np.array([[0.0, np.inf]] * 3)
    none = np.zeros((0, 2))
    A = [d(10), inf_mid, nan_mid, all_inf, d(6), all_inf, none, none, d(5), both]
    B = [d(30), d(40), inf_mid, d(12), all_inf, all_inf, none, d(7), none, nan_mid]
    dirs = utils.default_directions(5)
    out, ref = _check(ctx, A, B, 80, 80, dirs)                      # stale rows of 7.25 behind every count
    assert out[5] == 0.0 and out[6] == 0.0
    # count 0 with capacity 1
    rows = np.full((2, 1, 2), 7.25)
    out, st = engine.sliced_wasserstein_batch(rows, np.zeros(2, np.int32), rows, np.array([0, 1], np.int32), dirs, ctx=ctx,
                                              want_status=True)
    assert (st == 0).all() and out[0] == 0.0
    ref1 = sr.sliced_wasserstein(none, [[7.25, 7.25]], dirs)
    assert abs(out[1] - ref1) <= sr.tolerance(2, 5, ref1)
    # counts beyond the capacity and below zero are clamped, as in the other entry points
    ra, _ = _pack([d(8)], 8)
    rb, _ = _pack([d(8)], 8)
    out, st = engine.sliced_wasserstein_batch(ra, np.array([100], np.int32), rb, np.array([-3], np.int32), dirs, ctx=ctx,
                                              want_status=True)
    ref2 = sr.sliced_wasserstein(ra[0], none, dirs)
    assert st[0] == 0 and abs(out[0] - ref2) <= sr.tolerance(9, 5, ref2)


def _h0(b0, pers):
    p = np.asarray(pers, float)
    return np.stack([np.full(len(p), b0), b0 + p], 1)


def test_equal_birth_pairs(ctx):
    """H0-shaped diagrams: every birth 0, deaths tied.  Every projection of a row is s * d, and the direction (1, 0) makes
    every value of a list of rows equal."""
    rng = np.random.default_rng(24)
    f32 = lambda x: np.float32(x).astype(float)
    A, B = [], []
    for R, C in [(46, 122), (13, 64), (1, 50), (65, 66)]:
        A.append(_h0(0.0, f32(rng.uniform(0.01, 1.0, R)))); B.append(_h0(0.0, f32(rng.uniform(0.01, 1.0, C))))
        A.append(_h0(0.0, rng.integers(1, 9, R) / 8.0)); B.append(_h0(0.0, rng.integers(1, 17, C) / 16.0))       # tied deaths
        A.append(_h0(0.0, np.full(R, 0.75))); B.append(_h0(0.0, np.full(C, 0.75)))                              # all equal
        A.append(_h0(0.0, np.full(R, 0.75))); B.append(_h0(0.0, np.full(C, 0.5)))
    dirs = np.vstack([[[1.0, 0.0], [0.0, 1.0], [-1.0, 0.0]], utils.default_directions(6)])
    _check(ctx, A, B, 128, 128, dirs)
    out, st = _gpu(ctx, A, B, 128, 128, sr.XY[:1])                  # direction (1, 0) alone: rows project to 0, images to h
    assert (st == 0).all()
    assert np.array_equal(out, [sr.sliced_wasserstein(a, b, sr.XY[:1]) for a, b in zip(A, B)])     # halves of dyadic sums: exact


def test_index_arrays_and_pair_alone(ctx):
    rng = np.random.default_rng(25)
    A = [sr.random_diagram(rng, int(n)) for n in rng.integers(0, 40, 12)]
    B = [sr.random_diagram(rng, int(n)) for n in rng.integers(0, 90, 9)]
    ia, ib = rng.integers(0, 12, 30).astype(np.int32), rng.integers(0, 9, 30).astype(np.int32)
    ra, ca = _pack(A, 64)
    rb, cb = _pack(B, 128)
    dirs = utils.default_directions(10)
    got, st = engine.sliced_wasserstein_batch(ra, ca, rb, cb, dirs, idx_a=ia, idx_b=ib, ctx=ctx, want_status=True)
    ident, st2 = engine.sliced_wasserstein_batch(ra[ia], ca[ia], rb[ib], cb[ib], dirs, ctx=ctx, want_status=True)
    assert (st == 0).all() and (st2 == 0).all() and got.tobytes() == ident.tobytes()
    ref = np.array([sr.sliced_wasserstein(A[i], B[j], dirs) for i, j in zip(ia, ib)])
    N = np.array([sr.n_points(A[i], B[j]) for i, j in zip(ia, ib)])
    assert (np.abs(got - ref) <= sr.tolerance(N, 10, ref)).all()
    for k in (0, 7, 29):                                            # a pair alone: the bytes it has inside the batch
        one = engine.sliced_wasserstein_batch(ra[ia[k]:ia[k] + 1], ca[ia[k]:ia[k] + 1], rb[ib[k]:ib[k] + 1], cb[ib[k]:ib[k] + 1],
                                              dirs, ctx=ctx)
        assert one.tobytes() == got[k:k + 1].tobytes()
    # only one of the two index arrays
    half = engine.sliced_wasserstein_batch(ra[ia], ca[ia], rb, cb, dirs, idx_b=ib, ctx=ctx)
    assert half.tobytes() == got.tobytes()


def test_device_form_on_the_current_stream(ctx):
    import torch
    dev = torch.device("cuda", ctx.device)
    rng = np.random.default_rng(26)
    A = [sr.random_diagram(rng, int(n)) for n in rng.integers(0, 47, 20)]
    B = [sr.random_diagram(rng, int(n)) for n in rng.integers(0, 128, 20)]
    ra, ca = _pack(A, 47)
    rb, cb = _pack(B, 128)
    dirs = utils.default_directions(16)
    want = engine.sliced_wasserstein_batch(ra, ca, rb, cb, dirs, ctx=ctx)
    t = lambda a: torch.from_numpy(a).to(dev)
    out_t = torch.full((20,), -1.0, dtype=torch.float64, device=dev)
    st_t = torch.full((20,), -1, dtype=torch.int32, device=dev)
    o, s = engine.sliced_wasserstein_dev(t(ra), t(ca), t(rb), t(cb), t(dirs), out_t=out_t, status_t=st_t, ctx=ctx)
    torch.cuda.synchronize()
    assert o is out_t and s is st_t and (st_t.cpu().numpy() == 0).all() and out_t.cpu().numpy().tobytes() == want.tobytes()


def test_invalid_arguments(ctx):
    ra, ca = _pack([[[0.0, 1.0]]], 2)
    for bad in (np.zeros((0, 2)), utils.default_directions(128).repeat(2, 0)[:129], [[1.0, np.nan]], [[np.inf, 0.0]],
                np.zeros((4, 3)), np.zeros(6)):
        with pytest.raises(_lib.TdaError):
            engine.sliced_wasserstein_batch(ra, ca, ra, ca, bad, ctx=ctx)
    # the C entry points themselves refuse them with TDA_ERR_INVALID, before any launch
    out, st = np.empty(1), np.empty(1, np.int32)
    d = np.ascontiguousarray(utils.default_directions(128).repeat(2, 0))
    call = lambda dirs, M, cap=2: ctx.lib.tda_sliced_wasserstein_batch(ctx.h, _lib.ptr(ra), _lib.ptr(ca), 1, cap, _lib.ptr(ra),
                                                                       _lib.ptr(ca), 1, cap, None, None, 1, _lib.ptr(dirs), M,
                                                                       _lib.ptr(out), _lib.ptr(st))
    assert call(d, 0) == 1 and call(d, 129) == 1 and call(d, 1, cap=0) == 1 and call(d, 128) == 0
    nf = np.array([[0.0, 1.0], [np.nan, 0.0]])
    assert call(nf, 2) == 1 and call(nf, 1) == 0
    import torch
    dev = torch.device("cuda", ctx.device)
    t = lambda a: torch.from_numpy(a).to(dev)
    dev_call = lambda M: ctx.lib.tda_sliced_wasserstein_batch_dev(ctx.h, engine._tp(t(ra)), engine._tp(t(ca)), 2, engine._tp(t(ra)),
                                                                  engine._tp(t(ca)), 2, None, None, 1, engine._tp(t(d)), M,
                                                                  engine._tp(t(out)), engine._tp(t(st)), None)
    assert dev_call(0) == 1 and dev_call(129) == 1
    with pytest.raises(_lib.TdaError):
        engine.sliced_wasserstein_dev(t(ra), t(ca), t(ra), t(ca), t(np.zeros((3, 3))), ctx=ctx)
    torch.cuda.synchronize()


def test_gram_matrix(ctx):
    rng = np.random.default_rng(27)
    D = [sr.random_diagram(rng, int(n), ties=k % 3 == 0) for k, n in enumerate(rng.integers(0, 70, 12))]
    rows, cnt = _pack(D, 80)
    dirs = utils.default_directions(12)
    G = engine.sliced_wasserstein_gram(rows, cnt, dirs, ctx=ctx)
    assert G.shape == (12, 12) and G.tobytes() == G.T.copy().tobytes() and (np.diag(G) == 0.0).all()
    iu, ju = np.triu_indices(12, 1)
    pair = engine.sliced_wasserstein_batch(rows[iu], cnt[iu], rows[ju], cnt[ju], dirs, ctx=ctx)
    assert G[iu, ju].tobytes() == pair.tobytes()
    ref = np.array([sr.sliced_wasserstein(D[i], D[j], dirs) for i, j in zip(iu, ju)])
    N = np.array([sr.n_points(D[i], D[j]) for i, j in zip(iu, ju)])
    assert (np.abs(pair - ref) <= sr.tolerance(N, 12, ref)).all()
    K = utils.sliced_wasserstein_kernel(G, 0.5)
    assert (np.diag(K) == 1.0).all() and np.linalg.eigvalsh(K).min() > -1e-12


def test_safe_sliced_wasserstein_immediate_and_batched(ctx):
    rng = np.random.default_rng(28)
    pairs = [(sr.random_diagram(rng, int(m)), sr.random_diagram(rng, int(n))) for m, n in rng.integers(0, 50, (8, 2))]
    pairs[2] = (np.array([[0.0, np.inf], [0.125, 0.5]]), pairs[2][1])
    pairs[4] = (np.zeros(3), pairs[4][1])                          # not 2-D: the empty diagram
    bad = 5
    pairs[bad] = (np.zeros((4, 3)), pairs[bad][1])                 # malformed: three columns
    d7 = utils.default_directions(7)
    tables = [None if k % 2 == 0 else d7 for k in range(8)]        # two direction tables: default_directions(50) and d7
    now = [utils.safe_sliced_wasserstein(a, b, dirs=t) for (a, b), t in zip(pairs, tables)]
    for k, ((a, b), t) in enumerate(zip(pairs, tables)):
        if k == bad:
            assert np.isnan(now[k])
            continue
        dirs = utils.default_directions(50) if t is None else t
        ref = sr.sliced_wasserstein(a, b, dirs)
        assert abs(now[k] - ref) <= sr.tolerance(sr.n_points(a, b), len(dirs), ref)
    assert utils.safe_sliced_wasserstein(*pairs[0], M=7) == utils.safe_sliced_wasserstein(*pairs[0], dirs=d7)
    assert np.isnan(utils.safe_sliced_wasserstein(*pairs[0], dirs=np.zeros((2, 3))))
    with utils.batch():
        later = [utils.safe_sliced_wasserstein(a, b, dirs=t) for (a, b), t in zip(pairs, tables)]
        wrong = utils.safe_sliced_wasserstein(*pairs[0], dirs=np.zeros((2, 3)))
        w = utils.safe_wasserstein(*pairs[0])
    assert all(isinstance(x, utils.DeferredScalar) for x in later)
    vals = [float(x) for x in later]
    assert np.isnan(vals[bad]) and np.isnan(float(wrong))
    assert [x for k, x in enumerate(vals) if k != bad] == [x for k, x in enumerate(now) if k != bad]
    assert float(w) == utils.safe_wasserstein(*pairs[0])
