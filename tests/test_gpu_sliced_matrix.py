"""
The prepared route of the sliced Wasserstein distance on the GPU (csrc/sliced_matrix.hip): tda_sliced_prepare_dev against
np.sort of the header's projections, tda_sliced_prepared_pairs_dev against the bytes of the pair kernel
(engine.sliced_wasserstein_dev) and of its CPU restatement (sliced_ref.kernel_route), the Gram matrix against
engine.sliced_wasserstein_gram, and tda_sliced_matrix_dev against numpy's mean over the pair kernel's values for the pairs
that the pairing rules of tda_wasserstein_matrix_dev name.  Equalities are bit for bit; the one tolerance is the
contract's, (N + M + 1) * 2^-52 * value against math.fsum.
"""
import numpy as np
import pytest

import sliced_matrix_ref as smr
import sliced_ref as sr
from tda_eeg_audio_amd import _lib, engine, utils

pytestmark = pytest.mark.gpu

TOO_LARGE, NO_PAIR, DEGENERATE = _lib.TDA_WIN_TOO_LARGE, _lib.TDA_WIN_NO_PAIR, _lib.TDA_WIN_DEGENERATE
SENT = -777.0


def _pack(dgms, cap, fill=7.25):
    rows = np.full((len(dgms), cap, 2), fill)
    cnt = np.zeros(len(dgms), np.int32)
    for i, d in enumerate(dgms):
        d = np.asarray(d, float).reshape(-1, 2)
        assert len(d) <= cap
        rows[i, :len(d)] = d
        cnt[i] = len(d)
    return rows, cnt


@pytest.fixture(scope="module")
def dev(ctx):
    import torch
    return torch.device("cuda", ctx.device)


def _t(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _prep(ctx, dev, dgms, cap, dirs, **kw):
    rows, cnt = _pack(dgms, cap)
    return engine.sliced_prepare_dev(_t(rows, dev), _t(cnt, dev), _t(np.ascontiguousarray(dirs, dtype=np.float64), dev), ctx=ctx, **kw)


def _lists(table, slot_off, n_dirs, i):
    """(n_dirs, 2, s_i) view of the region of diagram i of a table on the host."""
    o0, o1 = int(slot_off[i]), int(slot_off[i + 1])
    return table[2 * n_dirs * o0:2 * n_dirs * o1].reshape(n_dirs, 2, o1 - o0)


# ---------------------------------------------------------------------------------------------------------------
# 1. prepare
# ---------------------------------------------------------------------------------------------------------------
PREP_M = [0, 1, 2, 63, 64, 65, 128, 129, 256, 257, 512]
PREP_CAP = 520


@pytest.fixture(scope="module")
def prep_set():
    """Diagrams with PREP_M finite rows, every other one with ties, non-finite rows in between from the third on."""
    rng = np.random.default_rng(51)
    out = []
    for i, m in enumerate(PREP_M):
        d = sr.random_diagram(rng, m, ties=i % 2 == 1)
        if m >= 2:
            d = np.insert(d, m // 2, [0.25, np.inf], axis=0)
            d = np.insert(d, 1, [np.nan, 0.5], axis=0)
        if m >= 65:
            d = np.insert(d, 66, [np.nan, np.nan], axis=0)                        # behind lane 63 too
        out.append(d)
    return out


def _expected_lists(D, dirs):
    C = sr.clean(D)
    h = 0.5 * (C[:, 0] + C[:, 1])
    return [(np.sort((c * C[:, 0]) + (s * C[:, 1])), np.sort((c * h) + (s * h))) for c, s in dirs]


@pytest.mark.parametrize("M", [1, 3, 5, 128])
@pytest.mark.parametrize("dense", [False, True])
def test_prepare_lists(ctx, dev, prep_set, M, dense):
    import torch
    dirs = utils.default_directions(M)
    rows, cnt = _pack(prep_set, PREP_CAP)
    n = len(prep_set)
    slot = np.arange(n + 1, dtype=np.int64) * PREP_CAP if dense else None
    n_rows = n * PREP_CAP
    table = torch.full((2 * M * n_rows,), SENT, dtype=torch.float64, device=dev)
    T = engine.sliced_prepare_dev(_t(rows, dev), _t(cnt, dev), _t(dirs, dev), table_t=table,
                                  slot_off=None if slot is None else _t(slot, dev), ctx=ctx)
    torch.cuda.synchronize()
    tab, so, m = T.table.cpu().numpy(), T.slot_off.cpu().numpy(), T.m.cpu().numpy()
    if not dense:                                                                 # the exclusive scan of max(min(cnt, cap), 1)
        assert so.tolist() == np.concatenate([[0], np.cumsum(np.clip(cnt, 1, PREP_CAP))]).tolist()
    assert m.tolist() == [max(v, 1) for v in PREP_M]
    written = 0
    for i, D in enumerate(prep_set):
        L = _lists(tab, so, M, i)
        for k, (p0, p1) in enumerate(_expected_lists(D, dirs)):
            assert (L[k, 0, :m[i]] == p0).all() and (L[k, 1, :m[i]] == p1).all(), (i, k)
        assert (L[:, :, m[i]:] == SENT).all()                                     # only the ranks < m are written
        written += 2 * M * m[i]
    assert int((tab != SENT).sum()) == written


def test_prepare_clamps_counts(ctx, dev):
    import torch
    rng = np.random.default_rng(52)
    d = sr.random_diagram(rng, 8)
    rows, _ = _pack([d, d, d], 8)
    cnt = np.array([100, -3, 8], np.int32)                                        # beyond the capacity, below zero
    dirs = utils.default_directions(3)
    T = engine.sliced_prepare_dev(_t(rows, dev), _t(cnt, dev), _t(dirs, dev), ctx=ctx)
    torch.cuda.synchronize()
    tab, so, m = T.table.cpu().numpy(), T.slot_off.cpu().numpy(), T.m.cpu().numpy()
    assert so.tolist() == [0, 8, 9, 17] and m.tolist() == [8, 1, 8]
    for i, D in enumerate([d, np.zeros((0, 2)), d]):
        L = _lists(tab, so, 3, i)
        for k, (p0, p1) in enumerate(_expected_lists(D, dirs)):
            assert (L[k, 0, :m[i]] == p0).all() and (L[k, 1, :m[i]] == p1).all()


def test_prepare_refusals_write_nothing(ctx, dev):
    import torch
    rng = np.random.default_rng(53)
    d = lambda n: sr.random_diagram(rng, n)
    dgms = [d(5), d(513), d(9), d(7), d(4)]
    rows, cnt = _pack(dgms, PREP_CAP)
    dirs = utils.default_directions(3)
    # diagram 1: 513 finite rows; diagram 2: a slot of 8 rows for 9; diagram 4: a slot that ends beyond the table
    slot = np.array([0, 5, 518, 526, 533, 537], np.int64)
    table_rows = 536
    table = torch.full((2 * 3 * table_rows,), SENT, dtype=torch.float64, device=dev)
    T = engine.sliced_prepare_dev(_t(rows, dev), _t(cnt, dev), _t(dirs, dev), table_t=table, slot_off=_t(slot, dev), ctx=ctx)
    torch.cuda.synchronize()
    tab, m = T.table.cpu().numpy(), T.m.cpu().numpy()
    assert m.tolist() == [5, -1, -1, 7, -1]
    for i in (1, 2):
        assert (_lists(tab, slot, 3, i) == SENT).all()
    assert (tab[2 * 3 * 533:] == SENT).all()
    assert int((tab != SENT).sum()) == 2 * 3 * (5 + 7)
    # and a pair with such a diagram on either side is a status
    out, st = engine.sliced_wasserstein_prepared_dev(T, T, _t(np.array([0, 1, 0, 3], np.int32), dev),
                                                     _t(np.array([3, 0, 4, 3], np.int32), dev), ctx=ctx)
    torch.cuda.synchronize()
    out, st = out.cpu().numpy(), st.cpu().numpy()
    assert st.tolist() == [0, TOO_LARGE, TOO_LARGE, 0] and np.isnan(out[[1, 2]]).all() and out[3] == 0.0 and out[0] > 0


# ---------------------------------------------------------------------------------------------------------------
# 2. prepared pairs
# ---------------------------------------------------------------------------------------------------------------
SIZES = [(0, 0), (1, 1), (1, 2), (3, 60), (31, 33), (32, 33), (46, 122), (63, 65), (64, 65), (100, 156), (128, 129), (200, 312),
         (256, 256)]
FEW = [0, 1, 2, 3, 5]


@pytest.fixture(scope="module")
def sized():
    rng = np.random.default_rng(54)
    A = [sr.random_diagram(rng, m, ties=i % 2 == 1) for i, (m, n) in enumerate(SIZES)]
    B = [sr.random_diagram(rng, n, ties=i % 2 == 1) for i, (m, n) in enumerate(SIZES)]
    return A, B


def _pairs(ctx, dev, A, B, cap_a, cap_b, dirs, idx_a=None, idx_b=None):
    """(prepared route, pair kernel) values and status words of the same inputs."""
    import torch
    ra, ca = _pack(A, cap_a)
    rb, cb = _pack(B, cap_b)
    ra, ca, rb, cb, dt = _t(ra, dev), _t(ca, dev), _t(rb, dev), _t(cb, dev), _t(np.ascontiguousarray(dirs, dtype=np.float64), dev)
    ia = None if idx_a is None else _t(np.asarray(idx_a, np.int32), dev)
    ib = None if idx_b is None else _t(np.asarray(idx_b, np.int32), dev)
    TA, TB = engine.sliced_prepare_dev(ra, ca, dt, ctx=ctx), engine.sliced_prepare_dev(rb, cb, dt, ctx=ctx)
    n = len(A) if ia is None else len(idx_a)
    out = torch.full((n,), SENT, dtype=torch.float64, device=dev)
    st = torch.full((n,), -7, dtype=torch.int32, device=dev)
    engine.sliced_wasserstein_prepared_dev(TA, TB, ia, ib, out_t=out, status_t=st, ctx=ctx)
    po, ps = engine.sliced_wasserstein_dev(ra, ca, rb, cb, dt, ia, ib, ctx=ctx)
    torch.cuda.synchronize()
    return out.cpu().numpy(), st.cpu().numpy(), po.cpu().numpy(), ps.cpu().numpy()


@pytest.mark.parametrize("M", [1, 3, 50])
def test_pairs_are_the_pair_kernels_bytes(ctx, dev, sized, M):
    A, B = sized
    pick = range(len(SIZES)) if M == 50 else FEW
    A, B = [A[i] for i in pick], [B[i] for i in pick]
    dirs = utils.default_directions(M)
    fwd, st, pair, pst = _pairs(ctx, dev, A, B, 512, 512, dirs)
    rev, rst, _, _ = _pairs(ctx, dev, B, A, 512, 512, dirs)
    assert (st == 0).all() and (pst == 0).all() and (rst == 0).all()
    assert fwd.tobytes() == pair.tobytes(), (fwd - pair).tolist()
    assert fwd.tobytes() == rev.tobytes()
    route = np.array([sr.kernel_route(a, b, dirs) for a, b in zip(A, B)])
    assert fwd.tobytes() == route.tobytes(), (fwd - route).tolist()
    ref = np.array([sr.sliced_wasserstein(a, b, dirs, order="fsum") for a, b in zip(A, B)])
    N = np.array([sr.n_points(a, b) for a, b in zip(A, B)])
    err, tol = np.abs(fwd - ref), sr.tolerance(N, M, ref)
    print("M", M, "largest error / bound against fsum:", float(np.max(err / np.maximum(tol, 1e-300))))
    assert (err <= tol).all()
    # a pair alone: the bytes it has inside the batch
    for k in (len(A) - 1, 3):
        one, s1, _, _ = _pairs(ctx, dev, A[k:k + 1], B[k:k + 1], 512, 512, dirs)
        assert s1[0] == 0 and one.tobytes() == fwd[k:k + 1].tobytes()


def test_pairs_known_answers_and_index_lists(ctx, dev):
    A, B = [k[0] for k in sr.KNOWN], [k[1] for k in sr.KNOWN]
    out, st, pair, _ = _pairs(ctx, dev, A, B, 4, 4, sr.XY)
    assert out.tolist() == [k[2] for k in sr.KNOWN] and (st == 0).all() and out.tobytes() == pair.tobytes()
    rng = np.random.default_rng(55)
    A = [sr.random_diagram(rng, int(n), ties=True) for n in rng.integers(0, 40, 12)]
    B = [sr.random_diagram(rng, int(n), ties=True) for n in rng.integers(0, 90, 9)]
    ia, ib = rng.integers(0, 12, 30), rng.integers(0, 9, 30)
    dirs = utils.default_directions(10)
    out, st, pair, pst = _pairs(ctx, dev, A, B, 64, 128, dirs, ia, ib)
    assert (st == 0).all() and (pst == 0).all() and out.tobytes() == pair.tobytes()
    # an index outside its table: NaN and TDA_WIN_NO_PAIR, the pairs beside it untouched
    ia2, ib2 = ia.copy(), ib.copy()
    ia2[4], ib2[9], ia2[11] = 12, -1, -5
    import torch
    TA, TB = _prep(ctx, dev, A, 64, dirs), _prep(ctx, dev, B, 128, dirs)
    o, s = engine.sliced_wasserstein_prepared_dev(TA, TB, _t(ia2.astype(np.int32), dev), _t(ib2.astype(np.int32), dev), ctx=ctx)
    torch.cuda.synchronize()
    o, s = o.cpu().numpy(), s.cpu().numpy()
    bad = [4, 9, 11]
    assert s[bad].tolist() == [NO_PAIR] * 3 and np.isnan(o[bad]).all()
    keep = np.setdiff1d(np.arange(30), bad)
    assert (s[keep] == 0).all() and o[keep].tobytes() == out[keep].tobytes()


def test_pairs_above_the_point_limit_and_bad_direction_counts(ctx, dev):
    import torch
    rng = np.random.default_rng(56)
    d = lambda n: sr.random_diagram(rng, n)
    A, B = [d(10), d(256), d(256), d(257), d(511)], [d(30), d(257), d(256), d(256), d(1)]
    dirs = utils.default_directions(16)
    out, st, pair, pst = _pairs(ctx, dev, A, B, 512, 300, dirs)
    assert st.tolist() == [0, TOO_LARGE, 0, TOO_LARGE, 0] == pst.tolist()
    assert np.isnan(out[[1, 3]]).all() and out[[0, 2, 4]].tobytes() == pair[[0, 2, 4]].tobytes()
    # n_dirs of 0 and 129: TDA_ERR_INVALID from the C entry points, nothing launched
    T = _prep(ctx, dev, A[:1], 16, dirs)
    o = torch.full((1,), SENT, dtype=torch.float64, device=dev)
    s = torch.full((1,), -7, dtype=torch.int32, device=dev)
    tp = engine._tp
    pairs_call = lambda M: ctx.lib.tda_sliced_prepared_pairs_dev(ctx.h, tp(T.table), tp(T.slot_off), tp(T.m), 1, tp(T.table),
                                                                 tp(T.slot_off), tp(T.m), 1, None, None, 1, M, tp(o), tp(s), None)
    ra, ca = _pack(A[:1], 16)
    ra, ca, dt = _t(ra, dev), _t(ca, dev), _t(np.ascontiguousarray(utils.default_directions(128).repeat(2, 0)), dev)
    m = torch.full((1,), -7, dtype=torch.int32, device=dev)
    big = torch.full((2 * 129 * 16,), SENT, dtype=torch.float64, device=dev)
    prep_call = lambda M, cap=16: ctx.lib.tda_sliced_prepare_dev(ctx.h, tp(ra), tp(ca), cap, 1, tp(dt), M, tp(T.slot_off), tp(big), 16,
                                                                 tp(m), None)
    i32 = lambda a: _t(np.asarray(a, np.int32), dev)
    seg, cls, stb = i32([0, 1]), i32([0]), i32([0])
    mo, mp, mf = o.clone(), s.clone(), s.clone()
    mat_call = lambda M: ctx.lib.tda_sliced_matrix_dev(ctx.h, tp(T.table), tp(T.slot_off), tp(T.m), 1, tp(seg), 1, tp(cls), tp(T.table),
                                                       tp(T.slot_off), tp(T.m), 1, tp(seg), 1, 1, tp(stb), M, tp(mo), tp(mp), tp(mf),
                                                       None)
    for call in (pairs_call, prep_call, mat_call):
        assert call(0) == 1 and call(129) == 1
    assert prep_call(3, cap=0) == 1
    torch.cuda.synchronize()
    assert o.item() == SENT and s.item() == -7 and m.item() == -7 and mo.item() == SENT and (big == SENT).all().item()
    assert pairs_call(16) == 0 and mat_call(16) == 0
    torch.cuda.synchronize()
    assert o.item() == 0.0 and s.item() == 0 and mo.item() == 0.0 and mp.item() == 1 and mf.item() == 0
    with pytest.raises(_lib.TdaError):
        engine.sliced_wasserstein_prepared_dev(T, _prep(ctx, dev, A[:1], 16, dirs[:5]), ctx=ctx)


# ---------------------------------------------------------------------------------------------------------------
# 3. the Gram matrix
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 9])
def test_gram_equals_the_pair_route(ctx, dev, n):
    import torch
    rng = np.random.default_rng(57 + n)
    D = [sr.random_diagram(rng, int(k), ties=i % 3 == 0) for i, k in enumerate(rng.integers(0, 70, n))]
    rows, cnt = _pack(D, 80)
    dirs = utils.default_directions(12)
    want = engine.sliced_wasserstein_gram(rows, cnt, dirs, ctx=ctx)
    G = engine.sliced_wasserstein_gram_dev(_t(rows, dev), _t(cnt, dev), _t(dirs, dev), ctx=ctx)
    torch.cuda.synchronize()
    assert G.shape == (n, n) and G.cpu().numpy().tobytes() == want.tobytes()


# ---------------------------------------------------------------------------------------------------------------
# 4. the matrix
# ---------------------------------------------------------------------------------------------------------------
N_CLS, N_COL = 2, 5
A_SIZES = [0, 1, 2, 15, 64, 65, 3, 15]
CLS_A = [0, 1, 0, 1, 0, 1, 2, 0]                  # group 6: a class out of range
B_SIZES = [64, 0, 2, 20, 1,                       # class 0; column 1 is empty; (0, 2) is shorter than the groups of 15 and 64
           1, 70, 15, 0, 10]                      # class 1
ROWS = [0, 1, 40, 65, 130, 200, 38, 43, 12]       # rows per diagram
CAP_A, CAP_B = 320, 256


def _matrix_set(n, seed, cap, big=None):
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        k = ROWS[(i * 5 + seed) % len(ROWS)]
        d = sr.random_diagram(rng, k, ties=i % 2 == 0)
        if k > 5 and i % 7 == 3:
            d = np.insert(d, 2, [np.nan, np.nan], axis=0)
        out.append(d)
    if big is not None:
        out[big] = sr.random_diagram(rng, cap)
    return out


@pytest.fixture(scope="module")
def matrix_case(ctx, dev):
    """The diagrams, the tables and, per direction count, the pair kernel's value of every pair the rules name."""
    seg_a = np.concatenate([[0], np.cumsum(A_SIZES)]).astype(np.int32)
    seg_b = np.concatenate([[0], np.cumsum(B_SIZES)]).astype(np.int32)
    A = _matrix_set(seg_a[-1], 1, CAP_A, big=seg_a[3] + 4)        # 320 rows at position 4 of the group of 15
    B = _matrix_set(seg_b[-1], 2, CAP_B)
    status_b = np.zeros(seg_b[-1], np.int32)
    status_b[[seg_b[0] + 1, seg_b[3] + 0, seg_b[6] + 66, seg_b[7] + 5]] = DEGENERATE     # middle, first, past every A group, middle
    status_b[seg_b[2] + 1] = _lib.TDA_WIN_H1_TRUNCATED                                   # another bit: still a pair
    B[seg_b[7] + 4] = sr.random_diagram(np.random.default_rng(3), CAP_B)                  # 320 + 256 rows: a pair with a status
    return dict(A=A, B=B, seg_a=seg_a, seg_b=seg_b, status_b=status_b)


def _matrix_expected(ctx, dev, S, dirs):
    """out / pairs / flags by the rules: per entry the positions i < min(len_a, len_b) whose B diagram is not degenerate
    are pairs, their values are the pair kernel's (one batched call over explicit index lists), then smr.matrix_entry."""
    import torch
    ia, ib, where = [], [], []
    n_seg = len(A_SIZES)
    for g in range(n_seg):
        k = CLS_A[g]
        if not 0 <= k < N_CLS or A_SIZES[g] > 64:
            continue
        for c in range(N_COL):
            p = k * N_COL + c
            for i in range(min(A_SIZES[g], B_SIZES[p])):
                if not S["status_b"][S["seg_b"][p] + i] & DEGENERATE:
                    ia.append(S["seg_a"][g] + i); ib.append(S["seg_b"][p] + i); where.append((g, c, i))
    ra, ca = _pack(S["A"], CAP_A)
    rb, cb = _pack(S["B"], CAP_B)
    w, st = engine.sliced_wasserstein_dev(_t(ra, dev), _t(ca, dev), _t(rb, dev), _t(cb, dev), _t(dirs, dev),
                                          _t(np.array(ia, np.int32), dev), _t(np.array(ib, np.int32), dev), ctx=ctx)
    torch.cuda.synchronize()
    w, st = w.cpu().numpy(), st.cpu().numpy()
    vals = {(g, c): (np.full(A_SIZES[g], np.nan), np.full(A_SIZES[g], NO_PAIR, np.int32)) for g in range(n_seg) for c in range(N_COL)}
    for (g, c, i), x, s in zip(where, w, st):
        vals[g, c][0][i], vals[g, c][1][i] = x, s
    out, pairs, flags = np.full((n_seg, N_COL), np.nan), np.zeros((n_seg, N_COL), np.int32), np.zeros((n_seg, N_COL), np.int32)
    for (g, c), (x, s) in vals.items():
        if A_SIZES[g] > 64:
            flags[g, c] = TOO_LARGE
        else:
            out[g, c], pairs[g, c], flags[g, c] = smr.matrix_entry(x, s)
    return out, pairs, flags, len(where), int((st != 0).sum())


@pytest.mark.parametrize("M", [16, 128])          # 64 and 8 positions of a group at a time
def test_matrix_equals_means_of_the_pair_kernel(ctx, dev, matrix_case, M):
    import torch
    S = matrix_case
    dirs = utils.default_directions(M)
    exp_out, exp_pairs, exp_flags, n_pairs, n_status = _matrix_expected(ctx, dev, S, dirs)
    TA, TB = _prep(ctx, dev, S["A"], CAP_A, dirs), _prep(ctx, dev, S["B"], CAP_B, dirs)
    n_seg = len(A_SIZES)
    out = torch.full((n_seg, N_COL), SENT, dtype=torch.float64, device=dev)
    pairs = torch.full((n_seg, N_COL), -7, dtype=torch.int32, device=dev)
    flags = torch.full((n_seg, N_COL), -7, dtype=torch.int32, device=dev)
    i32 = lambda a: _t(np.asarray(a, np.int32), dev)
    engine.sliced_matrix_dev(TA, i32(S["seg_a"]), i32(CLS_A), TB, i32(S["seg_b"]), i32(S["status_b"]), N_COL, out_t=out, pairs_t=pairs,
                             flags_t=flags, ctx=ctx)
    torch.cuda.synchronize()
    out, pairs, flags = out.cpu().numpy(), pairs.cpu().numpy(), flags.cpu().numpy()
    print("M", M, n_pairs, "pairs,", n_status, "with a status", "out", out, "pairs", pairs, "flags", flags, sep="\n")
    assert np.array_equal(np.isnan(out), np.isnan(exp_out)) and out[~np.isnan(out)].tobytes() == exp_out[~np.isnan(out)].tobytes()
    assert np.array_equal(pairs, exp_pairs) and np.array_equal(flags, exp_flags)
    # what the shape is there for
    assert n_pairs >= 150 and n_status >= 1
    assert (pairs[0] == 0).all() and np.isnan(out[0]).all()                                     # an empty A group
    assert (pairs[6] == 0).all() and np.isnan(out[6]).all() and not flags[6].any()              # a class out of range
    assert (pairs[[0, 2, 4, 7], 1] == 0).all() and np.isnan(out[[2, 4, 7], 1]).all()           # class 0, column 1: empty
    assert (flags[5] == TOO_LARGE).all() and (pairs[5] == 0).all() and np.isnan(out[5]).all()   # 65 diagrams
    assert pairs[4, 0] == 63 and pairs[4, 2] == 2 and pairs[7, 2] == 2                          # degenerate; B shorter than A
    assert flags[3, 2] == TOO_LARGE and np.isfinite(out[3, 2]) and pairs[3, 2] == 14            # 320 + 256 rows; degenerate
    assert not flags[[0, 1, 2, 4, 6, 7]].any()
    # one entry by hand: numpy's mean over the pair kernel's values
    g, c = 7, 3
    p = CLS_A[g] * N_COL + c
    idx = [i for i in range(min(A_SIZES[g], B_SIZES[p])) if not S["status_b"][S["seg_b"][p] + i] & DEGENERATE]
    ra, ca = _pack(S["A"], CAP_A)
    rb, cb = _pack(S["B"], CAP_B)
    w = engine.sliced_wasserstein_batch(ra, ca, rb, cb, dirs, idx_a=S["seg_a"][g] + np.array(idx), idx_b=S["seg_b"][p] + np.array(idx),
                                        ctx=ctx)
    v = np.full(A_SIZES[g], np.nan)
    v[idx] = w
    assert pairs[g, c] == len(idx) == 14 and out[g, c] == np.nanmean(v[:len(idx)])


def test_matrix_without_a_bank(ctx, dev, matrix_case):
    import torch
    S = matrix_case
    dirs = utils.default_directions(4)
    TA = _prep(ctx, dev, S["A"][:3], CAP_A, dirs)
    TB = _prep(ctx, dev, [], CAP_B, dirs)
    i32 = lambda a: _t(np.asarray(a, np.int32), dev)
    o, p, f = engine.sliced_matrix_dev(TA, i32([0, 1, 3]), i32([0, 1]), TB, i32(np.zeros(N_CLS * N_COL + 1)), i32([]), N_COL, ctx=ctx)
    torch.cuda.synchronize()
    assert o.shape == (2, N_COL) and np.isnan(o.cpu().numpy()).all() and not p.cpu().numpy().any() and not f.cpu().numpy().any()
