"""
The match-mismatch matrix on the GPU: engine.wasserstein_matrix_dev against the column-by-column route
(engine.wasserstein_cross_dev + engine.cross_rows_dev) and against explicit index arrays, engine.match_rows_dev against a
numpy restatement, and recordings.MatchMismatchPass end to end against recordings.ControlPass, the per-recording drivers
and the CPU oracle.
"""
import os

import numpy as np
import pytest
from scipy import signal

from tda_eeg_audio_amd import _lib, drivers, engine, preprocess, recordings, utils

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CORPUS = np.load(os.path.join(HERE, "golden", "corpus_n_samples.npy"))
FIX = [int(CORPUS.min()), int(CORPUS.max())] + [int(v) for v in np.unique(CORPUS)[[5, 17, 29, 40]]]
NO_PAIR, DEGENERATE = _lib.TDA_WIN_NO_PAIR, _lib.TDA_WIN_DEGENERATE
CAP = 256


def _t(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _i32(a, dev):
    return _t(np.asarray(a, dtype=np.int32), dev)


# ---------------------------------------------------------------------------------------------------------------
# 1. wasserstein_matrix_dev == wasserstein_cross_dev + cross_rows_dev per column, on synthetic diagrams
# ---------------------------------------------------------------------------------------------------------------
N_CLS, N_COL = 2, 5
A_SIZES = [0, 1, 3, 7, 8, 9, 15, 15, 2]           # 7, 8, 9: around the eight accumulators of numpy's sum
CLS_A = [0, 1, 0, 1, 0, 1, 0, 1, -1]              # the last group has no class: no entry anywhere
B_SIZES = [15, 0, 4, 20, 1,                       # class 0, columns 0..4
           1, 20, 15, 0, 4]                       # class 1
ROWS = [0, 1, 40, 65, 130, CAP, 38, 43]           # rows per diagram: 65 is one past the small layout


def _diagram_set(n, seed, h0):
    """(n, CAP, 2) rows and counts: H1-like (distinct births) or H0-like (births 0, deaths ascending: the 1-D path);
    some rows with an inf death, some NaN."""
    r = np.random.default_rng(seed)
    rows = np.zeros((n, CAP, 2))
    cnt = np.array([ROWS[(i * 3 + seed) % len(ROWS)] for i in range(n)], np.int32)
    for i in range(n):
        k = int(cnt[i])
        b = np.zeros(k) if h0 else r.uniform(0.0, 1.0, k)
        d = b + r.uniform(0.01, 0.8, k)
        if h0:
            d = np.sort(d)
        if k > 2 and i % 4 == 1:
            d[-1] = np.inf                          # the essential class of an H0 diagram, an open H1 class
        if k > 5 and i % 7 == 3:
            b[2], d[2] = np.nan, np.nan
        rows[i, :k, 0], rows[i, :k, 1] = b, d
    return rows, cnt


def _finite(rows, cnt, i):
    return int(np.isfinite(rows[i, :cnt[i]]).all(axis=1).sum())


@pytest.fixture(scope="module")
def synthetic(ctx):
    import torch
    dev = torch.device("cuda", ctx.device)
    seg_a = np.concatenate([[0], np.cumsum(A_SIZES)]).astype(np.int32)
    seg_b = np.concatenate([[0], np.cumsum(B_SIZES)]).astype(np.int32)
    status_b = np.zeros(seg_b[-1], np.int32)
    status_b[[seg_b[0] + 2, seg_b[3] + 0, seg_b[6] + 16, seg_b[7] + 5]] = DEGENERATE     # first, middle, past every A group
    status_b[seg_b[2] + 1] = _lib.TDA_WIN_H1_TRUNCATED                                   # another bit: still a pair
    return dict(dev=dev, seg_a=seg_a, seg_b=seg_b, status_b=status_b)


def _column_route(ctx, S, ra, ca, rb, cb, c):
    """Column c by the two-launch route: (mean, pairs, flags) per A group."""
    import torch
    dev = S["dev"]
    partner = [k * N_COL + c if 0 <= k < N_CLS else -1 for k in CLS_A]
    w, st = engine.wasserstein_cross_dev(ra, ca, _i32(S["seg_a"], dev), rb, cb, _i32(S["seg_b"], dev), _i32(S["status_b"], dev),
                                         _i32(partner, dev), ctx=ctx)
    fl = torch.full((len(A_SIZES),), -1, dtype=torch.int32, device=dev)
    rows = engine.cross_rows_dev(w, st, w, st, _i32(S["seg_a"], dev), seg_flags=fl, ctx=ctx)
    torch.cuda.synchronize()
    rows = rows.cpu().numpy()
    return rows[:, 1], rows[:, 3].astype(np.int32), fl.cpu().numpy(), w.cpu().numpy(), st.cpu().numpy()


@pytest.mark.parametrize("kind", ["h1", "h0"])
def test_matrix_equals_column_route(ctx, synthetic, kind):
    import torch
    S, dev = synthetic, synthetic["dev"]
    a_rows, a_cnt = _diagram_set(sum(A_SIZES), 1, kind == "h0")
    b_rows, b_cnt = _diagram_set(sum(B_SIZES), 2, kind == "h0")
    ra, ca, rb, cb = _t(a_rows, dev), _t(a_cnt, dev), _t(b_rows, dev), _t(b_cnt, dev)
    n_seg = len(A_SIZES)
    exp = [_column_route(ctx, S, ra, ca, rb, cb, c) for c in range(N_COL)]
    exp_out = np.stack([e[0] for e in exp], axis=1)
    exp_pairs = np.stack([e[1] for e in exp], axis=1)
    exp_flags = np.stack([e[2] for e in exp], axis=1)
    got = {}
    try:
        for scheme in (ctx.SCHEME_ONE, ctx.SCHEME_GRID, ctx.SCHEME_LISTS):
            ctx.set_launch_scheme(scheme)
            out = torch.full((n_seg, N_COL), -7.0, dtype=torch.float64, device=dev)
            pairs = torch.full((n_seg, N_COL), -7, dtype=torch.int32, device=dev)
            flags = torch.full((n_seg, N_COL), -7, dtype=torch.int32, device=dev)
            for _ in range(2):                                       # twice: the list of the first call is left empty
                engine.wasserstein_matrix_dev(ra, ca, _i32(S["seg_a"], dev), _i32(CLS_A, dev), rb, cb, _i32(S["seg_b"], dev),
                                              _i32(S["status_b"], dev), N_COL, out_t=out, pairs_t=pairs, flags_t=flags, ctx=ctx)
            torch.cuda.synchronize()
            got[scheme] = (out.cpu().numpy(), pairs.cpu().numpy(), flags.cpu().numpy())
    finally:
        ctx.set_launch_scheme(ctx.SCHEME_LISTS)
    for scheme, (out, pairs, flags) in got.items():
        print(kind, scheme, "out", out, "pairs", pairs, "flags", flags, sep="\n")
        assert np.array_equal(out, exp_out, equal_nan=True), scheme
        assert np.array_equal(pairs, exp_pairs) and np.array_equal(flags, exp_flags), scheme
    out, pairs, flags = got[ctx.SCHEME_LISTS]
    # what the shape is there for
    assert (pairs[0] == 0).all() and np.isnan(out[0]).all()            # an empty A group
    assert (pairs[8] == 0).all() and np.isnan(out[8]).all()            # a group without a class
    assert (pairs[:, 1][[0, 2, 4, 6]] == 0).all()                      # class 0, column 1: a column without audio
    assert np.isfinite(out).sum() >= 25 and (pairs == 15).any() and (pairs == 14).any()    # (14: a degenerate B diagram)
    assert not flags.any()
    # at least one pair does not fit the 64 x 64 layout of the first launch
    wide = 0
    for g, k in enumerate(CLS_A):
        for c in range(N_COL):
            if k < 0:
                continue
            p = k * N_COL + c
            for i in range(min(A_SIZES[g], B_SIZES[p])):
                ia, ib = S["seg_a"][g] + i, S["seg_b"][p] + i
                if not S["status_b"][ib] & DEGENERATE:
                    wide += max(_finite(a_rows, a_cnt, ia), _finite(b_rows, b_cnt, ib)) > 64
    assert wide >= 1
    # independently, a few entries from explicit index arrays and numpy's nanmean on the host
    for g, c in [(3, 0), (5, 1), (6, 3), (7, 2), (2, 2)]:
        p = CLS_A[g] * N_COL + c
        n_pos = min(A_SIZES[g], B_SIZES[p])
        idx = [i for i in range(n_pos) if not S["status_b"][S["seg_b"][p] + i] & DEGENERATE]
        w, st = engine.wasserstein_dev(ra, ca, rb, cb, _i32(S["seg_a"][g] + np.array(idx), dev), _i32(S["seg_b"][p] + np.array(idx), dev),
                                       ctx=ctx)
        torch.cuda.synchronize()
        assert not st.cpu().numpy().any()
        # the route's rule (cross_rows_kernel): the first len(idx) positions of the group are its pairs
        vals = np.full(n_pos, np.nan)
        vals[idx] = w.cpu().numpy()
        assert pairs[g, c] == len(idx) and out[g, c] == np.nanmean(vals[:len(idx)]), (g, c)


def test_matrix_empty_and_oversized(ctx, synthetic):
    import torch
    S, dev = synthetic, synthetic["dev"]
    a_rows, a_cnt = _diagram_set(sum(A_SIZES), 1, False)
    b_rows, b_cnt = _diagram_set(sum(B_SIZES), 2, False)
    ra, ca, rb, cb = _t(a_rows, dev), _t(a_cnt, dev), _t(b_rows, dev), _t(b_cnt, dev)
    seg_a, seg_b, cls, stb = _i32(S["seg_a"], dev), _i32(S["seg_b"], dev), _i32(CLS_A, dev), _i32(S["status_b"], dev)
    out = torch.full((16,), -7.0, dtype=torch.float64, device=dev)
    pairs = torch.full((16,), -7, dtype=torch.int32, device=dev)
    flags = torch.full((16,), -7, dtype=torch.int32, device=dev)
    tp, lib = engine._tp, ctx.lib
    for n_seg, n_col in ((0, N_COL), (len(A_SIZES), 0)):              # OK, and nothing is written
        ctx.check(lib.tda_wasserstein_matrix_dev(ctx.h, tp(ra), tp(ca), CAP, ra.shape[0], tp(seg_a), n_seg, tp(cls), tp(rb), tp(cb), CAP,
                                                 rb.shape[0], tp(seg_b), N_CLS, n_col, tp(stb), tp(out), tp(pairs), tp(flags),
                                                 engine._stream()))
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == -7.0).all() and (pairs.cpu().numpy() == -7).all() and (flags.cpu().numpy() == -7).all()
    with pytest.raises(_lib.TdaError):
        ctx.check(lib.tda_wasserstein_matrix_dev(ctx.h, tp(ra), tp(ca), CAP, ra.shape[0], tp(seg_a), -1, tp(cls), tp(rb), tp(cb), CAP,
                                                 rb.shape[0], tp(seg_b), N_CLS, N_COL, tp(stb), tp(out), tp(pairs), tp(flags),
                                                 engine._stream()))
    # no B side at all: NaN and 0 pairs everywhere
    e = engine.DeviceDiagrams(0, 128, CAP, dev)
    o, p, f = engine.wasserstein_matrix_dev(ra, ca, seg_a, cls, e.h1, e.c1, _i32(np.zeros(N_CLS * N_COL + 1), dev), e.status, N_COL, ctx=ctx)
    torch.cuda.synchronize()
    assert np.isnan(o.cpu().numpy()).all() and not p.cpu().numpy().any() and not f.cpu().numpy().any()
    # a group of more than 64 diagrams: NaN, 0 pairs, TDA_WIN_TOO_LARGE; the group beside it is untouched by that
    big = np.zeros((66, 4, 2))
    big[:, 0] = [0.1, 0.5]
    bc = np.ones(66, np.int32)
    o, p, f = engine.wasserstein_matrix_dev(_t(big, dev), _t(bc, dev), _i32([0, 65, 66], dev), _i32([0, 0], dev), _t(big, dev), _t(bc, dev),
                                            _i32([0, 66], dev), _i32(np.zeros(66), dev), 1, ctx=ctx)
    torch.cuda.synchronize()
    assert np.isnan(o.cpu().numpy()[0, 0]) and p.cpu().numpy()[0, 0] == 0 and f.cpu().numpy()[0, 0] == _lib.TDA_WIN_TOO_LARGE
    assert o.cpu().numpy()[1, 0] == 0.0 and p.cpu().numpy()[1, 0] == 1 and f.cpu().numpy()[1, 0] == 0


# ---------------------------------------------------------------------------------------------------------------
# 2. match_rows_dev against numpy
# ---------------------------------------------------------------------------------------------------------------
def _match_rows_numpy(dist, pairs, own_col):
    """[w_own, n_own_pairs, n_valid, n_less, n_equal, null_mean] per row of a (n, n_col) matrix."""
    n, n_col = dist.shape
    rows = np.full((n, 6), np.nan)
    rows[:, 1:5] = 0.0
    for g in range(n):
        own = int(own_col[g])
        others = np.isfinite(dist[g])
        if own >= 0:
            others[own] = False
            rows[g, 1] = pairs[g, own]
        w = dist[g, own] if own >= 0 else np.nan
        v = dist[g, others]
        rows[g, 0], rows[g, 2] = w, len(v)
        if not np.isnan(w):
            rows[g, 3], rows[g, 4] = np.sum(v < w), np.sum(v == w)
        if len(v):
            rows[g, 5] = v.mean()
    return rows


def _assert_match_rows(rows, ref):
    """Counts exactly; null_mean within (n_valid + 1) * 2^-52 relative (terms >= 0: any order of summation)."""
    assert np.array_equal(rows[:, :5], ref[:, :5], equal_nan=True)
    assert np.array_equal(np.isnan(rows[:, 5]), np.isnan(ref[:, 5]))
    ok = ~np.isnan(ref[:, 5])
    err = np.abs(rows[ok, 5] - ref[ok, 5])
    print("null_mean: max relative error", (err / ref[ok, 5]).max() if ok.any() else 0.0)
    assert (err <= (ref[ok, 2] + 1) * 2.0 ** -52 * ref[ok, 5]).all()


def test_match_rows(ctx):
    import torch
    dev = torch.device("cuda", ctx.device)
    r = np.random.default_rng(11)
    n, n_col = 11, 9
    dist = r.uniform(0.05, 2.0, (n, n_col)) * 10.0 ** r.integers(-2, 3, (n, n_col))
    pairs = r.integers(1, 16, (n, n_col)).astype(np.int32)
    own = np.array([0, 8, 3, 4, -1, 2, 5, 7, 1, 6, 0], np.int32)
    dist[2, [0, 5]] = dist[2, 3]                     # ties with the own value
    dist[3, 7] = dist[3, 4]
    dist[1, [2, 6]] = np.nan                         # NaN columns
    dist[6, :] = np.nan                              # nothing at all
    dist[7, 7] = np.nan                              # a NaN own entry
    dist[9, [0, 1, 2, 3, 4, 5, 7, 8]] = np.nan       # only the own column
    dist[10, 0] = dist[10].min() / 2                 # the own audio is the closest
    pairs[np.isnan(dist)] = 0
    flags = np.zeros((n, n_col), np.int32)
    flags[0, 3] = _lib.TDA_WIN_NOT_CONVERGED
    flags[5, [1, 8]] = [NO_PAIR, DEGENERATE]         # never set by the matrix; masked all the same
    seg = np.arange(0, 3 * n + 1, 3).astype(np.int32)
    status_a = np.zeros(3 * n, np.int32)
    status_a[seg[4] + 1] = _lib.TDA_WIN_CLASS_OVERFLOW
    status_a[seg[8]] = DEGENERATE
    sf = torch.full((n,), -1, dtype=torch.int32, device=dev)
    rows = engine.match_rows_dev(_t(dist, dev), _t(pairs, dev), _t(flags, dev), _t(own, dev), status_a=_t(status_a, dev),
                                 seg_off_a=_t(seg, dev), seg_flags=sf, ctx=ctx)
    torch.cuda.synchronize()
    rows, sf = rows.cpu().numpy(), sf.cpu().numpy()
    ref = _match_rows_numpy(dist, pairs, own)
    print(rows, ref, sep="\n")
    _assert_match_rows(rows, ref)
    assert rows[2, 4] == 2 and rows[3, 4] == 1 and rows[10, 3] == 0 and rows[10, 4] == 0
    assert np.isnan(rows[4, 0]) and rows[4, 2] == n_col and np.isnan(rows[7, 0]) and rows[7, 2] == n_col - 1 and rows[7, 1] == 0
    assert rows[6, 2] == 0 and np.isnan(rows[6, 5]) and rows[9, 2] == 0 and np.isfinite(rows[9, 0])
    exp = np.zeros(n, np.int32)
    exp[0], exp[4] = _lib.TDA_WIN_NOT_CONVERGED, _lib.TDA_WIN_CLASS_OVERFLOW
    assert np.array_equal(sf, exp)
    # without the A side's status words, and no group at all
    sf2 = torch.full((n,), -1, dtype=torch.int32, device=dev)
    engine.match_rows_dev(_t(dist, dev), _t(pairs, dev), _t(flags, dev), _t(own, dev), seg_flags=sf2, ctx=ctx)
    torch.cuda.synchronize()
    assert sf2.cpu().numpy().tolist() == [_lib.TDA_WIN_NOT_CONVERGED] + [0] * (n - 1)
    assert engine.match_rows_dev(_t(dist[:0], dev), _t(pairs[:0], dev), _t(flags[:0], dev), _t(own[:0], dev), ctx=ctx).shape == (0, 6)


# ---------------------------------------------------------------------------------------------------------------
# 3. MatchMismatchPass end to end (the 12 recordings of the control pass' test: corpus minimum and maximum lengths,
#    >= 3 shards, an envelope 62 samples shorter than its EEG, groups of 6, 9 and 15 windows)
# ---------------------------------------------------------------------------------------------------------------
E2E_L = [FIX[0], 746, FIX[1], FIX[2], 560, FIX[3], 2800, FIX[4], 3100, FIX[5], 900, FIX[0]]
E2E_LE = [FIX[0], 746, FIX[1], FIX[2] - 62, 560, FIX[3], 2800, FIX[4], 3100, FIX[5], 900, FIX[0]]
E2E_BUDGET = 12_000
N_REC = len(E2E_L)


def _raw(rng, L, n_ch=47):
    return rng.standard_normal((n_ch, L)) + 0.5 * rng.standard_normal((1, L))


def _env(rng, L):
    return np.abs(rng.standard_normal(L)).cumsum() * 0.01 + np.abs(rng.standard_normal(L))


def _driver_diagrams(raws, envs):
    """The per-recording level (mvm:36-85 through the drivers): per recording and band the EEG diagrams of the windows
    selected from the EEG's own count and the audio diagrams of get_audio_diagrams_from_windows; the band-passed windows
    are kept for the oracle."""
    bas = [signal.butter(4, [max(lo / 125, 0.001), min(hi / 125, 0.999)], btype="band") for lo, hi in preprocess.FREQ_BANDS.values()]
    out = []
    for raw, env in zip(raws, envs):
        per = []
        for b, (lo, hi) in enumerate(preprocess.FREQ_BANDS.values()):
            y = signal.sosfiltfilt(preprocess.design_bandpass_filter(lo, hi, 250), raw, axis=-1)
            aw = utils.create_windows(signal.filtfilt(bas[b][0], bas[b][1], env), 250, 62)
            n_e = int(preprocess.n_windows(raw.shape[1]))
            ew = np.stack([y[:, k * 62:k * 62 + 250] for k in recordings.select_windows(n_e)])
            h0, h1, st = engine.rips_dm_batch(engine.corr_dist_batch(ew, want_corr=False))
            assert not st.any()
            per.append(dict(eeg=[[a, c] for a, c in zip(h0, h1)], aud=drivers.get_audio_diagrams_from_windows(aw), ew=ew,
                            aw=aw[recordings.select_windows(len(aw))]))
        out.append(per)
    return out


@pytest.fixture(scope="module")
def e2e(ctx):
    import torch
    dev = torch.device("cuda", ctx.device)
    rng = np.random.default_rng(77)
    raws = [_raw(rng, L) for L in E2E_L]
    envs = [_env(rng, L) for L in E2E_LE]
    xh, _ = preprocess.pack_recordings(raws)
    eh, _ = preprocess.pack_recordings(envs)
    mp = recordings.MatchMismatchPass(E2E_L, E2E_LE, None, dev, shard_samples=E2E_BUDGET, n_sets=2, ctx=ctx)
    rows = mp.run(xh, eh).numpy().copy()
    return dict(mp=mp, raws=raws, envs=envs, xh=xh, eh=eh, dev=dev, rows=rows, dist=mp.dist_h.numpy().copy(),
                pairs=mp.pairs_h.numpy().copy())


def test_pass_shapes_and_plan(e2e):
    mp = e2e["mp"]
    assert len(mp.plan.shards) >= 3 and mp.n_col == N_REC and mp.own_col.tolist() == list(range(N_REC))
    assert e2e["rows"].shape == (N_REC, 5, 6) and e2e["dist"].shape == (N_REC, 5, N_REC) and e2e["pairs"].shape == (N_REC, 5, N_REC)
    assert e2e["dist"].dtype == np.float64 and e2e["pairs"].dtype == np.int32
    assert mp.plan.k_e[1] == 9 and mp.plan.k_e[4] == 6 and mp.plan.k_e[3] == mp.plan.k_a[3] == 15
    assert np.isfinite(e2e["dist"]).all() and (e2e["pairs"] >= 6).all()


def test_pass_equals_control_pass(e2e, ctx):
    """(a) the columns of three cyclic partner tables and the own column, bit for bit."""
    dist, pairs = e2e["dist"], e2e["pairs"]
    r = np.arange(N_REC)
    for s in (1, 5, 7):
        partner = (r + s) % N_REC
        cp = recordings.ControlPass(E2E_L, E2E_LE, partner, e2e["dev"], shard_samples=E2E_BUDGET, n_sets=2, ctx=ctx)
        rows = cp.run(e2e["xh"], e2e["eh"]).numpy()
        assert np.array_equal(dist[r, :, partner], rows[:, :, 1]), s
        assert np.array_equal(pairs[r, :, partner], rows[:, :, 3]), s
        assert np.array_equal(dist[r, :, r], rows[:, :, 0]) and np.array_equal(pairs[r, :, r], rows[:, :, 2]), s
    assert np.array_equal(e2e["rows"][:, :, 0], dist[r, :, r]) and np.array_equal(e2e["rows"][:, :, 1], pairs[r, :, r])


@pytest.fixture(scope="module")
def driver_dg(e2e):
    return _driver_diagrams(e2e["raws"], e2e["envs"])


def test_pass_equals_drivers(e2e, driver_dg):
    """(b) all 12 x 12 x 5 entries against the per-recording drivers, bit for bit."""
    dist, pairs = e2e["dist"], e2e["pairs"]
    ref, ref_n = np.empty_like(dist), np.empty_like(pairs)
    for r in range(N_REC):
        for c in range(N_REC):
            for b in range(5):
                eeg, aud = driver_dg[r][b]["eeg"], driver_dg[c][b]["aud"]
                ref[r, b, c], ref_n[r, b, c] = drivers.compute_cross_wasserstein(eeg, aud), min(len(eeg), len(aud))
    assert np.array_equal(pairs, ref_n)
    assert np.array_equal(dist, ref, equal_nan=True)
    assert set(np.unique(pairs)) >= {6, 9, 15}


def test_pass_against_cpu_oracle(e2e, driver_dg):
    """(c) four entries off the diagonal against the CPU oracle, within 1e-6."""
    from oracle import brute, port
    n_pairs = 0
    for r, c, b in [(1, 2, 0), (3, 0, 2), (5, 4, 4), (8, 11, 1)]:
        eeg = [port.rips_dm(port.corr_dist(w)[1])[1] for w in driver_dg[r][b]["ew"]]
        aw = driver_dg[c][b]["aw"]
        tau = int(port.compute_tau(aw[0], max_lag=125))
        aud = [port.audio_persistence(w, tau)[0][1] for w in aw]
        n = min(len(eeg), len(aud))
        vals = [brute.safe_wasserstein_oracle(eeg[i], aud[i]) for i in range(n)]
        print(r, c, b, n, e2e["dist"][r, b, c], np.nanmean(vals))
        assert e2e["pairs"][r, b, c] == n and abs(e2e["dist"][r, b, c] - np.nanmean(vals)) < 1e-6
        n_pairs += n
    assert n_pairs >= 40


def test_pass_rows_and_second_run(e2e):
    """(d) rows_h is match_rows applied to dist_h; (e) a second run returns identical arrays."""
    own = np.arange(N_REC)
    for b in range(5):
        _assert_match_rows(e2e["rows"][:, b], _match_rows_numpy(e2e["dist"][:, b], e2e["pairs"][:, b], own))
    mp = e2e["mp"]
    again = mp.run(e2e["xh"], e2e["eh"]).numpy()
    assert np.array_equal(again, e2e["rows"], equal_nan=True)
    assert np.array_equal(mp.dist_h.numpy(), e2e["dist"], equal_nan=True) and np.array_equal(mp.pairs_h.numpy(), e2e["pairs"])
    with pytest.raises(ValueError):
        recordings.MatchMismatchPass(E2E_L, E2E_LE, None, e2e["dev"], ctx=e2e["mp"].ctx, correlations=True)


# ---------------------------------------------------------------------------------------------------------------
# 4. a candidate sub-list, a recording without a window
# ---------------------------------------------------------------------------------------------------------------
def test_pass_sublist_and_empty(ctx):
    import torch
    dev = torch.device("cuda", ctx.device)
    rng = np.random.default_rng(9)
    L = [1500, 200, 1200]
    raws = [_raw(rng, v) for v in L]
    envs = [_env(rng, v) for v in L]
    xh, _ = preprocess.pack_recordings(raws)
    eh, _ = preprocess.pack_recordings(envs)
    mp = recordings.MatchMismatchPass(L, None, None, dev, ctx=ctx)
    assert mp.empty.tolist() == [1] and mp.plan.bank.tolist() == [0, 2] and mp.own_col.tolist() == [0, 1, 2]
    rows = mp.run(xh, eh).numpy().copy()
    dist, pairs = mp.dist_h.numpy().copy(), mp.pairs_h.numpy().copy()
    # the recording without a window: an all-NaN row and, as a candidate, an all-NaN column with 0 pairs
    assert np.isnan(dist[1]).all() and not pairs[1].any() and np.isnan(rows[1, :, [0, 5]]).all() and not rows[1, :, 1:5].any()
    assert np.isnan(dist[:, :, 1]).all() and not pairs[:, :, 1].any()
    assert np.isfinite(dist[[0, 2]][:, :, [0, 2]]).all() and (pairs[[0, 2]][:, :, [0, 2]] > 0).all()
    assert (rows[[0, 2], :, 2] == 1).all()                             # one other finite column each
    # columns in the order of the list
    sub = recordings.MatchMismatchPass(L, None, [2, 0], dev, ctx=ctx)
    assert sub.own_col.tolist() == [1, -1, 0] and sub.n_col == 2
    rows2 = sub.run(xh, eh).numpy()
    assert np.array_equal(sub.dist_h.numpy(), dist[:, :, [2, 0]], equal_nan=True)
    assert np.array_equal(sub.pairs_h.numpy(), pairs[:, :, [2, 0]])
    assert np.array_equal(rows2[[0, 2]], rows[[0, 2]], equal_nan=True)
    assert np.isnan(rows2[1]).sum() == 5 * 2 and not rows2[1, :, 1:5].any()
