"""
The control experiment (scripts/matched_vs_mismatched.py) on the GPU: the cross Wasserstein launch that resolves its
pairs from group tables (engine.wasserstein_cross_dev) against the launch with explicit index arrays, the rows kernel
(engine.cross_rows_dev) against engine.segment_nanmean, and recordings.ControlPass end to end against the per-recording
drivers, the CPU oracle and recordings.RaggedRecordingPass.
"""
import os

import numpy as np
import pytest
from scipy import signal

from tda_eeg_audio_amd import _lib, drivers, engine, preprocess, recordings, synth, utils

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CORPUS = np.load(os.path.join(HERE, "golden", "corpus_n_samples.npy"))
FIX = [int(CORPUS.min()), int(CORPUS.max())] + [int(v) for v in np.unique(CORPUS)[[5, 17, 29, 40]]]
NO_PAIR, DEGENERATE = _lib.TDA_WIN_NO_PAIR, _lib.TDA_WIN_DEGENERATE


def _i32(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)


# ---------------------------------------------------------------------------------------------------------------
# 1. wasserstein_cross_dev == wasserstein_dev on the pairs the tables describe
# ---------------------------------------------------------------------------------------------------------------
#   A group:          0    1    2    3    4    5    6
A_SIZES = [5, 0, 7, 4, 6, 3, 4]
#   B group:          0    1 (short)  2 (long)  3 (degenerate)  4
B_SIZES = [5, 3, 9, 4, 6]
#   A 0 -> B 0 (equal), A 1 empty, A 2 -> B 1 (B shorter), A 3 -> B 2 (B longer), A 4 -> -1, A 5 -> B 3 (degenerate),
#   A 6 -> B 2 (a B group used twice)
PARTNER = [0, 4, 1, 2, -1, 3, 2]


@pytest.fixture(scope="module")
def diagrams(ctx):
    """A: diagrams of EEG-like distance matrices (rips_dm_dev: H0 capacity 47, H1 256); B: diagrams of Takens clouds
    (takens_rips_dev: H0 capacity 128, H1 256), the windows of B group 3 so short that their clouds have 2 points."""
    import torch
    dev = torch.device("cuda", ctx.device)
    n_a, n_b = sum(A_SIZES), sum(B_SIZES)
    eeg = synth.eeg_windows(n_a, seed=7, windows_per_recording=5)
    A = engine.rips_dm_dev(engine.corr_dist_dev(torch.from_numpy(eeg).to(dev), ctx=ctx), ctx=ctx)
    off_b = np.concatenate([[0], np.cumsum(B_SIZES)])
    aud = torch.from_numpy(synth.audio_windows(n_b, "alpha", seed=3)).to(dev)
    full = engine.takens_rips_dev(aud, engine.tau_dev(aud, 125, ctx=ctx), ctx=ctx)
    short = engine.takens_rips_dev(aud[:B_SIZES[3], :12].contiguous(), torch.full((B_SIZES[3],), 4, dtype=torch.int32, device=dev),
                                   ctx=ctx)
    torch.cuda.synchronize()
    assert (short.status.cpu().numpy() & DEGENERATE).all() and (short.n_points.cpu().numpy() == 2).all()
    assert not (full.status.cpu().numpy() & DEGENERATE).any()
    B = engine.DeviceDiagrams(n_b, full.h0_cap, full.h1_cap, dev)
    for name in ("h0", "h1", "c0", "c1", "status", "n_points"):
        getattr(B, name).copy_(getattr(full, name))
        getattr(B, name)[off_b[3]:off_b[4]].copy_(getattr(short, name))
    return dict(A=A, B=B, dev=dev)


def _host_pairs(seg_a, seg_b, partner, status_b):
    """The pairs of the tables, as mvm:89 makes them: (A diagram, B diagram) by position."""
    ia, ib = [], []
    for g in range(len(seg_a) - 1):
        p = partner[g]
        if p < 0:
            continue
        for i in range(seg_a[g + 1] - seg_a[g]):
            if i < seg_b[p + 1] - seg_b[p] and not (status_b[seg_b[p] + i] & DEGENERATE):
                ia.append(seg_a[g] + i)
                ib.append(seg_b[p] + i)
    return np.array(ia, np.int32), np.array(ib, np.int32)


@pytest.mark.parametrize("dim", ["h0", "h1"])
def test_cross_equals_index_arrays(ctx, diagrams, dim):
    import torch
    A, B, dev = diagrams["A"], diagrams["B"], diagrams["dev"]
    ra, ca, rb, cb = (A.h0, A.c0, B.h0, B.c0) if dim == "h0" else (A.h1, A.c1, B.h1, B.c1)
    # both launch modes: capacities 47 against 128 take one launch, 256 against 256 the small launch and the wide one
    assert (ra.shape[1], rb.shape[1]) == ((47, 128) if dim == "h0" else (256, 256))
    seg_a = np.concatenate([[0], np.cumsum(A_SIZES)]).astype(np.int32)
    seg_b = np.concatenate([[0], np.cumsum(B_SIZES)]).astype(np.int32)
    status_b = B.status.cpu().numpy()
    ia, ib = _host_pairs(seg_a, seg_b, PARTNER, status_b)
    assert len(ia) == 5 + 3 + 4 + 4                               # groups 0, 2 (cut to 3), 3 and 6; none for 1, 4, 5
    ref, ref_st = engine.wasserstein_dev(ra, ca, rb, cb, _i32(ia, dev), _i32(ib, dev), ctx=ctx)
    for grp in (None, _i32(np.repeat(np.arange(len(A_SIZES)), A_SIZES), dev)):
        out, st = engine.wasserstein_cross_dev(ra, ca, _i32(seg_a, dev), rb, cb, _i32(seg_b, dev), B.status, _i32(PARTNER, dev),
                                               grp_a=grp, ctx=ctx)
        torch.cuda.synchronize()
        out, st = out.cpu().numpy(), st.cpu().numpy()
        has = np.zeros(sum(A_SIZES), bool)
        has[ia] = True
        assert np.array_equal(out[ia], ref.cpu().numpy()) and np.array_equal(st[ia], ref_st.cpu().numpy())
        assert (st[ia] == 0).all() and np.isfinite(out[ia]).all()
        assert np.isnan(out[~has]).all() and (st[~has] == NO_PAIR).all()
    assert NO_PAIR not in (1, 2, 4, 8, 16) and NO_PAIR & (NO_PAIR - 1) == 0


def test_cross_empty_and_invalid(ctx, diagrams):
    import torch
    A, B, dev = diagrams["A"], diagrams["B"], diagrams["dev"]
    seg_b = _i32(np.concatenate([[0], np.cumsum(B_SIZES)]), dev)
    # no diagram at all, and no group on the B side
    e = engine.DeviceDiagrams(0, 47, 256, dev)
    out, st = engine.wasserstein_cross_dev(e.h1, e.c1, _i32([0], dev), B.h1, B.c1, seg_b, B.status, _i32([], dev), ctx=ctx)
    assert out.numel() == 0 and st.numel() == 0
    seg_a = _i32(np.concatenate([[0], np.cumsum(A_SIZES)]), dev)
    out, st = engine.wasserstein_cross_dev(A.h1, A.c1, seg_a, e.h1, e.c1, _i32([0], dev), e.status, _i32([-1] * len(A_SIZES), dev),
                                           ctx=ctx)
    torch.cuda.synchronize()
    assert np.isnan(out.cpu().numpy()).all() and (st.cpu().numpy() == NO_PAIR).all()
    # partners that point outside the B table are "no pair", never a read out of bounds
    out, st = engine.wasserstein_cross_dev(A.h1, A.c1, seg_a, B.h1, B.c1, seg_b, B.status, _i32([99] * len(A_SIZES), dev), ctx=ctx)
    torch.cuda.synchronize()
    assert (st.cpu().numpy() == NO_PAIR).all()
    with pytest.raises(_lib.TdaError):                             # bad sizes: TDA_ERR_INVALID
        ctx.check(ctx.lib.tda_wasserstein_cross_dev(ctx.h, engine._tp(A.h1), engine._tp(A.c1), 256, -1, None, None, 1, None, None,
                                                    256, 0, None, 0, None, None, None, None, engine._stream()))
    with pytest.raises(_lib.TdaError):
        ctx.check(ctx.lib.tda_cross_rows_dev(ctx.h, None, None, None, None, None, -1, None, None, None, engine._stream()))


# ---------------------------------------------------------------------------------------------------------------
# 2. cross_rows_dev == segment_nanmean over each group's pairs, and the pair counts
# ---------------------------------------------------------------------------------------------------------------
def test_cross_rows(ctx):
    import torch
    dev = torch.device("cuda", ctx.device)
    sizes = [0, 1, 7, 9, 15, 200, 15, 9, 131, 4]
    #         pairs of the matched side and of the mismatched side (a prefix of the group, some shorter than it)
    n_m = [0, 1, 7, 8, 15, 200, 0, 9, 129, 4]
    n_x = [0, 0, 3, 9, 15, 137, 15, 1, 131, 4]
    seg = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    n = int(seg[-1])
    nan = float("nan")

    def side(pairs, seed):
        r = np.random.default_rng(seed)
        w, st = np.full(n, nan), np.full(n, NO_PAIR, np.int32)
        for g, m in enumerate(pairs):
            w[seg[g]:seg[g] + m] = r.uniform(0.1, 3.0, m) * 10.0 ** r.integers(-3, 4, m)
            st[seg[g]:seg[g] + m] = 0
        paired = np.flatnonzero(st == 0)
        bad = r.choice(paired, size=12, replace=False)                # a solver that gave up: NaN, status set
        w[bad], st[bad] = nan, _lib.TDA_WIN_NOT_CONVERGED
        return w, st
    wm, sm = side(n_m, 1)
    wx, sx = side(n_x, 2)
    sm[seg[9]:seg[10]] = _lib.TDA_WIN_NOT_CONVERGED                   # group 9, matched: every pair NaN
    wm[seg[9]:seg[10]] = nan
    status_a = np.zeros(n, np.int32)
    status_a[seg[4] + 3] = _lib.TDA_WIN_CLASS_OVERFLOW
    status_a[seg[7]] = DEGENERATE                                     # a result, not a flag
    flags = torch.full((len(sizes),), -1, dtype=torch.int32, device=dev)
    t = lambda a: torch.from_numpy(a).to(dev)                         # noqa: E731
    rows = engine.cross_rows_dev(t(wm), t(sm), t(wx), t(sx), t(seg), status_a=t(status_a), seg_flags=flags, ctx=ctx)
    torch.cuda.synchronize()
    rows, flags = rows.cpu().numpy(), flags.cpu().numpy()
    assert rows.shape == (len(sizes), 4)
    for col, (w, st, pairs) in enumerate([(wm, sm, n_m), (wx, sx, n_x)]):
        vals = np.concatenate([np.where(st[seg[g]:seg[g] + m] == 0, w[seg[g]:seg[g] + m], nan) for g, m in enumerate(pairs)])
        ref = engine.segment_nanmean(vals, np.concatenate([[0], np.cumsum(pairs)]).astype(np.int32), ctx=ctx)
        assert np.array_equal(rows[:, col], ref, equal_nan=True), col
        assert np.array_equal(rows[:, 2 + col], np.array(pairs, float))
        for g, m in enumerate(pairs):                                  # and numpy itself, group by group
            v = vals[sum(pairs[:g]):sum(pairs[:g]) + m]
            if m and not np.isnan(v).all():
                assert rows[g, col] == np.nanmean(v), (g, col)
            else:
                assert np.isnan(rows[g, col])
    assert np.isnan(rows[9, 0]) and rows[9, 2] == 4
    exp = np.zeros(len(sizes), np.int32)
    for g in range(len(sizes)):
        for st, pairs in ((sm, n_m), (sx, n_x)):
            exp[g] |= np.bitwise_or.reduce(st[seg[g]:seg[g] + pairs[g]], initial=0)
        exp[g] |= np.bitwise_or.reduce(status_a[seg[g]:seg[g + 1]], initial=0)
    exp &= ~(NO_PAIR | DEGENERATE)
    assert np.array_equal(flags, exp) and flags[4] & _lib.TDA_WIN_CLASS_OVERFLOW and not flags[7] & DEGENERATE
    # no group at all
    assert engine.cross_rows_dev(t(wm), t(sm), t(wx), t(sx), t(seg[:1]), ctx=ctx).shape == (0, 4)


# ---------------------------------------------------------------------------------------------------------------
# 3.-6. ControlPass end to end
# ---------------------------------------------------------------------------------------------------------------
#            subject bb01: 2 slow, 2 fast      bb02: 1 slow, 2 fast        bb03: 2 slow, 1 fast       bb04: slow only
E2E_NAMES = ["bb01_ut02.mat", "bb01_ut01.mat", "bb01_ut01.mat", "bb01_ut03.mat", "bb02_ut01.mat", "bb02_ut05.mat",
             "bb02_ut04.mat", "bb03_ut01.mat", "bb03_ut02.mat", "bb03_ut01.mat", "bb04_ut01.mat", "bb04_ut02.mat"]
E2E_CONDS = ["slow", "slow", "fast", "fast", "slow", "fast", "fast", "slow", "slow", "fast", "slow", "slow"]
#  746: 9 windows, 560: 6 windows; recording 3: envelope 62 samples shorter than the EEG (one window less)
E2E_L = [FIX[0], 746, FIX[1], FIX[2], 560, FIX[3], 2800, FIX[4], 3100, FIX[5], 900, FIX[0]]
E2E_LE = [FIX[0], 746, FIX[1], FIX[2] - 62, 560, FIX[3], 2800, FIX[4], 3100, FIX[5], 900, FIX[0]]
E2E_BUDGET = 12_000


def _raw(rng, L, n_ch=47):
    return rng.standard_normal((n_ch, L)) + 0.5 * rng.standard_normal((1, L))


def _env(rng, L):
    return np.abs(rng.standard_normal(L)).cumsum() * 0.01 + np.abs(rng.standard_normal(L))


def _bas():
    return [signal.butter(4, [max(lo / 125, 0.001), min(hi / 125, 0.999)], btype="band") for lo, hi in preprocess.FREQ_BANDS.values()]


def _driver_diagrams(raws, envs):
    """The per-recording level (mvm:36-85 through the drivers): per recording and band the EEG diagrams of the windows
    selected from the EEG's own count, and the audio diagrams of get_audio_diagrams_from_windows; the band-passed windows
    are kept for the oracle."""
    out = []
    for raw, env in zip(raws, envs):
        per = []
        for b, (lo, hi) in enumerate(preprocess.FREQ_BANDS.values()):
            y = signal.sosfiltfilt(preprocess.design_bandpass_filter(lo, hi, 250), raw, axis=-1)
            bb, aa = _bas()[b]
            aw = utils.create_windows(signal.filtfilt(bb, aa, env), 250, 62)
            n_e = int(preprocess.n_windows(raw.shape[1]))
            ew = np.stack([y[:, k * 62:k * 62 + 250] for k in recordings.select_windows(n_e)])
            h0, h1, st = engine.rips_dm_batch(engine.corr_dist_batch(ew, want_corr=False))
            assert not st.any()
            per.append(dict(eeg=[[a, c] for a, c in zip(h0, h1)], aud=drivers.get_audio_diagrams_from_windows(aw), ew=ew,
                            aw=aw[recordings.select_windows(len(aw))]))
        out.append(per)
    return out


def _driver_rows(dg, partner):
    rows = np.full((len(dg), 5, 4), np.nan)
    for r in range(len(dg)):
        for b in range(5):
            eeg, own = dg[r][b]["eeg"], dg[r][b]["aud"]
            mis = dg[partner[r]][b]["aud"] if partner[r] >= 0 else []
            rows[r, b] = [drivers.compute_cross_wasserstein(eeg, own), drivers.compute_cross_wasserstein(eeg, mis),
                          min(len(eeg), len(own)), min(len(eeg), len(mis))]
    return rows


@pytest.fixture(scope="module")
def e2e(ctx):
    import torch
    dev = torch.device("cuda", ctx.device)
    rng = np.random.default_rng(77)
    raws = [_raw(rng, L) for L in E2E_L]
    envs = [_env(rng, L) for L in E2E_LE]
    xh, _ = preprocess.pack_recordings(raws)
    eh, _ = preprocess.pack_recordings(envs)
    partner = recordings.mismatch_partners(E2E_NAMES, E2E_CONDS)
    cp = recordings.ControlPass(E2E_L, E2E_LE, partner, dev, shard_samples=E2E_BUDGET, n_sets=2, ctx=ctx)
    rows = cp.run(xh, eh).numpy().copy()
    return dict(cp=cp, raws=raws, envs=envs, xh=xh, eh=eh, dev=dev, partner=partner, rows=rows, dg=_driver_diagrams(raws, envs))


def test_control_pass_fixture_is_what_the_issue_asks(e2e):
    P, partner = e2e["cp"].plan, e2e["partner"]
    assert len(E2E_L) >= 10 and len(set(E2E_L) & set(CORPUS.tolist())) >= 6 and {CORPUS.min(), CORPUS.max()} <= set(E2E_L)
    assert partner.tolist() == [2, 2, 1, 1, 6, 4, 4, 9, 9, 7, -1, -1]
    assert len(P.shards) >= 3
    shard_of = np.concatenate([[i] * (b - a) for i, (a, b) in enumerate(P.shards)])
    assert sum(shard_of[r] != shard_of[q] for r, q in enumerate(partner) if q >= 0) >= 3     # partners in other shards
    assert P.k_e[1] == 9 and P.k_e[4] == 6 and P.k_e[3] == P.k_a[3] + 0 == 15                # (both capped at 15 ...)
    assert P.n_win_e[3] == P.n_win_a[3] + 1                                                  # ... from different counts
    assert not np.array_equal(P.picks_e[3], P.picks_a[3])


def test_control_pass_equals_drivers(e2e):
    rows, partner = e2e["rows"], e2e["partner"]
    ref = _driver_rows(e2e["dg"], partner)
    assert rows.shape == (len(E2E_L), 5, 4)
    for r in range(len(E2E_L)):
        print(r, "matched", rows[r, :, 0], ref[r, :, 0], "mismatched", rows[r, :, 1], ref[r, :, 1], "pairs", rows[r, 0, 2:], ref[r, 0, 2:])
    assert np.array_equal(np.isnan(rows), np.isnan(ref))
    assert np.array_equal(rows[:, :, 2:], ref[:, :, 2:])
    assert np.array_equal(rows, ref, equal_nan=True)
    # what the cases are there for
    assert (rows[1, :, 2] == 9).all() and (rows[1, :, 3] == 9).all()          # 9 EEG windows against 15 of the partner
    assert (rows[2, :, 2] == 15).all() and (rows[2, :, 3] == 9).all()         # 15 EEG windows against a partner with 9
    assert (rows[5, :, 3] == 6).all() and (rows[4, :, 2] == 6).all()
    assert np.isnan(rows[10:, :, 1]).all() and (rows[10:, :, 3] == 0).all() and np.isfinite(rows[10:, :, 0]).all()
    again = e2e["cp"].run(e2e["xh"], e2e["eh"]).numpy()
    assert np.array_equal(again, rows, equal_nan=True)


def test_control_pass_against_cpu_oracle(e2e):
    from oracle import brute, port
    rows, partner, dg = e2e["rows"], e2e["partner"], e2e["dg"]
    n_pairs = 0
    for r, b in [(1, 0), (3, 2), (5, 4), (8, 1)]:
        eeg = [port.rips_dm(port.corr_dist(w)[1])[1] for w in dg[r][b]["ew"]]
        for col, q in ((0, r), (1, partner[r])):
            aw = dg[q][b]["aw"]
            tau = int(port.compute_tau(aw[0], max_lag=125))
            aud = [port.audio_persistence(w, tau)[0][1] for w in aw]
            n = min(len(eeg), len(aud))
            vals = [brute.safe_wasserstein_oracle(eeg[i], aud[i]) for i in range(n)]
            print(r, b, col, n, rows[r, b, col], np.nanmean(vals))
            assert rows[r, b, 2 + col] == n and abs(rows[r, b, col] - np.nanmean(vals)) < 1e-6
            n_pairs += n
    assert n_pairs >= 40


def test_control_matched_equals_ragged_pass(e2e, ctx):
    rp = recordings.RaggedRecordingPass(E2E_L, E2E_LE, e2e["dev"], shard_samples=E2E_BUDGET, n_sets=2, ctx=ctx)
    cmp_rows = rp.run(e2e["xh"], e2e["eh"]).numpy()
    same = [r for r in range(len(E2E_L)) if E2E_L[r] == E2E_LE[r]]
    assert len(same) == len(E2E_L) - 1
    assert np.isfinite(e2e["rows"][same, :, 0]).all()
    assert np.array_equal(e2e["rows"][same, :, 0], cmp_rows[same, :, 1])
    assert np.array_equal(e2e["rows"][same, :, 2], cmp_rows[same, :, 3])
    # where the envelope gives another window count the two experiments select other windows: cmp:71 against mvm:44-49
    assert not np.array_equal(e2e["rows"][3, :, 0], cmp_rows[3, :, 1])


def test_control_pass_arbitrary_partner_table(e2e, ctx):
    rng = np.random.default_rng(5)
    n = len(E2E_L)
    while True:                                                    # a derangement: nobody is its own partner
        perm = rng.permutation(n)
        if (perm != np.arange(n)).all():
            break
    cp = recordings.ControlPass(E2E_L, E2E_LE, perm, e2e["dev"], shard_samples=E2E_BUDGET, n_sets=2, ctx=ctx)
    assert len(cp.plan.bank) == n
    rows = cp.run(e2e["xh"], e2e["eh"]).numpy()
    ref = _driver_rows(e2e["dg"], perm)
    assert np.array_equal(rows, ref, equal_nan=True)
    assert np.array_equal(rows[:, :, 0], e2e["rows"][:, :, 0], equal_nan=True)


def test_control_pass_recording_without_a_window(ctx):
    """A recording without an EEG window gets a NaN row with zero pair counts (mvm:73), and so does the mismatched side
    of the recording it is the partner of (mvm:52: no window, no audio list); one shard, no partner for the last."""
    import torch
    dev = torch.device("cuda", ctx.device)
    rng = np.random.default_rng(9)
    L = [1500, 200, 1200]
    raws = [_raw(rng, v) for v in L]
    envs = [_env(rng, v) for v in L]
    xh, _ = preprocess.pack_recordings(raws)
    eh, _ = preprocess.pack_recordings(envs)
    cp = recordings.ControlPass(L, None, np.array([1, 0, -1]), dev, ctx=ctx)
    assert len(cp.plan.shards) == 1 and cp.empty.tolist() == [1] and cp.plan.bank.tolist() == [0]
    rows = cp.run(xh, eh).numpy()
    dg = _driver_diagrams([raws[0], raws[2]], [envs[0], envs[2]])
    ref = _driver_rows(dg, np.array([-1, -1]))
    assert np.array_equal(rows[[0, 2]], ref, equal_nan=True)
    assert np.isfinite(rows[[0, 2], :, 0]).all() and np.isnan(rows[[0, 2], :, 1]).all()
    assert np.isnan(rows[1, :, :2]).all() and (rows[1, :, 2:] == 0).all()
