"""
The host side of the control experiment (scripts/matched_vs_mismatched.py), without a GPU: the partner table
(recordings.mismatch_partners), the plan of recordings.ControlPass (recordings.ControlPlan) and the statistics
(drivers.control_summary).
"""
import csv
import os

import numpy as np

from tda_eeg_audio_amd import drivers, preprocess, recordings

HERE = os.path.dirname(os.path.abspath(__file__))
CORPUS = np.load(os.path.join(HERE, "golden", "corpus_n_samples.npy"))
with open(os.path.join(HERE, "golden", "corpus_files.csv"), newline="", encoding="utf-8") as _f:
    FILES = [(r["filename"], r["condition"]) for r in csv.DictReader(_f)]
NAMES, CONDS = [f for f, _ in FILES], [c for _, c in FILES]


def _mvm_partners(names, conds):
    """mvm:98-118 restated: per condition the sorted file names of every subject; subjects of both conditions; the
    mismatched audio of a recording is the FIRST file of its subject in the other condition."""
    subj_files = {"slow": {}, "fast": {}}
    for cond in ("slow", "fast"):
        for name in sorted(n for n, c in zip(names, conds) if c == cond):
            subj_files[cond].setdefault(name[:-4].split("_")[0], []).append(name)
    common = sorted(set(subj_files["slow"]) & set(subj_files["fast"]))
    index = {(c, n): r for r, (n, c) in enumerate(zip(names, conds))}
    out = np.full(len(names), -1, np.int64)
    for s in common:
        for fn in subj_files["slow"][s]:
            out[index[("slow", fn)]] = index[("fast", subj_files["fast"][s][0])]
        for fn in subj_files["fast"][s]:
            out[index[("fast", fn)]] = index[("slow", subj_files["slow"][s][0])]
    return out, common


def test_fixture_goes_with_the_lengths():
    assert len(FILES) == len(CORPUS) == 1416 and len(set(FILES)) == 1416
    assert set(CONDS) == {"slow", "fast"}


def test_mismatch_partners_on_the_corpus():
    p = recordings.mismatch_partners(NAMES, CONDS)
    ref, common = _mvm_partners(NAMES, CONDS)
    assert p.dtype == np.int64 and np.array_equal(p, ref)
    assert len(common) == 45 and len(np.unique(p)) == 90 and (p >= 0).all()
    subj = [n[:-4].split("_")[0] for n in NAMES]
    for r, q in enumerate(p):
        assert subj[q] == subj[r] and CONDS[q] != CONDS[r]
        same = sorted(n for n, c, s in zip(NAMES, CONDS, subj) if c == CONDS[q] and s == subj[q])
        assert NAMES[q] == same[0]
    # stems instead of file names: the same table
    assert np.array_equal(recordings.mismatch_partners([n[:-4] for n in NAMES], CONDS), p)


def test_mismatch_partners_subject_in_one_condition():
    names = ["a_2.mat", "a_1.mat", "b_1.mat", "a_1.mat", "c_9.mat", "a_10.mat"]
    conds = ["slow", "slow", "slow", "fast", "fast", "fast"]
    p = recordings.mismatch_partners(names, conds)
    # a: slow sorted [a_1 (1), a_2 (0)], fast sorted [a_1 (3), a_10 (5)]; b only slow, c only fast
    assert p.tolist() == [3, 3, -1, 1, -1, 1]
    assert recordings.mismatch_partners(["a_1", "a_2"], ["slow", "slow"]).tolist() == [-1, -1]


def _check_tables(P):
    """Everything a shard's tables promise, from the lengths alone."""
    nb, win, step, n_ch = P.nb, P.win, P.step, P.n_ch
    assert P.shards[0][0] == 0 and P.shards[-1][1] == P.n_rec
    assert all(a[1] == b[0] for a, b in zip(P.shards, P.shards[1:])) and all(b > a for a, b in P.shards)
    for (r0, r1), t in zip(P.shards, P.tables):
        n = r1 - r0
        live, live_a = t["live"], t["live_a"]
        assert np.array_equal(live, np.flatnonzero(P.k_e[r0:r1] > 0)) and np.array_equal(live_a, np.flatnonzero(P.k_a[r0:r1] > 0))
        assert np.array_equal(np.diff(t["seg_off_e"]), np.tile(P.k_e[r0 + live], nb)) and t["seg_off_e"][0] == 0
        assert np.array_equal(np.diff(t["seg_off_a"]), np.tile(P.k_a[r0 + live_a], nb)) and t["seg_off_a"][0] == 0
        assert t["seg_off"] is t["seg_off_e"]
        assert len(t["grp_e"]) == t["seg_off_e"][-1]
        assert all((t["seg_off_e"][g] <= w < t["seg_off_e"][g + 1]) for w, g in enumerate(t["grp_e"]))
        assert len(t["eeg_start"]) == len(t["eeg_ld"]) == t["seg_off_e"][-1] and len(t["env_start"]) == t["seg_off_a"][-1]
        T, Te = int(t["eeg_off"][-1]), int(t["env_off"][-1])
        w = 0
        for b in range(nb):                                            # every EEG window inside its recording, by picks_e
            for j in live:
                for k in P.picks_e[r0 + j]:
                    s = t["eeg_start"][w] - b * n_ch * T - n_ch * t["eeg_off"][j]
                    assert s == k * step and 0 <= s and s + win <= P.L[r0 + j] and t["eeg_ld"][w] == P.L[r0 + j]
                    w += 1
        w = 0
        for b in range(nb):                                            # every envelope window inside its recording, by picks_a
            for j in live_a:
                for k in P.picks_a[r0 + j]:
                    s = t["env_start"][w] - b * Te - t["env_off"][j]
                    assert s == k * step and 0 <= s and s + win <= P.Le[r0 + j]
                    w += 1
        assert len(t["partner_own"]) == len(t["partner_bank"]) == nb * len(live)
        for b in range(nb):
            for e, j in enumerate(live):
                g, r = b * len(live) + e, r0 + j
                own, bank = t["partner_own"][g], t["partner_bank"][g]
                if P.k_a[r] == 0:
                    assert own == -1
                else:
                    assert own == b * len(live_a) + list(live_a).index(j)
                    assert t["seg_off_a"][own + 1] - t["seg_off_a"][own] == P.k_a[r]
                q = P.partner[r]
                if q < 0 or P.k_a[q] == 0:
                    assert bank == -1
                else:
                    assert bank == b * len(P.bank) + list(P.bank).index(q)
                    assert P.seg_off_bank[bank + 1] - P.seg_off_bank[bank] == P.k_a[q]
        assert n >= 1
    # the bank: windows of the partners' packed envelopes
    assert np.array_equal(np.diff(P.seg_off_bank), np.tile(P.k_a[P.bank], nb))
    Tb = int(P.bank_off[-1])
    assert Tb == P.Le[P.bank].sum() and len(P.bank_start) == P.seg_off_bank[-1]
    w = 0
    for b in range(nb):
        for j, u in enumerate(P.bank):
            for k in P.picks_a[u]:
                s = P.bank_start[w] - b * Tb - P.bank_off[j]
                assert s == k * step and s + win <= P.Le[u]
                w += 1


def test_control_plan_on_the_corpus():
    partner = recordings.mismatch_partners(NAMES, CONDS)
    P = recordings.ControlPlan(CORPUS, None, partner)
    assert len(P.shards) == len(recordings.RaggedPlan(CORPUS).shards) >= 2
    covered = np.concatenate([np.arange(a, b) for a, b in P.shards])
    assert np.array_equal(covered, np.arange(len(CORPUS)))
    assert len(P.U) == 90 and len(P.bank) == 90 and np.array_equal(P.U, np.unique(partner))
    assert (P.k_e == 15).all() and (P.k_a == 15).all() and P.seg_off_bank[-1] == 90 * 5 * 15
    _check_tables(P)
    # an arbitrary table: the bank is sized by it
    rng = np.random.default_rng(3)
    Q = recordings.ControlPlan(CORPUS, None, rng.permutation(len(CORPUS)))
    assert len(Q.bank) == len(CORPUS) and Q.seg_off_bank[-1] == len(CORPUS) * 5 * 15


def test_control_plan_hand_made():
    #        0: k_e 9, k_a 8   1: partner shorter   2: no window    3: no partner   4: 6 windows, partner of 1
    L = [746, 3000, 200, 1500, 560]
    Le = [746 - 62, 3000, 200, 1500, 560]
    partner = [1, 4, 3, -1, 2]          # 4's partner has no window at all
    P = recordings.ControlPlan(L, Le, partner, shard_samples=3800)
    assert P.k_e.tolist() == [9, 15, 0, 15, 6] and P.k_a.tolist() == [8, 15, 0, 15, 6]
    assert preprocess.n_windows(746) == 9 and preprocess.n_windows(684) == 8
    assert P.empty.tolist() == [2]
    assert len(P.shards) >= 2
    assert P.U.tolist() == [1, 2, 3, 4] and P.bank.tolist() == [1, 3, 4] and P.bank_pos.tolist() == [-1, 0, -1, 1, 2]
    _check_tables(P)
    # recording 1 (15 EEG windows) is paired with the 6 diagrams of recording 4; recording 4 with nothing
    for (r0, r1), t in zip(P.shards, P.tables):
        for e, j in enumerate(t["live"]):
            r = r0 + j
            if r == 1:
                g = t["partner_bank"][e]
                assert P.seg_off_bank[g + 1] - P.seg_off_bank[g] == 6
            if r in (3, 4):
                assert t["partner_bank"][e] == -1
    # no partner table at all: matched only
    N = recordings.ControlPlan(L, Le, None)
    assert len(N.bank) == 0 and all((t["partner_bank"] == -1).all() for t in N.tables)


def test_fdr_bh_by_hand():
    # sorted 0.005 0.01 0.03 0.04 0.5 -> * 5 / rank: 0.025 0.025 0.05 0.05 0.5; running minimum from the top: the same
    rej, adj = drivers.fdr_bh([0.04, 0.005, 0.5, 0.01, 0.03])
    assert np.allclose(adj, [0.05, 0.025, 0.5, 0.025, 0.05], rtol=0, atol=1e-15)
    assert rej.tolist() == [True, True, False, True, True]
    # the running minimum matters: 0.02 0.021 -> 0.04 0.021 -> both 0.021; clipped at 1
    rej, adj = drivers.fdr_bh([0.021, 0.02])
    assert np.allclose(adj, [0.021, 0.021], rtol=0, atol=1e-15)
    assert drivers.fdr_bh([0.9, 0.8, 1.0])[1].max() <= 1.0


def test_control_summary():
    from scipy.stats import wilcoxon
    rng = np.random.default_rng(12)
    bands = ["delta", "theta", "alpha", "beta", "gamma"]
    n_subj, per = 9, 4
    subjects = np.repeat([f"bb{i:02d}" for i in range(n_subj)], per)
    conditions = np.tile(["slow", "fast"], n_subj * per // 2)
    rows = np.empty((n_subj * per, 5, 4))
    rows[:, :, 0] = 1.0 + 0.1 * rng.standard_normal((n_subj * per, 5))
    rows[:, :, 1] = rows[:, :, 0] + 0.05 + 0.1 * rng.standard_normal((n_subj * per, 5))
    rows[:, :, 2:] = 15
    rows[:, 1, 1] = rows[:, 1, 0]                         # theta: every difference zero -> p = 1.0
    rows[per * 5:, 2, 1] = np.nan                         # alpha: only 5 subjects keep a row
    rows[per * 4:, 3, 0] = np.nan                         # beta: 4 subjects -> insufficient
    rows[3, 0, 0] = np.nan                                # delta: one row of subject 0 dropped
    res = drivers.control_summary(rows, subjects, conditions, bands)
    assert list(res) == bands
    assert res["beta"] == {"n": 4, "status": "insufficient"}
    assert res["alpha"]["n"] == 5 and res["theta"]["p"] == 1.0 and res["theta"]["n_matched_lower"] == 0
    for b, band in enumerate(bands):
        if band == "beta":
            continue
        ok = ~np.isnan(rows[:, b, 0]) & ~np.isnan(rows[:, b, 1])
        sm = np.array([[rows[ok & (subjects == s), b, 0].mean(), rows[ok & (subjects == s), b, 1].mean()]
                       for s in sorted(set(subjects[ok]))])
        diff = sm[:, 0] - sm[:, 1]
        r = res[band]
        assert r["n"] == len(sm)
        assert r["w_matched"] == sm[:, 0].mean() and r["w_mismatched"] == sm[:, 1].mean()
        assert r["direction"] == ("matched < mismatched" if sm[:, 0].mean() < sm[:, 1].mean() else "matched > mismatched")
        if band != "theta":
            assert r["p"] == wilcoxon(diff)[1]
        assert r["cohens_d"] == np.mean(diff) / (np.std(diff, ddof=1) + 1e-10)
        assert r["n_matched_lower"] == int((diff < 0).sum()) and r["pct_matched_lower"] == (diff < 0).sum() / len(sm) * 100
    pv = [res[b].get("p", 1.0) for b in bands]
    _, adj = drivers.fdr_bh(pv)
    for i, band in enumerate(bands):
        if band == "beta":
            assert "p_fdr" not in res[band]
        else:
            assert res[band]["p_fdr"] == adj[i] and res[band]["sig_fdr"] == bool(adj[i] <= 0.05)
    assert set(res["delta"]) == {"n", "w_matched", "w_mismatched", "direction", "p", "cohens_d", "n_matched_lower",
                                 "pct_matched_lower", "p_fdr", "sig_fdr"}
