"""
recordings.MatchMismatchPlan, the host plan of the match-mismatch pass: numpy only, no GPU.  The layout is the 12
recordings of the control pass' GPU test.
"""
import os

import numpy as np

from tda_eeg_audio_amd import recordings

HERE = os.path.dirname(os.path.abspath(__file__))
CORPUS = np.load(os.path.join(HERE, "golden", "corpus_n_samples.npy"))
FIX = [int(CORPUS.min()), int(CORPUS.max())] + [int(v) for v in np.unique(CORPUS)[[5, 17, 29, 40]]]
E2E_L = [FIX[0], 746, FIX[1], FIX[2], 560, FIX[3], 2800, FIX[4], 3100, FIX[5], 900, FIX[0]]
E2E_LE = [FIX[0], 746, FIX[1], FIX[2] - 62, 560, FIX[3], 2800, FIX[4], 3100, FIX[5], 900, FIX[0]]
E2E_BUDGET = 12_000
N, NB = len(E2E_L), 5


def _bank_windows(P):
    """{recording: per band the window offsets of its audio windows relative to its own band-passed envelope}."""
    out = {}
    for j, u in enumerate(P.bank):
        per = []
        for b in range(NB):
            g = b * len(P.bank) + j
            w = P.bank_start[P.seg_off_bank[g]:P.seg_off_bank[g + 1]]
            per.append(w - b * P.bank_off[-1] - P.bank_off[j])
        out[int(u)] = np.stack(per)
    return out


def test_default_candidates_are_all_recordings_in_order():
    P = recordings.MatchMismatchPlan(E2E_L, E2E_LE, None, E2E_BUDGET)
    assert P.candidates.tolist() == list(range(N)) and P.own_col.tolist() == list(range(N)) and P.n_col == N
    assert len(P.shards) >= 3
    # the bank is ControlPlan's for a partner table that names the same recordings
    C = recordings.ControlPlan(E2E_L, E2E_LE, np.roll(np.arange(N), 1), E2E_BUDGET)
    assert np.array_equal(P.bank, C.bank) and np.array_equal(P.bank_off, C.bank_off)
    assert np.array_equal(P.seg_off_bank, C.seg_off_bank) and np.array_equal(P.bank_start, C.bank_start)
    assert np.array_equal(P.seg_off_col, P.seg_off_bank)                 # every candidate has a window: no empty group
    assert P.shards == C.shards
    # the EEG side of every shard is ControlPlan's; the band and the own column of every EEG group
    for (r0, r1), t, tc in zip(P.shards, P.tables, C.tables):
        for key in ("eeg_off", "live", "seg_off", "seg_off_e", "grp_e", "eeg_start", "eeg_ld"):
            assert np.array_equal(t[key], tc[key]), key
        n_live = len(t["live"])
        assert t["cls_e"].tolist() == np.repeat(np.arange(NB), n_live).tolist() and t["cls_e"].dtype == np.int32
        assert t["own_col_e"].tolist() == np.tile(r0 + t["live"], NB).tolist() and len(t["cls_e"]) == len(t["seg_off"]) - 1
    # window selection: the EEG's own count and the envelope's own (recording 3: one audio window less, both capped)
    assert P.n_win_e[3] == P.n_win_a[3] + 1 and P.k_e[3] == P.k_a[3] == 15 and not np.array_equal(P.picks_e[3], P.picks_a[3])


def test_sublist_keeps_its_order():
    cand = [7, 2, 9, 0, 4]                                               # omits recordings, not sorted
    P = recordings.MatchMismatchPlan(E2E_L, E2E_LE, cand, E2E_BUDGET)
    assert P.candidates.tolist() == cand and P.n_col == 5
    assert P.own_col.tolist() == [3, -1, 1, -1, 4, -1, -1, 0, -1, 2, -1, -1]
    for c, r in enumerate(cand):
        assert P.own_col[r] == c
    assert P.bank.tolist() == cand                                       # the bank in the order of the columns
    assert np.array_equal(P.bank_off, np.concatenate([[0], np.cumsum(np.array(E2E_LE)[cand])]))
    assert np.array_equal(np.diff(P.seg_off_col), np.tile(P.k_a[cand], NB)) and len(P.seg_off_col) == NB * 5 + 1
    # the same windows per recording as ControlPlan's bank for a partner table naming these recordings (sorted there)
    partner = np.full(N, -1)
    partner[:5] = cand
    C = recordings.ControlPlan(E2E_L, E2E_LE, partner, E2E_BUDGET)
    assert C.bank.tolist() == sorted(cand)
    wp, wc = _bank_windows(P), _bank_windows(C)
    for r in cand:
        assert np.array_equal(wp[r], wc[r]) and np.array_equal(wp[r][0], P.picks_a[r] * P.step)
    for (r0, r1), t in zip(P.shards, P.tables):
        assert t["own_col_e"].tolist() == np.tile(P.own_col[r0 + t["live"]], NB).tolist()


def test_candidate_without_audio_window_keeps_its_column():
    L = [1500, 200, 1200]                                                # 200 samples: no window at all
    P = recordings.MatchMismatchPlan(L, None, None)
    assert P.k_a.tolist()[1] == 0 and P.k_e.tolist()[1] == 0 and P.empty.tolist() == [1]
    assert P.n_col == 3 and P.own_col.tolist() == [0, 1, 2] and P.bank.tolist() == [0, 2]
    k = np.diff(P.seg_off_col).reshape(NB, 3)
    assert (k[:, 1] == 0).all() and (k[:, 0] == P.k_a[0]).all() and (k[:, 2] == P.k_a[2]).all()
    # the empty groups take no window: the offsets index the bank's diagrams (band-major over the candidates WITH a window)
    assert P.seg_off_col[-1] == P.seg_off_bank[-1] and np.array_equal(np.unique(P.seg_off_col), np.unique(P.seg_off_bank))
    P2 = recordings.MatchMismatchPlan(L, None, [2, 1])
    assert P2.own_col.tolist() == [-1, 1, 0] and P2.bank.tolist() == [2]
    assert np.diff(P2.seg_off_col).reshape(NB, 2)[:, 1].tolist() == [0] * NB
    t = P.tables[0]
    assert t["live"].tolist() == [0, 2] and t["own_col_e"].tolist() == [0, 2] * NB
