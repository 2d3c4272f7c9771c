"""
The host plan of recordings.RaggedRecordingPass (no GPU): per recording the window count, picks and window tables of
process_recording at its own length (scripts/tda_eeg_audio_comparison.py:70-80, nb1:341), restated here with numpy, and
the shard split (contiguous ranges closed at a sample budget).
"""
import os

import numpy as np
import pytest

from tda_eeg_audio_amd import recordings

HERE = os.path.dirname(os.path.abspath(__file__))
CORPUS = np.load(os.path.join(HERE, "golden", "corpus_n_samples.npy"))
WIN, STEP, NB, NCH = 250, 62, 5, 47


def per_rec(n):                                   # nb1:341
    return (n - WIN) // STEP + 1 if n >= WIN else 0


def picks_of(n_win):                              # cmp:77-80
    return np.linspace(0, n_win - 1, 15, dtype=int) if n_win > 15 else np.arange(n_win)


def check_plan(L, Le, budget):
    P = recordings.RaggedPlan(L, Le, shard_samples=budget)
    n_win = np.array([min(per_rec(a), per_rec(b)) for a, b in zip(L, Le)])      # cmp:71
    assert np.array_equal(P.n_win, n_win)
    for r in range(len(L)):
        assert np.array_equal(P.picks[r], picks_of(n_win[r])), r
    assert np.array_equal(P.empty, np.flatnonzero(n_win == 0))
    # shards: every recording in exactly one, contiguous, within the budget unless alone
    covered = np.concatenate([np.arange(a, b) for a, b in P.shards])
    assert np.array_equal(covered, np.arange(len(L)))
    for a, b in P.shards:
        assert b > a
        assert L[a:b].sum() <= budget or b - a == 1
    for (a, b), (c, _) in zip(P.shards, P.shards[1:]):
        assert b == c and L[a:b + 1].sum() > budget                      # closed only when the next one does not fit
    # per shard tables against a direct restatement
    for (a, b), t in zip(P.shards, P.tables):
        off = np.concatenate([[0], np.cumsum(L[a:b])])
        offe = np.concatenate([[0], np.cumsum(Le[a:b])])
        live = [r for r in range(a, b) if n_win[r] > 0]
        seg, est, eld, ast = [0], [], [], []
        for band in range(NB):
            for r in live:
                p = picks_of(n_win[r])
                seg.append(seg[-1] + len(p))
                for j in p:
                    est.append(band * NCH * off[-1] + NCH * off[r - a] + j * STEP)
                    eld.append(L[r])
                    ast.append(band * offe[-1] + offe[r - a] + j * STEP)
        assert np.array_equal(t["live"], np.array(live, dtype=np.int64) - a)
        assert np.array_equal(t["seg_off"], np.array(seg))
        assert np.array_equal(t["eeg_start"], np.array(est, dtype=np.int64))
        assert np.array_equal(t["eeg_ld"], np.array(eld, dtype=np.int64))
        assert np.array_equal(t["env_start"], np.array(ast, dtype=np.int64))
    return P


def test_corpus_fixture():
    assert len(CORPUS) == 1416 and len(np.unique(CORPUS)) == 46
    assert CORPUS.min() == 2663 and CORPUS.max() == 5741 and CORPUS.sum() == 6_007_447


@pytest.mark.parametrize("budget", [recordings.DEFAULT_SHARD_SAMPLES, 400_000])
def test_plan_corpus(budget):
    P = check_plan(CORPUS, CORPUS, budget)
    assert len(P.shards) > 1 and P.k.sum() == 1416 * 15


def test_plan_short_cases():
    # 900 samples: 11 windows (k < 15); 200: no window; EEG != envelope length in both directions; 40: above the pad
    # length, no window; one recording alone above the budget
    L = np.array([2663, 900, 200, 5741, 3000, 4000, 40, 12000, 2700], dtype=np.int64)
    Le = np.array([2663, 900, 200, 5741, 2000, 4500, 40, 12000, 2700], dtype=np.int64)
    P = check_plan(L, Le, 10_000)
    assert P.n_win[1] == 11 and P.k[1] == 11
    assert P.n_win[4] == per_rec(2000) and P.n_win[5] == per_rec(4000)
    assert P.empty.tolist() == [2, 6]
    assert (7, 8) in P.shards


def test_plan_every_window_in_bounds():
    L = np.array([900, 2663, 5741, 200, 3210], dtype=np.int64)
    P = recordings.RaggedPlan(L, L + np.array([0, 100, -300, 0, 62]), shard_samples=6000)
    for (a, b), t in zip(P.shards, P.tables):
        T, Te = int(t["eeg_off"][-1]), int(t["env_off"][-1])
        band = np.repeat(np.arange(NB), len(t["eeg_start"]) // NB)
        # window of recording r: first sample and last row end inside the recording's block
        rec = np.searchsorted(NCH * t["eeg_off"][1:], t["eeg_start"] - band * NCH * T, side="right")
        end = t["eeg_start"] - band * NCH * T + (NCH - 1) * t["eeg_ld"] + WIN
        assert (end <= NCH * t["eeg_off"][rec + 1]).all()
        erec = np.searchsorted(t["env_off"][1:], t["env_start"] - band * Te, side="right")
        assert (t["env_start"] - band * Te + WIN <= t["env_off"][erec + 1]).all()
