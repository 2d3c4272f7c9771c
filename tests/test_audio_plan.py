"""
The host plan of the ragged audio front end (no GPU): preprocess.AudioPlan against scipy.signal.resample_poly's output
lengths, _resample_plan's filter and hilbert_envelope's g tables; the byte-budget shard plan of RaggedPlan
(RaggedAudioRecordingPass); the default RaggedPlan unchanged.
"""
import os

import numpy as np
import pytest
from scipy import signal

from tda_eeg_audio_amd import preprocess, recordings

HERE = os.path.dirname(os.path.abspath(__file__))
CORPUS = np.load(os.path.join(HERE, "golden", "corpus_n_samples.npy"))
# short (below the filter's 17,641 taps and below one output period of 882), odd / even, a few seconds
LENGTHS = [1, 2, 881, 882, 883, 5000, 17_640, 17_641, 44_100 * 3 + 17, 44_100 * 2 + 882, 2663 * 882 // 5]


def hilbert_g(n):                                 # hilbert_envelope: np.fft.ifft(hh).imag
    hh = np.zeros(n)
    if n % 2 == 0:
        hh[0] = hh[n // 2] = 1; hh[1:n // 2] = 2
    else:
        hh[0] = 1; hh[1:(n + 1) // 2] = 2
    return np.fft.ifft(hh).imag


def test_output_lengths_match_resample_poly():
    P = preprocess.AudioPlan(LENGTHS)
    for La, n in zip(LENGTHS, P.n_out):
        assert n == len(signal.resample_poly(np.zeros(La), 250, 44100)), La
    assert np.array_equal(P.out_off, np.concatenate([[0], np.cumsum(P.n_out)]))
    # the corpus recipe of tools/audio_frontend_bench.py: La = L * 882 // 5 resamples to exactly L
    L = CORPUS[:40]
    assert np.array_equal(preprocess.AudioPlan(L * 882 // 5).n_out, L)


@pytest.mark.parametrize("La", LENGTHS)
def test_filter_equals_resample_plan_up_to_trailing_zeros(La):
    P = preprocess.AudioPlan(LENGTHS)
    h, up, down, n_pre_remove, n_out = preprocess._resample_plan(La, 250, 44100)
    assert (P.up, P.down, P.n_pre_remove) == (up, down, n_pre_remove) == (5, 882, 11)
    m = min(len(h), len(P.h))
    assert np.array_equal(P.h[:m], h[:m]) and not P.h[m:].any() and not h[m:].any()
    # the polyphase table: hp[p, q] = h[p + up*q], zero past the end of h
    assert P.hp.shape == (up, P.nq) and P.nq * up >= len(P.h)
    for p in range(up):
        tap = p + up * np.arange(P.nq)
        assert np.array_equal(P.hp[p], np.where(tap < len(P.h), P.h[np.minimum(tap, len(P.h) - 1)], 0.0))


def test_hilbert_tables():
    lengths = np.array([7, 1, 2, 6, 7, 2, 5741, 6, 5740])
    ht = preprocess.HilbertTables(lengths)
    assert np.array_equal(ht.lengths, np.unique(lengths))
    assert len(ht.g) == int(np.unique(lengths).sum())                   # one table per DISTINCT length
    for n, o in zip(lengths, ht.g_off):
        assert np.array_equal(ht.g[o:o + n], hilbert_g(int(n))), n
    P = preprocess.AudioPlan(LENGTHS)
    for n, o in zip(P.n_out, P.hilbert.g_off):
        assert np.array_equal(P.hilbert.g[o:o + n], hilbert_g(int(n)))


def test_audio_plan_rejects_empty_audio():
    with pytest.raises(ValueError):
        preprocess.AudioPlan([44100, 0])


@pytest.mark.parametrize("budget", [1 << 26, 1 << 28, 1 << 30, 10 << 30])
def test_byte_budget_plan(budget):
    L = CORPUS.astype(np.int64)
    La = L * 882 // 5
    P = recordings.RaggedPlan(L, L, shard_bytes=budget, audio_lengths=La)
    cost = 8 * (47 * L + La)
    assert np.array_equal(P.cost, cost)
    covered = np.concatenate([np.arange(a, b) for a, b in P.shards])
    assert np.array_equal(covered, np.arange(len(L)))                   # every recording once, in order
    for a, b in P.shards:
        assert b > a and (cost[a:b].sum() <= budget or b - a == 1)
    for (a, b), (c, _) in zip(P.shards, P.shards[1:]):
        assert b == c and cost[a:b + 1].sum() > budget                 # closed only when the next one does not fit
    # the default of the audio lengths: the envelope lengths
    Q = recordings.RaggedPlan(L, L // 2, shard_bytes=budget)
    assert np.array_equal(Q.cost, 8 * (47 * L + L // 2))


def test_byte_budget_single_oversized_recording():
    P = recordings.RaggedPlan([1000, 5000, 1000], shard_bytes=8 * 48 * 1500, audio_lengths=[1000, 5000, 1000])
    assert P.shards == [(0, 1), (1, 2), (2, 3)]


def test_default_plan_unchanged():
    L = CORPUS.astype(np.int64)
    for budget in (300_000, recordings.DEFAULT_SHARD_SAMPLES):
        P = recordings.RaggedPlan(L, shard_samples=budget)
        Q = recordings.RaggedPlan(L, L, budget, 47, 5, 250, 1.0, 0.75, recordings.MAX_WINDOWS)
        # restated: contiguous ranges closed at a budget of EEG samples
        shards, r0, acc = [], 0, 0
        for r in range(len(L)):
            if r > r0 and acc + L[r] > budget:
                shards.append((r0, r)); r0, acc = r, 0
            acc += int(L[r])
        shards.append((r0, len(L)))
        assert P.shards == Q.shards == shards
