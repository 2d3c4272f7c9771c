"""
drivers.match_mismatch_summary and drivers.match_rows_host, host only: the per-band statistics of the match-mismatch
matrix on a seeded synthetic matrix with planted ties, NaNs and a missing own column.
"""
import numpy as np
import pytest
from scipy import stats

from tda_eeg_audio_amd import drivers

N, NB = 40, 5
BANDS = ["delta", "theta", "alpha", "beta", "gamma"]
SUBJECTS = [f"bb{r // 4:02d}" for r in range(N)]                          # ten infants, four recordings each


@pytest.fixture(scope="module")
def case():
    r = np.random.default_rng(2024)
    dist = r.uniform(0.5, 3.0, (N, NB, N))
    idx = np.arange(N)
    dist[idx, :, idx] *= np.linspace(0.3, 1.1, NB)[None, :]              # the own audio closer, band by band less so
    dist[3, 1, [5, 9, 11]] = dist[3, 1, 3]                               # ties with the own value
    dist[4, 0, 7] = dist[4, 0, 4]
    dist[6, 2, 6] = dist[6, 2].min() / 2                                 # rank 1 ...
    dist[8, 2, 30] = dist[8, 2, 8]                                       # ... and a tie for it
    dist[8, 2, 8] = dist[8, 2, 30] = dist[8, 2].min() / 2
    dist[10, :, [1, 2, 3]] = np.nan                                      # NaN columns
    dist[12, 3, :] = np.nan                                              # a (recording, band) without anything
    dist[14, :, 14] = np.nan                                             # a missing own column
    dist[:, :, 20] = np.nan                                              # a candidate without audio
    own = idx.copy()
    rows = np.zeros((N, NB, 6))
    m = drivers.match_rows_host(dist, own)
    rows[:, :, 0], rows[:, :, 2:] = m[:, :, 0], m[:, :, 1:]
    rows[:, :, 1] = np.where(np.isnan(rows[:, :, 0]), 0, 15)
    return dict(dist=dist, rows=rows, own=own)


def _midranks(dist, own_col, keep=None):
    """Midrank of the own audio among the finite candidates (scipy's average ranks), NaN where it has none."""
    out = np.full(dist.shape[:2], np.nan)
    n_valid = np.zeros(dist.shape[:2])
    for r in range(dist.shape[0]):
        for b in range(dist.shape[1]):
            use = np.isfinite(dist[r, b]) & (True if keep is None else keep[r])
            use[own_col[r]] = np.isfinite(dist[r, b, own_col[r]])
            n_valid[r, b] = use.sum() - use[own_col[r]]
            if use[own_col[r]]:
                cols = np.flatnonzero(use)
                out[r, b] = stats.rankdata(dist[r, b, cols], method="average")[list(cols).index(own_col[r])]
    return out, n_valid


def test_midranks_are_scipys(case):
    rows, dist = case["rows"], case["dist"]
    rank, n_valid = _midranks(dist, case["own"])
    got = 1 + rows[:, :, 3] + rows[:, :, 4] / 2
    ok = ~np.isnan(rank)
    assert np.array_equal(got[ok], rank[ok]) and np.array_equal(rows[:, :, 2], n_valid)
    assert np.isnan(rows[~ok][:, 0]).all() and not rows[~ok][:, 3:5].any()
    assert rows[3, 1, 4] == 3 and rows[4, 0, 4] == 1 and rank[6, 2] == 1 and rank[8, 2] == 1.5
    assert np.isnan(rows[14, :, 0]).all() and (rows[14, :, 2] == N - 2).all() and np.isnan(rows[12, 3, 5]) and rows[12, 3, 2] == 0
    # the null mean is numpy's over the other finite columns
    assert rows[10, 0, 5] == np.delete(dist[10, 0], [1, 2, 3, 10, 20]).mean() and rows[10, 0, 2] == N - 5


def test_summary_follows_from_the_ranks(case):
    rows, dist = case["rows"], case["dist"]
    res = drivers.match_mismatch_summary(rows, dist, SUBJECTS, None, BANDS)
    rank, n_valid = _midranks(dist, case["own"])
    raw_p = []
    for b, band in enumerate(BANDS):
        ok = ~np.isnan(rank[:, b]) & (n_valid[:, b] > 0)
        e = res[band]
        assert e["n"] == ok.sum() and e["n"] == N - 2 - (b == 3)      # without 14 and 20 (no own value), 12 in band 3
        assert e["top1"] == np.mean(rank[ok, b] == 1)
        assert e["mean_percentile"] == pytest.approx(np.mean((rank[ok, b] - 1) / n_valid[ok, b]), rel=1e-14)
        assert e["matched_mean"] == pytest.approx(rows[ok, b, 0].mean(), rel=1e-14)
        assert e["null_mean"] == pytest.approx(rows[ok, b, 5].mean(), rel=1e-14)
        diff = rows[ok, b, 0] - rows[ok, b, 5]
        assert e["p"] == stats.wilcoxon(diff)[1]
        assert e["cohens_d"] == pytest.approx(diff.mean() / (diff.std(ddof=1) + 1e-10), rel=1e-12)
        raw_p.append(e["p"])
    assert res["delta"]["top1"] > res["gamma"]["top1"] and res["delta"]["mean_percentile"] < 0.1 < res["gamma"]["mean_percentile"]
    assert res["alpha"]["top1"] < 1.0                                     # (recording 8 ties for rank 1: midrank 1.5)
    # Benjamini-Hochberg: control_summary's helper on the same raw p-values
    reject, adj = drivers.fdr_bh(raw_p)
    for b, band in enumerate(BANDS):
        assert res[band]["p_fdr"] == adj[b] and res[band]["sig_fdr"] == bool(reject[b])
    # too few recordings: no statistics, and the band counts as p = 1 in the correction
    few = drivers.match_mismatch_summary(rows[:4], dist[:4, :, :4], SUBJECTS[:4], None, BANDS)
    assert all(few[b] == {"n": 4, "status": "insufficient"} for b in BANDS)


def test_excluding_same_subject_columns(case):
    rows, dist, own = case["rows"], case["dist"], case["own"]
    subj = np.array(SUBJECTS)
    keep = subj[:, None] != subj[None, :]
    m = drivers.match_rows_host(dist, own, keep=keep)
    rank, n_valid = _midranks(dist, own, keep)
    ok = ~np.isnan(rank)
    assert np.array_equal((1 + m[:, :, 2] + m[:, :, 3] / 2)[ok], rank[ok]) and np.array_equal(m[:, :, 1], n_valid)
    assert np.array_equal(m[:, :, 0], rows[:, :, 0], equal_nan=True)       # the own column stays
    # three columns fewer where all are finite; recording 10 loses only column 11 this way (1, 2, 3 are NaN, 8 and 9 its
    # subject's), recording 14 has no own column to except
    assert m[0, 0, 1] == rows[0, 0, 2] - 3 and m[10, 0, 1] == rows[10, 0, 2] - 3 and m[14, 0, 1] == rows[14, 0, 2] - 3
    assert m[21, 0, 1] == rows[21, 0, 2] - 2                               # (column 20, its subject's, was NaN already)
    # exactly the rows with a same-subject column below or at the own value change their counts
    for r in range(N):
        for b in range(NB):
            mates = [c for c in range(N) if SUBJECTS[c] == SUBJECTS[r] and c != r and np.isfinite(dist[r, b, c])]
            w = dist[r, b, r]
            less = sum(dist[r, b, c] < w for c in mates) if np.isfinite(w) else 0
            equal = sum(dist[r, b, c] == w for c in mates) if np.isfinite(w) else 0
            assert m[r, b, 2] == rows[r, b, 3] - less and m[r, b, 3] == rows[r, b, 4] - equal
    res = drivers.match_mismatch_summary(rows, dist, SUBJECTS, None, BANDS, exclude_same_subject=True)
    plain = drivers.match_mismatch_summary(rows, dist, SUBJECTS, None, BANDS)
    for b, band in enumerate(BANDS):
        sel = ~np.isnan(rank[:, b]) & (n_valid[:, b] > 0)
        assert res[band]["top1"] == np.mean(rank[sel, b] == 1) and res[band]["top1"] >= plain[band]["top1"]
        assert res[band]["null_mean"] == pytest.approx(m[sel, b, 4].mean(), rel=1e-14)
    # with a candidate list: the columns' subjects are the candidates'
    cand = [5, 4, 20, 7, 0, 1, 2, 3, 6]
    sub = dist[:, :, cand]
    own2 = np.full(N, -1)
    own2[cand] = np.arange(len(cand))
    m2 = drivers.match_rows_host(sub, own2)
    rows2 = np.zeros((N, NB, 6))
    rows2[:, :, 0], rows2[:, :, 2:] = m2[:, :, 0], m2[:, :, 1:]
    ex = drivers.match_mismatch_summary(rows2, sub, SUBJECTS, None, BANDS, candidates=cand, exclude_same_subject=True)
    keep2 = subj[:, None] != subj[cand][None, :]
    m3 = drivers.match_rows_host(sub, own2, keep=keep2)
    assert m3[5, 0, 1] == 4 and m3[0, 0, 1] == 4 and m3[30, 0, 1] == 8    # bb01: 5, 4, 7, 6 / bb00: 0..3 / others: all but 20
    for b, band in enumerate(BANDS):
        sel = np.isfinite(m3[:, b, 0]) & (m3[:, b, 1] > 0)
        assert ex[band]["n"] == sel.sum() == 8 and ex[band]["null_mean"] == pytest.approx(m3[sel, b, 4].mean(), rel=1e-14)
