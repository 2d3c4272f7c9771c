"""
Host tests of the comparison drivers (no GPU): drivers.comparison_summary (cmp:161-220) against the reference's own recorded
results -- its detailed table in, its band_results out (tests/golden/reference_comparison.*, made by
make_comparison_fixture.py) -- and drivers.comparison_rows (cmp:145-157) on crafted pass outputs.
Two keys of the recorded JSON are not what the script as it stands computes (the program text is the contract there):
wass_h1_cohens_d was recorded with the population standard deviation (cmp:196 says ddof=1), and wass_h1_perm_p reproduces
for delta and theta only.
"""
import io
import json
import os

import numpy as np
import pytest

from tda_eeg_audio_amd import drivers

HERE = os.path.dirname(os.path.abspath(__file__))
BANDS = ["delta", "theta", "alpha", "beta", "gamma"]
REL_KEYS = ["wass_h0_slow", "wass_h0_fast", "wass_h0_p", "wass_h1_slow", "wass_h1_fast", "wass_h1_p", "corr_slow", "corr_fast",
            "corr_p", "wass_h1_p_fdr"]
EQ_KEYS = ["n_slow_lower", "wass_h1_direction", "wass_h1_sig_fdr", "n_subjects", "band"]


@pytest.fixture(scope="module")
def recorded():
    g = np.load(os.path.join(HERE, "golden", "reference_comparison.npz"))
    cols = [str(c) for c in g["value_columns"]]
    fn, cond, band = (g[k + "_names"][g[k + "_idx"]] for k in ("filename", "condition", "band"))
    table = []
    for i in range(len(fn)):
        row = {"filename": str(fn[i]), "condition": str(cond[i]), "subject": str(fn[i]).split("_")[0], "band": str(band[i])}
        row.update(zip(cols, (float(v) for v in g["values"][i])))
        table.append(row)
    with open(os.path.join(HERE, "golden", "reference_comparison.json")) as f:
        return table, json.load(f)


@pytest.fixture(scope="module")
def summary(recorded):
    return drivers.comparison_summary(recorded[0])


def _subject_differences(table, band):
    """slow - fast of the subjects' mean W_H1 (cmp:165-181), written out again for the permutation loop below."""
    cells = {}
    for r in table:
        if r["band"] == band:
            cells.setdefault((r["subject"], r["condition"]), []).append(r["wasserstein_h1"])
    subj = sorted({s for s, c in cells if c == "slow"} & {s for s, c in cells if c == "fast"})
    return np.array([np.mean(cells[s, "slow"]) - np.mean(cells[s, "fast"]) for s in subj])


def test_summary_reproduces_the_recorded_band_results(recorded, summary):
    table, ref = recorded
    assert len(table) == 7080 and list(summary) == BANDS == list(ref)
    for band in BANDS:
        got, exp = summary[band], ref[band]
        assert list(got) == list(exp), band                              # the keys of the recorded JSON, in its order
        assert got["n_subjects"] == 45
        for k in REL_KEYS:
            rel = abs(got[k] - exp[k]) / abs(exp[k])
            print(band, k, got[k], exp[k], rel)
            assert rel < 1e-12, (band, k, got[k], exp[k])
        for k in EQ_KEYS:
            assert got[k] == exp[k] and type(got[k]) is type(exp[k]), (band, k)


def test_cohens_d_uses_the_sample_standard_deviation(recorded, summary):
    _, ref = recorded
    for band in BANDS:
        exp = ref[band]["wass_h1_cohens_d"] * np.sqrt(44 / 45)             # recorded with ddof=0; cmp:196 says ddof=1
        rel = abs(summary[band]["wass_h1_cohens_d"] - exp) / abs(exp)
        print(band, summary[band]["wass_h1_cohens_d"], exp, rel)
        assert rel < 1e-9, band


def test_permutation_p_follows_the_definition(recorded, summary):
    table, ref = recorded
    for band in BANDS:
        d1 = _subject_differences(table, band)
        assert len(d1) == 45
        rng = np.random.default_rng(42)                                    # anew per band
        exceed = 0
        for _ in range(1000):
            flips = rng.choice([-1, 1], len(d1))
            if abs(np.mean(d1 * flips)) >= abs(np.mean(d1)):
                exceed += 1
        assert summary[band]["wass_h1_perm_p"] == (exceed + 1) / 1001, band
    assert summary["delta"]["wass_h1_perm_p"] == ref["delta"]["wass_h1_perm_p"] == 1 / 1001
    assert summary["theta"]["wass_h1_perm_p"] == ref["theta"]["wass_h1_perm_p"] == 2 / 1001
    # fewer draws: the argument is used
    assert drivers.comparison_summary(table, n_permutations=9)["delta"]["wass_h1_perm_p"] in [k / 10 for k in range(1, 11)]


def _row(subject, condition, band, w0, w1, c, rec=1):
    return {"filename": f"{subject}_ut{rec:02d}.mat", "condition": condition, "subject": subject, "band": band,
            "wasserstein_h0": w0, "wasserstein_h1": w1, "corr_mean_persistence_r": c, "corr_persistence_entropy_r": 0.0}


def test_summary_edges():
    # 4 common subjects (a fifth in one condition only): the band is counted, not tested, and still gets the FDR keys
    table = [_row(f"bb{s:02d}", c, "delta", 10.0 + s + (c == "fast"), 1.0 + 0.1 * s + 0.05 * (c == "fast"), 0.1 * s)
             for s in range(4) for c in ("slow", "fast")] + [_row("bb09", "slow", "delta", 1.0, 1.0, 0.0)]
    out = drivers.comparison_summary(table, bands=["delta"])
    assert out == {"delta": {"n_subjects": 4, "band": "delta", "wass_h1_p_fdr": 1.0, "wass_h1_sig_fdr": False}}
    # 6 common subjects, all differences zero: every Wilcoxon p is 1.0 (cmp:184-186); bb09 (slow only) is left out
    table = [_row(f"bb{s:02d}", c, "theta", 10.0 + s, 1.0 + s, 0.5) for s in range(6) for c in ("slow", "fast")] + \
        [_row("bb09", "slow", "theta", 99.0, 99.0, 0.9)]
    th = drivers.comparison_summary(table, bands=["delta", "theta"])
    assert th["delta"] == {"n_subjects": 0, "band": "delta", "wass_h1_p_fdr": 1.0, "wass_h1_sig_fdr": False}
    t = th["theta"]
    assert t["n_subjects"] == 6 and t["wass_h0_p"] == t["wass_h1_p"] == t["corr_p"] == 1.0 and t["wass_h1_p_fdr"] == 1.0
    assert t["wass_h1_perm_p"] == 1.0 and t["n_slow_lower"] == 0 and t["wass_h1_direction"] == "slow > fast"
    assert t["wass_h0_slow"] == t["wass_h0_fast"] == 12.5 and t["corr_slow"] == 0.5          # bb09's 99.0 is not in the means
    # several recordings of a subject are averaged first (cmp:165-169): 7 subjects, slow = mean(1, 3) = 2 < fast = 2.5
    table = []
    for s in range(7):
        table += [_row(f"bb{s:02d}", "slow", "alpha", 5.0, 1.0 + s, 0.0, 1), _row(f"bb{s:02d}", "slow", "alpha", 7.0, 3.0 + s, 0.2, 2),
                  _row(f"bb{s:02d}", "fast", "alpha", 6.5, 2.5 + s + 0.01 * s, 0.3, 1)]
    a = drivers.comparison_summary(table, bands=["alpha"])["alpha"]
    assert a["n_subjects"] == 7 and a["wass_h0_slow"] == 6.0 and a["wass_h0_fast"] == 6.5 and a["n_slow_lower"] == 7
    assert a["wass_h1_direction"] == "slow < fast" and a["corr_slow"] == pytest.approx(0.1) and a["wass_h1_p"] == 2 / 2 ** 7
    # a DataFrame with the columns is taken as well
    import pandas as pd
    assert drivers.comparison_summary(pd.DataFrame(table), bands=["alpha"])["alpha"] == a


def test_comparison_rows_and_csv_round_trip():
    import pandas as pd
    n_rec, nb = 4, 5
    rng = np.random.default_rng(3)
    rows = rng.random((n_rec, nb, 48)) + 1.0
    rows[:, :, 2] = rng.integers(1, 100, (n_rec, nb))                      # tau
    rows[:, :, 3] = 15                                                      # n_windows
    corr = rng.uniform(-1, 1, (n_rec, nb, 10))
    rows[1] = np.nan; rows[1, :, 3] = 0; corr[1] = np.nan                   # a recording without a window
    rows[2, 3, :2] = np.nan; corr[2, 3] = np.nan                            # a band none of whose windows reached the distances
    corr[3, 0] = [0.0, 1.0] * 5                                             # guarded cells are results, not gaps
    names = ["bb01_ut01.mat", "bb01_ut02.mat", "bb17_ut09.mat", "bb17x_a_b.mat"]
    conds = ["slow", "slow", "fast", "fast"]
    table = drivers.comparison_rows(rows, corr, names, conds)
    assert len(table) == 3 * 5 - 1
    assert all(list(t) == drivers.DETAILED_COLUMNS for t in table)
    assert [(t["filename"], t["band"]) for t in table] == \
        [(names[r], b) for r in (0, 2, 3) for b in BANDS if not (r == 2 and b == "beta")]
    assert [t["subject"] for t in table[::5]] == ["bb01", "bb17", "bb17x"] and table[-1]["condition"] == "fast"
    t = table[1]                                                            # recording 0, theta
    assert t["wasserstein_h0"] == rows[0, 1, 0] and t["wasserstein_h1"] == rows[0, 1, 1]
    assert t["tau"] == int(rows[0, 1, 2]) and type(t["tau"]) is int and t["n_windows"] == 15 and type(t["n_windows"]) is int
    assert [t[c] for c in drivers.DETAILED_COLUMNS[8:]] == corr[0, 1].tolist()
    assert t["corr_mean_persistence_r"] == corr[0, 1, 0] and t["corr_n_features_p"] == corr[0, 1, 9]
    # the reference's file: header line and values back
    text = pd.DataFrame(table, columns=drivers.DETAILED_COLUMNS).to_csv(index=False)
    header = ("filename,condition,subject,band,wasserstein_h0,wasserstein_h1,n_windows,tau,corr_mean_persistence_r,"
              "corr_mean_persistence_p,corr_total_persistence_r,corr_total_persistence_p,corr_persistence_entropy_r,"
              "corr_persistence_entropy_p,corr_max_persistence_r,corr_max_persistence_p,corr_n_features_r,corr_n_features_p")
    assert text.splitlines()[0] == header and len(text.splitlines()) == 1 + len(table)
    back = pd.read_csv(io.StringIO(text), float_precision="round_trip")
    assert back.to_dict("records") == table
    assert drivers.comparison_summary(back)["delta"]["n_subjects"] == 0     # (bb01 is slow only, bb17 fast only)
    with pytest.raises(AssertionError):
        drivers.comparison_rows(rows, corr[:, :, :8], names, conds)
