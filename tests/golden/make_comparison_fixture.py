#!/usr/bin/env python3
"""
tests/golden/make_comparison_fixture.py -- recorded results of the reference's scripts/tda_eeg_audio_comparison.py, for the
test of drivers.comparison_summary (tests/test_comparison_summary.py):
  reference_comparison.npz   of results/eeg_audio_tda_detailed.csv (7,080 rows = 1,416 recordings x 5 bands): the labels
                             filename, condition and band (the distinct values and an index per row) and the four value
                             columns the summary reads -- wasserstein_h0, wasserstein_h1, corr_mean_persistence_r,
                             corr_persistence_entropy_r -- as float64, bit for bit what the file's text parses to
  reference_comparison.json  the `band_results` of results/eeg_audio_tda_comparison.json, as recorded
Data the reference's programs wrote, nothing of their text.  The subject of a row is filename.split("_")[0] (cmp:51) and
is not stored.
Run once where the reference tree is available (TDA_REFERENCE, default /root/reference).
"""
import csv
import json
import os

import numpy as np

REF = os.environ.get("TDA_REFERENCE", "/root/reference")
HERE = os.path.dirname(os.path.abspath(__file__))
VALUES = ["wasserstein_h0", "wasserstein_h1", "corr_mean_persistence_r", "corr_persistence_entropy_r"]


def main():
    with open(os.path.join(REF, "results", "eeg_audio_tda_detailed.csv"), newline="", encoding="utf-8") as f:
        rows = list(csv.DictReader(f))
    out = {}
    for key in ("filename", "condition", "band"):
        names = sorted({r[key] for r in rows})
        pos = {n: i for i, n in enumerate(names)}
        out[key + "_names"] = np.array(names)
        out[key + "_idx"] = np.array([pos[r[key]] for r in rows], dtype=np.int16)
    out["value_columns"] = np.array(VALUES)
    out["values"] = np.array([[float(r[c]) for c in VALUES] for r in rows], dtype=np.float64)
    np.savez_compressed(os.path.join(HERE, "reference_comparison.npz"), **out)
    with open(os.path.join(REF, "results", "eeg_audio_tda_comparison.json"), encoding="utf-8") as f:
        band_results = json.load(f)["band_results"]
    with open(os.path.join(HERE, "reference_comparison.json"), "w", encoding="utf-8") as f:
        json.dump(band_results, f, indent=1)
        f.write("\n")
    print(f"{len(rows)} rows, {len(out['filename_names'])} file names, bands {list(band_results)}")


if __name__ == "__main__":
    main()
