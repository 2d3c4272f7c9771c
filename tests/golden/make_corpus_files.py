#!/usr/bin/env python3
"""
tests/golden/make_corpus_files.py -- the file name and the condition of every recording of the study, in the order of the
reference's results/preprocessing_metadata.csv (columns filename, condition): 1,416 recordings; row r goes with
corpus_n_samples.npy[r].  The same file name occurs in both conditions, so a recording is (condition, filename).
Names and labels only: the committed fixture (corpus_files.csv) is what the control plan test and
tools/control_bench.py make the partner table from (recordings.mismatch_partners); nothing else of the reference is
stored.
Run once where the reference tree is available (TDA_REFERENCE, default /root/reference).
"""
import csv
import os

REF = os.environ.get("TDA_REFERENCE", "/root/reference")
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "corpus_files.csv")


def main():
    with open(os.path.join(REF, "results", "preprocessing_metadata.csv"), newline="", encoding="utf-8") as f:
        rows = [(r["filename"], r["condition"]) for r in csv.DictReader(f)]
    with open(OUT, "w", newline="", encoding="utf-8") as f:
        w = csv.writer(f, lineterminator="\n")
        w.writerow(["filename", "condition"])
        w.writerows(rows)
    print(f"{OUT}: {len(rows)} recordings, {len(set(rows))} distinct (filename, condition), "
          f"conditions {sorted({c for _, c in rows})}")


if __name__ == "__main__":
    main()
