#!/usr/bin/env python3
"""
tests/golden/make_corpus_lengths.py -- the EEG length of every recording of the study, in the order of the reference's
results/preprocessing_metadata.csv (column n_samples): 1,416 recordings, 46 distinct lengths from 2,663 to 5,741
samples.  Data only: the committed fixture (corpus_n_samples.npy, int64) is what the ragged plan test and
tools/ragged_bench.py read; nothing else of the reference is stored.
Run once where the reference tree is available (TDA_REFERENCE, default /root/reference).
"""
import csv
import os

import numpy as np

REF = os.environ.get("TDA_REFERENCE", "/root/reference")
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "corpus_n_samples.npy")


def main():
    with open(os.path.join(REF, "results", "preprocessing_metadata.csv"), newline="", encoding="utf-8") as f:
        n = np.array([int(r["n_samples"]) for r in csv.DictReader(f)], dtype=np.int64)
    np.save(OUT, n)
    print(f"{OUT}: {len(n)} recordings, {len(np.unique(n))} distinct lengths, {n.min()}..{n.max()}, sum {n.sum()}")


if __name__ == "__main__":
    main()
