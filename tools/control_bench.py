#!/usr/bin/env python3
"""
tools/control_bench.py -- the control experiment (recordings.ControlPass) on the study's REAL lengths and partner table,
one JSON line:
    python3 tools/control_bench.py [--runs 5] [--shard-samples N]
1,416 recordings at the lengths of tests/golden/corpus_n_samples.npy (envelope length = EEG length), the partner table
of recordings.mismatch_partners on tests/golden/corpus_files.csv (90 distinct partners), synthetic samples as in
tools/ragged_bench.py.  In the same process and on the same inputs, alternating run by run: ControlPass.run and
RaggedRecordingPass.run, the comparison the control stands beside.
Reported: ms per run of both (median, and every run: the spread is the reader's to judge), their ratio, the time of
phase 1 alone (the partners' bank), pairs/s (matched + mismatched pairs), h2d GB/s.
"""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def once(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--shard-samples", type=int, default=None)
    a = ap.parse_args()
    import torch
    from ragged_bench import synth
    from tda_eeg_audio_amd import _lib, recordings
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    ctx = _lib.get_ctx(0)
    L = np.load(os.path.join(ROOT, "tests", "golden", "corpus_n_samples.npy"))
    with open(os.path.join(ROOT, "tests", "golden", "corpus_files.csv"), newline="", encoding="utf-8") as f:
        files = [(r["filename"], r["condition"]) for r in csv.DictReader(f)]
    partner = recordings.mismatch_partners([n for n, _ in files], [c for _, c in files])
    kw = {} if a.shard_samples is None else {"shard_samples": a.shard_samples}
    cp = recordings.ControlPass(L, None, partner, dev, ctx=ctx, **kw)
    rp = recordings.RaggedRecordingPass(L, None, dev, ctx=ctx, **kw)
    raw_h, env_h = synth(47 * int(L.sum()), int(L.sum()), 909)
    rows_c = cp.run(raw_h, env_h)                                        # untimed: lazy initialisations
    rows_r = rp.run(raw_h, env_h)
    t_c, t_r, t_1 = [], [], []
    for _ in range(a.runs):                                              # alternating, same process, same inputs
        t_c.append(once(lambda: cp.run(raw_h, env_h, rows_c))[0])
        t_r.append(once(lambda: rp.run(raw_h, env_h, rows_r))[0])
        t_1.append(once(lambda: cp._phase1(env_h.view(-1)))[0])
    mc, mr = float(np.median(t_c)), float(np.median(t_r))
    n_pairs = int(np.nansum(rows_c.numpy()[:, :, 2:]))
    nbytes = (raw_h.numel() + env_h.numel()) * 8
    rc = rows_c.numpy()
    same = bool(np.array_equal(rc[:, :, 0], rows_r.numpy()[:, :, 1], equal_nan=True))    # L = Le: matched == cmp's W_H1
    print(json.dumps({
        "value": n_pairs / (mc * 1e-3), "unit": "diagram pairs/s", "control_ms": mc, "ragged_ms": mr, "ratio": mc / mr,
        "control_ms_runs": [round(t, 2) for t in t_c], "ragged_ms_runs": [round(t, 2) for t in t_r],
        "phase1_ms": float(np.median(t_1)), "phase1_ms_runs": [round(t, 2) for t in t_1],
        "h2d_GBps": nbytes / (mc * 1e-3) / 1e9, "ragged_h2d_GBps": nbytes / (mr * 1e-3) / 1e9,
        "pairs": n_pairs, "bank_recordings": int(len(cp.plan.bank)), "bank_diagrams": int(cp.n_bank_win),
        "shards": len(cp.plan.shards), "recordings": len(L), "repairs": [cp.repairs, rp.repairs],
        "rows_finite": bool(np.isfinite(rc).all()), "matched_equals_ragged_w_h1": same}))


if __name__ == "__main__":
    main()
