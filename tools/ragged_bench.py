#!/usr/bin/env python3
"""
tools/ragged_bench.py -- the raw-recordings leg on the study's REAL length column, one JSON line:
    python3 tools/ragged_bench.py [--runs 2] [--shard-samples N] [--correlations]
1,416 recordings at the lengths of tests/golden/corpus_n_samples.npy (sum 6,007,447 samples x 47 channels, envelope
length = EEG length), synthetic samples as in bench.recordings_leg, through recordings.RaggedRecordingPass; beside it,
in the same process, the equal-length recordings.RecordingPass at 1,416 x 4,243 samples (the corpus mean) in shards of 236.
Reported: window pairs/s, ms per run, h2d GB/s, shards, and the same for the equal-length leg.
--correlations: the ragged leg once more in the same process with RaggedRecordingPass(correlations=True) (Spearman r and p
of the five H1 feature series per recording-band, cmp:104-114, beside the rows): its ms per run next to the plain one,
whether the rows are bit-identical to the plain pass', and how many correlation cells are finite.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def synth(n_ch_samples, n_env, seed):
    import torch
    g = torch.Generator(device="cpu")
    g.manual_seed(seed)
    raw = torch.randn(n_ch_samples, generator=g, dtype=torch.float64)
    env = (torch.randn(n_env, generator=g, dtype=torch.float64).abs()
           + 0.3 * torch.randn(n_env, generator=g, dtype=torch.float64).cumsum(0).abs() * 0.02)
    return raw.pin_memory(), env.pin_memory()


def timed(run, runs):
    import torch
    rows = run(None)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(runs):
        rows = run(rows)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / runs, rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--shard-samples", type=int, default=None)
    ap.add_argument("--correlations", action="store_true")
    a = ap.parse_args()
    import torch
    from tda_eeg_audio_amd import _lib, recordings
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    ctx = _lib.get_ctx(0)
    L = np.load(os.path.join(ROOT, "tests", "golden", "corpus_n_samples.npy"))
    kw = {} if a.shard_samples is None else {"shard_samples": a.shard_samples}
    rp = recordings.RaggedRecordingPass(L, None, dev, ctx=ctx, **kw)
    raw_h, env_h = synth(47 * int(L.sum()), int(L.sum()), 909)
    dt, rows = timed(lambda r: rp.run(raw_h, env_h, r), a.runs)
    n_pairs = int(rp.plan.k.sum()) * len(rp.bands)
    nbytes = (raw_h.numel() + env_h.numel()) * 8
    out = {"value": n_pairs / dt, "unit": "window pairs/s", "ms_per_run": dt * 1e3, "h2d_GBps": nbytes / dt / 1e9,
           "shards": len(rp.plan.shards), "recordings": len(L), "samples": int(L.sum()), "window_pairs": n_pairs,
           "rows_finite": bool(torch.isfinite(rows).all().item()), "repairs": rp.repairs}
    if a.correlations:
        rows_plain = rows.clone()
        cp = recordings.RaggedRecordingPass(L, None, dev, ctx=ctx, correlations=True, **kw)
        # on the plain pass' streams: which hardware queue a stream lands on depends on how many were made before it, and
        # that alone moves this leg by 2.6 ms (the second of two identical passes built in one process: 59.6 against 57.0)
        cp.copy, cp.back = rp.copy, rp.back
        for sc, sp in zip(cp.set, rp.set):
            sc["main"], sc["side"] = sp["main"], sp["side"]
        dtc, rows_c = timed(lambda r: cp.run(raw_h, env_h, r), a.runs)
        out["correlations"] = {"value": n_pairs / dtc, "ms_per_run": dtc * 1e3, "ms_over_plain": (dtc - dt) * 1e3,
                               "rows_identical": bool(np.array_equal(rows_c.numpy(), rows_plain.numpy(), equal_nan=True)),
                               "cells_finite": int(torch.isfinite(cp.corr_h).sum().item()), "cells": cp.corr_h.numel(),
                               "d2h_bytes": cp.corr_h.numel() * 8, "repairs": cp.repairs}
        del cp, rows_plain, rows_c
    del rp, raw_h, env_h
    # the equal-length leg at the corpus mean, same process
    n_eq, S = int(round(L.mean())), 236
    eq = recordings.RecordingPass(n_eq, S, dev, ctx=ctx)
    raw_e, env_e = synth(len(L) * 47 * n_eq, len(L) * n_eq, 909)
    raw_e, env_e = raw_e.view(len(L), 47, n_eq), env_e.view(len(L), n_eq)
    dte, _ = timed(lambda r: eq.run(raw_e, env_e, r), a.runs)
    pe = len(L) * len(eq.bands) * eq.k
    be = (raw_e.numel() + env_e.numel()) * 8
    out["equal_length"] = {"value": pe / dte, "ms_per_run": dte * 1e3, "h2d_GBps": be / dte / 1e9, "n_samples": n_eq,
                           "shards": -(-len(L) // S), "window_pairs": pe}
    out["ratio_pairs_per_s"] = out["value"] / out["equal_length"]["value"]
    print(json.dumps(out))
    if a.correlations and not out["correlations"]["rows_identical"]:
        sys.exit("rows of the pass with correlations differ from the plain pass' rows")


if __name__ == "__main__":
    main()
