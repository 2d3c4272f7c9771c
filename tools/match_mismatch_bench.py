#!/usr/bin/env python3
"""
tools/match_mismatch_bench.py -- the match-mismatch matrix (recordings.MatchMismatchPass) on the study's REAL lengths, one
JSON line:
    python3 tools/match_mismatch_bench.py [--runs 3] [--stage-runs 5] [--shard-samples N] [--skip-pass]
1,416 recordings at the lengths of tests/golden/corpus_n_samples.npy (envelope length = EEG length), all of them
candidates, synthetic samples as in tools/ragged_bench.py.
(a) MatchMismatchPass.run: ms per run (median, and every run), the time of phase 1 alone (the candidates' bank), diagram
    pairs/s over the whole matrix.  --skip-pass leaves (a) out (a profiler run of the matrix stage alone).
(b) The matrix stage alone, on resident diagrams: the EEG diagrams of one shard against the bank of a FIXED subset of 64
    candidates.  In the same process, alternating run by run: one engine.wasserstein_matrix_dev launch, and the route
    the engine had before it -- per column a partner table (uploaded beforehand), engine.wasserstein_cross_dev and
    engine.cross_rows_dev.  ms of both (median, and every run), their ratio, and whether the 64 columns are equal bit for
    bit (out, pairs, flags).  With (a), also the matrix stage of the same shard at the full width of 1,416 columns.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

N_SUB = 64


def once(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, r


def note(*a):
    print(*a, file=sys.stderr, flush=True)


def resident_shard(mp):
    """The shard whose EEG diagrams the first buffer set still holds after a run, its set, tables and Workspace view."""
    i = max(j for j in range(len(mp.shards)) if j % mp.n_sets == 0)
    st = mp.set[0]
    return i, st, mp.shards[i], st["views"][i]


def matrix_stage(mp, st, d, v):
    import torch
    from tda_eeg_audio_amd import engine
    n = v.n_seg * mp.n_col
    mat, pairs, flags = (st[k].view(-1)[:n].view(v.n_seg, mp.n_col) for k in ("mat", "mat_pairs", "mat_flags"))
    with torch.cuda.stream(st["main"]):
        engine.wasserstein_matrix_dev(v.eeg.h1, v.eeg.c1, v.seg_off, d["cls_e"], mp.bank.h1, mp.bank.c1, mp.col_seg_off,
                                      mp.bank.status, mp.n_col, out_t=mat, pairs_t=pairs, flags_t=flags, ctx=mp.ctx)
    return mat, pairs, flags


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--stage-runs", type=int, default=5)
    ap.add_argument("--shard-samples", type=int, default=None)
    ap.add_argument("--skip-pass", action="store_true")
    a = ap.parse_args()
    import torch
    from ragged_bench import synth
    from tda_eeg_audio_amd import _lib, engine, recordings
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    ctx = _lib.get_ctx(0)
    L = np.load(os.path.join(ROOT, "tests", "golden", "corpus_n_samples.npy"))
    kw = {} if a.shard_samples is None else {"shard_samples": a.shard_samples}
    raw_h, env_h = synth(47 * int(L.sum()), int(L.sum()), 909)
    out = {"unit": "diagram pairs/s", "recordings": len(L)}

    if not a.skip_pass:
        mp = recordings.MatchMismatchPass(L, None, None, dev, ctx=ctx, **kw)
        t0, rows = once(lambda: mp.run(raw_h, env_h))                    # untimed: lazy initialisations
        note(f"first run {t0:.0f} ms")
        t_p, t_1 = [], []
        for _ in range(a.runs):
            t_p.append(once(lambda: mp.run(raw_h, env_h, rows))[0])
            t_1.append(once(lambda: mp._phase1(env_h.view(-1)))[0])
            note(f"run {t_p[-1]:.0f} ms, phase 1 {t_1[-1]:.0f} ms")
        i, st, d, v = resident_shard(mp)
        t_full = [once(lambda: matrix_stage(mp, st, d, v))[0] for _ in range(a.stage_runs)]
        n_pairs = int(mp.pairs_h.numpy().sum(dtype=np.int64))
        ms = float(np.median(t_p))
        out.update({"value": n_pairs / (ms * 1e-3), "pass_ms": ms, "pass_ms_runs": [round(t, 1) for t in t_p],
                    "phase1_ms": float(np.median(t_1)), "phase1_ms_runs": [round(t, 1) for t in t_1], "pairs": n_pairs,
                    "columns": int(mp.n_col), "bank_diagrams": int(mp.n_bank_win), "shards": len(mp.plan.shards),
                    "repairs": mp.repairs, "dist_finite": bool(np.isfinite(mp.dist_h.numpy()).all()),
                    "matrix_full_ms": float(np.median(t_full)), "matrix_full_ms_runs": [round(t, 1) for t in t_full],
                    "matrix_full_shard": {"groups": int(v.n_seg), "columns": int(mp.n_col),
                                          "pairs": int(mp.pairs_h.numpy()[d["r0"]:d["r1"]].sum(dtype=np.int64))}})
        del mp, st, d, v
        torch.cuda.empty_cache()

    # (b) 64 fixed columns: the new entry point against the column-by-column route
    cand = np.linspace(0, len(L) - 1, N_SUB).astype(np.int64)
    sp = recordings.MatchMismatchPass(L, None, cand, dev, ctx=ctx, **kw)
    sp.run(raw_h, env_h)
    i, st, d, v = resident_shard(sp)
    n_e = d["n_win"]
    w, ws_ = torch.empty(n_e, dtype=torch.float64, device=dev), torch.empty(n_e, dtype=torch.int32, device=dev)
    crow = torch.empty((N_SUB, v.n_seg, 4), dtype=torch.float64, device=dev)
    cflag = torch.empty((N_SUB, v.n_seg), dtype=torch.int32, device=dev)
    partner = [(d["cls_e"] * N_SUB + c).to(torch.int32).contiguous() for c in range(N_SUB)]
    grp = engine.group_table(v.seg_off, n_e)

    def columns():
        with torch.cuda.stream(st["main"]):
            for c in range(N_SUB):
                engine.wasserstein_cross_dev(v.eeg.h1, v.eeg.c1, v.seg_off, sp.bank.h1, sp.bank.c1, sp.col_seg_off, sp.bank.status,
                                             partner[c], grp_a=grp, out_t=w, status_t=ws_, ctx=ctx)
                engine.cross_rows_dev(w, ws_, w, ws_, v.seg_off, out_t=crow[c], seg_flags=cflag[c], ctx=ctx)

    matrix_stage(sp, st, d, v), columns()                               # untimed
    t_new, t_old = [], []
    for _ in range(a.stage_runs):                                       # alternating, same process, same diagrams
        t_new.append(once(lambda: matrix_stage(sp, st, d, v))[0])
        t_old.append(once(columns)[0])
        note(f"matrix {t_new[-1]:.2f} ms, columns {t_old[-1]:.2f} ms")
    mat, pairs, flags = (t.cpu().numpy() for t in matrix_stage(sp, st, d, v))
    torch.cuda.synchronize()
    cr, cf = crow.cpu().numpy(), cflag.cpu().numpy()
    equal = bool(np.array_equal(mat, cr[:, :, 1].T, equal_nan=True) and np.array_equal(pairs, cr[:, :, 3].T.astype(np.int32))
                 and np.array_equal(flags, cf.T))
    m_new, m_old = float(np.median(t_new)), float(np.median(t_old))
    out.update({"matrix_ms": m_new, "columns_ms": m_old, "ratio": m_old / m_new, "equal": equal,
                "matrix_ms_runs": [round(t, 3) for t in t_new], "columns_ms_runs": [round(t, 3) for t in t_old],
                "stage": {"shard": i, "groups": int(v.n_seg), "eeg_diagrams": int(n_e), "columns": N_SUB,
                          "bank_diagrams": int(sp.n_bank_win), "pairs": int(pairs.sum(dtype=np.int64)),
                          "entries_finite": int(np.isfinite(mat).sum())}})
    print(json.dumps(out))
    if not equal:
        sys.exit("the matrix differs from the column-by-column route")


if __name__ == "__main__":
    main()
