#!/usr/bin/env python3
"""
tools/sliced_matrix_bench.py -- the sliced Wasserstein matrix by the prepared route (csrc/sliced_matrix.hip) on the inputs
of tools/match_mismatch_bench.py: the corpus' 1,416 real lengths, synthetic samples, M = 16 directions.
    python3 tools/sliced_matrix_bench.py [--legs 1,2,3] [--runs 5] [--out profiles/sliced_matrix_bench.json]
Every figure is the median of --runs with every run listed; the routes of a leg alternate run by run in one process on the
same resident diagrams.  A leg can be run alone (under a time limit of its own); its keys are merged into the JSON file.
  leg 1  the 64-column matrix stage of one shard, three routes: engine.wasserstein_matrix_dev (the exact distance);
         the prepared route -- sliced_prepare_dev of both sides + sliced_matrix_dev, timed together and apart; and the pair
         route, the yardstick: explicit pair lists through engine.sliced_wasserstein_dev, the values scattered to their
         positions, then the means by engine.cross_rows_dev per column.  ratio = pair route / prepared route, and `equal`
         over out / pairs / flags of the two, bit for bit.
  leg 2  the stage of one shard at the full width of 1,416 columns, prepared route only (prepare of the shard's EEG side +
         sliced_matrix_dev; the bank is prepared once per run and timed apart), and the pair route of leg 1's 64 columns
         SCALED by 1,416 / 64 (labelled as scaled: it was not run at full width).
  leg 3  MatchMismatchPass.run with and without sliced=, alternating.
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

N_SUB, N_DIRS = 64, 16


def once(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, r


def note(*a):
    print(*a, file=sys.stderr, flush=True)


def med(ts):
    return {"ms": float(np.median(ts)), "runs": [round(t, 3) for t in ts]}


def resident_shard(mp):
    i = max(j for j in range(len(mp.shards)) if j % mp.n_sets == 0)
    st = mp.set[0]
    return i, st, mp.shards[i], st["views"][i]


def sliced_stage(mp, st, d, v, what="all"):
    """The prepared route of a shard as the pass runs it: prepare of the EEG side, (prepare of the bank,) the matrix."""
    import torch
    from tda_eeg_audio_amd import engine
    n = v.n_seg * mp.n_col
    mat, pairs, flags = (st[k].view(-1)[:n].view(v.n_seg, mp.n_col) for k in ("slc_mat", "slc_mat_pairs", "slc_mat_flags"))
    with torch.cuda.stream(st["main"]):
        if what in ("all", "prepare", "eeg+matrix"):
            n_e = v.eeg.h1.shape[0]
            slot = engine.sliced_slots_dev(v.eeg.c1[:n_e], v.eeg.h1.shape[1], out=st["slc_slot"][:n_e + 1])
            st["ta"] = engine.sliced_prepare_dev(v.eeg.h1, v.eeg.c1, mp.slc_dirs_t, table_t=st["slc_table"], slot_off=slot,
                                                 m_t=st["slc_m"], ctx=mp.ctx)
        if what in ("all", "prepare"):
            engine.sliced_prepare_dev(mp.bank.h1, mp.bank.c1, mp.slc_dirs_t, table_t=mp.slc_bank.table, slot_off=mp.slc_bank.slot_off,
                                      m_t=mp.slc_bank.m, ctx=mp.ctx)
        if what in ("all", "matrix", "eeg+matrix"):
            engine.sliced_matrix_dev(st["ta"], v.seg_off, d["cls_e"], mp.slc_bank, mp.col_seg_off, mp.bank.status, mp.n_col,
                                     out_t=mat, pairs_t=pairs, flags_t=flags, ctx=mp.ctx)
    return mat, pairs, flags


def exact_stage(mp, st, d, v):
    import torch
    from tda_eeg_audio_amd import engine
    n = v.n_seg * mp.n_col
    mat, pairs, flags = (st[k].view(-1)[:n].view(v.n_seg, mp.n_col) for k in ("mat", "mat_pairs", "mat_flags"))
    with torch.cuda.stream(st["main"]):
        engine.wasserstein_matrix_dev(v.eeg.h1, v.eeg.c1, v.seg_off, d["cls_e"], mp.bank.h1, mp.bank.c1, mp.col_seg_off,
                                      mp.bank.status, mp.n_col, out_t=mat, pairs_t=pairs, flags_t=flags, ctx=mp.ctx)


def leg1(a, ctx, dev, L, raw_h, env_h, dirs, kw):
    import torch
    from tda_eeg_audio_amd import _lib, engine, recordings
    cand = np.linspace(0, len(L) - 1, N_SUB).astype(np.int64)
    sp = recordings.MatchMismatchPass(L, None, cand, dev, ctx=ctx, sliced=dirs, **kw)
    sp.run(raw_h, env_h)
    i, st, d, v = resident_shard(sp)
    n_e, n_seg = d["n_win"], v.n_seg
    # the pairs the rules name, per column: A diagram w at position p of group g against B diagram seg_off_col[k * 64 + c] + p
    seg_a, cls = v.seg_off.cpu().numpy(), d["cls_e"].cpu().numpy()
    seg_b, stb = sp.col_seg_off.cpu().numpy(), sp.bank.status.cpu().numpy()
    grp = np.repeat(np.arange(n_seg), np.diff(seg_a))
    pos = np.arange(n_e) - seg_a[grp]
    ia, ib, flat = [], [], []
    for c in range(N_SUB):
        p = cls[grp] * N_SUB + c
        has = pos < (seg_b[p + 1] - seg_b[p])
        b = seg_b[p] + pos
        has &= (stb[np.where(has, b, 0)] & _lib.TDA_WIN_DEGENERATE) == 0
        w = np.flatnonzero(has)
        ia.append(w); ib.append(b[w]); flat.append(c * n_e + w)
    up = lambda x, dt: torch.from_numpy(np.ascontiguousarray(np.concatenate(x))).to(device=dev, dtype=dt)      # noqa: E731
    ia, ib, flat = up(ia, torch.int32), up(ib, torch.int32), up(flat, torch.int64)
    n_pairs = ia.numel()
    o, s = torch.empty(n_pairs, dtype=torch.float64, device=dev), torch.empty(n_pairs, dtype=torch.int32, device=dev)
    W = torch.empty((N_SUB, n_e), dtype=torch.float64, device=dev)
    S = torch.empty((N_SUB, n_e), dtype=torch.int32, device=dev)
    crow = torch.empty((N_SUB, n_seg, 4), dtype=torch.float64, device=dev)
    cflag = torch.empty((N_SUB, n_seg), dtype=torch.int32, device=dev)

    def pair_route():
        with torch.cuda.stream(st["main"]):
            W.fill_(float("nan")); S.fill_(_lib.TDA_WIN_NO_PAIR)
            engine.sliced_wasserstein_dev(v.eeg.h1, v.eeg.c1, sp.bank.h1, sp.bank.c1, sp.slc_dirs_t, ia, ib, out_t=o, status_t=s, ctx=ctx)
            W.view(-1).index_copy_(0, flat, o); S.view(-1).index_copy_(0, flat, s)
            for c in range(N_SUB):
                engine.cross_rows_dev(W[c], S[c], W[c], S[c], v.seg_off, out_t=crow[c], seg_flags=cflag[c], ctx=ctx)

    exact_stage(sp, st, d, v), sliced_stage(sp, st, d, v), pair_route()          # untimed
    t = {k: [] for k in ("exact", "new", "prepare", "matrix", "pairs")}
    for _ in range(a.runs):                                                       # alternating, same process, same diagrams
        t["exact"].append(once(lambda: exact_stage(sp, st, d, v))[0])
        t["new"].append(once(lambda: sliced_stage(sp, st, d, v))[0])
        t["prepare"].append(once(lambda: sliced_stage(sp, st, d, v, "prepare"))[0])
        t["matrix"].append(once(lambda: sliced_stage(sp, st, d, v, "matrix"))[0])
        t["pairs"].append(once(pair_route)[0])
        note("leg 1: " + ", ".join(f"{k} {x[-1]:.2f} ms" for k, x in t.items()))
    mat, pairs, flags = (x.cpu().numpy() for x in sliced_stage(sp, st, d, v))
    torch.cuda.synchronize()
    cr, cf = crow.cpu().numpy(), cflag.cpu().numpy()
    equal = bool(np.array_equal(mat, cr[:, :, 1].T, equal_nan=True) and np.array_equal(pairs, cr[:, :, 3].T.astype(np.int32))
                 and np.array_equal(flags, cf.T))
    m = sp.slc_bank.m.cpu().numpy()
    res = {"wasserstein_matrix": med(t["exact"]), "prepared_route": med(t["new"]), "prepare_both_sides": med(t["prepare"]),
           "sliced_matrix_alone": med(t["matrix"]), "pair_route": med(t["pairs"]),
           "ratio_pair_over_prepared": float(np.median(t["pairs"]) / np.median(t["new"])),
           "ratio_prepared_over_exact": float(np.median(t["new"]) / np.median(t["exact"])), "equal": equal,
           "stage": {"shard": i, "groups": int(n_seg), "eeg_diagrams": int(n_e), "columns": N_SUB, "pairs": int(n_pairs),
                     "bank_diagrams": int(sp.n_bank_win), "entries_finite": int(np.isfinite(mat).sum()),
                     "flags_set": int((flags != 0).sum()), "mean_rows_eeg": float(st["ta"].m.float().mean().item()),
                     "mean_rows_bank": float(m.mean()), "bank_table_MB": float(sp.slc_bank.slot_off[-1].item() * 2 * N_DIRS * 8 / 1e6)}}
    return res, equal


def leg23(a, ctx, dev, L, raw_h, env_h, dirs, kw, legs, pair_ms_64):
    import torch
    from tda_eeg_audio_amd import recordings
    res = {}
    on = recordings.MatchMismatchPass(L, None, None, dev, ctx=ctx, sliced=dirs, **kw)
    t0, rows_on = once(lambda: on.run(raw_h, env_h))
    note(f"first run with sliced= {t0:.0f} ms")
    if 3 in legs:
        off = recordings.MatchMismatchPass(L, None, None, dev, ctx=ctx, **kw)
        t0, rows_off = once(lambda: off.run(raw_h, env_h))
        t_on, t_off = [], []
        for _ in range(a.runs):
            t_off.append(once(lambda: off.run(raw_h, env_h, rows_off))[0])
            t_on.append(once(lambda: on.run(raw_h, env_h, rows_on))[0])
            note(f"leg 3: off {t_off[-1]:.0f} ms, on {t_on[-1]:.0f} ms")
        sd = on.slc_dist_h.numpy()
        res["leg3"] = {"pass_off": med(t_off), "pass_on": med(t_on), "shards": len(on.plan.shards), "repairs": [off.repairs, on.repairs],
                       "rows_equal": bool(rows_on.numpy().tobytes() == rows_off.numpy().tobytes()
                                          and on.dist_h.numpy().tobytes() == off.dist_h.numpy().tobytes()),
                       "slc_dist_finite": bool(np.isfinite(sd).all()), "pairs": int(on.slc_pairs_h.numpy().sum(dtype=np.int64))}
        del off
    if 2 in legs:
        i, st, d, v = resident_shard(on)
        sliced_stage(on, st, d, v)
        t_full, t_bank = [], []
        for _ in range(a.runs):
            t_full.append(once(lambda: sliced_stage(on, st, d, v, "eeg+matrix"))[0])
            t_bank.append(once(lambda: on._phase1(env_h.view(-1)))[0])
            note(f"leg 2: stage {t_full[-1]:.1f} ms, phase 1 with the bank's prepare {t_bank[-1]:.1f} ms")
        n_pairs = int(on.slc_pairs_h.numpy()[d["r0"]:d["r1"]].sum(dtype=np.int64))
        res["leg2"] = {"prepared_route_full_width": med(t_full), "phase1_with_bank_prepare": med(t_bank),
                       "groups": int(v.n_seg), "columns": int(on.n_col), "pairs": n_pairs,
                       "ns_per_pair": float(np.median(t_full)) * 1e6 / max(n_pairs, 1),
                       "bank_table_MB": float(on.slc_bank.slot_off[-1].item() * 2 * N_DIRS * 8 / 1e6),
                       "pair_route_SCALED_ms": None if pair_ms_64 is None else pair_ms_64 * on.n_col / N_SUB,
                       "pair_route_note": "scaled from the 64 columns of leg 1 by columns / 64; not run at full width"}
    del on
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="1,2,3")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--shard-samples", type=int, default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sliced_matrix_bench.json"))
    a = ap.parse_args()
    legs = {int(x) for x in a.legs.split(",")}
    import torch
    from ragged_bench import synth
    from tda_eeg_audio_amd import _lib, utils
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    ctx = _lib.get_ctx(0)
    L = np.load(os.path.join(ROOT, "tests", "golden", "corpus_n_samples.npy"))
    kw = {} if a.shard_samples is None else {"shard_samples": a.shard_samples}
    raw_h, env_h = synth(47 * int(L.sum()), int(L.sum()), 909)
    dirs = utils.default_directions(N_DIRS)
    out = {}
    if os.path.exists(a.out):
        out = json.load(open(a.out))
    out.update({"recordings": len(L), "n_dirs": N_DIRS, "runs": a.runs})
    equal = True
    if 1 in legs:
        out["leg1"], equal = leg1(a, ctx, dev, L, raw_h, env_h, dirs, kw)
        torch.cuda.empty_cache()
    if legs & {2, 3}:
        pair_ms = out.get("leg1", {}).get("pair_route", {}).get("ms")
        out.update(leg23(a, ctx, dev, L, raw_h, env_h, dirs, kw, legs, pair_ms))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))
    if not equal:
        sys.exit("the prepared route differs from the pair route")


if __name__ == "__main__":
    main()
