#!/usr/bin/env python3
"""The Frechet mean stage beside the Wasserstein and order-2 Wasserstein stages of the same step, on the same diagrams.

The benchmark's corpus mix (1,416 recordings x 15 windows x 5 bands = 106,200 windows in 7,080 groups, all bands as ONE
batch) runs through pipeline.run_step on a Workspace(wasserstein_q=(2, "l2"), frechet=(cap, max_iter)), launched eagerly
with HIP events around the stages.  Then each of the three diagram sets (EEG H0, EEG H1, audio H1) is launched on its own
through engine.frechet_mean_dev and timed, and its iteration histogram, largest mean and status counts are read back.
The yardstick of a set is (sum over the groups of iterations x kept diagrams) x (the order-2 pair time of
profiles/wasserstein_q_bench.json, h0 or h1 leg): what the same number of matchings costs as independent pairs.

    python tools/frechet_bench.py [--recordings 1416] [--steps 5] [--warmup 1] [--cap 256] [--max-iter 32]
                                  [--out profiles/frechet_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

STAGES = ["wasserstein_h0", "wasserstein_h1", "wasserstein_q_h0", "wasserstein_q_h1", "frechet"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--recordings", type=int, default=1416)
    ap.add_argument("--windows-per-recording", type=int, default=15)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--cap", type=int, default=256)
    ap.add_argument("--max-iter", type=int, default=32)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frechet_bench.json"))
    args = ap.parse_args()

    import torch
    from tda_eeg_audio_amd import _lib, engine, pipeline, synth
    if not torch.cuda.is_available():
        print("frechet_bench.py needs an MI355X: the HIP path has no CPU fallback", file=sys.stderr)
        return 2
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    ctx = _lib.get_ctx(0)
    n_rec, wpr, bands = args.recordings, args.windows_per_recording, synth.BANDS
    nb = len(bands)
    eeg = torch.cat(synth.corpus_eeg_dev(np.arange(n_rec), wpr, nb, dev, seed=42))
    aud_all = synth.corpus_audio(n_rec, wpr, bands, seed=4242)
    aud = torch.cat([torch.from_numpy(np.ascontiguousarray(aud_all[b].reshape(-1, 250))).to(dev) for b in bands])
    n_win = nb * n_rec * wpr
    seg_off = np.arange(0, n_win + 1, wpr, dtype=np.int32)
    ws = pipeline.Workspace(n_win, seg_off, dev, wasserstein_q=(2, "l2"), frechet=(args.cap, args.max_iter))
    for _ in range(max(1, args.warmup)):
        pipeline.run_step(eeg, aud, ws, ctx=ctx)
    torch.cuda.synchronize()
    log = []
    for _ in range(args.steps):
        timers = {s: (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for s in STAGES}
        pipeline.run_step(eeg, aud, ws, ctx=ctx, timers=timers)
        torch.cuda.synchronize()
        log.append({s: timers[s][0].elapsed_time(timers[s][1]) for s in STAGES})
    ms = {s: float(np.median([t[s] for t in log])) for s in STAGES}

    # the W2 pair times of the committed profile, for the yardstick
    pair_ms = {}
    ref = os.path.join(ROOT, "profiles", "wasserstein_q_bench.json")
    if os.path.exists(ref):
        with open(ref) as f:
            doc = json.load(f)
        v = doc["variants"]["2,l2"]["stage_ms_median"]
        pair_ms = {"h0": v["wasserstein_q_h0"] / doc["pairs_per_leg"], "h1": v["wasserstein_q_h1"] / doc["pairs_per_leg"]}

    skip = _lib.TDA_WIN_DEGENERATE | _lib.TDA_WIN_TOO_LARGE
    sets = {"eeg_h0": (ws.eeg.h0, ws.eeg.c0, None, 0, "h0"), "eeg_h1": (ws.eeg.h1, ws.eeg.c1, None, 0, "h1"),
            "aud_h1": (ws.aud.h1, ws.aud.c1, ws.aud.status, skip, "h1")}
    per_set = {}
    for name, (rows, cnt, status, mask, leg) in sets.items():
        times = []
        for _ in range(args.steps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            res = engine.frechet_mean_dev(rows, cnt, seg_off_t=ws.seg_off, status_t=status, skip_mask=mask,
                                          max_iter=args.max_iter, out=ws.fm_out, ctx=ctx)
            b.record()
            torch.cuda.synchronize()
            times.append(a.elapsed_time(b))
        _, mc, var, it, st = (t.cpu().numpy() for t in res)
        kept = np.full(len(mc), wpr) if status is None else np.add.reduceat(((status.cpu().numpy() & mask) == 0).astype(int), seg_off[:-1])
        matchings = int((it.astype(np.int64) * kept).sum())
        rec = {"kernel_ms_median": round(float(np.median(times)), 4), "kernel_ms_all": [round(t, 4) for t in times],
               "groups": int(len(mc)), "mean_rows_in": float(cnt.float().mean()), "matchings": matchings,
               "iters_histogram": {str(k): int(v) for k, v in zip(*np.unique(it, return_counts=True))},
               "largest_mean": int(mc.max()), "mean_rows_out": float(mc.mean()),
               "status_counts": {str(k): int(v) for k, v in zip(*np.unique(st, return_counts=True))},
               "mean_variance": float(np.nanmean(var))}
        if pair_ms:
            rec["yardstick_ms"] = round(matchings * pair_ms[leg], 4)
            rec["ratio_to_yardstick"] = round(rec["kernel_ms_median"] / rec["yardstick_ms"], 3)
        per_set[name] = rec
        print(f"{name}: {rec['kernel_ms_median']:.3f} ms, iterations {rec['iters_histogram']}, largest mean {rec['largest_mean']}")
    out = {"tool": "frechet_bench", "windows": n_win, "groups": int(len(seg_off) - 1), "steps": args.steps, "cap": args.cap,
           "max_iter": args.max_iter, "stage_ms_median": {s: round(v, 4) for s, v in ms.items()},
           "stage_ms_all": {s: [round(t[s], 4) for t in log] for s in STAGES},
           "w2_pair_ms_of_profile": pair_ms or None, "sets": per_set}
    for s in STAGES:
        print(f"{s:18s} {ms[s]:9.3f} ms   (median of {args.steps})")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
