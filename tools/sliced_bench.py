#!/usr/bin/env python3
"""The sliced Wasserstein stages beside the Wasserstein and bottleneck stages of the same step, on the same diagram pairs.

The benchmark's corpus mix (1,416 recordings x 15 windows x 5 bands = 106,200 window pairs, all bands as ONE batch) runs
through pipeline.run_step on a Workspace(bottleneck=True, sliced=dirs), launched eagerly with HIP events around the six
distance stages.  The steps alternate between the direction tables default_directions(16) and default_directions(50) in
one process, on the same resident diagrams.  Prints the median stage times of the timed steps and one JSON line, and
writes it to profiles/sliced_bench.json.

    python tools/sliced_bench.py [--recordings 1416] [--steps 5] [--warmup 1] [--out profiles/sliced_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

STAGES = ["wasserstein_h0", "wasserstein_h1", "bottleneck_h0", "bottleneck_h1", "sliced_h0", "sliced_h1"]
TABLES = (16, 50)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--recordings", type=int, default=1416)
    ap.add_argument("--windows-per-recording", type=int, default=15)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sliced_bench.json"))
    args = ap.parse_args()

    import torch
    from tda_eeg_audio_amd import _lib, pipeline, synth, utils
    if not torch.cuda.is_available():
        print("sliced_bench.py needs an MI355X: the HIP path has no CPU fallback", file=sys.stderr)
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
    ws = pipeline.Workspace(n_win, seg_off, dev, bottleneck=True, sliced=utils.default_directions(TABLES[0]))
    # one workspace, two resident direction tables: the step reads ws.sliced_dirs
    tables = {M: torch.from_numpy(utils.default_directions(M)).to(dev) for M in TABLES}

    log = {M: [] for M in TABLES}
    values = {}
    for it in range(max(1, args.warmup) + args.steps):
        for M in TABLES:
            ws.sliced_dirs = tables[M]
            timers = {s: (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for s in STAGES}
            pipeline.run_step(eeg, aud, ws, ctx=ctx, timers=timers)
            torch.cuda.synchronize()
            if it >= max(1, args.warmup):
                log[M].append({s: timers[s][0].elapsed_time(timers[s][1]) for s in STAGES})
            values[M] = (ws.s0.cpu().numpy(), ws.s1.cpu().numpy(), ws.ss0.cpu().numpy(), ws.ss1.cpu().numpy())
    w0, w1 = ws.w0.cpu().numpy(), ws.w1.cpu().numpy()
    c = [t.cpu().numpy() for t in (ws.eeg.c0, ws.aud.c0, ws.eeg.c1, ws.aud.c1)]
    out = {"tool": "sliced_bench", "pairs_per_leg": n_win, "steps": args.steps,
           "mean_rows": {"eeg_h0": float(c[0].mean()), "aud_h0": float(c[1].mean()), "eeg_h1": float(c[2].mean()), "aud_h1": float(c[3].mean())},
           "mean_wasserstein": [float(np.nanmean(w0)), float(np.nanmean(w1))], "directions": {}}
    for M in TABLES:
        ms = {s: float(np.median([t[s] for t in log[M]])) for s in STAGES}
        s0, s1, ss0, ss1 = values[M]
        out["directions"][str(M)] = {
            "stage_ms_median": {s: round(v, 4) for s, v in ms.items()},
            "stage_ms_all": {s: [round(t[s], 4) for t in log[M]] for s in STAGES},
            "status_nonzero": [int((ss0 != 0).sum()), int((ss1 != 0).sum())],
            "mean_sliced": [float(np.nanmean(s0)), float(np.nanmean(s1))],
            "sliced_le_twice_wasserstein": bool((s0 <= 2 * w0 * (1 + 1e-9))[np.isfinite(w0)].all()
                                                and (s1 <= 2 * w1 * (1 + 1e-9))[np.isfinite(w1)].all()),
        }
        for s in STAGES:
            print(f"M={M:3d} {s:16s} {ms[s]:9.3f} ms   ({n_win} pairs, median of {args.steps})")
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
