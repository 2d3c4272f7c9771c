#!/usr/bin/env python3
"""The bottleneck stages beside the Wasserstein stages of the same step, on the same diagram pairs.

The benchmark's corpus mix (1,416 recordings x 15 windows x 5 bands = 106,200 window pairs, all bands as ONE batch) runs
through pipeline.run_step on a Workspace(bottleneck=True), launched eagerly with HIP events around the four distance
stages.  Prints the median stage times of the timed steps and one JSON line.

    python tools/bottleneck_bench.py [--recordings 1416] [--steps 5] [--warmup 1]

With a TDA_PROFILE build (TDA_LIB=libtdaeeg_prof.so, make -C tda_eeg_audio_amd/csrc PROFILE=1) the cycle counters of the
solver's phases are printed for one more step.
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

STAGES = ["wasserstein_h0", "wasserstein_h1", "bottleneck_h0", "bottleneck_h1"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--recordings", type=int, default=1416)
    ap.add_argument("--windows-per-recording", type=int, default=15)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    args = ap.parse_args()

    import torch
    from tda_eeg_audio_amd import _lib, pipeline, synth
    if not torch.cuda.is_available():
        print("bottleneck_bench.py needs an MI355X: the HIP path has no CPU fallback", file=sys.stderr)
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
    ws = pipeline.Workspace(n_win, seg_off, dev, bottleneck=True)

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
    bs0, bs1 = ws.bs0.cpu().numpy(), ws.bs1.cpu().numpy()
    b0, b1 = ws.b0.cpu().numpy(), ws.b1.cpu().numpy()
    w0, w1 = ws.w0.cpu().numpy(), ws.w1.cpu().numpy()
    c = [t.cpu().numpy() for t in (ws.eeg.c0, ws.aud.c0, ws.eeg.c1, ws.aud.c1)]
    out = {
        "tool": "bottleneck_bench", "pairs_per_leg": n_win, "steps": args.steps,
        "stage_ms_median": {s: round(v, 4) for s, v in ms.items()},
        "stage_ms_all": {s: [round(t[s], 4) for t in log] for s in STAGES},
        "status_nonzero": [int((bs0 != 0).sum()), int((bs1 != 0).sum())],
        "mean_rows": {"eeg_h0": float(c[0].mean()), "aud_h0": float(c[1].mean()), "eeg_h1": float(c[2].mean()), "aud_h1": float(c[3].mean())},
        "mean_bottleneck": [float(np.nanmean(b0)), float(np.nanmean(b1))],
        "mean_wasserstein": [float(np.nanmean(w0)), float(np.nanmean(w1))],
        "bottleneck_le_wasserstein": bool((b0 <= w0 + 1e-12).all() and (b1 <= w1 + 1e-12).all()),
    }
    for s in STAGES:
        print(f"{s:16s} {ms[s]:9.3f} ms   ({n_win} pairs, median of {args.steps})")

    lib = ctypes.CDLL(_lib.LIB_PATH)
    if hasattr(lib, "tda_profile_read_bn"):
        from tda_eeg_audio_amd import engine
        buf = (ctypes.c_ulonglong * 16)()
        prof = {}
        for name, (ra, ca, rb, cb) in (("h0", (ws.eeg.h0, ws.eeg.c0, ws.aud.h0, ws.aud.c0)),
                                       ("h1", (ws.eeg.h1, ws.eeg.c1, ws.aud.h1, ws.aud.c1))):
            lib.tda_profile_read_bn(buf, 1)
            engine.bottleneck_dev(ra, ca, rb, cb, ctx=ctx)
            torch.cuda.synchronize()
            lib.tda_profile_read_bn(buf, 1)
            v = np.array(list(buf), dtype=np.float64)
            n = max(v[5], 1.0)
            prof[name] = {"pairs": int(v[5]), "points_a": v[9] / n, "points_b": v[10] / n,
                          "cycles_per_pair": {"load": v[0] / n, "bounds": v[1] / n, "candidate_scans": v[2] / n,
                                              "adjacency_builds": v[3] / n, "cover_searches": v[4] / n},
                          "probes_per_pair": v[6] / n, "searches_per_pair": v[7] / n, "expansions_per_pair": v[8] / n}
            print(f"bottleneck {name}:", json.dumps(prof[name]))
        out["profile"] = prof
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
