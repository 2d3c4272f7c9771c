#!/usr/bin/env python3
"""The persistence-image stage beside the finishing pass of the same step, on the same diagrams.

The benchmark's corpus mix (1,416 recordings x 15 windows x 5 bands = 106,200 windows, all bands as ONE batch) runs through
pipeline.run_step on a Workspace(images=(xe, ye, sigma, power)), launched eagerly with HIP events around the `finish` and
the `image` stage; then the image stage alone on the diagrams the step left; then whole steps with the option on and off.
Prints the medians and one JSON line, and writes profiles/image_bench.json.

    python tools/image_bench.py [--recordings 1416] [--steps 5] [--warmup 1] [--side 20] [--sigma 0.05] [--power 1]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

STAGES = ["finish", "image"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--recordings", type=int, default=1416)
    ap.add_argument("--windows-per-recording", type=int, default=15)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--side", type=int, default=20)
    ap.add_argument("--sigma", type=float, default=0.05)
    ap.add_argument("--power", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "image_bench.json"))
    args = ap.parse_args()
    steps = max(5, args.steps)

    import torch
    from tda_eeg_audio_amd import _lib, pipeline, synth, utils
    if not torch.cuda.is_available():
        print("image_bench.py needs an MI355X: the HIP path has no CPU fallback", file=sys.stderr)
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
    xe, ye = utils.default_image_edges(args.side, args.side)
    ws = pipeline.Workspace(n_win, seg_off, dev, images=(xe, ye, args.sigma, args.power))

    def ev():
        return torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    for _ in range(max(1, args.warmup)):
        pipeline.run_step(eeg, aud, ws, ctx=ctx)
    torch.cuda.synchronize()
    # 1. inside the step, beside `finish`
    log = []
    for _ in range(steps):
        timers = {s: ev() for s in STAGES}
        pipeline.run_step(eeg, aud, ws, ctx=ctx, timers=timers)
        torch.cuda.synchronize()
        log.append({s: timers[s][0].elapsed_time(timers[s][1]) for s in STAGES})
    ms = {s: float(np.median([t[s] for t in log])) for s in STAGES}
    # 2. the stage alone, on the diagrams of the last step
    alone = []
    for _ in range(steps):
        a, b = ev()
        a.record()
        pipeline.OUTPUT_BY_NAME["img"].set_stage(ws, ctx, audio=True)
        b.record()
        torch.cuda.synchronize()
        alone.append(a.elapsed_time(b))
    # 3. whole steps, option on and off (eager, back to back, one event pair around all of them)
    def per_step(w):
        pipeline.run_step(eeg, aud, w, ctx=ctx)
        torch.cuda.synchronize()
        a, b = ev()
        a.record()
        for _ in range(steps):
            pipeline.run_step(eeg, aud, w, ctx=ctx)
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / steps
    on = per_step(ws)
    img = ws.img.cpu().numpy()
    c = [float(t.float().mean()) for t in (ws.eeg.c0, ws.eeg.c1, ws.aud.c1)]
    kept = int(((ws.aud.status & (_lib.TDA_WIN_DEGENERATE | _lib.TDA_WIN_TOO_LARGE)) == 0).sum())
    del ws
    torch.cuda.empty_cache()
    off = per_step(pipeline.Workspace(n_win, seg_off, dev))

    rows_read = n_win * (c[0] + c[1] + c[2]) * 16
    out = {
        "tool": "image_bench", "windows": n_win, "groups": len(seg_off) - 1, "n_x": args.side, "n_y": args.side,
        "sigma": args.sigma, "power": args.power,
        "steps": steps,
        "stage_ms_median": {s: round(v, 4) for s, v in ms.items()},
        "stage_ms_all": {s: [round(t[s], 4) for t in log] for s in STAGES},
        "image_alone_ms_median": round(float(np.median(alone)), 4), "image_alone_ms_all": [round(v, 4) for v in alone],
        "ms_per_step": {"images_on": round(on, 3), "images_off": round(off, 3)},
        "mean_rows": {"eeg_h0": c[0], "eeg_h1": c[1], "aud_h1": c[2]}, "audio_windows_kept": kept,
        "bytes": {"diagram_rows_read": int(rows_read), "written": int(img.size * 8)},
        "nan_groups": int(np.isnan(img).any(axis=(1, 2, 3)).sum()),
        "mean_image_mass": [float(np.nanmean(img[:, s].sum(axis=(1, 2)))) for s in range(3)],
    }
    for s in STAGES:
        print(f"{s:16s} {ms[s]:9.3f} ms   (in the step, median of {steps})")
    print(f"{'image alone':16s} {out['image_alone_ms_median']:9.3f} ms   (median of {steps})")
    print(f"ms per step: {on:.3f} with images, {off:.3f} without")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
