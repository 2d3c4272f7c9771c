#!/usr/bin/env python3
"""The order-2 / L-infinity Wasserstein stages beside the Wasserstein and bottleneck stages of the same step, on the same
diagram pairs.

The benchmark's corpus mix (1,416 recordings x 15 windows x 5 bands = 106,200 window pairs, all bands as ONE batch) runs
through pipeline.run_step on a Workspace(bottleneck=True, wasserstein_q=variant), launched eagerly with HIP events around
the six distance stages, once per new variant: (2, "l2"), (1, "linf"), (2, "linf").  Then, per variant and leg, one more
launch with the pruning counters (tda_set_wasserstein_counter) read back.  Prints the median stage times of the timed
steps and writes one JSON document.

    python tools/wasserstein_q_bench.py [--recordings 1416] [--steps 5] [--warmup 1] [--out profiles/wasserstein_q_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

STAGES = ["wasserstein_h0", "wasserstein_h1", "bottleneck_h0", "bottleneck_h1", "wasserstein_q_h0", "wasserstein_q_h1"]
VARIANTS = [(2, "l2"), (1, "linf"), (2, "linf")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--recordings", type=int, default=1416)
    ap.add_argument("--windows-per-recording", type=int, default=15)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wasserstein_q_bench.json"))
    args = ap.parse_args()

    import torch
    from tda_eeg_audio_amd import _lib, engine, pipeline, synth
    if not torch.cuda.is_available():
        print("wasserstein_q_bench.py needs an MI355X: the HIP path has no CPU fallback", file=sys.stderr)
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
    # One Workspace for the three variants (a second one of 106,200 windows would double the diagram buffers): the buffers
    # of `wq` do not depend on the variant, and run_step reads (order, ground) from ws.wasserstein_q alone, so the loop
    # below assigns that attribute -- each value validated through step_outputs first, and ws.outputs kept in step.
    ws = pipeline.Workspace(n_win, seg_off, dev, bottleneck=True, wasserstein_q=VARIANTS[0])
    counter = torch.zeros(3, dtype=torch.int64, device=dev)
    legs = {"h0": (ws.eeg.h0, ws.eeg.c0, ws.aud.h0, ws.aud.c0), "h1": (ws.eeg.h1, ws.eeg.c1, ws.aud.h1, ws.aud.c1)}

    out = {"tool": "wasserstein_q_bench", "pairs_per_leg": n_win, "steps": args.steps, "variants": {}}
    for order, ground in VARIANTS:
        (rec,) = pipeline.step_outputs(wasserstein_q=(order, ground))
        ws.wasserstein_q = rec.params
        ws.outputs = [rec if o.name == "wq" else o for o in ws.outputs]
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
        q = [t.cpu().numpy() for t in (ws.q0, ws.q1, ws.qs0, ws.qs1)]
        b0, b1 = ws.b0.cpu().numpy(), ws.b1.cpu().numpy()
        w0, w1 = ws.w0.cpu().numpy(), ws.w1.cpu().numpy()
        # the pruning counters of one launch per leg: short cuts, rows + columns trimmed, pairs solved
        ctrs = {}
        ctx.set_wasserstein_counter(counter.data_ptr())
        for name, leg in legs.items():
            counter.zero_()
            engine.wasserstein_q_dev(*leg, order=order, ground=ground, ctx=ctx)
            torch.cuda.synchronize()
            c = counter.cpu().numpy()
            ctrs[name] = {"short_cuts": int(c[0]), "rows_and_columns_trimmed": int(c[1]), "pairs": int(c[2])}
        ctx.set_wasserstein_counter(None)
        key = f"{order},{ground}"
        out["variants"][key] = {
            "stage_ms_median": {s: round(v, 4) for s, v in ms.items()},
            "stage_ms_all": {s: [round(t[s], 4) for t in log] for s in STAGES},
            "status_nonzero": [int((q[2] != 0).sum()), int((q[3] != 0).sum())],
            "mean_distance": [float(np.nanmean(q[0])), float(np.nanmean(q[1]))],
            "pruning_counters": ctrs,
            # the chain the variant belongs to, per pair: against the bottleneck distance with 1e-9 of slack (both built
            # from the same exactly rounded costs); against tda_wasserstein_batch with 1e-6, because that entry's point
            # costs follow sklearn's expansion (up to 7.3e-8 X each, include/tdaeeg.h) and are summed over the pair
            "le_wasserstein_1_l2": bool((q[0] <= w0 + 1e-6).all() and (q[1] <= w1 + 1e-6).all()),
            "ge_bottleneck": bool((b0 <= q[0] + 1e-9).all() and (b1 <= q[1] + 1e-9).all()) if ground == "linf" else None,
        }
        print(f"--- order {order}, ground {ground}")
        for s in STAGES:
            print(f"{s:18s} {ms[s]:9.3f} ms   ({n_win} pairs, median of {args.steps})")
        print("counters:", json.dumps(ctrs))
    c = [t.cpu().numpy() for t in (ws.eeg.c0, ws.aud.c0, ws.eeg.c1, ws.aud.c1)]
    out["mean_rows"] = {"eeg_h0": float(c[0].mean()), "aud_h0": float(c[1].mean()), "eeg_h1": float(c[2].mean()),
                        "aud_h1": float(c[3].mean())}
    out["mean_wasserstein"] = [float(np.nanmean(ws.w0.cpu().numpy())), float(np.nanmean(ws.w1.cpu().numpy()))]
    out["mean_bottleneck"] = [float(np.nanmean(ws.b0.cpu().numpy())), float(np.nanmean(ws.b1.cpu().numpy()))]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
