#!/usr/bin/env python3
"""The kernel-distance stages beside the Wasserstein and sliced stages of the same step, and the Gram matrices of one
band's recordings.

The benchmark's corpus mix (1,416 recordings x 15 windows x 5 bands = 106,200 window pairs, all bands as ONE batch) runs
through pipeline.run_step on a Workspace(sliced=default_directions(50), kernel_distance=kernel), launched eagerly with HIP
events around the six distance stages.  Then the symmetric H0 and H1 Gram matrices of the first band's 1,416 groups of
EEG diagrams (engine.diagram_kernel_gram_dev), by HIP events, with the terms they add up per second.  Prints the medians
and writes one JSON document.

    python tools/diagram_kernel_bench.py [--recordings 1416] [--steps 5] [--warmup 1] [--gram-steps 3] [--gram-groups 0]
                                         [--out profiles/diagram_kernel_bench.json]
TDA_LIB=libtdaeeg_<variant>.so runs a variant build of the library (csrc/Makefile), e.g. the workgroup-per-pair build of
DESIGN.md 3.15.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

STAGES = ["wasserstein_h0", "wasserstein_h1", "sliced_h0", "sliced_h1", "kernel_distance_h0", "kernel_distance_h1"]
KERNELS = [("pss", 0.1), ("pwg", 0.1, 2.0)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--recordings", type=int, default=1416)
    ap.add_argument("--windows-per-recording", type=int, default=15)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--gram-steps", type=int, default=3)
    ap.add_argument("--gram-groups", type=int, default=0, help="groups of the Gram matrices (0: every recording of the band)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "diagram_kernel_bench.json"))
    args = ap.parse_args()

    import torch
    from tda_eeg_audio_amd import _lib, engine, pipeline, synth, utils
    if not torch.cuda.is_available():
        print("diagram_kernel_bench.py needs an MI355X: the HIP path has no CPU fallback", file=sys.stderr)
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
    # one Workspace for both kernels: the buffers of `kd` do not depend on the kernel, and run_step reads it from
    # ws.kernel_distance alone (validated through step_outputs first, ws.outputs kept in step)
    ws = pipeline.Workspace(n_win, seg_off, dev, sliced=utils.default_directions(50), kernel_distance=KERNELS[0])
    out = {"tool": "diagram_kernel_bench", "pairs_per_leg": n_win, "steps": args.steps, "kernels": {}}
    ev = lambda: torch.cuda.Event(enable_timing=True)
    for kernel in KERNELS:
        (rec,) = pipeline.step_outputs(kernel_distance=kernel)
        ws.kernel_distance = rec.params
        ws.outputs = [rec if o.name == "kd" else o for o in ws.outputs]
        for _ in range(max(1, args.warmup)):
            pipeline.run_step(eeg, aud, ws, ctx=ctx)
        torch.cuda.synchronize()
        log = []
        for _ in range(args.steps):
            timers = {s: (ev(), ev()) for s in STAGES}
            pipeline.run_step(eeg, aud, ws, ctx=ctx, timers=timers)
            torch.cuda.synchronize()
            log.append({s: timers[s][0].elapsed_time(timers[s][1]) for s in STAGES})
        ms = {s: float(np.median([t[s] for t in log])) for s in STAGES}
        k = [t.cpu().numpy() for t in (ws.k0, ws.k1, ws.ks0, ws.ks1)]
        # the Gram matrices of the first band's groups of EEG diagrams, symmetric route
        n_g = min(args.gram_groups, n_rec) if args.gram_groups > 0 else n_rec
        off_t = ws.seg_off[:n_g + 1].contiguous()
        grams = {}
        for name, rows, cnt in (("h0", ws.eeg.h0, ws.eeg.c0), ("h1", ws.eeg.h1, ws.eeg.c1)):
            rows, cnt = rows[:n_g * wpr], cnt[:n_g * wpr]
            m = torch.minimum(cnt, torch.full_like(cnt, rows.shape[1]))
            live = torch.arange(rows.shape[1], device=dev)[None, :] < m[:, None]
            fin = (torch.isfinite(rows).all(dim=2) & live).sum(dim=1).view(n_g, wpr).sum(dim=1).double().cpu().numpy()
            staged = m.view(n_g, wpr).sum(dim=1).double().cpu().numpy()
            tri = lambda r: float((r.sum() ** 2 + (r * r).sum()) / 2.0)          # sum over g <= h of r_g r_h
            G = torch.empty((n_g, n_g), dtype=torch.float64, device=dev)
            engine.diagram_kernel_gram_dev(rows, cnt, kernel, seg_off_a=off_t, out_t=G, ctx=ctx)
            torch.cuda.synchronize()
            t_ms = []
            for _ in range(args.gram_steps):
                e0, e1 = ev(), ev()
                e0.record()
                engine.diagram_kernel_gram_dev(rows, cnt, kernel, seg_off_a=off_t, out_t=G, ctx=ctx)
                e1.record()
                torch.cuda.synchronize()
                t_ms.append(e0.elapsed_time(e1))
            med = float(np.median(t_ms))
            Gh = G.cpu().numpy()
            grams[name] = {"groups": n_g, "ms_all": [round(t, 3) for t in t_ms], "ms_median": round(med, 3),
                           "terms_finite": tri(fin), "terms_computed": tri(staged),
                           "terms_per_s": tri(staged) / (med * 1e-3), "finite": bool(np.isfinite(Gh).all()),
                           "symmetric_bytes": bool(Gh.tobytes() == Gh.T.copy().tobytes()),
                           "min_eig_over_trace": float(np.linalg.eigvalsh(Gh).min() / np.trace(Gh))}
        out["kernels"][",".join(str(v) for v in kernel)] = {
            "stage_ms_median": {s: round(v, 4) for s, v in ms.items()},
            "stage_ms_all": {s: [round(t[s], 4) for t in log] for s in STAGES},
            "status_nonzero": [int((k[2] != 0).sum()), int((k[3] != 0).sum())],
            "mean_distance": [float(np.nanmean(k[0])), float(np.nanmean(k[1]))],
            "gram": grams,
        }
        print(f"--- kernel {kernel}")
        for s in STAGES:
            print(f"{s:20s} {ms[s]:9.3f} ms   ({n_win} pairs, median of {args.steps})")
        for name, g in grams.items():
            print(f"gram {name}: {g['ms_median']:.1f} ms, {g['terms_computed']:.3e} terms, {g['terms_per_s']:.3e} terms/s")
    c = [t.cpu().numpy() for t in (ws.eeg.c0, ws.aud.c0, ws.eeg.c1, ws.aud.c1)]
    out["mean_rows"] = {"eeg_h0": float(c[0].mean()), "aud_h0": float(c[1].mean()), "eeg_h1": float(c[2].mean()),
                        "aud_h1": float(c[3].mean())}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
