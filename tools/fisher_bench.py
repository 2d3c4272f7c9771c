#!/usr/bin/env python3
"""The persistence Fisher stages beside the Wasserstein and kernel-distance stages of the same step, and the distance
matrix of one band's first EEG H1 diagrams.

The benchmark's corpus mix (1,416 recordings x 15 windows x 5 bands = 106,200 window pairs, all bands as ONE batch) runs
through pipeline.run_step on a Workspace(kernel_distance=("pwg", 0.1, 2.0), fisher=sigma), launched eagerly with HIP events
around the six distance stages.  A term is one exponential of the definition (include/tdaeeg.h): a pair with N = m + n
finite rows has 4 N^2 of them.  Then the (256, 256) distance matrix of the first band's first 256 EEG H1 diagrams
(engine.persistence_fisher_gram_dev: the pairs i <= j in one launch), by HIP events.  Prints the medians and writes one JSON
document.

    python tools/fisher_bench.py [--recordings 1416] [--steps 5] [--warmup 1] [--sigma 0.1] [--matrix 256]
                                 [--out profiles/fisher_bench.json]
TDA_LIB=libtdaeeg_<variant>.so runs a variant build of the library (csrc/Makefile), e.g. the 256-thread build of DESIGN.md
3.16.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

STAGES = ["wasserstein_h0", "wasserstein_h1", "kernel_distance_h0", "kernel_distance_h1", "fisher_h0", "fisher_h1"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--recordings", type=int, default=1416)
    ap.add_argument("--windows-per-recording", type=int, default=15)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--sigma", type=float, default=0.1)
    ap.add_argument("--matrix", type=int, default=256, help="diagrams of the distance matrix")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fisher_bench.json"))
    args = ap.parse_args()

    import torch
    from tda_eeg_audio_amd import _lib, engine, pipeline, synth
    if not torch.cuda.is_available():
        print("fisher_bench.py needs an MI355X: the HIP path has no CPU fallback", file=sys.stderr)
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
    ws = pipeline.Workspace(n_win, seg_off, dev, kernel_distance=("pwg", 0.1, 2.0), fisher=args.sigma)
    ev = lambda: torch.cuda.Event(enable_timing=True)
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

    def finite(rows, cnt):
        m = torch.clamp(cnt, 0, rows.shape[1])
        live = torch.arange(rows.shape[1], device=dev)[None, :] < m[:, None]
        return (torch.isfinite(rows).all(dim=2) & live).sum(dim=1).double()

    legs = {}
    for k, (e, a, d, st) in enumerate((((ws.eeg.h0, ws.eeg.c0), (ws.aud.h0, ws.aud.c0), ws.f0, ws.fs0),
                                       ((ws.eeg.h1, ws.eeg.c1), (ws.aud.h1, ws.aud.c1), ws.f1, ws.fs1))):
        N = finite(*e) + finite(*a)
        ok = st == 0
        terms = float((4.0 * N * N)[ok].sum())
        t = ms[f"fisher_h{k}"]
        dh = d.cpu().numpy()
        legs[f"h{k}"] = {"points_2N_mean": float(2.0 * N.mean()), "points_2N_max": float(2.0 * N.max()), "terms": terms,
                         "terms_per_s": terms / (t * 1e-3), "status_nonzero": int((~ok).sum()),
                         "mean_distance": float(np.nanmean(dh)), "max_distance": float(np.nanmax(dh))}
    # the distance matrix of the first band's first diagrams, EEG H1
    n_m = min(args.matrix, n_rec * wpr)
    rows, cnt = ws.eeg.h1[:n_m].contiguous(), ws.eeg.c1[:n_m].contiguous()
    G = engine.persistence_fisher_gram_dev(rows, cnt, args.sigma, ctx=ctx)
    torch.cuda.synchronize()
    t_ms = []
    for _ in range(args.steps):
        e0, e1 = ev(), ev()
        e0.record()
        G = engine.persistence_fisher_gram_dev(rows, cnt, args.sigma, ctx=ctx)
        e1.record()
        torch.cuda.synchronize()
        t_ms.append(e0.elapsed_time(e1))
    Gh = G.cpu().numpy()
    f = finite(rows, cnt).cpu().numpy()
    iu, ju = np.triu_indices(n_m)
    m_terms = float((4.0 * (f[iu] + f[ju]) ** 2).sum())
    med = float(np.median(t_ms))
    out = {"tool": "fisher_bench", "pairs_per_leg": n_win, "steps": args.steps, "sigma": args.sigma,
           "lib": os.environ.get("TDA_LIB", "libtdaeeg.so"),
           "stage_ms_median": {s: round(v, 4) for s, v in ms.items()},
           "stage_ms_all": {s: [round(t[s], 4) for t in log] for s in STAGES},
           "legs": legs,
           "matrix": {"diagrams": n_m, "pairs": int(len(iu)), "ms_all": [round(t, 3) for t in t_ms], "ms_median": round(med, 3),
                      "includes": "index lists, the launch and the mirroring", "terms": m_terms,
                      "terms_per_s": m_terms / (med * 1e-3), "finite": bool(np.isfinite(Gh).all()),
                      "symmetric_bytes": bool(Gh.tobytes() == Gh.T.copy().tobytes()),
                      "zero_diagonal": bool((np.diag(Gh) == 0.0).all()), "max": float(Gh.max())}}
    c = [t.cpu().numpy() for t in (ws.eeg.c0, ws.aud.c0, ws.eeg.c1, ws.aud.c1)]
    out["mean_rows"] = {"eeg_h0": float(c[0].mean()), "aud_h0": float(c[1].mean()), "eeg_h1": float(c[2].mean()),
                        "aud_h1": float(c[3].mean())}
    for s in STAGES:
        print(f"{s:20s} {ms[s]:9.3f} ms   ({n_win} pairs, median of {args.steps})")
    for name, g in legs.items():
        print(f"fisher {name}: 2N mean {g['points_2N_mean']:.1f}, {g['terms']:.3e} terms, {g['terms_per_s']:.3e} terms/s")
    print(f"matrix: {n_m} diagrams, {med:.3f} ms, {m_terms:.3e} terms, {out['matrix']['terms_per_s']:.3e} terms/s")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
