"""The recurrence curves on the bench's 106,200 audio windows (1,416 recordings x 15 windows x 5 bands, the inputs of
bench.py) with their delays, 64 grid points on [0, 2], theiler 1, l_min = v_min = 2, HIP events around whole launches, two
warm-ups and the median of `reps` launches with their spread:
  recurrence / recurrence_hist   engine.recurrence_takens_dev without / with the line-length histograms
  recurrence_mean                engine.recurrence_mean_dev (counts and measures) over the 7,080 (recording, band) groups
  network_takens / takens_rips   engine.network_takens_dev and engine.takens_rips_dev on the same windows, for scale
Every step is a child process of its own under a time limit of its own; after a step that fails or runs out of time no
further step is started, and the file says which steps were and were not measured.  Beside each recurrence launch the
work of its erosion loop read off its own output: per window and grid point the loop runs max(diag_longest, vert_longest)
+ 1 times (nominal: a grid point whose recurrence count repeats that of its wave's previous grid point keeps that one's
results).  There is no speed gate.  Writes profiles/recurrence_bench.json, or `out`.
    python tools/recurrence_bench.py [n_rec] [reps] [out]"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PER_REC, N_GRID = 15, 64
PAR = (1, 2, 2)
STEPS = (("recurrence", 240), ("recurrence_hist", 240), ("network_takens", 240), ("takens_rips", 240))


def step(name, n_rec, reps):
    """One step in this process: the result dict of the step, printed as one JSON line."""
    import numpy as np
    import torch
    from tda_eeg_audio_amd import _lib, engine, synth
    from euler_bench import summary, timed
    ctx = _lib.get_ctx(0)
    dev = torch.device("cuda", 0)
    aud = synth.corpus_audio(n_rec, PER_REC)
    A = torch.from_numpy(np.concatenate([aud[b].reshape(-1, 250) for b in synth.BANDS])).to(dev)
    n = A.shape[0]
    seg_t = torch.arange(0, n + 1, PER_REC, dtype=torch.int32, device=dev)
    grid_t = torch.linspace(0.0, 2.0, N_GRID, dtype=torch.float64, device=dev)
    tau_w = torch.empty(n, dtype=torch.int32, device=dev)
    engine.tau_segments_dev(A, seg_t, 125, tau_win_t=tau_w, ctx=ctx)
    npts = torch.empty(n, dtype=torch.int32, device=dev)
    res = {}
    if name in ("recurrence", "recurrence_hist"):
        hist = name == "recurrence_hist"
        rq = engine.DeviceRecurrenceCurves(n, N_GRID, _lib.MAX_POINTS, dev, hist)
        ts = timed(lambda: engine.recurrence_takens_dev(A, tau_w, grid_t, *PAR, hist, out=rq, n_points_t=npts, ctx=ctx), reps)
        ok = rq.status == 0
        loops = (torch.maximum(rq.counts[:, 3], rq.counts[:, 6]).to(torch.int64) + 1) * ok[:, None]
        ms = float(np.median(ts))
        res[name] = summary(ts, windows=int(n), windows_flagged=int((~ok).sum().item()),
                            points_mean=float(npts.double().mean().item()),
                            erosion_steps_per_window=round(loops.sum().item() / n, 1),
                            g_erosion_steps_per_s=round(loops.sum().item() / ms / 1e6, 3),
                            mean_recurrence_rate_at_t1=float(rq.measures[:, 0, N_GRID // 2].mean().item()),
                            mean_determinism_at_t1=float(rq.measures[:, 1, N_GRID // 2].mean().item()),
                            max_diag_longest=int(rq.counts[:, 3].max().item()), us_per_window=round(1e3 * ms / n, 4))
        if not hist:
            res["recurrence_mean"] = summary(timed(lambda: engine.recurrence_mean_dev(
                rq.counts, rq.measures, None, n, N_GRID, _lib.MAX_POINTS, seg_t, rq.status, 4 | 16, ctx=ctx), reps))
    elif name == "network_takens":
        net = engine.DeviceNetworkCurves(n, N_GRID, _lib.MAX_POINTS, dev, False)
        ts = timed(lambda: engine.network_takens_dev(A, tau_w, grid_t, False, out=net, n_points_t=npts, ctx=ctx), reps)
        res[name] = summary(ts, windows=int(n), windows_flagged=int((net.status != 0).sum().item()))
    elif name == "takens_rips":
        da = engine.DeviceDiagrams(n, _lib.MAX_POINTS, engine.DEFAULT_H1_CAP, dev)
        ts = timed(lambda: engine.takens_rips_dev(A, tau_w, out=da, ctx=ctx), reps)
        res[name] = summary(ts, windows=int(n), windows_flagged=int((da.status & ~4 != 0).sum().item()))
    else:
        raise SystemExit(f"unknown step {name!r}")
    print("RESULT " + json.dumps(res))


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--step":
        return step(sys.argv[2], int(sys.argv[3]), int(sys.argv[4]))
    n_rec = int(sys.argv[1]) if len(sys.argv) > 1 else 1416
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    out_path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "recurrence_bench.json")
    res = dict(tool="recurrence_bench", windows=n_rec * PER_REC * 5, reps=reps, warmups=2, n_grid=N_GRID, grid=[0.0, 2.0],
               theiler=PAR[0], l_min=PAR[1], v_min=PAR[2], measured=[], not_measured=[])
    for k, (name, limit) in enumerate(STEPS):
        why = None
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", name, str(n_rec), str(reps)],
                               capture_output=True, text=True, timeout=limit)
            lines = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
            if p.returncode != 0 or not lines:
                why = f"exit status {p.returncode}: {p.stderr.strip().splitlines()[-1:] or ''}"
        except subprocess.TimeoutExpired:
            why = f"ended at its time limit of {limit} s"
        if why is not None:
            # nothing more is started on the GPU after a step that failed
            res["not_measured"] = [dict(step=name, why=why)] + [dict(step=s, why="not started") for s, _ in STEPS[k + 1:]]
            break
        res.update(json.loads(lines[-1][len("RESULT "):]))
        res["measured"].append(name)
        print(f"{name}: {res[name]['ms_median']} ms", flush=True)
    for a, b in (("recurrence", "network_takens"), ("recurrence", "takens_rips"), ("recurrence_hist", "recurrence")):
        if a in res and b in res:
            res[f"{a}_over_{b}"] = round(res[a]["ms_median"] / res[b]["ms_median"], 3)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({k: (v["ms_median"], v["spread"]) if isinstance(v, dict) else v for k, v in res.items()
                      if (isinstance(v, dict) and "ms_median" in v) or "_over_" in k or k in ("measured", "not_measured")}))
    return 1 if res["not_measured"] else 0


if __name__ == "__main__":
    sys.exit(main())
