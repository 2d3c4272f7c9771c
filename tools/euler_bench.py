"""The Euler characteristic curves on the bench's 106,200 window pairs (1,416 recordings x 15 windows x 5 bands, the inputs
of bench.py), 64 grid points on [0, 2], HIP events around whole launches, medians of `reps` launches with their spread, in
ONE run:
  eeg_euler_k3 / eeg_euler_k2      engine.euler_dm_dev on the 47 x 47 distance matrices of the EEG windows, max_dim 3 / 2
  eeg_rips                         engine.rips_dm_dev on the same matrices (the Rips stage of the same windows)
  audio_euler_k3 / audio_euler_k2  engine.euler_takens_dev on the audio windows with their delays, max_dim 3 / 2
  audio_rips                       engine.takens_rips_dev on the same windows
  eeg_mean / audio_mean            engine.euler_mean_dev over the 7,080 (recording, band) groups
Beside each Euler launch the inner steps it ran, read off its own output: sum over windows and grid points of f_2 (one step
of the tetrahedron loop per triangle, max_dim 3) or of f_1 (one mask intersection per present edge, max_dim 2), and the
steps per second.  The rate is nominal: a grid point whose edge count repeats that of its wave's previous grid point keeps
that one's counts and is counted here although it was not run again.  Writes profiles/euler_bench.json, or `out`
(an A/B run keeps one file per library: TDA_LIB=libtdaeeg_<variant>.so selects a variant build).
    python tools/euler_bench.py [n_rec] [reps] [out]"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tda_eeg_audio_amd import _lib, engine, synth      # noqa: E402

PER_REC, N_GRID = 15, 64


def timed(fn, reps):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(round(a.elapsed_time(b), 4))
    return ts


def summary(ts, **kw):
    return dict(ms_all=ts, ms_median=float(np.median(ts)), ms_min=min(ts), ms_max=max(ts),
                spread=round((max(ts) - min(ts)) / float(np.median(ts)), 4), **kw)


def euler_summary(ts, out_t, st_t, K):
    """Timing plus the work the launch did, counted from its own output (int64 sums on the device)."""
    n_win = out_t.shape[0]
    tri = int(out_t[:, 2].sum(dtype=torch.int64).item())
    edges = int(out_t[:, 1].sum(dtype=torch.int64).item())
    steps = tri if K == 3 else edges
    ms = float(np.median(ts))
    return summary(ts, windows=n_win, max_dim=K, windows_flagged=int((st_t != 0).sum().item()),
                   sum_f1=edges, sum_f2=tri, sum_f3=int(out_t[:, 3].sum(dtype=torch.int64).item()) if K == 3 else None,
                   inner_steps=steps, inner_steps_per_window=round(steps / n_win, 1),
                   gsteps_per_s=round(steps / ms / 1e6, 3), us_per_window=round(1e3 * ms / n_win, 4))


def main():
    n_rec = int(sys.argv[1]) if len(sys.argv) > 1 else 1416
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    out_path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "euler_bench.json")
    ctx = _lib.get_ctx(0)
    dev = torch.device("cuda", 0)
    nb = len(synth.BANDS)
    aud = synth.corpus_audio(n_rec, PER_REC)
    A = torch.from_numpy(np.concatenate([aud[b].reshape(-1, 250) for b in synth.BANDS])).to(dev)
    E = torch.cat(synth.corpus_eeg_dev(np.arange(n_rec), PER_REC, nb, dev))
    n = A.shape[0]
    assert E.shape == (n, 47, 250)
    seg_t = torch.arange(0, n + 1, PER_REC, dtype=torch.int32, device=dev)
    grid_t = torch.linspace(0.0, 2.0, N_GRID, dtype=torch.float64, device=dev)
    D = engine.corr_dist_dev(E, ctx=ctx)
    del E
    tau_w = torch.empty(n, dtype=torch.int32, device=dev)
    engine.tau_segments_dev(A, seg_t, 125, tau_win_t=tau_w, ctx=ctx)
    res = dict(tool="euler_bench", lib=os.path.basename(_lib.LIB_PATH), windows=int(n), reps=reps, n_grid=N_GRID,
               grid=[0.0, 2.0])

    st = torch.empty(n, dtype=torch.int32, device=dev)
    for K in (3, 2):
        out = torch.empty((n, K + 2, N_GRID), dtype=torch.int32, device=dev)
        ts = timed(lambda: engine.euler_dm_dev(D, grid_t, K, out_t=out, status_t=st, ctx=ctx), reps)
        res[f"eeg_euler_k{K}"] = euler_summary(ts, out, st, K)
        if K == 3:
            mean = torch.empty((n // PER_REC, K + 2, N_GRID), dtype=torch.float64, device=dev)
            res["eeg_mean"] = summary(timed(lambda: engine.euler_mean_dev(out, n, K, N_GRID, seg_t, mean_t=mean, ctx=ctx), reps))
            res["eeg_mean_chi_at_t1"] = float(mean[:, 4, N_GRID // 2].mean().item())
        ts = timed(lambda: engine.euler_takens_dev(A, tau_w, grid_t, K, out_t=out, status_t=st, ctx=ctx), reps)
        res[f"audio_euler_k{K}"] = euler_summary(ts, out, st, K)
        if K == 3:
            res["audio_mean"] = summary(timed(lambda: engine.euler_mean_dev(out, n, K, N_GRID, seg_t, st, 4 | 16, mean, ctx=ctx), reps))
        del out
    dg = engine.DeviceDiagrams(n, 47, engine.DEFAULT_H1_CAP, dev)
    res["eeg_rips"] = summary(timed(lambda: engine.rips_dm_dev(D, out=dg, ctx=ctx), reps),
                              windows_flagged=int((dg.status != 0).sum().item()))
    del dg
    da = engine.DeviceDiagrams(n, _lib.MAX_POINTS, engine.DEFAULT_H1_CAP, dev)
    res["audio_rips"] = summary(timed(lambda: engine.takens_rips_dev(A, tau_w, out=da, ctx=ctx), reps),
                                windows_flagged=int((da.status & ~4 != 0).sum().item()))
    res["audio_points_mean"] = float(da.n_points.double().mean().item())
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({k: (v["ms_median"], v.get("gsteps_per_s"), v["spread"]) for k, v in res.items()
                      if isinstance(v, dict) and "ms_median" in v}))


if __name__ == "__main__":
    main()
