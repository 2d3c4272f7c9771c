"""The network curves on the bench's 106,200 window pairs (1,416 recordings x 15 windows x 5 bands, the inputs of bench.py),
64 grid points on [0, 2], HIP events around whole launches, medians of `reps` launches with their spread, in ONE run on
the same windows:
  eeg_network / eeg_network_nodal      engine.network_dm_dev on the 47 x 47 distance matrices, without / with nodal
  eeg_euler_k2 / eeg_rips              engine.euler_dm_dev at max_dim 2 and engine.rips_dm_dev on the same matrices
  audio_network / audio_network_nodal  engine.network_takens_dev on the audio windows with their delays
  audio_euler_k2 / audio_rips          engine.euler_takens_dev at max_dim 2 and engine.takens_rips_dev on the same windows
  eeg_mean / audio_mean                engine.network_mean_dev (counts and measures) over the 7,080 (recording, band) groups
Beside each network launch the work of the lockstep search, read off its own output, per window (summed over the grid
points): the search levels, min(diameter + 1, n - 1), and the row-ORs, n + 2 pairs (every source ORs the row of every
vertex it visits).  Both are nominal: a grid point whose edge count repeats that of its wave's previous grid point keeps
that one's results, and a source that has seen all n vertices skips the ORs of its last frontier.  Writes
profiles/network_bench.json, or `out`.
    python tools/network_bench.py [n_rec] [reps] [out]"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tda_eeg_audio_amd import _lib, engine, synth      # noqa: E402
from euler_bench import summary, timed                 # noqa: E402

PER_REC, N_GRID = 15, 64


def network_summary(ts, net, n_pts_t):
    """Timing plus the work of the search, counted from the launch's own output (int64 sums on the device)."""
    n_win = net.counts.shape[0]
    ok = (net.status == 0)
    n = n_pts_t.to(torch.int64) * ok
    pairs, diam = net.counts[:, 7].to(torch.int64), net.counts[:, 9].to(torch.int64)
    levels = torch.minimum(diam + 1, (n - 1).clamp(min=0)[:, None]) * ok[:, None]
    row_ors = (n[:, None] + 2 * pairs) * ok[:, None]
    ms = float(np.median(ts))
    return summary(ts, windows=n_win, windows_flagged=int((~ok).sum().item()),
                   search_levels_per_window=round(levels.sum().item() / n_win, 1),
                   row_ors_per_window=round(row_ors.sum().item() / n_win, 1),
                   max_diameter=int(diam.max().item()), mean_components_at_t1=float(net.counts[:, 5, N_GRID // 2].double().mean().item()),
                   g_row_ors_per_s=round(row_ors.sum().item() / ms / 1e6, 3), us_per_window=round(1e3 * ms / n_win, 4))


def main():
    n_rec = int(sys.argv[1]) if len(sys.argv) > 1 else 1416
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    out_path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "network_bench.json")
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
    res = dict(tool="network_bench", lib=os.path.basename(_lib.LIB_PATH), windows=int(n), reps=reps, n_grid=N_GRID,
               grid=[0.0, 2.0])

    st = torch.empty(n, dtype=torch.int32, device=dev)
    eul = torch.empty((n, 4, N_GRID), dtype=torch.int32, device=dev)
    n47 = torch.full((n,), 47, dtype=torch.int32, device=dev)
    npts = torch.empty(n, dtype=torch.int32, device=dev)
    for nodal in (False, True):
        tag = "_nodal" if nodal else ""
        net = engine.DeviceNetworkCurves(n, N_GRID, 47, dev, nodal)
        ts = timed(lambda: engine.network_dm_dev(D, grid_t, nodal, out=net, ctx=ctx), reps)
        res["eeg_network" + tag] = network_summary(ts, net, n47)
        if not nodal:
            res["eeg_mean"] = summary(timed(lambda: engine.network_mean_dev(net.counts, net.measures, None, n, N_GRID, 47, seg_t,
                                                                            ctx=ctx), reps))
        del net
        net = engine.DeviceNetworkCurves(n, N_GRID, _lib.MAX_POINTS, dev, nodal)
        ts = timed(lambda: engine.network_takens_dev(A, tau_w, grid_t, nodal, out=net, n_points_t=npts, ctx=ctx), reps)
        res["audio_network" + tag] = network_summary(ts, net, npts)
        if not nodal:
            res["audio_mean"] = summary(timed(lambda: engine.network_mean_dev(net.counts, net.measures, None, n, N_GRID,
                                                                              _lib.MAX_POINTS, seg_t, net.status, 4 | 16, ctx=ctx),
                                              reps))
        del net
    res["eeg_euler_k2"] = summary(timed(lambda: engine.euler_dm_dev(D, grid_t, 2, out_t=eul, status_t=st, ctx=ctx), reps))
    res["audio_euler_k2"] = summary(timed(lambda: engine.euler_takens_dev(A, tau_w, grid_t, 2, out_t=eul, status_t=st, ctx=ctx),
                                          reps))
    dg = engine.DeviceDiagrams(n, 47, engine.DEFAULT_H1_CAP, dev)
    res["eeg_rips"] = summary(timed(lambda: engine.rips_dm_dev(D, out=dg, ctx=ctx), reps),
                              windows_flagged=int((dg.status != 0).sum().item()))
    del dg
    da = engine.DeviceDiagrams(n, _lib.MAX_POINTS, engine.DEFAULT_H1_CAP, dev)
    res["audio_rips"] = summary(timed(lambda: engine.takens_rips_dev(A, tau_w, out=da, ctx=ctx), reps),
                                windows_flagged=int((da.status & ~4 != 0).sum().item()))
    res["audio_points_mean"] = float(da.n_points.double().mean().item())
    for side in ("eeg", "audio"):
        for tag in ("", "_nodal"):
            res[f"{side}_network{tag}_over_euler_k2"] = round(res[f"{side}_network{tag}"]["ms_median"] /
                                                              res[f"{side}_euler_k2"]["ms_median"], 3)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({k: (v["ms_median"], v.get("row_ors_per_window"), v["spread"]) if isinstance(v, dict) else v
                      for k, v in res.items() if (isinstance(v, dict) and "ms_median" in v) or k.endswith("_over_euler_k2")}))


if __name__ == "__main__":
    main()
