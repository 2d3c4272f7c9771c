"""The generators and representative cycles on the bench's 106,200 window pairs (1,416 recordings x 15 windows x 5 bands,
the inputs of bench.py), HIP events around whole launches, medians of `reps` launches with their spread, in ONE run:
  eeg_rips / audio_rips            engine.rips_dm_dev on the 47 x 47 distance matrices of the EEG windows /
                                   engine.takens_rips_dev on the audio windows with their delays: the yardstick
  eeg_gen_full / audio_gen_full    engine.generators_dm_dev / generators_takens_dev on the diagrams those launches wrote:
                                   edges, cycles, participation and the H0 forest edges
  *_gen_no_h0                      the same without h0_edge (no work item per H0 run)
  *_gen_edges_only                 without h0_edge, cyc and part: birth and death edges, lengths and flags
  eeg_mean                         engine.generators_mean_dev over the 7,080 (recording, band) groups
Beside each launch the work it did, from the kernel's own counters (work, a separate launch that is not timed): searches and
search levels per window, and the flagged rows.  Writes profiles/generators_bench.json, or `out`
(an A/B run keeps one file per library: TDA_LIB=libtdaeeg_<variant>.so selects a variant build).
    python tools/generators_bench.py [n_rec] [reps] [out]"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tda_eeg_audio_amd import _lib, engine, synth      # noqa: E402

PER_REC, CYC_CAP = 15, 64


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


def variants(run, dg, n, n_part, dev, reps, res, name):
    """The three output sets of one input form; `run(out, part, h0_edge, work)` launches the kernel."""
    h0_cap, h1_cap = dg.h0_cap, dg.h1_cap
    for tag, part, h0e, cyc in (("full", True, True, True), ("no_h0", True, False, True), ("edges_only", False, False, False)):
        out = engine.DeviceGenerators(n, h0_cap, h1_cap, CYC_CAP, n_part, dev, part=part, h0_edge=h0e, cyc=cyc)
        ts = timed(lambda: run(out, part, h0e, False), reps)
        # the counters of the same work, in a launch of its own
        cnt = engine.DeviceGenerators(n, h0_cap, h1_cap, CYC_CAP, n_part, dev, part=part, h0_edge=h0e, work=True, cyc=cyc)
        run(cnt, part, h0e, True)
        torch.cuda.synchronize()
        work = cnt.work.sum(dim=1, dtype=torch.int64)
        rows = torch.clamp(dg.c1, max=h1_cap).sum(dtype=torch.int64).item()
        ms = float(np.median(ts))
        res[f"{name}_gen_{tag}"] = summary(
            ts, windows=n, cyc_cap=CYC_CAP, h1_cap=h1_cap, h1_rows=int(rows), rows_flagged=int((cnt.h1_flag != 0).sum().item()),
            windows_with_status=int((cnt.status != 0).sum().item()),
            searches_per_window=round(work[:, 0].double().mean().item(), 2), searches_max=int(work[:, 0].max().item()),
            levels_per_window=round(work[:, 1].double().mean().item(), 2), levels_max=int(work[:, 1].max().item()),
            longest_cycle=int(cnt.cyc_len.max().item()), us_per_window=round(1e3 * ms / n, 4))
        if tag == "full":
            keep = out
        else:
            del out
        del cnt
    return keep


def main():
    n_rec = int(sys.argv[1]) if len(sys.argv) > 1 else 1416
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    out_path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "generators_bench.json")
    ctx = _lib.get_ctx(0)
    dev = torch.device("cuda", 0)
    nb = len(synth.BANDS)
    aud = synth.corpus_audio(n_rec, PER_REC)
    A = torch.from_numpy(np.concatenate([aud[b].reshape(-1, 250) for b in synth.BANDS])).to(dev)
    E = torch.cat(synth.corpus_eeg_dev(np.arange(n_rec), PER_REC, nb, dev))
    n = A.shape[0]
    assert E.shape == (n, 47, 250)
    seg_t = torch.arange(0, n + 1, PER_REC, dtype=torch.int32, device=dev)
    D = engine.corr_dist_dev(E, ctx=ctx)
    del E
    tau_w = torch.empty(n, dtype=torch.int32, device=dev)
    engine.tau_segments_dev(A, seg_t, 125, tau_win_t=tau_w, ctx=ctx)
    res = dict(tool="generators_bench", lib=os.path.basename(_lib.LIB_PATH), windows=int(n), reps=reps)

    dg = engine.DeviceDiagrams(n, 47, engine.DEFAULT_H1_CAP, dev)
    res["eeg_rips"] = summary(timed(lambda: engine.rips_dm_dev(D, out=dg, ctx=ctx), reps),
                              windows_flagged=int((dg.status != 0).sum().item()))
    full = variants(lambda out, part, h0e, work: engine.generators_dm_dev(D, dg, cyc_cap=CYC_CAP, part=part, h0_edge=h0e,
                                                                          work=work, out=out, ctx=ctx),
                    dg, n, 47, dev, reps, res, "eeg")
    mean = torch.empty((n // PER_REC, 47), dtype=torch.float64, device=dev)
    res["eeg_mean"] = summary(timed(lambda: engine.generators_mean_dev(full.part, n, 47, seg_t, mean_t=mean, ctx=ctx), reps))
    res["eeg_mean_participation"] = float(mean.mean().item())
    del dg, full

    da = engine.DeviceDiagrams(n, _lib.MAX_POINTS, engine.DEFAULT_H1_CAP, dev)
    res["audio_rips"] = summary(timed(lambda: engine.takens_rips_dev(A, tau_w, out=da, ctx=ctx), reps),
                                windows_flagged=int((da.status & ~4 != 0).sum().item()))
    res["audio_points_mean"] = float(da.n_points.double().mean().item())
    variants(lambda out, part, h0e, work: engine.generators_takens_dev(A, tau_w, da, cyc_cap=CYC_CAP, part=part, h0_edge=h0e,
                                                                       work=work, out=out, ctx=ctx),
             da, n, _lib.MAX_POINTS, dev, reps, res, "audio")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({k: (v["ms_median"], v.get("searches_per_window"), v["spread"]) for k, v in res.items()
                      if isinstance(v, dict) and "ms_median" in v}))


if __name__ == "__main__":
    main()
