"""The phase-locking value route on the bench's 106,200 windows (1,416 recordings x 15 windows x 5 bands, the inputs of
bench.py), HIP events around whole launches, medians of `reps` launches with their spread, in ONE run:
  kernel          the PLV kernel alone (engine.plv_dist_dev, distances only) on the 106,200 stacked windows
  kernel_pass     the same on 276,120 windows, a whole pass over the corpus (1,416 x 39 x 5), read in place through a window
                  table that walks the 106,200 resident windows 2.6 times: no second copy of the input; with the useful
                  float64 operations per second of the definition (2 n_ch n_t^2 for the circulant product, 8 n_t per channel
                  pair for the Gram sums) and of what the kernel issues (flops_executed) beside the chip's vector float64 rate
  stage           the `phase_locking` stage of run_step on a Workspace(phase_locking=True): PLV, Rips with its ladder, the
                  finishing pass, two Wasserstein launches, the 24 group means
  step_default / step_phase_locking   run_step of the same Workspace with the option off / on (eager, retry "one")
Writes profiles/plv_bench.json.
    python tools/plv_bench.py [n_rec] [reps]"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tda_eeg_audio_amd import _lib, engine, pipeline, synth      # noqa: E402

PER_REC, PER_REC_PASS = 15, 39
FP64_VECTOR_TFLOPS = 78.6        # MI355X data sheet: vector float64 (its matrix float64 rate is the same)


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


def flops(n_ch, n_t):
    return 2 * n_ch * n_t * n_t + 8 * n_t * (n_ch * (n_ch - 1) // 2)


def flops_executed(n_ch, n_t):
    """What the kernel issues: for an even n_t half of the circulant products are with the table's exact zeros and are left
    out; the Gram sums run over whole 2 x 4 tiles of the channels padded to a multiple of 4."""
    ncp = (n_ch + 3) // 4 * 4
    nbt = ncp // 4
    return (1 if n_t % 2 == 0 else 2) * n_ch * n_t * n_t + 8 * n_t * 8 * (nbt * nbt + nbt)


def kernel_alone(E, n_win, reps, ctx):
    n, n_ch, n_t = E.shape
    dev = E.device
    dist = torch.empty((n_win, n_ch, n_ch), dtype=torch.float64, device=dev)
    st = torch.empty(n_win, dtype=torch.int32, device=dev)
    if n_win == n:
        ts = timed(lambda: engine.plv_dist_dev(E, out=dist, status_t=st, ctx=ctx), reps)
    else:
        start = (torch.arange(n_win, device=dev) % n) * (n_ch * n_t)
        ld = torch.full_like(start, n_t)
        ts = timed(lambda: engine.plv_dist_dev(E.view(-1), n_t, start, ld, n_ch, out=dist, status_t=st, ctx=ctx), reps)
    assert int(st.max().item()) == 0 and bool(torch.isfinite(dist).all())
    ms = float(np.median(ts))
    f = flops(n_ch, n_t) * n_win
    fx = flops_executed(n_ch, n_t) * n_win
    return summary(ts, windows=n_win, flop_per_window=flops(n_ch, n_t), tflops=round(f / ms / 1e9, 3),
                   fraction_of_vector_fp64=round(f / ms / 1e9 / FP64_VECTOR_TFLOPS, 4),
                   flop_executed_per_window=flops_executed(n_ch, n_t), tflops_executed=round(fx / ms / 1e9, 3),
                   fraction_of_vector_fp64_executed=round(fx / ms / 1e9 / FP64_VECTOR_TFLOPS, 4),
                   us_per_window=round(1e3 * ms / n_win, 4),
                   bytes_read=n_win * n_ch * n_t * 8, bytes_written=n_win * (n_ch * n_ch * 8 + 4))


def main():
    n_rec = int(sys.argv[1]) if len(sys.argv) > 1 else 1416
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    ctx = _lib.get_ctx(0)
    dev = torch.device("cuda", 0)
    nb = len(synth.BANDS)
    aud = synth.corpus_audio(n_rec, PER_REC)
    A = torch.from_numpy(np.concatenate([aud[b].reshape(-1, 250) for b in synth.BANDS])).to(dev)
    E = torch.cat(synth.corpus_eeg_dev(np.arange(n_rec), PER_REC, nb, dev))
    n = A.shape[0]
    assert E.shape == (n, 47, 250)
    seg_off = np.arange(0, n + 1, PER_REC, dtype=np.int32)
    res = dict(tool="plv_bench", lib=os.path.basename(_lib.LIB_PATH), windows=int(n), reps=reps,
               fp64_vector_tflops=FP64_VECTOR_TFLOPS)
    res["kernel"] = kernel_alone(E, n, reps, ctx)
    res["kernel_pass"] = kernel_alone(E, n_rec * PER_REC_PASS * nb, reps, ctx)
    torch.cuda.empty_cache()
    ws = pipeline.Workspace(n, seg_off, dev, phase_locking=True)
    t_on = timed(lambda: pipeline.run_step(E, A, ws, ctx=ctx, retry="one"), reps)
    pl = ws.pl.cpu().numpy().copy()

    def stage():
        with ctx.deferred("one"):
            pipeline._phase_locking_stage(ws, ctx, E, None, None)
    t_stage = timed(stage, reps)
    res["stage"] = summary(t_stage)
    keep, ws.pl = ws.pl, None                                        # the same Workspace, the stage skipped
    t_off = timed(lambda: pipeline.run_step(E, A, ws, ctx=ctx, retry="one"), reps)
    ws.pl = keep
    res["step_phase_locking"] = summary(t_on)
    res["step_default"] = summary(t_off)
    res["pl_finite_columns_0_21"] = bool(np.isfinite(pl[:, :22]).all())
    res["pl_means"] = dict(h0_total_persistence=float(pl[:, 9].mean()), h1_n_features=float(pl[:, 11].mean()),
                           w_h0=float(np.nanmean(pl[:, 22])), w_h1=float(np.nanmean(pl[:, 23])))
    res["windows_flagged"] = int((ws.pl_st != 0).sum().item()) + int((ws.pl_dgm.status != 0).sum().item())
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "plv_bench.json"), "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({k: (v["ms_median"] if isinstance(v, dict) and "ms_median" in v else v) for k, v in res.items()
                      if k.startswith(("kernel", "stage", "step"))}))
    print(json.dumps({k: [res[k]["tflops"], res[k]["fraction_of_vector_fp64"], res[k]["spread"]] for k in ("kernel", "kernel_pass")}))


if __name__ == "__main__":
    main()
