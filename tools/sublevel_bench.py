"""The sublevel-set persistence on the bench's 106,200 windows (1,416 recordings x 15 windows x 5 bands, the inputs of
bench.py), HIP events around whole launches, in ONE run:
  kernel_eeg      the sublevel kernel alone on the EEG windows, 47 signals per window (engine.sublevel_dev), every diagram
                  kept: bytes read (samples) and written (rows, counts, status words) per second beside the HBM copy rate
  kernel_audio    the same on the audio windows, one signal per window
  stage_sublevel  the `sublevel` stage of run_step on a Workspace(sublevel=True): both signal kinds through the bounded
                  scratch (sublevel + features launch per chunk), channel means, the 22 group means
  step_default / step_sublevel   run_step of the same Workspace with the option off / on (eager, retry "one")
Writes profiles/sublevel_bench.json.
    python tools/sublevel_bench.py [n_rec] [reps]"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tda_eeg_audio_amd import _lib, engine, pipeline, synth      # noqa: E402

PER_REC = 15
HBM_COPY_TBS = 6.29              # measured float4 copy on an MI355X (79 % of the 8 TB/s peak)


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


def kernel_alone(sig_t, reps, ctx):
    """The kernel on (n_win, n_ch, n_t) with buffers for every diagram: times, bytes, rows."""
    n_win, n_ch, n_t = sig_t.shape
    n_sig, cap = n_win * n_ch, engine.sublevel_rows(n_t)
    dgm = torch.empty((n_sig, cap, 2), dtype=torch.float64, device=sig_t.device)
    cnt = torch.empty(n_sig, dtype=torch.int32, device=sig_t.device)
    st = torch.empty(n_sig, dtype=torch.int32, device=sig_t.device)
    ts = timed(lambda: engine.sublevel_dev(sig_t, dgm_t=dgm, cnt_t=cnt, status_t=st, ctx=ctx), reps)
    rows = int(cnt.sum().item())
    assert int(st.max().item()) == 0
    rd, wr = n_sig * n_t * 8, rows * 16 + n_sig * 8
    ms = float(np.median(ts))
    return dict(signals=n_sig, n_t=n_t, ms_all=ts, ms_median=ms, rows_mean=round(rows / n_sig, 3), bytes_read=rd,
                bytes_written=wr, tb_per_s=round((rd + wr) / ms / 1e9, 4),
                fraction_of_hbm_copy=round((rd + wr) / ms / 1e9 / HBM_COPY_TBS, 4), ns_per_signal=round(1e6 * ms / n_sig, 3))


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
    res = dict(tool="sublevel_bench", lib=os.path.basename(_lib.LIB_PATH), windows=int(n), reps=reps,
               hbm_copy_tb_per_s=HBM_COPY_TBS, scratch_bytes=engine.SL_SCRATCH_BYTES)
    res["kernel_eeg"] = kernel_alone(E, reps, ctx)
    res["kernel_audio"] = kernel_alone(A.view(n, 1, 250), reps, ctx)
    torch.cuda.empty_cache()
    ws = pipeline.Workspace(n, seg_off, dev, sublevel=True)
    t_stage = timed(lambda: pipeline._sublevel_stage(ws, ctx, E, A, None, None), reps)
    sc = ws.sl_scratch[(47, 250)]
    res["stage_sublevel"] = dict(ms_all=t_stage, ms_median=float(np.median(t_stage)), chunk_windows=sc.chunk_windows,
                                 chunks_eeg=sc.n_chunks(n), chunks_audio=ws.sl_scratch[(1, 250)].n_chunks(n))
    t_on = timed(lambda: pipeline.run_step(E, A, ws, ctx=ctx, retry="one"), reps)
    sl = ws.sl.cpu().numpy().copy()
    ws.sublevel = False                                              # the same Workspace, the stage skipped
    t_off = timed(lambda: pipeline.run_step(E, A, ws, ctx=ctx, retry="one"), reps)
    res["step_sublevel"] = dict(ms_all=t_on, ms_median=float(np.median(t_on)))
    res["step_default"] = dict(ms_all=t_off, ms_median=float(np.median(t_off)))
    res["sl_finite"] = bool(np.isfinite(sl).all())
    res["sl_mean_rows"] = dict(audio_n_features=float(sl[:, 0].mean()), eeg_n_features=float(sl[:, 11].mean()))
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "sublevel_bench.json"), "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({k: (v["ms_median"] if isinstance(v, dict) and "ms_median" in v else v) for k, v in res.items()
                      if k.startswith(("kernel", "stage", "step"))}))
    print(json.dumps({k: res[k]["tb_per_s"] for k in ("kernel_eeg", "kernel_audio")}))


if __name__ == "__main__":
    main()
