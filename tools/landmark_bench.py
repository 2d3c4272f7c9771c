"""The landmark Rips route on the bench's 106,200 audio windows (all five bands, tau per recording-band as bench.py has
it), HIP events around whole launches, in ONE run:
  rips_audio_landmarks   the call the rips_audio stage of Workspace(takens=(3, 1, 128)) makes, into ws.aud / ws.lm, under
                         the step's policies (deferred H1 order, first pass + one widening pass)
  landmarks_alone        the landmark kernel alone on the same windows (engine.takens_landmarks_dev)
  rips_audio_default     the call the stage of the default Workspace makes (dim 3, subsample 2, every point)
and the distribution of r_cover per band.  Writes profiles/landmark_bench.json.
    python tools/landmark_bench.py [n_rec] [reps]"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tda_eeg_audio_amd import _lib, engine, pipeline, synth      # noqa: E402

TAKENS = (3, 1, 128)
PER_REC = 15


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


def main():
    n_rec = int(sys.argv[1]) if len(sys.argv) > 1 else 1416
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    ctx = _lib.get_ctx(0)
    dev = torch.device("cuda", 0)
    aud = synth.corpus_audio(n_rec, PER_REC)
    W = torch.from_numpy(np.concatenate([aud[b].reshape(-1, 250) for b in synth.BANDS])).to(dev)
    n = W.shape[0]
    seg_off = np.arange(0, n + 1, PER_REC, dtype=np.int32)
    ws_lm = pipeline.Workspace(n, seg_off, dev, takens=TAKENS)
    ws = pipeline.Workspace(n, seg_off, dev)
    for w in (ws_lm, ws):
        engine.tau_segments_dev(W, w.seg_off, 125, w.tau_seg, w.tau_win, ctx=ctx)
    dim, sub, n_perm = TAKENS
    alone = engine.DeviceLandmarks(n, n_perm, dim, dev)
    with ctx.deferred("one"):
        t_lm = timed(lambda: engine.takens_rips_landmarks_dev(W, ws_lm.tau_win, ws_lm.aud, ws_lm.lm, dim=dim, subsample=sub,
                                                              ctx=ctx), reps)
        t_alone = timed(lambda: engine.takens_landmarks_dev(W, ws_lm.tau_win, alone, dim=dim, subsample=sub, ctx=ctx), reps)
        t_def = timed(lambda: engine.takens_rips_dev(W, ws.tau_win, ws.aud, ctx=ctx), reps)
    assert alone.lm.cpu().numpy().tobytes() == ws_lm.lm.lm.cpu().numpy().tobytes()
    rc, n_full, n_lm = (t.cpu().numpy() for t in (ws_lm.lm.r_cover, ws_lm.lm.n_full, ws_lm.lm.n_lm))
    st_lm, st_def = ws_lm.aud.status.cpu().numpy(), ws.aud.status.cpu().numpy()
    bands = {}
    per_band = n // len(synth.BANDS)
    for bi, band in enumerate(synth.BANDS):
        sl = slice(bi * per_band, (bi + 1) * per_band)
        r, big = rc[sl], n_full[sl] > n_perm
        q = np.percentile(r[big], [0, 25, 50, 75, 100]).round(6).tolist() if big.any() else None
        bands[band] = dict(windows=int(per_band), points_min=int(n_full[sl].min()), points_max=int(n_full[sl].max()),
                           above_n_perm=int(big.sum()), r_cover_min_q25_median_q75_max=q)
    med = lambda t: float(np.median(t))                          # noqa: E731
    res = dict(tool="landmark_bench", lib=os.path.basename(_lib.LIB_PATH), windows=int(n), takens=list(TAKENS), reps=reps,
               policies="deferred H1 order, first pass + one widening pass (pipeline.run_step)",
               ms_median=dict(rips_audio_landmarks=med(t_lm), landmarks_alone=med(t_alone), rips_audio_default=med(t_def)),
               ms_all=dict(rips_audio_landmarks=t_lm, landmarks_alone=t_alone, rips_audio_default=t_def),
               us_per_window=dict(rips_audio_landmarks=round(1e3 * med(t_lm) / n, 4), landmarks_alone=round(1e3 * med(t_alone) / n, 4),
                                  rips_audio_default=round(1e3 * med(t_def) / n, 4)),
               landmarks_mean=float(n_lm.mean()), points_mean=float(n_full.mean()),
               status_left_landmarks=int(((st_lm & ~_lib.TDA_WIN_DEGENERATE) != 0).sum()),
               status_left_default=int(((st_def & ~_lib.TDA_WIN_DEGENERATE) != 0).sum()),
               r_cover_per_band=bands)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "landmark_bench.json"), "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res["ms_median"]), json.dumps(res["us_per_window"]))


if __name__ == "__main__":
    main()
