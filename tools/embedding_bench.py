"""The delay and dimension selection on the bench's 106,200 audio windows (1,416 recordings x 15 windows x 5 bands, the
inputs of bench.py), HIP events around whole launches, two warm-ups and the median of `reps` launches with their spread:
  ami / ami_segments   engine.ami_dev (max_lag 62, 16 bins: 63 lags of every window) and engine.ami_segments_dev (the
                       delay of the 7,080 (recording, band) groups from their first windows, ending at the first minimum)
  fnn                  engine.fnn_dev (d_max 5, theiler 1, the delays of ami_segments), with the pair evaluations it made
                       read off its own inputs: per window M_1^2 pairs (i, j), M_1 = 250 - tau, each carried through up to
                       d_max dimensions
  tau / takens_rips    engine.tau_dev (the autocorrelation delay the AMI one stands beside) and engine.takens_rips_dev on
                       the same windows, the stage the two parameters feed, for scale
Every step is a child process of its own under a time limit of its own; after a step that fails or runs out of time no
further step is started, and the file says which steps were and were not measured.  There is no speed gate.  Writes
profiles/embedding_bench.json, or `out`.
    python tools/embedding_bench.py [n_rec] [reps] [out]"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PER_REC, MAX_LAG, N_BINS, D_MAX, THEILER = 15, 62, 16, 5, 1
STEPS = (("ami", 240), ("fnn", 240), ("tau", 240), ("takens_rips", 240))


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
    tau_seg = torch.empty(n // PER_REC, dtype=torch.int32, device=dev)
    tau_w = torch.empty(n, dtype=torch.int32, device=dev)
    res = {}
    if name == "ami":
        out = engine.DeviceEmbedding(n, MAX_LAG + 1, 0, dev)
        ts = timed(lambda: engine.ami_dev(A, MAX_LAG, N_BINS, out=out, ctx=ctx), reps)
        ms = float(np.median(ts))
        tau = out.tau.cpu().numpy()
        res["ami"] = summary(ts, windows=int(n), lags=MAX_LAG + 1, windows_flagged=int((out.ami_status != 0).sum().item()),
                             windows_without_minimum=int((tau == 0).sum()), tau_median=float(np.median(tau[tau > 0])),
                             mean_ami_at_lag_0=float(out.ami[:, 0].mean().item()),
                             m_sample_pairs_per_s=round(n * sum(250 - L for L in range(MAX_LAG + 1)) / ms / 1e3, 1),
                             us_per_window=round(1e3 * ms / n, 4))
        ts = timed(lambda: engine.ami_segments_dev(A, seg_t, MAX_LAG, N_BINS, tau_seg, tau_w, ctx=ctx), reps)
        res["ami_segments"] = summary(ts, groups=int(tau_seg.numel()), tau_median=float(tau_seg.double().median().item()))
    elif name == "fnn":
        engine.ami_segments_dev(A, seg_t, MAX_LAG, N_BINS, tau_seg, tau_w, ctx=ctx)
        out = engine.DeviceEmbedding(n, 0, D_MAX, dev)
        ts = timed(lambda: engine.fnn_dev(A, tau_w, D_MAX, THEILER, out=out, ctx=ctx), reps)
        ms = float(np.median(ts))
        m1 = (250 - tau_w.long()).clamp(min=0)
        pairs = int((m1 * m1).sum().item())
        dims = torch.bincount(out.dim, minlength=D_MAX + 1).tolist()
        res["fnn"] = summary(ts, windows=int(n), d_max=D_MAX, theiler=THEILER,
                             windows_flagged=int((out.fnn_status != 0).sum().item()), pairs=pairs,
                             g_pairs_per_s=round(pairs / ms / 1e6, 3), windows_by_dim=dims,
                             mean_fraction=[round(v, 4) for v in out.frac.mean(0).tolist()], us_per_window=round(1e3 * ms / n, 4))
    elif name == "tau":
        ts = timed(lambda: engine.tau_dev(A, 125, tau_w, ctx=ctx), reps)
        res["tau"] = summary(ts, windows=int(n), us_per_window=round(1e3 * float(np.median(ts)) / n, 4))
    elif name == "takens_rips":
        engine.tau_segments_dev(A, seg_t, 125, tau_win_t=tau_w, ctx=ctx)
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
    out_path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "embedding_bench.json")
    res = dict(tool="embedding_bench", windows=n_rec * PER_REC * 5, reps=reps, warmups=2, max_lag=MAX_LAG, n_bins=N_BINS,
               d_max=D_MAX, theiler=THEILER, measured=[], not_measured=[])
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
    for a, b in (("ami", "takens_rips"), ("fnn", "takens_rips"), ("ami", "tau"), ("ami_segments", "tau")):
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
