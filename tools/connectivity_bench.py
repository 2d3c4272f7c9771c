"""The analytic-signal connectivity kernels on the bench's 106,200 windows of 47 x 250 (1,416 recordings x 15 windows x 5
bands, the inputs of bench.py), each measure's kernel alone (engine.connectivity_dist_dev, distances only) beside
plv_dist_kernel (engine.plv_dist_dev) on the same input in the same run: HIP events around whole launches, medians of `reps`
launches after 2 warm-ups with their spread, and the float64 operations a window issues beside the chip's vector rate.
Writes profiles/connectivity_bench.json.
    python tools/connectivity_bench.py [n_rec] [reps]"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tda_eeg_audio_amd import _lib, engine, synth      # noqa: E402

PER_REC = 15
FP64_VECTOR_TFLOPS = 78.6        # MI355X data sheet: vector float64
# float64 operations per pair and sample in the pair sums (an fma counts 2): wpli 2 mul + sub + 2 add; imcoh / coh the
# same s and one add, two fmas for R; aec one fma; plv four fmas
PAIR_OPS = {"wpli": 5, "imcoh": 8, "coh": 8, "aec": 2, "plv": 8}
PAIR_INSTR = {"wpli": 5, "imcoh": 6, "coh": 6, "aec": 1, "plv": 4}


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


def issued(name, n_ch, n_t):
    """(float64 operations, float64 instructions) a window issues: the Hilbert chains (for an even n_t the products with the
    table's exact zeros are left out), the pair sums over whole 2 x 4 tiles of the channels padded to a multiple of 4, the
    per-channel sums, and for aec the 6 subtractions of the shifts per tile and sample."""
    ncp = (n_ch + 3) // 4 * 4
    nbt = ncp // 4
    tiles = nbt * nbt + nbt
    chain = (1 if n_t % 2 == 0 else 2) * n_ch * n_t * n_t // 2          # fmas
    ops = 2 * chain + PAIR_OPS[name] * 8 * tiles * n_t
    ins = chain + PAIR_INSTR[name] * 8 * tiles * n_t
    if name == "aec":
        ops += (6 * tiles + 4 * n_ch) * n_t
        ins += (6 * tiles + 3 * n_ch) * n_t
    elif name != "plv":
        ops += 4 * n_ch * n_t
        ins += 2 * n_ch * n_t
    return ops, ins


def main():
    n_rec = int(sys.argv[1]) if len(sys.argv) > 1 else 1416
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    ctx = _lib.get_ctx(0)
    dev = torch.device("cuda", 0)
    E = torch.cat(synth.corpus_eeg_dev(np.arange(n_rec), PER_REC, len(synth.BANDS), dev))
    n, n_ch, n_t = E.shape
    assert (n_ch, n_t) == (47, 250)
    dist = torch.empty((n, n_ch, n_ch), dtype=torch.float64, device=dev)
    st = torch.empty(n, dtype=torch.int32, device=dev)
    res = dict(tool="connectivity_bench", lib=os.path.basename(_lib.LIB_PATH), windows=int(n), reps=reps,
               fp64_vector_tflops=FP64_VECTOR_TFLOPS)
    calls = {"plv": lambda: engine.plv_dist_dev(E, out=dist, status_t=st, ctx=ctx)}
    for m in engine.CONNECTIVITY_MEASURES:
        calls[m] = (lambda m=m: engine.connectivity_dist_dev(E, measure=m, out=dist, status_t=st, ctx=ctx))
    for name, fn in calls.items():
        ts = timed(fn, reps)
        assert int(st.max().item()) == 0 and bool(torch.isfinite(dist).all())
        ms = float(np.median(ts))
        ops, ins = issued(name, n_ch, n_t)
        res[name] = dict(ms_all=ts, ms_median=ms, ms_min=min(ts), ms_max=max(ts), spread=round((max(ts) - min(ts)) / ms, 4),
                         us_per_window=round(1e3 * ms / n, 4), flop_issued_per_window=ops, fp64_instructions_per_window=ins,
                         tflops_issued=round(ops * n / ms / 1e9, 3),
                         fraction_of_vector_fp64=round(ops * n / ms / 1e9 / FP64_VECTOR_TFLOPS, 4))
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "connectivity_bench.json"), "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({k: [v["ms_median"], v["spread"], v["tflops_issued"]] for k, v in res.items() if isinstance(v, dict)}))


if __name__ == "__main__":
    main()
