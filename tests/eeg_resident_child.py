"""The RES = true family of the fused EEG kernel (eeg_window_kernel<3, true, ...>, eeg_window_ragged_kernel<3, true, ...> and
the last rung behind them): the window stays in registers between the two passes of cd_window_products.  The library
selects it with TDA_EEG_RESIDENT, read once per process, so tests/test_gpu_eeg_shapes.py starts this script in a fresh
child with the variable set:

    TDA_EEG_RESIDENT=1 python tests/eeg_resident_child.py

A cut of the fused grid of tests/eeg_shape_cases.py -- 33, 47 and 48 channels, 2, 9, 33, 250 and 256 samples -- through the
three window sources and the three first-pass widths (32, 64, 128 class bits: the RES retry kernels run behind the narrow
ones), then the 48-channel batch with more than 512 classes alive at once through the three sources.  Everything equals
corr_dist_dev + rips_dm_dev, which do not read the variable, and those equal the oracle.

Prints "RESIDENT OK cases <n>"; exits 1 on a mismatch, 2 when the variable is not set."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.dirname(HERE)]

import eeg_shape_cases as sc                                    # noqa: E402
from oracle import brute                                        # noqa: E402


def _same_multiset(a, b):
    return np.array_equal(brute.sort_rows(a), brute.sort_rows(b))


def _sources(engine, ctx, W, h1_cap):
    """The three window sources on the stack W (8 windows): [(name, run)], run() -> (diagrams, dist, corr, order)."""
    import torch
    dev = torch.device("cuda", ctx.device)
    n, n_ch, n_t = W.shape
    sig, packed, start, ld, order = sc.as_recordings(W)
    wt, sig_t, packed_t = (sc.to_device(x, dev) for x in (W, sig, packed))
    start_t, ld_t = torch.from_numpy(start).to(dev), torch.from_numpy(ld).to(dev)

    def mats():
        d = torch.full((n, n_ch, n_ch), -7.0, dtype=torch.float64, device=dev)
        return d, torch.full_like(d, -7.0)

    def stacked():
        d, c = mats()
        return engine.eeg_window_dev(wt, h1_cap=h1_cap, dist_t=d, corr_t=c, ctx=ctx), d, c, np.arange(n)

    def sliding():
        d, c = mats()
        return engine.eeg_window_sliding_dev(sig_t, n_t, n_t, h1_cap=h1_cap, dist_t=d, corr_t=c, ctx=ctx)[0], d, c, np.arange(n)

    def table():
        d, c = mats()
        return engine.eeg_window_ragged_dev(packed_t, start_t, ld_t, n_t, h1_cap=h1_cap, dist_t=d, corr_t=c, n_ch=n_ch,
                                            ctx=ctx), d, c, order

    return wt, [("stacked", stacked), ("sliding", sliding), ("table", table)]


def _reference(engine, ctx, wt, h1_cap):
    """corr_dist_dev + rips_dm_dev (no variable read there), checked against the oracle."""
    import torch
    from oracle import port
    dist = torch.empty((wt.shape[0], wt.shape[1], wt.shape[1]), dtype=torch.float64, device=wt.device)
    corr = torch.empty_like(dist)
    engine.corr_dist_dev(wt, dist, corr, ctx=ctx)
    two = engine.rips_dm_dev(dist, h1_cap=h1_cap, ctx=ctx)
    torch.cuda.synchronize()
    b0, b1 = two.to_lists()
    oc, od = port.corr_dist_batch(wt.cpu().numpy())
    ok = int(two.status.max()) == 0 and np.array_equal(dist.cpu().numpy(), od) and np.array_equal(corr.cpu().numpy(), oc)
    for w in range(wt.shape[0]):
        o = port.rips_dm(od[w])
        ok = ok and _same_multiset(b0[w], o[0]) and _same_multiset(b1[w], o[1])
    return ok, dist, corr, two


def _check(run, dist, corr, two):
    import torch
    got, d, c, order = run()
    torch.cuda.synchronize()
    idx = torch.from_numpy(np.asarray(order)).to(dist.device)
    ref = two.head(two.n_win)
    ref.h0, ref.h1, ref.c0, ref.c1, ref.status = two.h0[idx], two.h1[idx], two.c0[idx], two.c1[idx], two.status[idx]
    return sc.same_diagrams(got, ref) and sc.bytes_equal(d, dist[idx]) and sc.bytes_equal(c, corr[idx])


def main():
    if not os.environ.get("TDA_EEG_RESIDENT"):
        print("TDA_EEG_RESIDENT is not set: this process would run the streaming family")
        return 2
    from tda_eeg_audio_amd import _lib, engine
    ctx = _lib.get_ctx(0)
    n = bad = 0
    for n_ch in sc.RESIDENT_CH:
        for n_t in sc.RESIDENT_LENGTHS:
            wt, sources = _sources(engine, ctx, sc.windows(n_ch, n_t), engine.DEFAULT_H1_CAP)
            ref_ok, dist, corr, two = _reference(engine, ctx, wt, engine.DEFAULT_H1_CAP)
            for name, run in sources:
                for words in (0, 1, 2):
                    ctx.set_class_words(words, 1)
                    try:
                        ok = _check(run, dist, corr, two)
                    finally:
                        ctx.set_class_words(2, 1)
                    n += 1
                    if not (ok and ref_ok):
                        bad += 1
                        print(f"MISMATCH n_ch={n_ch} n_t={n_t} {name} first-pass words={words} (reference ok: {ref_ok})")
    # the last rung of the fused ladder behind the resident kernels
    W, _ = sc.batch_48()
    wt, sources = _sources(engine, ctx, W, 1024)
    ref_ok, dist, corr, two = _reference(engine, ctx, wt, 1024)
    for name, run in sources:
        ok = _check(run, dist, corr, two)
        n += 1
        if not (ok and ref_ok):
            bad += 1
            print(f"MISMATCH 48-channel batch with more than 512 classes, {name} (reference ok: {ref_ok})")
    if bad:
        print(f"RESIDENT FAILED {bad} of {n} cases")
        return 1
    print(f"RESIDENT OK cases {n}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
