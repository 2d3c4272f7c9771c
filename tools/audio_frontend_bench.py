#!/usr/bin/env python3
"""
tools/audio_frontend_bench.py -- the ragged 44.1 kHz audio front end on the study's REAL length column, one JSON line:
    python3 tools/audio_frontend_bench.py [--runs 3] [--recordings N] [--loop-recordings M] [--no-pass]
Recording r of tests/golden/corpus_n_samples.npy (L_r EEG samples) gets La_r = L_r * 882 // 5 synthetic audio samples,
which resample to exactly L_r envelope samples (1,416 recordings: sum La = 1.06 G samples, 8.48 GB float64).
  front_end   audio resident in HBM: preprocess.envelopes_ragged_dev (ragged resampler, ragged Hilbert envelope,
              low-pass; one launch each) per corpus; beside it, in the same process, the same signals through the
              per-signal kernels (tda_upfirdn_dev, tda_hilbert_envelope_dev, tda_filtfilt_dev) in a loop over the first
              --loop-recordings recordings, scaled to the corpus; achieved FLOP/s against the fp64 vector peak (spec).
  pass        recordings.RaggedAudioRecordingPass from pinned host EEG + audio: window pairs/s, ms per run, H2D GB/s;
              beside it recordings.RaggedRecordingPass fed the envelopes of the same audio.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FP64_VECTOR_PEAK_SPEC = 78.6e12        # MI355X fp64 vector, FLOP/s (datasheet value, not measured)


def pinned_randn(n, seed, chunk=1 << 26):
    import torch
    g = torch.Generator(device="cpu")
    g.manual_seed(seed)
    out = torch.empty(n, dtype=torch.float64).pin_memory()
    for o in range(0, n, chunk):
        m = min(chunk, n - o)
        out[o:o + m].copy_(torch.randn(m, generator=g, dtype=torch.float64))
    return out


def timed(fn, runs):
    import torch
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(runs):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / runs


def per_signal_loop(ctx, x_t, P, n_rec, b, a):
    """The per-signal _dev kernels of resample_audio / compute_envelope, one recording after the other."""
    import torch
    from scipy import signal
    from tda_eeg_audio_amd import preprocess
    h = torch.from_numpy(P.h).to(x_t.device)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    zi = np.ascontiguousarray(signal.lfilter_zi(b, a))
    ntaps = len(b)
    Lmax = int(P.n_out[:n_rec].max())
    rs = torch.empty(Lmax, dtype=torch.float64, device=x_t.device)
    hil, env = torch.empty_like(rs), torch.empty_like(rs)
    work = torch.empty(Lmax + 6 * ntaps, dtype=torch.float64, device=x_t.device)
    gs = {int(n): torch.from_numpy(preprocess._hilbert_g(int(n))).to(x_t.device) for n in np.unique(P.n_out[:n_rec])}
    bb, aa = np.ascontiguousarray(b, dtype=np.float64), np.ascontiguousarray(a, dtype=np.float64)

    def run():
        for r in range(n_rec):
            n_in, n_out = int(P.La[r]), int(P.n_out[r])
            xp = C.c_void_p(x_t.data_ptr() + 8 * int(P.in_tb.off_h[r]))
            ctx.check(ctx.lib.tda_upfirdn_dev(ctx.h, xp, n_in, C.c_void_p(h.data_ptr()), len(P.h), P.up, P.down, P.n_pre_remove,
                                              n_out, C.c_void_p(rs.data_ptr()), st))
            ctx.check(ctx.lib.tda_hilbert_envelope_dev(ctx.h, C.c_void_p(rs.data_ptr()), n_out, C.c_void_p(gs[n_out].data_ptr()),
                                                       C.c_void_p(hil.data_ptr()), st))
            ctx.check(ctx.lib.tda_filtfilt_dev(ctx.h, C.c_void_p(hil.data_ptr()), 1, n_out, preprocess.ptr(bb), preprocess.ptr(aa),
                                               preprocess.ptr(zi), ntaps, 3 * ntaps, C.c_void_p(env.data_ptr()),
                                               C.c_void_p(work.data_ptr()), st))
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--recordings", type=int, default=None, help="the first N recordings of the corpus (default all)")
    ap.add_argument("--loop-recordings", type=int, default=200, help="recordings timed through the per-signal kernels")
    ap.add_argument("--no-pass", action="store_true", help="front end only")
    a = ap.parse_args()
    import torch
    from tda_eeg_audio_amd import _lib, preprocess, recordings
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    ctx = _lib.get_ctx(0)
    L = np.load(os.path.join(ROOT, "tests", "golden", "corpus_n_samples.npy")).astype(np.int64)
    if a.recordings:
        L = L[:a.recordings]
    La = L * 882 // 5
    P = preprocess.AudioPlan(La).upload(dev)
    assert np.array_equal(P.n_out, L)
    audio_h = pinned_randn(int(La.sum()), 4410)
    out = {"recordings": len(L), "audio_samples": int(La.sum()), "audio_GB": La.sum() * 8 / 1e9}

    # ---- front end alone, audio resident in HBM ----
    x_t = audio_h.to(dev)
    env_t = torch.empty(int(L.sum()), dtype=torch.float64, device=dev)
    work_t = torch.empty(3 * int(L.sum()) + 30 * len(L), dtype=torch.float64, device=dev)
    dt = timed(lambda: preprocess.envelopes_ragged_dev(x_t, P, out_t=env_t, work_t=work_t, ctx=ctx), a.runs)
    macs_rs = float(L.sum()) * 17641 / 5                     # nonzero taps per output (the Kaiser filter over up)
    macs_hb = float((L.astype(np.float64) ** 2).sum())
    flops = 2 * (macs_rs + macs_hb)
    b, a_ = preprocess.envelope_lowpass(250)
    n_loop = min(a.loop_recordings, len(L))
    dt_loop = timed(per_signal_loop(ctx, x_t, P, n_loop, b, a_), 1)
    share = float(La[:n_loop].sum() / La.sum())
    loop_corpus = dt_loop / share
    out["front_end"] = {"ms_per_corpus": dt * 1e3, "fp64_multiply_adds": macs_rs + macs_hb, "resample_macs": macs_rs,
                        "hilbert_macs": macs_hb, "achieved_TFLOPs": flops / dt / 1e12,
                        "share_of_fp64_vector_peak_spec": flops / dt / FP64_VECTOR_PEAK_SPEC,
                        "per_signal_loop": {"recordings": n_loop, "ms": dt_loop * 1e3, "ms_per_corpus_scaled": loop_corpus * 1e3},
                        "speedup_vs_per_signal": loop_corpus / dt}
    out["value"], out["unit"] = dt * 1e3, "ms per corpus (front end, HBM-resident)"
    env_ref = env_t.clone()
    del x_t, work_t
    torch.cuda.synchronize()

    # ---- the pass from host memory ----
    if not a.no_pass:
        raw_h = pinned_randn(47 * int(L.sum()), 909)
        rp = recordings.RaggedAudioRecordingPass(L, La, dev, ctx=ctx)
        rows = torch.empty((len(L), 5, 48), dtype=torch.float64).pin_memory()
        dtp = timed(lambda: rp.run(raw_h, audio_h, rows), a.runs)
        n_pairs = int(rp.plan.k.sum()) * len(rp.bands)
        nbytes = (raw_h.numel() + audio_h.numel()) * 8
        out["pass"] = {"window_pairs_per_s": n_pairs / dtp, "ms_per_run": dtp * 1e3, "h2d_GBps": nbytes / dtp / 1e9,
                       "h2d_GB": nbytes / 1e9, "shards": len(rp.plan.shards), "window_pairs": n_pairs,
                       "rows_finite_share": float(torch.isfinite(rows[:, :, :2]).float().mean()), "repairs": rp.repairs}
        del rp
        env_h = torch.empty(env_ref.numel(), dtype=torch.float64).pin_memory()
        env_h.copy_(env_ref.cpu())
        re = recordings.RaggedRecordingPass(L, L, dev, ctx=ctx)
        rows_e = torch.empty_like(rows)
        dte = timed(lambda: re.run(raw_h, env_h, rows_e), a.runs)
        be = (raw_h.numel() + env_h.numel()) * 8
        out["envelope_pass"] = {"window_pairs_per_s": n_pairs / dte, "ms_per_run": dte * 1e3, "h2d_GBps": be / dte / 1e9,
                                "shards": len(re.plan.shards)}
        out["pass_rows_equal_envelope_pass"] = bool(np.array_equal(rows.numpy(), rows_e.numpy(), equal_nan=True))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
