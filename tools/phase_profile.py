#!/usr/bin/env python3
"""Phase-cycle breakdown of the Rips kernels (diagnostic build: make -C tda_eeg_audio_amd/csrc PROFILE=1)."""
import ctypes as C, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tda_eeg_audio_amd import _lib
# TDA_PROF_LIB=libtdaeeg_<name>.so: another diagnostic build in the same directory (an A/B of two trees)
_lib.LIB_PATH = os.path.join(ROOT, "tda_eeg_audio_amd", os.path.basename(os.environ.get("TDA_PROF_LIB", "libtdaeeg_prof.so")))
from tda_eeg_audio_amd import engine, synth
ctx = _lib.get_ctx(0)
lib = ctx.lib
buf = (C.c_ulonglong * 48)()
def tri_list(v):
    """the listing rounds of phase d (counters 43-47): every round, also those that end with an empty list"""
    r = max(v[47], 1)
    return (f"\n     listing rounds/win={v[47]/v[8]:.2f}: trips of the busiest lane/round={v[43]/r:.2f} "
            f"triangles/round={v[44]/r:.1f} waves with triangles/round={v[45]/r:.2f} "
            f"rounds that listed more than twice the capacity/win={v[46]/v[8]:.3f}")
NW = int(sys.argv[1]) if len(sys.argv) > 1 else 256      # 256 = one workgroup per CU (latency); 4096: CUs shared
if os.environ.get("TDA_CLASS_WORDS"):                      # e.g. "1,1": the first-pass widths bench.py uses
    ctx.set_class_words(*[int(x) for x in os.environ["TDA_CLASS_WORDS"].split(",")])
W_ = synth.eeg_windows(NW, seed=3)
dist_ = engine.corr_dist_batch(W_, want_corr=False, ctx=ctx)
engine.rips_dm_batch(dist_, ctx=ctx); lib.tda_profile_read(buf, 1)
engine.rips_dm_batch(dist_, ctx=ctx); lib.tda_profile_read(buf, 1)
v = np.array(list(buf), dtype=np.float64); n = v[8]
print(f"eeg: windows={int(n)} E/win={v[9]/n:.0f} cycles/win: keygen={v[0]/n:.0f} sort={v[1]/n:.0f} "
      f"sweep={v[3]/n:.0f} [mask={v[4]/n:.0f} candidates={v[5]/n:.0f} deps={v[6]/n:.0f} scan+kills={v[7]/n:.0f}] kills/win={v[10]/n:.1f} "
      f"list rounds/win={v[11]/n:.1f} entries/round={v[12]/max(v[11],1):.1f} overflow rounds/win={v[13]/n:.2f}\n     phase d: closure={v[16]/n:.0f} list={v[17]/n:.0f} reduce={(v[18]+v[30]+v[31])/n:.0f} (setup {v[30]/n:.0f} + kill loop {v[31]/n:.0f} + rows/barrier {v[18]/n:.0f}) table={v[19]/n:.0f} rest={v[7]/n:.0f}; candidates walked/win={v[20]/n:.0f} [phase b: to barrier={v[21]/n:.0f} walk={v[22]/n:.0f} publish={v[5]/n:.0f}] chunks/win={v[23]/n:.1f} shortened={v[14]/n:.2f} quiet={v[24]/n:.1f} scan rounds/win={v[41]/n:.2f} chunks started on a scan hit/win={v[42]/n:.2f} scans entered from a busy chunk/win={v[2]/n:.2f} ended early={v[25]/n:.2f}; triangles to test/win={v[27]/n:.0f} on {v[29]/n:.0f} of {v[28]/n:.0f} apparent edges; dependency rounds/win={v[32]/n:.1f} for {v[33]/n:.0f} in-chunk dependent edges in {v[34]/n:.1f} busy chunks; edges skipped to the next candidate/win={v[35]/n:.0f}" + tri_list(v))
for band in (os.environ.get("TDA_PROFILE_BANDS", "beta,delta").split(",")):
    wins = synth.audio_windows(NW, band, seed=1)
    tau = engine.tau_batch(wins[:1], 125, ctx=ctx)[0]
    engine.takens_rips_batch(wins, tau, ctx=ctx)
    lib.tda_profile_read(buf, 1)
    engine.takens_rips_batch(wins, tau, ctx=ctx)
    lib.tda_profile_read(buf, 1)
    v = np.array(list(buf), dtype=np.float64)
    n = v[8]
    print(f"audio {band} tau={tau}: windows={int(n)} E/win={v[9]/n:.0f} cycles/win: keygen={v[0]/n:.0f} sort={v[1]/n:.0f} "
          f"sweep={v[3]/n:.0f} [mask={v[4]/n:.0f} candidates={v[5]/n:.0f} deps={v[6]/n:.0f} scan+kills={v[7]/n:.0f}] kills/win={v[10]/n:.1f} "
          f"list rounds/win={v[11]/n:.1f} entries/round={v[12]/max(v[11],1):.1f} overflow rounds/win={v[13]/n:.2f}\n     phase d: closure={v[16]/n:.0f} list={v[17]/n:.0f} reduce={(v[18]+v[30]+v[31])/n:.0f} (setup {v[30]/n:.0f} + kill loop {v[31]/n:.0f} + rows/barrier {v[18]/n:.0f}) table={v[19]/n:.0f} rest={v[7]/n:.0f}; candidates walked/win={v[20]/n:.0f} [phase b: to barrier={v[21]/n:.0f} walk={v[22]/n:.0f} publish={v[5]/n:.0f}] chunks/win={v[23]/n:.1f} shortened={v[14]/n:.2f} quiet={v[24]/n:.1f} scan rounds/win={v[41]/n:.2f} chunks started on a scan hit/win={v[42]/n:.2f} scans entered from a busy chunk/win={v[2]/n:.2f} ended early={v[25]/n:.2f}; triangles to test/win={v[27]/n:.0f} on {v[29]/n:.0f} of {v[28]/n:.0f} apparent edges; dependency rounds/win={v[32]/n:.1f} for {v[33]/n:.0f} in-chunk dependent edges in {v[34]/n:.1f} busy chunks; edges skipped to the next candidate/win={v[35]/n:.0f}" + tri_list(v) +
          f"\n     ranks whose class vectors are needed/win={v[39]/n:.0f} of Ev={v[40]/n:.0f}; windows needing > 4096 / 4608 / 5120: {v[36]/n:.4f} / {v[37]/n:.4f} / {v[38]/n:.4f}")

# ---- Wasserstein phases on pipeline diagrams ----
W = synth.eeg_windows(256, seed=3)
aw = synth.audio_windows(256, "beta", seed=4)
dist = engine.corr_dist_batch(W, want_corr=False, ctx=ctx)
e0, ec0, e1, ec1, est = engine.rips_dm_batch(dist, ctx=ctx, raw=True)
a0, ac0, a1, ac1, npts, ast = engine.takens_rips_batch(aw, 3, ctx=ctx, raw=True)
pairs = {"H0 beta": (e0, ec0, a0, ac0), "H1 beta": (e1, ec1, a1, ac1)}
for band in ("delta", "theta", "alpha", "gamma"):                 # trimmed sizes and short cuts per band
    awb = synth.audio_windows(256, band, seed=4)
    taub = int(engine.tau_batch(awb[:1], 125, ctx=ctx)[0])
    b0_, bc0, b1_, bc1, _, _ = engine.takens_rips_batch(awb, taub, ctx=ctx, raw=True)
    pairs["H0 " + band] = (e0, ec0, b0_, bc0)
    pairs["H1 " + band] = (e1, ec1, b1_, bc1)
for name, (x, cx, y, cy) in pairs.items():
    engine.wasserstein_batch(x, cx, y, cy, ctx=ctx)
    lib.tda_profile_read_ws(buf, 1)
    engine.wasserstein_batch(x, cx, y, cy, ctx=ctx)
    lib.tda_profile_read_ws(buf, 1)
    v = np.array(list(buf), dtype=np.float64); n = v[4]
    print(f"wasserstein {name}: pairs={int(n)} rows={v[5]/n:.1f} cols={v[6]/n:.1f} cycles/pair: setup={v[0]/n:.0f} "
          f"solve={v[1]/n:.0f} total={v[2]/n:.0f}; dijkstra steps/pair={v[3]/n:.1f} -> {v[1]/max(v[3],1):.0f} cycles/step")
    if v[8]:
        print(f"     pruning: 1-D pairs={int(v[8])} live rows={v[9]/v[8]:.1f} live cols={v[10]/v[8]:.1f} (wavefront steps "
              f"{(v[9]+v[10])/v[8]-1:.1f} of {(v[5]+v[6])/n-1:.1f})")
    if n - v[8]:
        print(f"     pruning: all-diagonal short cuts={int(v[7])} of {int(n-v[8])} general pairs")
