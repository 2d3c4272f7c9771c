"""
The temporal correlation of the H1 feature series (cmp:90-91,104-114) on the device, through every layer:
features.hip::temporal_corr_kernel against scipy.stats.spearmanr and engine.spearman_batch on crafted groups, the step
(pipeline.Workspace(correlations=True), eager and replayed from a graph), the batched passes of recordings.py against
drivers.process_recording_arrays on every recording alone, and drivers.run_comparison's files.
The bars |r - r_scipy| < 1e-12 and |p - p_scipy| < 1e-10 are the project's for this quantity
(test_gpu_mirror.py::test_spearman_matches_scipy).  One pass per class of pass and module: the Rips retry lists are keyed
by stream.
"""
import json
import os

import numpy as np
import pytest
from scipy import signal
from scipy.stats import spearmanr

from tda_eeg_audio_amd import drivers, engine, pipeline, preprocess, recordings, synth, utils

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CORPUS = np.load(os.path.join(HERE, "golden", "corpus_n_samples.npy"))
FIX = [int(CORPUS.min()), int(CORPUS.max())] + [int(v) for v in np.unique(CORPUS)[[5, 17, 29, 40]]]
SKIP = 4 | 16                      # TDA_WIN_DEGENERATE | TDA_WIN_TOO_LARGE
COLS = engine.SPEARMAN_COLS


def _scipy_cell(x, y):
    """cmp:110-114 on one pair of series."""
    if len(x) >= 5 and np.std(x) > 1e-10 and np.std(y) > 1e-10:
        r, p = spearmanr(x, y)
        return float(r), float(p)
    return 0.0, 1.0


def _check_against_scipy(out, fa, fe, seg, status, label=""):
    """Every group and column of out (n_seg, 10) against scipy on the compacted series; returns the number of cells that
    were not under the guard."""
    free = 0
    for s in range(len(seg) - 1):
        a, b = int(seg[s]), int(seg[s + 1])
        keep = np.ones(b - a, bool) if status is None else (status[a:b] & SKIP) == 0
        if not keep.any():
            assert np.isnan(out[s]).all(), (label, s)
            continue
        for k, c in enumerate(COLS):
            x, y = fa[a:b, c][keep], fe[a:b, c][keep]
            rr, pp = _scipy_cell(x, y)
            r, p = out[s, 2 * k], out[s, 2 * k + 1]
            print(label, "group", s, "m", int(keep.sum()), "col", c, "r", r, rr, "p", p, pp)
            assert abs(r - rr) < 1e-12 and abs(p - pp) < 1e-10, (label, s, k, r, rr, p, pp)
            if abs(r) == 1.0:
                assert p == 0.0, (label, s, k)
            free += (rr, pp) != (0.0, 1.0)
    return free


# ------------------------------------------------------------------------------------------------ 1. the kernel
def _crafted():
    rng = np.random.default_rng(77)
    sizes, masks = [], []

    def group(n, mask=None):
        sizes.append(n)
        masks.append(np.zeros(n, np.int32) if mask is None else np.asarray(mask, np.int32))

    for n in (3, 5, 15, 64, 65, 89, 200):                      # plain
        group(n)
    for n in (15, 64, 65, 89, 200):                            # scattered: bits 4, 16, both; 1, 2 and 8 do not skip a window
        m = rng.choice([0, 0, 0, 4, 16, 20, 1, 2, 8, 5], size=n).astype(np.int32)
        group(n, m)
    m = np.full(15, 4, np.int32); m[[2, 7, 9, 14]] = 0         # fewer than 5 survivors
    group(15, m)
    m = np.full(89, 16, np.int32); m[-9:] = [0, 1, 0, 2, 0, 0, 8, 0, 0]     # survivors only at the end
    group(89, m)
    m = np.full(200, 20, np.int32); m[-70:] = 0                # ... of a long group: 70 at the end
    group(200, m)
    group(15, np.full(15, 4, np.int32))                        # covered altogether
    group(70, np.full(70, 16, np.int32))
    m = np.zeros(200, np.int32); m[::3] = 4                    # 133 survivors: more than the staged 128
    group(200, m)
    group(0)                                                   # an empty group
    seg = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    n = int(seg[-1])
    fa, fe = rng.random((n, 11)), rng.random((n, 11))
    fa[:, 0] = np.round(fa[:, 0] * 6); fe[:, 0] = np.round(fe[:, 0] * 6)          # n_features: integers, many ties
    for s in range(len(sizes)):
        a, b = seg[s], seg[s + 1]
        if s % 4 == 1:
            fe[a:b, 9] = fa[a:b, 9]                            # identical: r = 1, p = 0
        if s % 4 == 2:
            fe[a:b, 8] = 1.0 - fa[a:b, 8]                      # reversed: r = -1
        if s % 4 == 3:
            fa[a:b, 6] = 0.25                                  # constant: guarded
        if s % 5 == 0:
            fe[a:b, 10] = np.round(fe[a:b, 10] * 3) / 3        # ties in one series only
    return fa, fe, seg, np.concatenate(masks)


def test_kernel_matches_scipy_and_spearman_batch(ctx):
    import torch
    fa, fe, seg, status = _crafted()
    out = engine.temporal_corr_batch(fa, fe, seg, status, ctx=ctx)
    assert out.shape == (len(seg) - 1, 10)
    free = _check_against_scipy(out, fa, fe, seg, status, "crafted")
    assert free > 5 * 12
    # r bit-equal to spearman_kernel on the compacted series
    keep = (status & SKIP) == 0
    m = np.array([keep[seg[s]:seg[s + 1]].sum() for s in range(len(seg) - 1)])
    seg_c = np.concatenate([[0], np.cumsum(m)]).astype(np.int32)
    r_c, _ = engine.spearman_batch(fa[keep], fe[keep], seg_c, ctx=ctx)
    live = m > 0
    assert np.array_equal(out[live][:, 0::2], r_c[live])
    assert np.isnan(out[~live]).all() and (~live).sum() == 3
    short = (m > 0) & (m < 5)
    assert short.sum() == 2 and (out[short][:, 0::2] == 0).all() and (out[short][:, 1::2] == 1).all()
    # the ends: identical and reversed series (p is exactly 0 where r is exactly +-1: _check_against_scipy)
    ends = out[live & (m >= 5)][:, 0::2]
    assert (ends > 1 - 1e-15).any() and (ends < -1 + 1e-15).any()
    # no status array == an all-zero one
    none = engine.temporal_corr_batch(fa, fe, seg, None, ctx=ctx)
    zero = engine.temporal_corr_batch(fa, fe, seg, np.zeros_like(status), ctx=ctx)
    assert np.array_equal(none, zero, equal_nan=True)
    _check_against_scipy(none, fa, fe, seg, None, "unmasked")
    # the device entry point on tensors, other columns (more than one trip of eight)
    dev = torch.device("cuda", ctx.device)
    cols = [6, 9, 10, 8, 0, 2, 3, 4, 5, 7]
    t = lambda a: torch.from_numpy(a).to(dev)                  # noqa: E731
    got = engine.temporal_corr_dev(t(fa), t(fe), t(seg), t(status), cols=cols, ctx=ctx).cpu().numpy()
    assert got.shape == (len(seg) - 1, 20) and np.array_equal(got[:, :10], out, equal_nan=True)
    one = engine.temporal_corr_batch(fa, fe, seg, status, cols=cols[5:], ctx=ctx)
    assert np.array_equal(got[:, 10:], one, equal_nan=True)
    with pytest.raises(ValueError):
        engine.temporal_corr_batch(fa, fe, seg, status, cols=[11], ctx=ctx)


# ------------------------------------------------------------------------------------------------ 2. the step
def test_step_and_graph_replay(ctx):
    import torch
    dev = torch.device("cuda", ctx.device)
    seg_off = np.array([0, 15, 30, 34, 45], np.int32)          # a 4-window group: guarded
    n_win = int(seg_off[-1])
    eeg = torch.from_numpy(synth.eeg_windows(n_win, seed=3, windows_per_recording=15)).to(dev)
    aud = torch.from_numpy(synth.audio_windows(n_win, "alpha", seed=4)).to(dev)
    plain = pipeline.Workspace(n_win, seg_off, dev)
    ws = pipeline.Workspace(n_win, seg_off, dev, correlations=True)
    assert plain.corr is None and ws.corr.shape == (4, 10) and ws.result.shape == plain.result.shape == (4, 48)
    ref = pipeline.run_step(eeg, aud, plain, ctx=ctx).cpu().numpy()
    res = pipeline.run_step(eeg, aud, ws, ctx=ctx).cpu().numpy()
    assert np.array_equal(res, ref, equal_nan=True)
    corr = ws.corr.cpu().numpy()
    fa1, fe1, st = ws.fa1.cpu().numpy(), ws.fe1.cpu().numpy(), ws.aud.status.cpu().numpy()
    assert np.array_equal(corr, engine.temporal_corr_batch(fa1, fe1, seg_off, st, ctx=ctx), equal_nan=True)
    assert _check_against_scipy(corr, fa1, fe1, seg_off, st, "step") >= 10
    assert (corr[2, 0::2] == 0).all() and (corr[2, 1::2] == 1).all()
    v = ws.view(seg_off[:3])
    assert v.corr.shape == (2, 10) and v.corr.data_ptr() == ws.corr.data_ptr()
    # through the lanes: captured once, replayed; equal to eager
    lanes = pipeline.Lanes(1, n_win, seg_off, dev, graph=True, correlations=True)
    for rnd in range(3):
        b = lanes.submit(eeg, aud, ctx=ctx, post=lambda r: r.clone())
        lanes.drain()
        torch.cuda.synchronize()
        assert np.array_equal(b.result().cpu().numpy(), ref, equal_nan=True), rnd
        assert np.array_equal(lanes.ws[0].corr.cpu().numpy(), corr, equal_nan=True), rnd
        lanes.ws[0].corr.fill_(-7.0)                           # the next replay has to write it again
    assert len(lanes.graphs) == 1


# ------------------------------------------------------------------------------------------------ 3. the ragged pass
E2E_L = [FIX[0], 900, FIX[1], 200, FIX[2], 3100, 40, FIX[3], 2800, FIX[4], FIX[5]]
E2E_LE = [FIX[0], 900, FIX[1], 200, FIX[2], 2600, 40, FIX[3], 3300, FIX[4], FIX[5]]
E2E_BUDGET = 12_000
NAMES = [f"bb{1 + r // 2:02d}_ut{r:02d}.mat" for r in range(len(E2E_L))]
CONDS = ["slow" if r % 2 == 0 else "fast" for r in range(len(E2E_L))]


def _raw(rng, L, n_ch=47):
    return rng.standard_normal((n_ch, L)) + 0.5 * rng.standard_normal((1, L))


def _env(rng, L):
    return np.abs(rng.standard_normal(L)).cumsum() * 0.01 + np.abs(rng.standard_normal(L))


def _bas():
    return [signal.butter(4, [max(lo / 125, 0.001), min(hi / 125, 0.999)], btype="band") for lo, hi in preprocess.FREQ_BANDS.values()]


@pytest.fixture(scope="module")
def e2e(ctx):
    import torch
    dev = torch.device("cuda", ctx.device)
    rng = np.random.default_rng(21)
    raws = [_raw(rng, L) for L in E2E_L]
    envs = [_env(rng, L) for L in E2E_LE]
    xh, _ = preprocess.pack_recordings(raws)
    eh, _ = preprocess.pack_recordings(envs)
    rp = recordings.RaggedRecordingPass(E2E_L, E2E_LE, dev, shard_samples=E2E_BUDGET, n_sets=2, ctx=ctx, correlations=True)
    rows = rp.run(xh, eh).numpy().copy()
    corr = rp.corr_h.numpy().copy()
    return dict(rp=rp, raws=raws, envs=envs, rows=rows, corr=corr, xh=xh, eh=eh, dev=dev)


def test_ragged_pass_correlations_equal_the_per_recording_driver(ctx, e2e):
    rp, raws, envs, rows, corr = e2e["rp"], e2e["raws"], e2e["envs"], e2e["rows"], e2e["corr"]
    P = rp.plan
    assert len(P.shards) >= 3 and len(set(E2E_L)) >= 6 + 2 and E2E_L != E2E_LE
    assert rows.shape == (len(E2E_L), 5, 48) and corr.shape == (len(E2E_L), 5, 10)
    plain = recordings.RaggedRecordingPass(E2E_L, E2E_LE, e2e["dev"], shard_samples=E2E_BUDGET, n_sets=2, ctx=ctx)
    assert plain.corr_h is None and plain.set[0]["ws"].corr is None
    ref_rows = plain.run(e2e["xh"], e2e["eh"]).numpy()
    assert plain.corr_h is None
    assert np.array_equal(rows, ref_rows, equal_nan=True)
    assert sorted(rp.empty.tolist()) == [3, 6]
    for r in rp.empty:
        assert np.isnan(corr[r]).all() and corr[r].size == 50
    live = [r for r in range(len(E2E_L)) if P.k[r] > 0]
    bas = _bas()
    cells = free = 0
    for r in live:
        aw, ed = {}, {}
        for b, (name, (lo, hi)) in enumerate(preprocess.FREQ_BANDS.items()):
            y = signal.sosfiltfilt(preprocess.design_bandpass_filter(lo, hi, 250), raws[r], axis=-1)
            ya = signal.filtfilt(bas[b][0], bas[b][1], envs[r])
            aw[name] = utils.create_windows(ya, 250, 62)
            n_e = int(preprocess.n_windows(E2E_L[r]))
            ed[name] = engine.corr_dist_batch(np.stack([y[:, k * 62:k * 62 + 250] for k in range(n_e)]), want_corr=False, ctx=ctx)
        one = drivers.process_recording_arrays(aw, ed)
        for b, name in enumerate(preprocess.FREQ_BANDS):
            fc = one[name]["feature_correlations"]
            assert one[name]["n_windows"] == rows[r, b, 3] and one[name]["tau"] == rows[r, b, 2]
            for k, f in enumerate(engine.SPEARMAN_FEATURES):
                got_r, got_p = corr[r, b, 2 * k], corr[r, b, 2 * k + 1]
                print("rec", r, name, f, "r", got_r, fc[f]["r"], "p", got_p, fc[f]["p"])
                assert got_r == fc[f]["r"], (r, name, f, got_r, fc[f]["r"])
                assert abs(got_p - fc[f]["p"]) < 1e-10, (r, name, f, got_p, fc[f]["p"])
                cells += 1
                free += (got_r, got_p) != (0.0, 1.0)
    # the test must not pass on the guard alone (the reference's own table has under 2 % guarded cells)
    print("unguarded cells", free, "of", cells)
    assert cells == len(live) * 25 and 2 * free >= cells
    again = rp.run(e2e["xh"], e2e["eh"]).numpy()
    assert np.array_equal(again, rows, equal_nan=True)
    assert np.array_equal(rp.corr_h.numpy(), corr, equal_nan=True)


# ------------------------------------------------------------------------------------------------ 4. the other passes
def test_recording_pass_equals_ragged_pass(ctx):
    import torch
    dev = torch.device("cuda", ctx.device)
    rng = np.random.default_rng(34)
    n_rec, L = 7, 1500
    raw = rng.standard_normal((n_rec, 47, L)) + 0.5 * rng.standard_normal((n_rec, 1, L))
    env = np.abs(rng.standard_normal((n_rec, L))).cumsum(axis=1) * 0.01 + np.abs(rng.standard_normal((n_rec, L)))
    eq = recordings.RecordingPass(L, 3, dev, ctx=ctx, correlations=True)
    rows = eq.run(torch.from_numpy(raw).pin_memory(), torch.from_numpy(env).pin_memory()).numpy().copy()
    assert eq.corr_h.shape == (n_rec, 5, 10) and eq.corr_h.is_pinned()
    rp = recordings.RaggedRecordingPass([L] * n_rec, None, dev, shard_samples=3 * L, n_sets=2, ctx=ctx, correlations=True)
    got = rp.run(torch.from_numpy(raw.ravel()).pin_memory(), torch.from_numpy(env.ravel()).pin_memory()).numpy()
    assert np.array_equal(got, rows, equal_nan=True)
    assert np.array_equal(rp.corr_h.numpy(), eq.corr_h.numpy(), equal_nan=True)
    assert np.isfinite(eq.corr_h.numpy()).all() and (eq.corr_h.numpy()[:, :, 1::2] < 1).sum() > n_rec * 25 // 2


PASS_L = [1500, 2663, 200, 900, 1240]
PASS_LE = [1400, 2663, 300, 1000, 1240]


def test_audio_pass_equals_envelope_pass(ctx):
    import torch
    dev = torch.device("cuda", ctx.device)
    rng = np.random.default_rng(14)
    La = [le * 882 // 5 - (i % 3) * 37 for i, le in enumerate(PASS_LE)]
    t = [np.arange(n) / 44100.0 for n in La]
    auds = [(1.0 + 0.5 * np.sin(2 * np.pi * 3.0 * ti)) * np.sin(2 * np.pi * (120 + 25 * i) * ti) + 0.1 * rng.standard_normal(len(ti))
            for i, ti in enumerate(t)]
    raws = [_raw(rng, L) for L in PASS_L]
    xh, _ = preprocess.pack_recordings(raws)
    ah, lah = preprocess.pack_recordings(auds)
    cost = 8 * (47 * np.array(PASS_L) + lah)
    ap = recordings.RaggedAudioRecordingPass(PASS_L, lah, dev, shard_bytes=int(cost.max()), n_sets=2, ctx=ctx, correlations=True)
    rows = ap.run(xh, ah).numpy().copy()
    corr = ap.corr_h.numpy().copy()
    env, le = preprocess.envelopes_ragged_dev(ah.to(dev), lah, ctx=ctx)
    torch.cuda.synchronize()
    eh = torch.empty(env.numel(), dtype=torch.float64).pin_memory()
    eh.copy_(env.cpu())
    rp = recordings.RaggedRecordingPass(PASS_L, le, dev, shard_samples=3000, n_sets=2, ctx=ctx, correlations=True)
    ref = rp.run(xh, eh).numpy()
    assert np.array_equal(rows, ref, equal_nan=True)
    assert np.array_equal(corr, rp.corr_h.numpy(), equal_nan=True)
    assert ap.empty.tolist() == [2] and np.isnan(corr[2]).all() and np.isfinite(corr[[0, 1, 3, 4]]).all()


def test_control_pass_has_no_correlations():
    with pytest.raises(ValueError):
        recordings.ControlPass([1500, 1500], None, [1, 0], correlations=True)


# ------------------------------------------------------------------------------------------------ 5. all windows
def test_all_windows_of_the_longest_recordings(ctx):
    import torch
    dev = torch.device("cuda", ctx.device)
    rng = np.random.default_rng(89)
    lengths = [FIX[1], FIX[5]]
    raws = [_raw(rng, L) for L in lengths]
    envs = [_env(rng, L) for L in lengths]
    xh, _ = preprocess.pack_recordings(raws)
    eh, _ = preprocess.pack_recordings(envs)
    rp = recordings.RaggedRecordingPass(lengths, None, dev, n_sets=1, ctx=ctx, max_windows=1000, correlations=True)
    assert len(rp.plan.shards) == 1 and rp.plan.k[0] == 89 == preprocess.n_windows(CORPUS.max())
    rows = rp.run(xh, eh).numpy()
    assert (rows[:, :, 3] == rp.plan.k[:, None]).all()
    v = rp.set[0]["views"][0]                                              # the step's own per-window features
    torch.cuda.synchronize()
    fa1, fe1, st, seg = v.fa1.cpu().numpy(), v.fe1.cpu().numpy(), v.aud.status.cpu().numpy(), v.seg_off.cpu().numpy()
    assert len(seg) - 1 == 10 and seg[1] == 89
    band_major = rp.corr_h.numpy().transpose(1, 0, 2).reshape(10, 10)       # groups are (band, recording)
    assert _check_against_scipy(band_major, fa1, fe1, seg, st, "all windows") >= 25


# ------------------------------------------------------------------------------------------------ 6. the files
def test_run_comparison_writes_the_table_and_the_summary(ctx, e2e, tmp_path):
    import pandas as pd
    out_csv, out_json = tmp_path / "results" / "detailed.csv", tmp_path / "results" / "comparison.json"
    rows, corr, table, summary = drivers.run_comparison(e2e["rp"], e2e["xh"], e2e["eh"], NAMES, CONDS, out_csv, out_json)
    assert np.array_equal(rows, e2e["rows"], equal_nan=True) and np.array_equal(corr, e2e["corr"], equal_nan=True)
    assert table == drivers.comparison_rows(rows, corr, NAMES, CONDS)
    assert len(table) == 9 * 5 and {t["filename"] for t in table} == {NAMES[r] for r in range(len(NAMES)) if r not in (3, 6)}
    text = out_csv.read_text().splitlines()
    assert text[0] == ",".join(drivers.DETAILED_COLUMNS) and len(text) == 1 + len(table)
    back = pd.read_csv(out_csv, float_precision="round_trip")
    assert back.to_dict("records") == table
    doc = json.loads(out_json.read_text())
    assert list(doc["band_results"]) == drivers.BANDS and doc["n_recordings"] == 9
    assert doc["band_results"] == json.loads(json.dumps(summary))
    # bb01, bb03 and bb05 have a slow and a fast recording; bb02 and bb04 lose one to the empty recordings, bb06 has one
    assert all(doc["band_results"][b]["n_subjects"] == 3 for b in drivers.BANDS)
    assert all(set(doc["band_results"][b]) == {"n_subjects", "band", "wass_h1_p_fdr", "wass_h1_sig_fdr"} for b in drivers.BANDS)
    import types
    with pytest.raises(ValueError):                                        # a pass without the option
        drivers.run_comparison(types.SimpleNamespace(correlations=False), None, None, [], [])
