"""
recordings.MatchMismatchPass(sliced=dirs) end to end: slc_dist_h / slc_pairs_h / slc_rows_h against the pair kernel
(engine.sliced_wasserstein_dev), numpy's mean and engine.match_rows_dev on the diagrams the per-recording drivers make for
the same plan, and rows_h / dist_h / pairs_h byte for byte with the option on and off.  Five short recordings in three
shards; recording 1 has no window: no row of its own and, as a candidate, a column without audio.
"""
import numpy as np
import pytest
from scipy import signal

from tda_eeg_audio_amd import _lib, drivers, engine, preprocess, recordings, utils

pytestmark = pytest.mark.gpu

L = [1500, 200, 1200, 900, 746]
N_REC, N_DIRS, BUDGET = len(L), 16, 2000


def _driver_diagrams(raws, envs):
    """Per recording and band the H1 diagrams of the selected EEG windows and of the selected audio windows, by the
    per-recording level (tests/test_gpu_match_mismatch.py shows the pass' own diagrams are these, bit for bit)."""
    bas = [signal.butter(4, [max(lo / 125, 0.001), min(hi / 125, 0.999)], btype="band") for lo, hi in preprocess.FREQ_BANDS.values()]
    out = []
    for raw, env in zip(raws, envs):
        per = []
        for b, (lo, hi) in enumerate(preprocess.FREQ_BANDS.values()):
            n_e = int(preprocess.n_windows(raw.shape[1]))
            eeg, aud = [], []
            if n_e > 0:
                y = signal.sosfiltfilt(preprocess.design_bandpass_filter(lo, hi, 250), raw, axis=-1)
                ew = np.stack([y[:, k * 62:k * 62 + 250] for k in recordings.select_windows(n_e)])
                _, h1, st = engine.rips_dm_batch(engine.corr_dist_batch(ew, want_corr=False))
                assert not st.any()
                eeg = list(h1)
            if len(env) >= 250:
                aw = utils.create_windows(signal.filtfilt(bas[b][0], bas[b][1], env), 250, 62)
                aud = [d[1] for d in drivers.get_audio_diagrams_from_windows(aw)]
            per.append((eeg, aud))
        out.append(per)
    return out


@pytest.fixture(scope="module")
def case(ctx):
    import torch
    dev = torch.device("cuda", ctx.device)
    rng = np.random.default_rng(91)
    raws = [rng.standard_normal((47, v)) + 0.5 * rng.standard_normal((1, v)) for v in L]
    envs = [np.abs(rng.standard_normal(v)).cumsum() * 0.01 + np.abs(rng.standard_normal(v)) for v in L]
    xh, _ = preprocess.pack_recordings(raws)
    eh, _ = preprocess.pack_recordings(envs)
    dirs = utils.default_directions(N_DIRS)
    on = recordings.MatchMismatchPass(L, None, None, dev, shard_samples=BUDGET, n_sets=2, ctx=ctx, sliced=dirs)
    rows_on = on.run(xh, eh).numpy().copy()
    res = dict(rows=rows_on, dist=on.dist_h.numpy().copy(), pairs=on.pairs_h.numpy().copy(), slc_dist=on.slc_dist_h.numpy().copy(),
               slc_pairs=on.slc_pairs_h.numpy().copy(), slc_rows=on.slc_rows_h.numpy().copy())
    again = on.run(xh, eh).numpy().copy()
    res.update(rows2=again, slc_dist2=on.slc_dist_h.numpy().copy(), slc_rows2=on.slc_rows_h.numpy().copy())
    off = recordings.MatchMismatchPass(L, None, None, dev, shard_samples=BUDGET, n_sets=2, ctx=ctx)
    res.update(rows_off=off.run(xh, eh).numpy().copy(), dist_off=off.dist_h.numpy().copy(), pairs_off=off.pairs_h.numpy().copy(),
               off=off, on=on, dev=dev, dirs=dirs, dg=_driver_diagrams(raws, envs))
    return res


def test_option_off_is_untouched(case):
    off, on = case["off"], case["on"]
    assert len(on.plan.shards) >= 3 and on.empty.tolist() == [1] and on.n_col == N_REC
    assert off.slc_dist_h is None and off.slc_pairs_h is None and off.slc_rows_h is None and off.slc_dirs is None
    assert case["rows"].tobytes() == case["rows_off"].tobytes()
    assert case["dist"].tobytes() == case["dist_off"].tobytes() and case["pairs"].tobytes() == case["pairs_off"].tobytes()
    assert case["rows2"].tobytes() == case["rows"].tobytes()                         # a second run: the same bytes
    assert case["slc_dist2"].tobytes() == case["slc_dist"].tobytes() and case["slc_rows2"].tobytes() == case["slc_rows"].tobytes()
    with pytest.raises(_lib.TdaError):
        recordings.MatchMismatchPass(L, None, None, case["dev"], ctx=on.ctx, sliced=np.zeros((3, 3)))


def test_shapes_and_the_recording_without_a_window(case):
    sd, sp, sr_ = case["slc_dist"], case["slc_pairs"], case["slc_rows"]
    assert sd.shape == (N_REC, 5, N_REC) and sd.dtype == np.float64 and sp.shape == sd.shape and sp.dtype == np.int32
    assert sr_.shape == (N_REC, 5, 6)
    assert np.isnan(sd[1]).all() and not sp[1].any() and np.isnan(sr_[1][:, [0, 5]]).all() and not sr_[1][:, 1:5].any()
    assert np.isnan(sd[:, :, 1]).all() and not sp[:, :, 1].any()                      # the candidate without audio
    live = [0, 2, 3, 4]
    assert np.isfinite(sd[live][:, :, live]).all() and (sp[live][:, :, live] >= 9).all()
    assert np.array_equal(sp, case["pairs"])                                          # the pairing rules are the same


def test_entries_are_means_of_the_pair_kernel(case, ctx):
    import torch
    dev, dg = case["dev"], case["dg"]
    dt = torch.from_numpy(case["dirs"]).to(dev)
    ref = np.full((N_REC, 5, N_REC), np.nan)
    ref_n = np.zeros((N_REC, 5, N_REC), np.int32)
    for b in range(5):
        eeg = [d for r in range(N_REC) for d in dg[r][b][0]]
        aud = [d for r in range(N_REC) for d in dg[r][b][1]]
        eo = np.concatenate([[0], np.cumsum([len(dg[r][b][0]) for r in range(N_REC)])])
        ao = np.concatenate([[0], np.cumsum([len(dg[r][b][1]) for r in range(N_REC)])])
        ra, ca = engine.pack_diagrams(eeg, cap=256)
        rb, cb = engine.pack_diagrams(aud, cap=256)
        ia, ib, where = [], [], []
        for r in range(N_REC):
            for c in range(N_REC):
                n = min(eo[r + 1] - eo[r], ao[c + 1] - ao[c])
                ref_n[r, b, c] = n
                ia += list(eo[r] + np.arange(n)); ib += list(ao[c] + np.arange(n)); where += [(r, c)] * n
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        w, st = engine.sliced_wasserstein_dev(t(ra), t(ca), t(rb), t(cb), dt, t(np.array(ia, np.int32)), t(np.array(ib, np.int32)), ctx=ctx)
        torch.cuda.synchronize()
        w, st, where = w.cpu().numpy(), st.cpu().numpy(), np.array(where)
        assert not st.any()
        for r in range(N_REC):
            for c in range(N_REC):
                v = w[(where[:, 0] == r) & (where[:, 1] == c)]
                if len(v):
                    ref[r, b, c] = np.mean(v)
    assert np.array_equal(case["slc_pairs"], ref_n)
    assert np.array_equal(np.isnan(case["slc_dist"]), np.isnan(ref))
    ok = ~np.isnan(ref)
    assert case["slc_dist"][ok].tobytes() == ref[ok].tobytes(), np.abs(case["slc_dist"][ok] - ref[ok]).max()
    assert set(np.unique(ref_n)) >= {0, 9, 15}


def test_rows_are_match_rows_of_the_matrix(case, ctx):
    import torch
    dev = case["dev"]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    own = t(np.arange(N_REC, dtype=np.int32))
    for b in range(5):
        d, p = case["slc_dist"][:, b], case["slc_pairs"][:, b]
        rows = engine.match_rows_dev(t(d), t(p), t(np.zeros_like(p)), own, ctx=ctx)
        torch.cuda.synchronize()
        rows = rows.cpu().numpy()
        live = [0, 2, 3, 4]
        assert case["slc_rows"][live, b].tobytes() == rows[live].tobytes()
        assert (case["slc_rows"][live, b, 2] == 3).all()                              # three other finite columns each
        assert np.array_equal(case["slc_rows"][live, b, 0], d[live, live]) and np.array_equal(case["slc_rows"][live, b, 1], p[live, live])
