"""
GPU tests of the public front ends of the generators and representative cycles: utils.compute_eeg_generators /
compute_audio_generators (the twins of compute_eeg_persistence / compute_audio_persistence, with n_perm) and
drivers.channel_participation_from_distances, against numpy on the definition in tests/generators_ref.py.
"""
import numpy as np
import pytest

import euler_ref as er
import generators_ref as gr

pytestmark = pytest.mark.gpu


def _pack(dgms):
    h0, h1 = (np.asarray(d, dtype=np.float64).reshape(-1, 2) for d in dgms)
    return h0, len(h0), (h1 if len(h1) else np.zeros((1, 2))), len(h1)


def _check(res, keys, thresh=2.0, idx=None):
    """res against (b) on the same rows; idx maps the vertex numbers (n_perm)."""
    h0, c0, h1, c1 = _pack(res["dgms"])
    ref = gr.generators(keys, h0, c0, h1, c1, thresh)
    back = (lambda a: np.asarray(a, dtype=np.int64)) if idx is None else \
        (lambda a: np.where(np.asarray(a) >= 0, idx[np.maximum(np.asarray(a, dtype=np.int64), 0)], -1))
    assert np.array_equal(res["h0_edges"], back(ref["h0_edge"][:c0]))
    assert np.array_equal(res["h1_birth_edges"], back(ref["h1_gen"][:c1, :2]))
    assert np.array_equal(res["h1_death_edges"], back(ref["h1_gen"][:c1, 2:]))
    assert res["flags"].tobytes() == ref["h1_flag"][:c1].tobytes()
    assert len(res["cycles"]) == c1
    for r in range(c1):
        assert np.array_equal(res["cycles"][r], back(ref["cyc"][r, :ref["cyc_len"][r]]))
    assert res["participation"].tobytes() == ref["part"].tobytes()
    return ref


def test_compute_eeg_generators(ctx):
    from oracle import brute, port
    from tda_eeg_audio_amd import synth, utils
    win = synth.eeg_windows(1, seed=70, windows_per_recording=1)[0]
    _, dist = port.corr_dist(win)
    res = utils.compute_eeg_generators(dist)
    dg = utils.compute_eeg_persistence(dist)
    assert np.array_equal(res["dgms"][0], dg[0]) and np.array_equal(res["dgms"][1], dg[1])
    ref = _check(res, er.keys_dm(dist))
    assert len(res["dgms"][1]) > 4 and not res["flags"].any() and res["participation"].shape == (47,)
    assert all(len(c) >= 4 for c in res["cycles"]) and res["participation"].max() > 0
    # which electrodes carry the most persistent loop: its cycle, and every vertex of it has at least its persistence
    h1 = res["dgms"][1]
    top = int(np.argmax(h1[:, 1] - h1[:, 0]))
    assert (res["participation"][res["cycles"][top]] >= (h1[top, 1] - h1[top, 0])).all()
    # thresh is passed on; the matrix is symmetrised as compute_eeg_persistence does it
    skew = dist + np.triu(np.full_like(dist, 0.01), 1)
    res2 = utils.compute_eeg_generators(skew, thresh=1.2)
    _check(res2, er.keys_dm(skew), 1.2)
    assert np.array_equal(brute.sort_rows(res2["dgms"][1]), brute.sort_rows(port.rips_dm(skew, 1.2)[1]))
    with pytest.raises(ValueError):
        utils.compute_eeg_generators(dist[:, :5])
    assert ref["h0_edge"][46:].tolist() == [[-1, -1]]


def test_compute_audio_generators(ctx):
    from oracle import port
    from tda_eeg_audio_amd import _lib, synth, utils
    sig = synth.audio_windows(1, "alpha", seed=71)[0]
    pc = port.takens(sig, 3, 9, 2)
    res = utils.compute_audio_generators(pc)
    dg = utils.compute_audio_persistence(pc)
    assert np.array_equal(res["dgms"][0], dg[0]) and np.array_equal(res["dgms"][1], dg[1])
    _check(res, er.keys_cloud(pc))
    assert res["participation"].shape == (len(pc),) and len(res["cycles"]) == len(dg[1]) > 0
    with pytest.raises(_lib.TdaError):
        utils.compute_audio_generators(pc[:2])
    with pytest.raises(_lib.TdaError):
        utils.compute_audio_generators(np.random.default_rng(0).random((129, 3)))
    # n_perm: the complex of the landmarks, indices mapped back to rows of the cloud
    rng = np.random.default_rng(4)
    th = rng.random(300) * 2 * np.pi
    big = np.stack([np.cos(th), np.sin(th)], 1) + rng.standard_normal((300, 2)) * 0.03
    res = utils.compute_audio_generators(big, n_perm=40)
    idx, _, _ = utils.greedy_landmarks(big, 40)
    assert np.array_equal(res["idx_perm"], idx) and len(idx) == 40
    dg = utils.compute_audio_persistence(big, n_perm=40)
    assert np.array_equal(res["dgms"][1], dg[1])
    _check(res, er.keys_cloud(port.minmax_normalise(big)[idx], False), idx=idx.astype(np.int64))
    h1 = res["dgms"][1]
    top = int(np.argmax(h1[:, 1] - h1[:, 0]))
    assert set(res["cycles"][top].tolist()) <= set(idx.tolist()) and len(res["cycles"][top]) >= 8     # the circle itself
    assert res["participation"].shape == (40,)


def test_channel_participation_from_distances(ctx):
    from oracle import port
    from tda_eeg_audio_amd import drivers, engine, synth
    win = synth.eeg_windows(7, seed=72, windows_per_recording=7)
    dist = np.stack([port.corr_dist(w)[1] for w in win])
    groups = [dist[:4], dist[:0], dist[4:]]                          # three groups, one empty
    mean, flagged = drivers.channel_participation_from_distances(groups)
    assert mean.dtype == np.float64 and mean.shape == (3, 47) and flagged == 0
    h0, c0, h1, c1, _ = engine.rips_dm_batch(dist, raw=True)
    part = np.stack([gr.generators(er.keys_dm(d), h0[w], c0[w], h1[w], c1[w])["part"] for w, d in enumerate(dist)])
    ref = gr.mean_part(part, np.array([0, 4, 4, 7], np.int32))
    assert mean.tobytes() == ref.tobytes() and np.isnan(mean[1]).all() and mean[0].max() > 0
    # thresh is passed on; quantised matrices report their flagged rows
    q = np.round(dist * 12) / 12
    mean2, flagged2 = drivers.channel_participation_from_distances([q[:3], q[3:]], thresh=1.5)
    h0, c0, h1, c1, _ = engine.rips_dm_batch(q, thresh=1.5, raw=True, h1_cap=1024)
    refs = [gr.generators(er.keys_dm(d), h0[w], c0[w], h1[w], c1[w], 1.5) for w, d in enumerate(q)]
    assert mean2.tobytes() == gr.mean_part(np.stack([r["part"] for r in refs]), np.array([0, 3, 7], np.int32)).tobytes()
    assert flagged2 == sum(int((r["h1_flag"] != 0).sum()) for r in refs) > 0
    # every group empty
    m3, f3 = drivers.channel_participation_from_distances([dist[:0], dist[:0]])
    assert m3.shape == (2, 47) and np.isnan(m3).all() and f3 == 0
    assert len(drivers.participation_names(drivers.BANDS, 47)) == len(drivers.BANDS) * mean[0].size
