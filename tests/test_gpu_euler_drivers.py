"""
GPU tests of the public front ends of the Euler characteristic curves: utils.compute_eeg_euler_curve /
compute_audio_euler_curve (the twins of compute_eeg_persistence / compute_audio_persistence) and
drivers.euler_curves_from_distances / euler_names, against tests/euler_ref.py.
"""
import numpy as np
import pytest

import euler_ref as er

pytestmark = pytest.mark.gpu


def test_compute_eeg_euler_curve(ctx):
    from oracle import port
    from tda_eeg_audio_amd import synth, utils
    win = synth.eeg_windows(1, seed=70, windows_per_recording=1)[0]
    _, dist = port.corr_dist(win)
    grid = np.linspace(0.0, 2.0, 11)
    out = utils.compute_eeg_euler_curve(dist, grid)
    assert out.dtype == np.int32 and out.shape == (5, 11)
    assert out.tobytes() == er.counts_mat(er.keys_dm(dist), grid).tobytes()
    # max_dim and thresh are passed on; the matrix is symmetrised as compute_eeg_persistence does it
    skew = dist + np.triu(np.full_like(dist, 0.01), 1)
    out2 = utils.compute_eeg_euler_curve(skew, grid, max_dim=2, thresh=1.2)
    assert out2.shape == (4, 11) and out2.tobytes() == er.counts_mat(er.keys_dm(skew), grid, 1.2, 2).tobytes()
    with pytest.raises(ValueError):
        utils.compute_eeg_euler_curve(dist[:, :5], grid)
    with pytest.raises(ValueError):
        utils.compute_eeg_euler_curve(dist, grid, max_dim=4)


def test_compute_audio_euler_curve(ctx):
    from oracle import port
    from tda_eeg_audio_amd import _lib, synth, utils
    sig = synth.audio_windows(1, "alpha", seed=71)[0]
    pc = port.takens(sig, 3, 9, 2)
    grid = np.linspace(0.0, 0.8, 9)
    out = utils.compute_audio_euler_curve(pc, grid)
    assert out.dtype == np.int32 and out.shape == (5, 9)
    assert out.tobytes() == er.counts_mat(er.keys_cloud(pc), grid).tobytes()
    assert out.tobytes() == er.block_takens(sig, 9, grid)[0].tobytes()
    # fewer than 3 points: zeros, as the diagrams are [[0, 0]]; more than 128: an error, not a CPU route
    assert not utils.compute_audio_euler_curve(pc[:2], grid).any()
    with pytest.raises(_lib.TdaError):
        utils.compute_audio_euler_curve(np.random.default_rng(0).random((129, 3)), grid)


def test_euler_curves_from_distances(ctx):
    from oracle import port
    from tda_eeg_audio_amd import drivers, synth
    win = synth.eeg_windows(7, seed=72, windows_per_recording=7)
    dist = np.stack([port.corr_dist(w)[1] for w in win])
    groups = [dist[:4], dist[:0], dist[4:]]                          # three groups, one empty
    grid = np.linspace(0.0, 2.0, 6)
    out = drivers.euler_curves_from_distances(groups, grid)
    assert out.dtype == np.float64 and out.shape == (3, 5, 6)
    blocks = np.stack([er.counts_mat(er.keys_dm(d), grid) for d in dist])
    ref = er.mean_exact(blocks, np.array([0, 4, 4, 7], np.int32))
    assert out.tobytes() == ref.tobytes() and np.isnan(out[1]).all()
    out2 = drivers.euler_curves_from_distances(groups, grid, max_dim=2, thresh=1.0)
    blocks2 = np.stack([er.counts_mat(er.keys_dm(d), grid, 1.0, 2) for d in dist])
    assert out2.tobytes() == er.mean_np(blocks2, np.array([0, 4, 4, 7], np.int32)).tobytes()
    # every group empty
    assert np.isnan(drivers.euler_curves_from_distances([dist[:0], dist[:0]], grid)).all()
    names = drivers.euler_names(drivers.BANDS, 3, grid)
    assert len(names) == len(drivers.BANDS) * out[0].size
