"""
GPU tests of the front ends of the network curves: the utils twins and drivers.network_curves_from_distances against the
means of tests/network_ref.py (for the float64 measures the sequential sum, not np.mean), and
drivers.connectivity_network_curves_from_windows against the composition of its three device calls.
"""
import numpy as np
import pytest

import euler_ref as er
import network_ref as nr

pytestmark = pytest.mark.gpu

GRID = np.array([1.1, 0.2, 0.6, 0.35, 0.9])


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda", 0))


def _sym_random(n_win, n, seed, hi=2.2):
    rng = np.random.default_rng(seed)
    d = rng.random((n_win, n, n)) * hi
    return (d + d.transpose(0, 2, 1)) / 2


def test_utils_twins(ctx):
    from tda_eeg_audio_amd import _lib, utils
    d = _sym_random(1, 20, 1)[0]
    rows = utils.compute_eeg_network_curves(d, GRID, nodal=True)
    cnt, mea, nod = nr.block_dm(d, GRID)
    assert list(rows) == list(_lib.NET_COUNT_NAMES + _lib.NET_MEASURE_NAMES) + ["nodal_" + k for k in _lib.NET_NODAL_NAMES]
    for k, name in enumerate(_lib.NET_COUNT_NAMES):
        assert rows[name].dtype == np.int32 and rows[name].tobytes() == cnt[k].tobytes(), name
    for k, name in enumerate(_lib.NET_MEASURE_NAMES):
        assert rows[name].dtype == np.float64 and rows[name].tobytes() == mea[k].tobytes(), name
    for k, name in enumerate(_lib.NET_NODAL_NAMES):
        assert rows["nodal_" + name].shape == (5, 20) and rows["nodal_" + name].tobytes() == nod[k].tobytes(), name
    assert "nodal_degree" not in utils.compute_eeg_network_curves(d, GRID)
    with pytest.raises(ValueError):
        utils.compute_eeg_network_curves(d[:3], GRID)
    with pytest.raises(ValueError):
        utils.compute_eeg_network_curves(d, [])
    # a point cloud, and one of fewer than 3 points: zeros
    pc = np.random.default_rng(2).random((30, 3))
    g = GRID * 0.4
    rows = utils.compute_audio_network_curves(pc, g, nodal=True)
    cnt, mea, nod = nr.curves(er.keys_cloud(pc), g)
    assert rows["edges"].tobytes() == cnt[0].tobytes() and rows["efficiency"].tobytes() == mea[2].tobytes()
    assert rows["nodal_farness"].tobytes() == nod[3].tobytes() and cnt[0].max() > 0
    rows = utils.compute_audio_network_curves(pc[:2], g, nodal=True)
    assert all(not v.any() for v in rows.values()) and rows["nodal_degree"].shape == (5, 2)


def test_network_curves_from_distances(ctx):
    from tda_eeg_audio_amd import drivers
    dms = _sym_random(7, 47, 3)
    groups = [dms[:3], dms[3:3], dms[3:]]
    means, nodal = drivers.network_curves_from_distances(groups, GRID, nodal=True)
    cnt, mea, nod = nr.stack([nr.block_dm(d, GRID) for d in dms])
    seg = np.array([0, 3, 3, 7], np.int32)
    assert means.shape == (3, 14, 5) and nodal.shape == (3, 5, 5, 47)
    assert means[:, :10].tobytes() == nr.mean_exact(cnt, seg).tobytes()
    assert means[:, 10:].tobytes() == nr.mean_seq(mea, seg).tobytes()
    assert nodal.tobytes() == nr.mean_exact(nod, seg).tobytes()
    assert np.isnan(means[1]).all() and np.isnan(nodal[1]).all() and not np.isnan(means[[0, 2]]).any()
    plain = drivers.network_curves_from_distances(groups, GRID)
    assert plain.tobytes() == means.tobytes()
    # thresh reaches the kernel
    cut = drivers.network_curves_from_distances(groups, GRID, thresh=0.5)
    c5 = np.stack([nr.block_dm(d, GRID, 0.5)[0] for d in dms])
    assert cut[:, :10].tobytes() == nr.mean_exact(c5, seg).tobytes() and cut.tobytes() != means.tobytes()
    # no window at all
    none = drivers.network_curves_from_distances([dms[:0], dms[:0]], GRID)
    assert none.shape == (2, 14, 5) and np.isnan(none).all()


@pytest.mark.parametrize("measure,method", [("pearson", "euclidean"), ("plv", "euclidean"), ("wpli", "euclidean"),
                                            ("aec", "sqrt")])
def test_connectivity_network_curves(ctx, measure, method):
    import torch
    from tda_eeg_audio_amd import drivers, engine, synth
    win = synth.eeg_windows(6, seed=9, windows_per_recording=6)[:, :20, :128].copy()
    if measure != "pearson":
        win[4, 3, 17] = np.inf                                      # flagged by the kernel: left out of its group's mean
    groups = [win[:2], win[2:2], win[2:]]
    grid = np.linspace(0.2, 1.6, 6)
    got = drivers.connectivity_network_curves_from_windows(groups, measure, grid, method=method)
    # the composition: distances, curves, means
    win_t, grid_t, seg_t = _dev(win), _dev(grid), _dev(np.array([0, 2, 2, 6], np.int32))
    if measure == "pearson":
        dist, st = engine.corr_dist_dev(win_t, ctx=ctx), None
    elif measure == "plv":
        dist, _, st = engine.plv_dist_dev(win_t, method=method, ctx=ctx)
    else:
        dist, _, st = engine.connectivity_dist_dev(win_t, measure=measure, method=method, ctx=ctx)
    net = engine.network_dm_dev(dist, grid_t, ctx=ctx)
    if st is None:
        st = torch.zeros(6, dtype=torch.int32, device=win_t.device)
    else:
        assert st.cpu().numpy().tolist() == [0, 0, 0, 0, 64, 0]
    mc, mm, _ = engine.network_mean_dev(net.counts, net.measures, None, 6, 6, 20, seg_t, st, 0x7fffffff, ctx=ctx)
    want = torch.cat([mc, mm], dim=1).cpu().numpy()
    assert got.shape == (3, 14, 6) and got.tobytes() == want.tobytes()
    assert np.isnan(got[1]).all() and not np.isnan(got[[0, 2]]).any()
    # ... and against the reference means of the device's own distances
    keep = [w for w in range(6) if not int(st[w])]
    blocks = [nr.block_dm(d, grid) for d in dist.cpu().numpy()]
    cnt, mea, _ = nr.stack(blocks)
    seg, sti = np.array([0, 2, 2, 6], np.int32), st.cpu().numpy()
    assert got[:, :10].tobytes() == nr.mean_exact(cnt, seg, sti, 0x7fffffff).tobytes()
    assert got[:, 10:].tobytes() == nr.mean_seq(mea, seg, sti, 0x7fffffff).tobytes()
    assert len(keep) == (6 if measure == "pearson" else 5) and cnt[keep, 0].max() > 0
