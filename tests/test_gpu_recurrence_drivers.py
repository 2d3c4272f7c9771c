"""
GPU tests of the front ends of the recurrence curves: the three utils calls and drivers.recurrence_curves_from_windows
against the host statement of tests/recurrence_ref.py (bytes for the integers and the ratio measures, the entropy bar of
recurrence_ref for rows 3 and 6) and against the composition of the device calls.
"""
import numpy as np
import pytest

import euler_ref as er
import recurrence_cases as rc
import recurrence_ref as rr

pytestmark = pytest.mark.gpu

GRID = np.array([1.1, 0.2, 0.6, 0.35, 0.9])
RATIO, ENT = list(rr.RATIO_ROWS), list(rr.ENTROPY_ROWS)


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda", 0))


def _rows_match(rows, ref, hist_cols=None):
    from tda_eeg_audio_amd import _lib
    cnt, mea, his = ref
    for k, name in enumerate(_lib.RQA_COUNT_NAMES):
        assert rows[name].dtype == np.int32 and rows[name].tobytes() == cnt[k].tobytes(), name
    for k, name in enumerate(_lib.RQA_MEASURE_NAMES):
        assert rows[name].dtype == np.float64 and rows[name].shape == mea[k].shape, name
        if k in RATIO:
            assert rows[name].tobytes() == mea[k].tobytes(), name
        else:
            assert (np.abs(rows[name] - mea[k]) <= rr.ENTROPY_BAR).all(), name
    if hist_cols is not None:
        assert rows["diag_hist"].shape == (len(mea[0]), hist_cols) and rows["diag_hist"].tobytes() == his[0].tobytes()
        assert rows["vert_hist"].tobytes() == his[1].tobytes()


def test_utils_calls(ctx):
    from tda_eeg_audio_amd import _lib, utils
    d = rc.trajectory_dm(1, 40, 1)[0]
    rows = utils.compute_recurrence_curves_from_distances(d, GRID, theiler=2, l_min=3, v_min=1, histograms=True)
    assert list(rows) == list(_lib.RQA_COUNT_NAMES + _lib.RQA_MEASURE_NAMES) + ["diag_hist", "vert_hist"]
    _rows_match(rows, rr.block_dm(d, GRID, 2, 3, 1), 40)
    assert rows["diag_longest"].max() >= 10
    plain = utils.compute_recurrence_curves_from_distances(d, GRID)
    assert "diag_hist" not in plain
    _rows_match(plain, rr.block_dm(d, GRID))
    with pytest.raises(ValueError):
        utils.compute_recurrence_curves_from_distances(d[:3], GRID)
    with pytest.raises(ValueError):
        utils.compute_recurrence_curves_from_distances(d, [])
    with pytest.raises(ValueError):
        utils.compute_recurrence_curves_from_distances(d, GRID, theiler=0)
    # a signal and its delay embedding as a cloud: one plot
    sig = np.sin(np.arange(250) * 0.17) + 0.3 * np.sin(np.arange(250) * 0.041)
    g = GRID * 0.3
    rows = utils.compute_signal_recurrence_curves(sig, 9, g, theiler=3, histograms=True)
    ref, st = rr.block_takens(sig, 9, g, 3, 2, 2)
    assert st == 0
    _rows_match(rows, ref, 128)
    assert rows["diag_longest"].max() >= 10 and rows["determinism"].max() > 0.5
    pc = utils.takens_embedding(sig, 3, 9, 2)
    cloud = utils.compute_audio_recurrence_curves(pc, g, theiler=3, histograms=True)
    _rows_match(cloud, rr.curves(er.keys_cloud(pc), g, 3, 2, 2), len(pc))
    for name in _lib.RQA_COUNT_NAMES + _lib.RQA_MEASURE_NAMES:
        assert cloud[name].tobytes() == rows[name].tobytes(), name
    assert cloud["diag_hist"].tobytes() == np.ascontiguousarray(rows["diag_hist"][:, :len(pc)]).tobytes()
    # fewer than 3 points: zeros
    rows = utils.compute_audio_recurrence_curves(pc[:2], g, histograms=True)
    assert all(not v.any() for v in rows.values()) and rows["vert_hist"].shape == (5, 2)
    rows = utils.compute_signal_recurrence_curves(sig, 124, g)
    assert all(not v.any() for v in rows.values())


def test_recurrence_curves_from_windows(ctx):
    import torch
    from tda_eeg_audio_amd import drivers, engine, synth
    sig = synth.audio_windows(7, "alpha", seed=5)
    groups = [sig[:3], sig[3:3], sig[3:]]
    taus = [11, 5, np.array([7, 124, 30, 0])]                       # the last group: a degenerate and a refused window
    grid = np.array([0.1, 0.35, 0.2, 0.6])
    par = (2, 2, 3)
    means, hist = drivers.recurrence_curves_from_windows(groups, taus, grid, *par, histograms=True)
    tau_w = np.array([11, 11, 11, 7, 124, 30, 0], np.int32)
    seg = np.array([0, 3, 3, 7], np.int32)
    # the composition of the device calls
    rq = engine.recurrence_takens_dev(_dev(sig), _dev(tau_w), _dev(grid), *par, True, seg_off_t=_dev(seg), skip_mask=4 | 16, ctx=ctx)
    assert means.tobytes() == torch.cat([rq.mean_counts, rq.mean_measures], dim=1).cpu().numpy().tobytes()
    assert hist.tobytes() == rq.mean_hist.cpu().numpy().tobytes()
    # the host statement
    blocks, st = zip(*[rr.block_takens(sig[w], int(tau_w[w]), grid, *par) for w in range(7)])
    st = np.array(st, np.int32)
    assert st.tolist() == [0, 0, 0, 0, 4, 0, 16] and rq.status.cpu().numpy().tolist() == st.tolist()
    cnt, mea, his = rr.stack(blocks)
    assert means.shape == (3, 14, 4) and hist.shape == (3, 2, 4, 128)
    assert means[:, :7].tobytes() == rr.mean_exact(cnt, seg, st, 4 | 16).tobytes()
    want = rr.mean_seq(mea, seg, st, 4 | 16)
    got = means[:, 7:]
    assert np.ascontiguousarray(got[:, RATIO]).tobytes() == np.ascontiguousarray(want[:, RATIO]).tobytes()
    assert (np.abs(got[[0, 2]][:, ENT] - want[[0, 2]][:, ENT]) <= rr.ENTROPY_BAR).all()
    assert hist.tobytes() == rr.mean_exact(his, seg, st, 4 | 16).tobytes()
    assert np.isnan(means[1]).all() and np.isnan(hist[1]).all() and not np.isnan(means[[0, 2]]).any()
    assert cnt[:, 3].max() >= 10
    plain = drivers.recurrence_curves_from_windows(groups, taus, grid, *par)
    assert plain.tobytes() == means.tobytes()
    # thresh reaches the kernel
    cut = drivers.recurrence_curves_from_windows(groups, taus, grid, *par, thresh=0.25)
    c5 = np.stack([rr.block_takens(sig[w], int(tau_w[w]), grid, *par, 0.25)[0][0] for w in range(7)])
    assert cut[:, :7].tobytes() == rr.mean_exact(c5, seg, st, 4 | 16).tobytes() and cut.tobytes() != means.tobytes()
