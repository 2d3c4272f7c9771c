"""
The Frechet mean kernel (csrc/frechet.hip) against tests/frechet_ref.py.  Every comparison is on bytes: the groups are the
seeded ones of frechet_ref.GROUPS, whose matchings tests/test_frechet_model.py certifies as unique, so mean, count,
variance and iteration count have to be those of the written definition bit for bit.
"""
import numpy as np
import pytest

import frechet_ref as fr
from tda_eeg_audio_amd import engine
from tda_eeg_audio_amd._lib import TdaError, TDA_WIN_H1_TRUNCATED, TDA_WIN_NOT_CONVERGED, TDA_WIN_TOO_LARGE

pytestmark = pytest.mark.gpu


def _pack(groups, cap=None):
    """Diagram buffers of the groups' diagrams in order, and their segment table."""
    dgms = [d for g in groups for d in g]
    cap = cap or max([len(d) for d in dgms] + [1])
    rows = np.zeros((len(dgms), cap, 2)); cnt = np.zeros(len(dgms), np.int32)
    for i, d in enumerate(dgms):
        rows[i, :len(d)] = d
        cnt[i] = len(d)
    return rows, cnt, np.cumsum([0] + [len(g) for g in groups]).astype(np.int32)


def _gpu(ctx, rows, cnt, seg_off=None, status=None, mask=0, max_iter=32, cap_out=None):
    import torch
    dev = torch.device("cuda", ctx.device)
    t = lambda a, dt: None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)
    out = engine.frechet_mean_dev(t(rows, np.float64), t(cnt, np.int32), seg_off_t=t(seg_off, np.int32),
                                  status_t=t(status, np.int32), skip_mask=mask, max_iter=max_iter, cap_out=cap_out, ctx=ctx)
    torch.cuda.synchronize()
    return tuple(o.cpu().numpy() for o in out)


def _same(got, want):
    """mean (NaN beyond the count on both sides), count, variance, iters, status: the same bytes."""
    names = ("mean", "cnt", "var", "iters", "status")
    for name, g, w in zip(names, got, want):
        assert g.shape == w.shape and g.dtype == w.dtype, name
        assert np.array_equal(g, w, equal_nan=g.dtype.kind == "f"), (name, g, w)
    fin = ~np.isnan(want[0])
    assert got[0][fin].tobytes() == want[0][fin].tobytes() and got[2].tobytes() == want[2].tobytes()


@pytest.fixture(scope="module")
def seeded():
    """All seeded groups as one batch, the reference evaluated once."""
    names = list(fr.GROUPS)
    rows, cnt, off = _pack([fr.GROUPS[n] for n in names])
    return names, rows, cnt, off, fr.batch(rows, cnt, off, max_iter=32, cap_out=192)


def test_seeded_groups_bit_for_bit(ctx, seeded):
    names, rows, cnt, off, want = seeded
    got = _gpu(ctx, rows, cnt, off, cap_out=192)
    _same(got, want)
    by = dict(zip(names, range(len(names))))
    assert want[1][by["mean_over_64"]] > 64 and want[1][by["inputs_over_128"]] > 128      # past the CW = 2 / 4 lane slots
    assert want[1][by["all_empty"]] == 0 and want[2][by["all_empty"]] == 0.0
    assert (want[4] == 0).all() and want[3].max() >= 5


def test_group_alone_and_in_batch(ctx, seeded):
    names, rows, cnt, off, want = seeded
    for name in ("m15_s0", "h0_like", "with_empty"):
        g = names.index(name)
        sl = slice(off[g], off[g + 1])
        alone = _gpu(ctx, rows[sl], cnt[sl], np.array([0, off[g + 1] - off[g]], np.int32), cap_out=192)
        _same(alone, tuple(w[g:g + 1] for w in want))


def test_narrow_buffers_and_cap_out(ctx):
    """The same groups in buffers of their own capacity (another LDS layout), and a cap_out below the count."""
    for name in ("m5_s1", "m15_s1"):
        rows, cnt, off = _pack([fr.GROUPS[name]])
        _same(_gpu(ctx, rows, cnt, off, cap_out=64), fr.batch(rows, cnt, off, cap_out=64))
        got = _gpu(ctx, rows, cnt, off, cap_out=5)
        want = fr.batch(rows, cnt, off, cap_out=5)
        _same(got, want)
        assert got[4][0] == TDA_WIN_H1_TRUNCATED and got[1][0] > 5 and np.isfinite(got[2][0])


def test_skip_mask_moves_the_start(ctx):
    g = fr.GROUPS["m5_s0"]
    rows, cnt, off = _pack([g, fr.GROUPS["m3_s1"]])
    status = np.zeros(len(cnt), np.int32)
    status[0] = 4                                   # the first diagram of the first group: the start moves to the second
    status[5:] = 16                                 # nothing kept in the second group
    got = _gpu(ctx, rows, cnt, off, status=status, mask=4 | 16)
    want = fr.batch(rows, cnt, off, status=status, skip_mask=4 | 16)
    _same(got, want)
    assert got[1][1] == 0 and np.isnan(got[2][1]) and got[4][1] == 0
    r0, c0, o0 = _pack([g[1:]], cap=rows.shape[1])
    _same(tuple(x[:1] for x in got), fr.batch(r0, c0, o0))
    assert not np.array_equal(got[0][0], _gpu(ctx, rows, cnt, off)[0][0], equal_nan=True)


def test_no_seg_off_and_many_groups(ctx):
    """Every diagram its own group, more groups than workgroups resident at once: the mean is the diagram's finite rows."""
    rng = np.random.default_rng(5)
    dgms = fr.singles(525)
    rows, cnt, _ = _pack([dgms])
    got = _gpu(ctx, rows, cnt, cap_out=16)
    _same(got, fr.batch(rows, cnt, cap_out=16))
    for i in rng.integers(0, 525, 20):
        fin = fr.finite_rows(dgms[i])
        assert got[1][i] == len(fin) and np.array_equal(got[0][i, :len(fin)], fin)
        assert got[2][i] == 0.0 and got[3][i] == 1


def test_max_iter_1_keeps_the_output(ctx):
    rows, cnt, off = _pack([fr.GROUPS["m15_s0"]])
    got = _gpu(ctx, rows, cnt, off, max_iter=1)
    want = fr.batch(rows, cnt, off, max_iter=1)
    _same(got, want)
    assert got[4][0] == TDA_WIN_NOT_CONVERGED and got[3][0] == 1
    fin = fr.finite_rows(fr.GROUPS["m15_s0"][0])
    assert got[1][0] == len(fin) and np.array_equal(got[0][0, :len(fin)], fin) and np.isfinite(got[2][0])


def test_too_large(ctx):
    other = fr.other_groups()
    rows, cnt, off = _pack([other["far_9x60"], other["far_8x60"], [fr.GROUPS["m1_s0"][0]] * 65])
    got = _gpu(ctx, rows, cnt, off)
    want = fr.batch(rows, cnt, off)
    _same(got, want)
    assert got[4].tolist() == [TDA_WIN_TOO_LARGE, 0, TDA_WIN_TOO_LARGE]
    assert got[1].tolist() == [0, 480, 0] and np.isnan(got[2][[0, 2]]).all()


def test_invalid_arguments_launch_nothing(ctx):
    import torch
    dev = torch.device("cuda", ctx.device)
    rows, cnt, off = _pack([fr.GROUPS["m2_s0"]])
    for kw in (dict(max_iter=0), dict(max_iter=65), dict(cap_out=0), dict(max_iter=True)):
        with pytest.raises(TdaError):
            _gpu(ctx, rows, cnt, off, **kw)
    # the C entry itself: the outputs keep their bytes
    out = tuple(torch.full(s, 7, dtype=dt, device=dev) for s, dt in (((1, 8, 2), torch.float64), ((1,), torch.int32),
                ((1,), torch.float64), ((1,), torch.int32), ((1,), torch.int32)))
    r, c, o = (torch.from_numpy(a).to(dev) for a in (rows, cnt, off))
    lib, st = ctx.lib, engine._stream()
    tp = engine._tp
    for cap, n_seg, seg, it, cap_out in ((rows.shape[1], 1, o, 0, 8), (rows.shape[1], 1, o, 65, 8), (0, 1, o, 4, 8),
                                         (rows.shape[1], 1, o, 4, 0), (rows.shape[1], 1, None, 4, 8), (rows.shape[1], -1, o, 4, 8)):
        rc = lib.tda_frechet_mean_dev(ctx.h, tp(r), tp(c), cap, rows.shape[0], tp(seg), n_seg, None, 0, it, tp(out[0]), tp(out[1]),
                                      cap_out, tp(out[2]), tp(out[3]), tp(out[4]), st)
        assert rc == 1
    torch.cuda.synchronize()
    assert all((x.cpu().numpy() == 7).all() for x in out)


def test_host_form_against_dev_form(ctx, seeded):
    names, rows, cnt, off, want = seeded
    host = engine.frechet_mean_batch(rows, cnt, seg_off=off, cap_out=192, ctx=ctx)
    _same(host, want)
    status = np.zeros(len(cnt), np.int32); status[::3] = 4
    _same(engine.frechet_mean_batch(rows, cnt, seg_off=off, status=status, skip_mask=4, cap_out=192, ctx=ctx),
          _gpu(ctx, rows, cnt, off, status=status, mask=4, cap_out=192))
    # seg_off = NULL: every diagram its own group
    _same(engine.frechet_mean_batch(rows[:3], cnt[:3], cap_out=192, ctx=ctx), _gpu(ctx, rows[:3], cnt[:3], cap_out=192))


def test_utils_frechet_mean(ctx):
    from tda_eeg_audio_amd import utils
    g = fr.GROUPS["m5_s0"]
    want = fr.frechet_mean(g)
    mean, var, iters, converged = utils.frechet_mean(g)
    assert mean.shape == (want.cnt, 2) and mean.tobytes() == want.mean[:want.cnt].tobytes()
    assert (var, iters, converged) == (want.var, want.iters, True)
    mean1, var1, iters1, converged1 = utils.frechet_mean(g, max_iter=1)
    assert not converged1 and iters1 == 1 and np.array_equal(mean1, fr.finite_rows(g[0])) and var1 > var
    mean0, var0, iters0, converged0 = utils.frechet_mean([])
    assert mean0.shape == (0, 2) and np.isnan(var0) and iters0 == 0 and converged0
    assert utils.frechet_mean([np.zeros((0, 2)), []])[0].shape == (0, 2)
    with pytest.raises(ValueError):
        utils.frechet_mean([np.zeros((3, 3))])
    with pytest.raises(TdaError):
        utils.frechet_mean([g[0]] * 65)
    with pytest.raises(TdaError):
        utils.frechet_mean(g, max_iter=65)


def test_frechet_means_from_distances(ctx):
    """The driver: the Rips launch of features_from_distances, then the kernel per diagram set and group; a group without a
    window has an empty mean."""
    from tda_eeg_audio_amd import drivers

    def dms(k, seed, n=9):
        p = np.random.default_rng(seed).random((k, n, 3))
        return np.linalg.norm(p[:, :, None] - p[:, None], axis=-1)
    dist_list = [dms(3, 1), np.zeros((0, 9, 9)), dms(2, 2)]
    out = drivers.frechet_means_from_distances(dist_list, max_iter=16)
    assert len(out) == 3 and all(set(o) == {"h0", "h1"} for o in out)
    h0, c0, h1, c1, st = engine.rips_dm_batch(np.concatenate([dist_list[0], dist_list[2]]), thresh=2.0, raw=True)
    seg = np.array([0, 3, 3, 5], np.int32)
    for name, rows, cnt in (("h0", h0, c0), ("h1", h1, c1)):
        mean, mc, var, it, fst = engine.frechet_mean_batch(rows, cnt, seg_off=seg, max_iter=16, ctx=ctx)
        for g in range(3):
            m, v, i, s = out[g][name]
            assert m.tobytes() == mean[g, :mc[g]].tobytes() and (i, s) == (it[g], fst[g])
            assert v == var[g] or (np.isnan(v) and np.isnan(var[g]))
    assert out[1]["h0"][0].shape == (0, 2) and np.isnan(out[1]["h0"][1])
    assert out[0]["h0"][0].shape == (8, 2) and out[0]["h0"][1] > 0 and out[0]["h0"][3] == 0        # 9 points: 8 finite H0 rows
