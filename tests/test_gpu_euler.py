"""
GPU tests of the Euler characteristic curves (csrc/euler.hip; include/tdaeeg.h, "Euler characteristic curves"): bytes
against tests/euler_ref.py.  The shapes are the smallest that can break the kernel: the mask word boundary and the last bit
of each word (63, 64, 65, 127, 128), the one- and two-word templates, fewer and more grid points than waves, every
max_dim, the key rules, the three input forms with their status words, batches, means and the refusals.
"""
import ctypes as C
from math import comb

import numpy as np
import pytest

import euler_ref as er

pytestmark = pytest.mark.gpu

SENT = -7


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda", 0))


def _sym_random(n_win, n, seed, hi=2.2):
    rng = np.random.default_rng(seed)
    d = rng.random((n_win, n, n)) * hi
    return (d + d.transpose(0, 2, 1)) / 2


def _grid(n_grid, seed):
    """Unsorted scales inside and a little outside the keys' range, so that every density occurs."""
    rng = np.random.default_rng(seed)
    return np.concatenate([[1.1], rng.random(n_grid - 1) * 1.6 + 0.2])[:n_grid]


def _ref_dm(dms, grid, K, thresh=2.0, symmetrise=True, counts=er.counts_mat):
    return np.stack([counts(er.keys_dm(d, symmetrise), grid, thresh, K) for d in dms])


def _euler_dm(dms, grid, K, thresh=2.0, symmetrise=True, ctx=None):
    from tda_eeg_audio_amd import engine
    out_t, st_t, _ = engine.euler_dm_dev(_dev(dms), _dev(np.asarray(grid, dtype=np.float64)), K, thresh, symmetrise, ctx=ctx)
    return out_t.cpu().numpy(), st_t.cpu().numpy()


# (n, n_grid, max_dim, windows)
DM_CASES = [(1, 1, 3, 3), (2, 3, 3, 3), (3, 5, 3, 3), (4, 5, 3, 3), (47, 5, 1, 3), (47, 5, 2, 3), (47, 5, 3, 3), (63, 3, 3, 2),
            (64, 5, 3, 2), (65, 3, 1, 2), (65, 5, 2, 2), (65, 3, 3, 2), (127, 3, 3, 1), (128, 5, 3, 1), (9, 256, 3, 2)]


@pytest.mark.parametrize("n,n_grid,K,n_win", DM_CASES)
def test_distance_matrices(ctx, n, n_grid, K, n_win):
    dms = _sym_random(n_win, n, 1000 + n)
    grid = _grid(n_grid, n_grid)
    out, st = _euler_dm(dms, grid, K, ctx=ctx)
    ref = _ref_dm(dms, grid, K)
    assert out.dtype == np.int32 and out.shape == (n_win, K + 2, n_grid)
    assert out.tobytes() == ref.tobytes(), np.argwhere(out != ref)[:5]
    assert (st == 0).all()
    if n <= 9 and n_grid <= 5:
        assert out.tobytes() == _ref_dm(dms, grid, K, counts=er.counts_comb).tobytes()
    if n >= 9 and K == 3:
        assert out[:, 3].max() > 0                                 # the case does reach the tetrahedra


def test_complete_128_point_window(ctx):
    d = np.full((1, 128, 128), 0.5)
    below = float(np.nextafter(np.float64(np.float32(0.5)), -np.inf))
    out, _ = _euler_dm(d, [0.5, below, 1.0], 3, ctx=ctx)
    full = [comb(128, j + 1) for j in range(4)]
    assert full[3] == 10_668_000
    chi = full[0] - full[1] + full[2] - full[3]
    assert out[0].T.tolist() == [full + [chi], [128, 0, 0, 0, 128], full + [chi]]


def test_key_rules(ctx):
    n = 13
    rng = np.random.default_rng(11)
    # all keys equal
    d = np.full((1, n, n), 0.75)
    out, _ = _euler_dm(d, [0.7, 0.75, 0.8], 3, ctx=ctx)
    assert out.tobytes() == _ref_dm(d, [0.7, 0.75, 0.8], 3).tobytes()
    assert out[0, :4, 0].tolist() == [n, 0, 0, 0] and out[0, :4, 1].tolist() == [comb(n, j + 1) for j in range(4)]
    # grid points equal to keys and one ulp (of the double) below them
    d = _sym_random(2, n, 12)
    keys = er.keys_dm(d[0])
    picks = np.sort(keys[np.tril_indices(n, -1)].astype(np.float64))[[3, 20, 40, 70]]
    grid = np.concatenate([picks, np.nextafter(picks, -np.inf)])
    out, _ = _euler_dm(d, grid, 3, ctx=ctx)
    assert out.tobytes() == _ref_dm(d, grid, 3).tobytes()
    assert (out[0, 1, :4] - out[0, 1, 4:] >= 1).all()              # the edge of that key is in at t = key, out just below
    # thresh cutting the filtration: (float)thresh is what the keys are compared with
    for thresh in (0.9, float(picks[2]), float(np.nextafter(picks[2], -np.inf))):
        out, _ = _euler_dm(d, grid, 3, thresh=thresh, ctx=ctx)
        assert out.tobytes() == _ref_dm(d, grid, 3, thresh=thresh).tobytes(), thresh
    # symmetrise 0 and 1 on a matrix that is not symmetric and has negative entries
    raw = rng.random((2, n, n)) * 2.4 - 0.4
    g5 = _grid(5, 13)
    o1, _ = _euler_dm(raw, g5, 3, symmetrise=True, ctx=ctx)
    o0, _ = _euler_dm(raw, g5, 3, symmetrise=False, ctx=ctx)
    assert o1.tobytes() == _ref_dm(raw, g5, 3, symmetrise=True).tobytes()
    assert o0.tobytes() == _ref_dm(raw, g5, 3, symmetrise=False).tobytes()
    assert o0.tobytes() != o1.tobytes()
    # a NaN entry, and a NaN in a descending grid
    d = _sym_random(1, n, 14)
    d[0, 7, 3] = d[0, 3, 7] = np.nan
    grid = np.array([2.5, 1.4, np.nan, 0.9, 0.3])
    out, _ = _euler_dm(d, grid, 3, thresh=3.0, ctx=ctx)
    assert out.tobytes() == _ref_dm(d, grid, 3, thresh=3.0).tobytes()
    assert out[0, :, 2].tolist() == [n, 0, 0, 0, n] and out[0, 1, 0] == comb(n, 2) - 1


@pytest.mark.parametrize("n", [13, 70])
def test_repeated_and_saturated_scales(ctx, n):
    """A wave keeps the counts of its previous grid point (g - 4) when the edge count has not changed: scales that repeat,
    scales past the largest key, scales below the smallest, a NaN after an empty complex, and neighbours that differ."""
    d = _sym_random(2, n, 15, hi=1.5)
    grid = np.array([3.0, 0.001, 0.6, np.nan, 2.5, 0.0005, 0.6, -1.0, 1.6, 0.9, 0.61, np.nan, 0.3, 0.9, 0.6, 0.0, 9.0])
    for K in (2, 3):
        out, _ = _euler_dm(d, grid, K, ctx=ctx)
        assert out.tobytes() == _ref_dm(d, grid, K).tobytes(), K
    assert (out[:, :, 0] == out[:, :, 4]).all() and (out[:, :, 4] == out[:, :, 8]).all() and out[0, 3, 0] == comb(n, 4)
    assert not out[:, 1, [1, 5, 3, 7, 11, 15]].any()


# ---------------------------------------------------------------- cloud forms
CLOUD_P = [2, 3, 64, 65, 128, 129]


def _clouds(dim, seed, p_cap=129):
    rng = np.random.default_rng(seed)
    pc = rng.random((len(CLOUD_P) + 1, p_cap, dim)) * 3.0 - 1.0
    n_pts = np.array(CLOUD_P + [40], np.int32)
    pc[-1, :, 0] = 0.25                                           # a constant column: range 0 -> 1
    return pc, n_pts


@pytest.mark.parametrize("dim,normalise", [(1, True), (3, True), (3, False), (4, True)])
def test_clouds(ctx, dim, normalise):
    from tda_eeg_audio_amd import engine
    pc, n_pts = _clouds(dim, 20 + dim)
    grid = np.array([0.12, 0.3, 0.2]) if normalise else np.array([0.4, 0.9, 0.6])
    out_t, st_t, _ = engine.euler_cloud_dev(_dev(pc), _dev(n_pts), _dev(grid), 3, normalise, ctx=ctx)
    out, st = out_t.cpu().numpy(), st_t.cpu().numpy()
    for w, P in enumerate(n_pts):
        ref, rst = er.block_cloud(pc[w], int(P), grid, 2.0, 3, normalise)
        assert st[w] == rst, (w, P)
        assert out[w].tobytes() == ref.tobytes(), (w, P, np.argwhere(out[w] != ref)[:5])
    assert st.tolist() == [4, 0, 0, 0, 0, 16, 0]
    assert not out[0].any() and not out[5].any() and out[4, 3].max() > 0
    # the one-word template on the same clouds: p_cap = 64
    sub, n_sub = np.ascontiguousarray(pc[[1, 2, 6], :64]), np.array([3, 64, 40], np.int32)
    o64, s64, _ = engine.euler_cloud_dev(_dev(sub), _dev(n_sub), _dev(grid), 3, normalise, ctx=ctx)
    assert o64.cpu().numpy().tobytes() == out[[1, 2, 6]].tobytes() and not s64.cpu().numpy().any()
    # a window with more points than p_cap is too large, whatever p_cap is
    o, s, _ = engine.euler_cloud_dev(_dev(sub), _dev(np.array([65, 64, 2], np.int32)), _dev(grid), 2, normalise, ctx=ctx)
    assert s.cpu().numpy().tolist() == [16, 0, 4] and not o.cpu().numpy()[[0, 2]].any()


def test_cloud_form_equals_distance_matrix_form(ctx):
    from oracle import port
    from tda_eeg_audio_amd import engine
    rng = np.random.default_rng(31)
    pc = rng.standard_normal((3, 70, 3))
    grid = np.array([0.15, 0.4, 0.25, 2.0, 0.0])
    oc, _, _ = engine.euler_cloud_dev(_dev(pc), _dev(np.full(3, 70, np.int32)), _dev(grid), 3, True, ctx=ctx)
    # the key of a > b is cloud_dm[a][b] (|x_a|^2 is added first); symmetrise = 0 reads the entry (b, a): the transpose
    dms = np.stack([port.cloud_dm(port.minmax_normalise(p)).T for p in pc])
    od, _ = _euler_dm(dms, grid, 3, symmetrise=False, ctx=ctx)
    assert oc.cpu().numpy().tobytes() == od.tobytes()
    assert od.tobytes() == np.stack([er.counts_mat(er.keys_cloud(p), grid) for p in pc]).tobytes()


def test_takens_windows(ctx):
    from tda_eeg_audio_amd import engine, synth
    taus = np.array([102, 2, 0, 125, 124, 40, -3], np.int32)        # P = 23, 123, refused, 0, 1, 85, refused
    sig = synth.audio_windows(len(taus), "alpha", seed=3)
    grid = np.array([0.1, 0.35, 0.2, 0.6])
    import torch
    npts_t = torch.full((len(taus),), SENT, dtype=torch.int32, device="cuda:0")
    out_t, st_t, _ = engine.euler_takens_dev(_dev(sig), _dev(taus), _dev(grid), 3, n_points_t=npts_t, ctx=ctx)
    out, st, npts = out_t.cpu().numpy(), st_t.cpu().numpy(), npts_t.cpu().numpy()
    for w, tau in enumerate(taus):
        ref, rst = er.block_takens(sig[w], int(tau), grid)
        assert st[w] == rst and out[w].tobytes() == ref.tobytes(), (w, tau)
    assert st.tolist() == [0, 0, 16, 4, 4, 0, 16]
    assert npts[:2].tolist() == [23, 123] and npts[3:6].tolist() == [0, 1, 85]
    assert out[1, 3].max() > 0
    # other embeddings: dim 1, 2, 4 and subsample 1, 3
    for dim, sub, tau in ((1, 3, 5), (2, 2, 7), (4, 1, 45), (4, 3, 1)):
        t = np.full(2, tau, np.int32)
        o, s, _ = engine.euler_takens_dev(_dev(sig[:2]), _dev(t), _dev(grid), 2, dim=dim, subsample=sub, ctx=ctx)
        for w in range(2):
            ref, rst = er.block_takens(sig[w], tau, grid, 2.0, 2, dim, sub)
            assert int(s[w]) == rst and o[w].cpu().numpy().tobytes() == ref.tobytes(), (dim, sub, tau, w)
    # the host form
    oh, nh, sh = engine.euler_takens_batch(sig, taus, grid, 3, ctx=ctx)
    assert oh.tobytes() == out.tobytes() and sh.tobytes() == st.tobytes() and nh.tolist() == npts.tolist()
    # ... with n_points = NULL
    p = engine.ptr
    w, tau, o2, s2 = engine.f64(sig), engine.i32(taus), np.zeros_like(oh), np.zeros_like(sh)
    ctx.check(ctx.lib.tda_euler_takens_batch(ctx.h, p(w), p(tau), len(taus), sig.shape[1], 3, 2, 2.0, p(grid), len(grid), 3,
                                             p(o2), None, p(s2)))
    assert o2.tobytes() == out.tobytes() and s2.tobytes() == st.tobytes()


# ---------------------------------------------------------------- batches, host forms
def test_batch_behaviour(ctx):
    import torch
    from tda_eeg_audio_amd import engine
    dms = _sym_random(64, 47, 40)
    grid = _grid(5, 41)
    grid_t = _dev(grid)
    # an oversized out_t / status_t: the tail is not touched
    out_t = torch.full((70, 5, 5), SENT, dtype=torch.int32, device="cuda:0")
    st_t = torch.full((70,), SENT, dtype=torch.int32, device="cuda:0")
    engine.euler_dm_dev(_dev(dms), grid_t, 3, out_t=out_t, status_t=st_t, ctx=ctx)
    out, st = out_t.cpu().numpy(), st_t.cpu().numpy()
    assert (out[64:] == SENT).all() and (st[64:] == SENT).all() and not st[:64].any()
    # a window alone and inside the batch
    for w in (0, 17, 63):
        alone, _ = _euler_dm(dms[w:w + 1], grid, 3, ctx=ctx)
        assert alone[0].tobytes() == out[w].tobytes()
    ref = _ref_dm(dms[[17, 63]], grid, 3)
    assert out[[17, 63]].tobytes() == ref.tobytes()
    # the host forms
    oh, sh = engine.euler_dm_batch(dms, grid, 3, ctx=ctx)
    assert oh.tobytes() == out[:64].tobytes() and not sh.any()
    pc, n_pts = _clouds(3, 42)
    och, sch = engine.euler_cloud_batch(pc, grid * 0.2, 2, n_pts=n_pts, ctx=ctx)
    ocd, scd, _ = engine.euler_cloud_dev(_dev(pc), _dev(n_pts), _dev(grid * 0.2), 2, ctx=ctx)
    assert och.tobytes() == ocd.cpu().numpy().tobytes() and sch.tobytes() == scd.cpu().numpy().tobytes()


# ---------------------------------------------------------------- means and refusals
def test_group_means(ctx):
    from tda_eeg_audio_amd import engine
    pc, n_pts = _clouds(3, 50)                                     # statuses 4, 0, 0, 0, 0, 16, 0
    grid = np.array([0.12, 0.3, 0.2])
    grid_t = _dev(grid)
    seg = np.array([0, 0, 1, 6, 7], np.int32)                       # sizes 0, 1 (degenerate alone), 5, 1
    out_t, st_t, mean_t = engine.euler_cloud_dev(_dev(pc), _dev(n_pts), grid_t, 3, seg_off_t=_dev(seg),
                                                 skip_mask=4 | 16, ctx=ctx)
    out, st, mean = out_t.cpu().numpy(), st_t.cpu().numpy(), mean_t.cpu().numpy()
    ref = er.mean_exact(out, seg, st, 4 | 16)
    assert mean.shape == (4, 5, 3) and mean.tobytes() == ref.tobytes() == er.mean_np(out, seg, st, 4 | 16).tobytes()
    assert np.isnan(mean[0]).all() and np.isnan(mean[1]).all() and not np.isnan(mean[2:]).any()
    # nothing skipped: the flagged windows' zeros are members
    m0 = engine.euler_mean_dev(out_t, 7, 3, 3, seg_off_t=_dev(seg), ctx=ctx).cpu().numpy()
    assert m0.tobytes() == er.mean_np(out, seg).tobytes() and not m0[1].any()
    # seg_off = NULL: every window its own group
    own = engine.euler_mean_dev(out_t, 7, 3, 3, ctx=ctx).cpu().numpy()
    assert own.tobytes() == out.astype(np.float64).tobytes()
    _, _, own2 = engine.euler_cloud_dev(_dev(pc), _dev(n_pts), grid_t, 3, mean_t=True, ctx=ctx)
    assert own2.cpu().numpy().tobytes() == own.tobytes()
    # the host form, and a sum that needs more than 32 bits
    big = np.full((5, 5, 2), 2_000_000_000, np.int32)
    big[3] = -7
    mh = np.full((2, 5, 2), np.nan)
    seg2 = np.array([0, 5, 5], np.int32)
    ctx.check(ctx.lib.tda_euler_mean(ctx.h, big.ctypes.data_as(C.c_void_p), 5, 3, 2, seg2.ctypes.data_as(C.c_void_p), 2, None, 0,
                                     mh.ctypes.data_as(C.c_void_p)))
    assert mh.tobytes() == er.mean_exact(big, seg2).tobytes() and mh[0, 0, 0] == (4 * 2_000_000_000 - 7) / 5
    # the host form with status_in given, and with seg_off = NULL
    hp = lambda a: a.ctypes.data_as(C.c_void_p)                    # noqa: E731
    mh4, mh7 = np.full((4, 5, 3), -1.0), np.full((7, 5, 3), -1.0)
    ctx.check(ctx.lib.tda_euler_mean(ctx.h, hp(out), 7, 3, 3, hp(seg), 4, hp(st), 4 | 16, hp(mh4)))
    ctx.check(ctx.lib.tda_euler_mean(ctx.h, hp(out), 7, 3, 3, None, 7, None, 0, hp(mh7)))
    assert mh4.tobytes() == mean.tobytes() and mh7.tobytes() == own.tobytes()


def _msg(ctx):
    buf = C.create_string_buffer(512)
    ctx.lib.tda_last_error(ctx.h, buf, 512)
    return buf.value.decode()


def test_refusals(ctx):
    import torch
    from tda_eeg_audio_amd import _lib, engine
    dev = torch.device("cuda", 0)
    p = engine._tp
    dm = torch.zeros((2, 129, 129), dtype=torch.float64, device=dev)
    grid = torch.zeros(_lib.MAX_GRID + 1, dtype=torch.float64, device=dev)
    out = torch.full((2 * 5 * (_lib.MAX_GRID + 1),), SENT, dtype=torch.int32, device=dev)
    st = torch.full((2,), SENT, dtype=torch.int32, device=dev)
    mean = torch.full((2 * 5 * 4,), -7.0, dtype=torch.float64, device=dev)
    tau = torch.ones(2, dtype=torch.int32, device=dev)
    lib, h = ctx.lib, ctx.h
    calls = [
        lambda: lib.tda_euler_dm_batch_dev(h, p(dm), 2, 129, 2.0, 1, p(grid), 4, 3, p(out), p(st), None),      # n
        lambda: lib.tda_euler_dm_batch_dev(h, p(dm), 2, 0, 2.0, 1, p(grid), 4, 3, p(out), p(st), None),
        lambda: lib.tda_euler_dm_batch_dev(h, p(dm), 2, 9, 2.0, 1, p(grid), 0, 3, p(out), p(st), None),        # n_grid
        lambda: lib.tda_euler_dm_batch_dev(h, p(dm), 2, 9, 2.0, 1, p(grid), _lib.MAX_GRID + 1, 3, p(out), p(st), None),
        lambda: lib.tda_euler_dm_batch_dev(h, p(dm), 2, 9, 2.0, 1, p(grid), 4, 0, p(out), p(st), None),        # max_dim
        lambda: lib.tda_euler_dm_batch_dev(h, p(dm), 2, 9, 2.0, 1, p(grid), 4, 4, p(out), p(st), None),
        lambda: lib.tda_euler_cloud_batch_dev(h, p(dm), p(tau), 2, 8, 5, 1, 2.0, p(grid), 4, 3, p(out), p(st), None),   # dim
        lambda: lib.tda_euler_cloud_batch_dev(h, p(dm), p(tau), 2, 8, 0, 1, 2.0, p(grid), 4, 3, p(out), p(st), None),
        lambda: lib.tda_euler_cloud_batch_dev(h, p(dm), p(tau), 2, 0, 3, 1, 2.0, p(grid), 4, 3, p(out), p(st), None),   # p_cap
        lambda: lib.tda_euler_takens_batch_dev(h, p(dm), p(tau), 2, 250, 5, 2, 2.0, p(grid), 4, 3, p(out), None, p(st), None),
        lambda: lib.tda_euler_takens_batch_dev(h, p(dm), p(tau), 2, 250, 3, 2, 2.0, p(grid), 4, 4, p(out), None, p(st), None),
        lambda: lib.tda_euler_mean_dev(h, p(out), 2, 3, 4, None, 1, None, 0, p(mean), None),                  # n_seg != n_win
        lambda: lib.tda_euler_mean_dev(h, p(out), 2, 4, 4, None, 2, None, 0, p(mean), None),
        lambda: lib.tda_euler_mean_dev(h, p(out), 2, 3, 0, None, 2, None, 0, p(mean), None),
    ]
    for k, call in enumerate(calls):
        assert call() == 1, k                                      # TDA_ERR_INVALID
        assert _msg(ctx), k
    torch.cuda.synchronize()
    assert (out == SENT).all() and (st == SENT).all() and (mean == -7.0).all()
    # the host forms refuse before anything is staged or written
    oh = np.full((2, 5, 4), SENT, np.int32)
    hp = lambda a: a.ctypes.data_as(C.c_void_p)                   # noqa: E731
    dmh, gh, sh = np.zeros((2, 9, 9)), np.zeros(4), np.full(2, SENT, np.int32)
    assert lib.tda_euler_dm_batch(h, hp(dmh), 2, 9, 2.0, 1, hp(gh), 4, 4, hp(oh), hp(sh)) == 1
    assert lib.tda_euler_dm_batch(h, hp(dmh), 2, 129, 2.0, 1, hp(gh), 4, 3, hp(oh), hp(sh)) == 1
    assert lib.tda_euler_mean(h, hp(oh), 2, 3, 4, None, 1, None, 0, hp(np.zeros(40))) == 1
    assert (oh == SENT).all() and (sh == SENT).all()
    # the Python front end refuses with ValueError before any call
    with pytest.raises(ValueError):
        engine.euler_dm_dev(dm[:, :9, :9].contiguous(), grid[:4].contiguous(), 4, ctx=ctx)
    with pytest.raises(ValueError):
        engine.euler_dm_dev(dm[:, :9, :9].contiguous(), grid, 3, ctx=ctx)
    # an empty batch is no error and touches nothing
    assert lib.tda_euler_dm_batch_dev(h, None, 0, 9, 2.0, 1, None, 4, 3, None, None, None) == 0


# ---------------------------------------------------------------- composition with the EEG route
def test_eeg_windows_curve_and_diagram_are_one_complex(ctx):
    from oracle import port
    from tda_eeg_audio_amd import engine, synth
    win = synth.eeg_windows(8, seed=60, windows_per_recording=4)
    assert win.shape == (8, 47, 250)
    grid = np.linspace(0.0, 2.0, 9)
    win_t = _dev(win)
    out_t, st_t, _ = engine.euler_eeg_windows_dev(win_t, _dev(grid), 3, ctx=ctx)
    out = out_t.cpu().numpy()
    ref = np.stack([er.counts_mat(er.keys_dm(port.corr_dist(w)[1]), grid) for w in win])
    assert out.tobytes() == ref.tobytes() and not st_t.cpu().numpy().any()
    # against the fused kernel's own diagrams of the same windows: f_0 - f_1 + f_2 >= beta_0 - beta_1, with equality
    # wherever there is no triangle
    e0, e1 = engine.eeg_window_dev(win_t, h1_cap=1024, ctx=ctx).to_lists()
    equal = 0
    for w in range(8):
        for g, t in enumerate(grid):
            lhs = int(out[w, 0, g]) - int(out[w, 1, g]) + int(out[w, 2, g])
            rhs = er.betti(e0[w], t) - er.betti(e1[w], t)
            assert lhs >= rhs, (w, t, lhs, rhs)
            if out[w, 2, g] == 0:
                assert lhs == rhs, (w, t, lhs, rhs)
                equal += 1
    assert equal >= 8 and out[:, 2].max() > 0
