"""
The audio branch off the reference's single configuration (n_t = 250, dim = 3, subsample = 2, max_lag = 125): tau_kernel
for lengths 2..8192 and every kind of max_lag, the Takens / cloud Rips kernels for dim 1..4, subsample 1..3 and per-window
point counts, and the four methods of corr_to_dist_kernel -- each against the CPU oracle (or the expression written
out) on the seeded inputs of tests/audio_param_cases.py, which tests/test_audio_params_model.py holds against plain
restatements first.

Bars: delays equal; diagrams bit-exact as sorted multisets of (birth, death) rows; distances bit-exact.
"""
import contextlib
import functools

import numpy as np
import pytest

import audio_param_cases as apc
from oracle import brute, port
from tda_eeg_audio_amd import _lib, engine, graphs, synth

pytestmark = pytest.mark.gpu

H1_CAP = 4096
DEGENERATE = [[0.0, 0.0]]


def _same_multiset(a, b):
    return np.array_equal(brute.sort_rows(a), brute.sort_rows(b))


@contextlib.contextmanager
def _words(ctx, words):
    """First-pass class widths (dm, cloud) for the block, the defaults afterwards."""
    ctx.set_class_words(*words)
    try:
        yield
    finally:
        ctx.set_class_words(2, 1)


def _dev(ctx):
    import torch
    return torch.device("cuda", ctx.device)


# ------------------------------------------------------------------ tau
def test_tau_every_length_and_max_lag_equals_oracle(ctx):
    """864 windows, one call per (n_t, max_lag) pair: lengths around every multiple of the 64-lag chunk, max_lag absent, 1,
    2, inside, at and beyond the length.  The oracle's delays reach every chunk of the lag loop."""
    chunks = [0] * len(apc.LAG_CHUNKS)
    for n_t, max_lag, sig in apc.tau_cases():
        ref = np.array([port.compute_tau(s, max_lag) for s in sig], np.int32)
        got = engine.tau_batch(sig, max_lag, ctx=ctx)
        assert np.array_equal(got, ref), (n_t, max_lag, got, ref)
        for t in ref:
            chunks[apc.lag_chunk(int(t))] += 1
    assert sum(chunks) == 864 and all(chunks), chunks


def _slow_cosines(n_win, n_t, periods, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(n_t, dtype=np.float64)
    return np.stack([np.cos(2.0 * np.pi * t / periods[w % len(periods)]) + 0.01 * rng.standard_normal(n_t)
                     for w in range(n_win)])


def test_tau_segments_first_window_of_each_group(ctx):
    """n_t = 1000, max_lag = 500, groups of 3, 0 and 4 windows whose windows all have different delays: tau_seg is the delay
    of the group's FIRST window (0 for the empty group) and tau_win carries it to every window of the group."""
    import torch
    wins = _slow_cosines(7, 1000, (1300.0, 300.0, 90.0, 700.0, 1800.0, 150.0, 500.0), seed=5)
    seg_off = np.array([0, 3, 3, 7], np.int32)
    each = engine.tau_batch(wins, 500, ctx=ctx)
    assert np.array_equal(each, [port.compute_tau(w, 500) for w in wins])
    assert len(set(each.tolist())) == 7 and each[0] > 256, each             # the first window decides, beyond chunk four
    dev = _dev(ctx)
    tau_win = torch.full((7,), -1, dtype=torch.int32, device=dev)
    tau_seg = engine.tau_segments_dev(torch.from_numpy(wins).to(dev), torch.from_numpy(seg_off).to(dev), 500,
                                      tau_win_t=tau_win, ctx=ctx)
    torch.cuda.synchronize()
    assert tau_seg.cpu().tolist() == [int(each[0]), 0, int(each[3])]
    assert tau_win.cpu().tolist() == [int(each[0])] * 3 + [int(each[3])] * 4


def test_tau_longest_window_and_length_limits(ctx):
    """n_t = 8192 (64 KB of LDS for the centred signal) with max_lag = None (2048 lags, the delay near lag 700); 8193 and 1
    are refused with an error and the context goes on working."""
    win = _slow_cosines(1, 8192, (2800.0,), seed=6)
    ref = port.compute_tau(win[0], None)
    assert 600 < ref < 800
    assert engine.tau_batch(win, None, ctx=ctx)[0] == ref
    for n_t in (8193, 1):
        with pytest.raises(_lib.TdaError, match="n_t must be in"):
            engine.tau_batch(np.zeros((1, n_t)), None, ctx=ctx)
    assert engine.tau_batch(win[:, :250], 125, ctx=ctx)[0] == port.compute_tau(win[0, :250], 125)


# ------------------------------------------------------------------ Takens + Rips
@functools.lru_cache(maxsize=None)
def _takens_oracle():
    """Per case of takens_cases(): [((h0, h1), P)] of its six windows.  Computed once, shared, never written to."""
    return [[port.audio_persistence(s, tau, dim, sub) for s in wins] for dim, sub, n_t, tau, wins in apc.takens_cases()]


@pytest.mark.parametrize("words", [(2, 1), (2, 2)])
def test_takens_every_dim_and_subsample_equals_oracle(ctx, words):
    """dim 1..4 (the generic distance loop beside the unrolled dim = 3), subsample 1..3, clouds of 8..128 points: the narrow
    first pass, the wide one (dim = 4, P > 124) and, under (2, 2), the 64-bit first pass."""
    with _words(ctx, words):
        for (dim, sub, n_t, tau, wins), ora in zip(apc.takens_cases(), _takens_oracle()):
            h0, h1, npts, st = engine.takens_rips_batch(wins, tau, dim=dim, subsample=sub, h1_cap=H1_CAP, ctx=ctx)
            P = apc.takens_points(n_t, dim, tau, sub)
            for w, ((o0, o1), oP) in enumerate(ora):
                tag = (words, dim, sub, n_t, tau, apc.TAKENS_WINDOWS[w])
                assert npts[w] == oP == P, tag
                assert (st[w] & ~4) == 0, (tag, st[w])
                assert _same_multiset(h0[w], o0) and _same_multiset(h1[w], o1), tag
                if P <= apc.BRUTE_P:
                    dm = port.cloud_dm(port.minmax_normalise(apc.takens_cloud(wins[w], dim, tau, sub))).astype(np.float32)
                    assert _same_multiset(h1[w], brute.rips_brute(dm.astype(np.float64), 2.0)[1]), tag


def test_takens_oversized_valid_and_degenerate_windows_in_one_batch(ctx):
    """dim = 3, subsample = 1, n_t = 250: p_max at tau = 1 is 248 and is clamped to 128, so one launch holds windows of 130
    points and tau = 0 (too large: flagged, zero counts), of 128 and 126 points (valid) and of 2 and 0 points (degenerate)."""
    wins, tau = apc.mixed_tau_batch()
    m = apc.MIXED_TAU
    h0, h1, npts, st = engine.takens_rips_batch(wins, tau, dim=m["dim"], subsample=m["subsample"], h1_cap=H1_CAP, ctx=ctx)
    assert tuple(npts) == apc.MIXED_P
    assert tuple(st) == apc.MIXED_STATUS, st
    for w, s in enumerate(apc.MIXED_STATUS):
        if s == 16:
            assert len(h0[w]) == 0 and len(h1[w]) == 0
        elif s == 4:
            assert np.array_equal(h0[w], DEGENERATE) and np.array_equal(h1[w], DEGENERATE)
        else:
            (o0, o1), P = port.audio_persistence(wins[w], int(tau[w]), m["dim"], m["subsample"])
            assert P == apc.MIXED_P[w] and _same_multiset(h0[w], o0) and _same_multiset(h1[w], o1), w


def test_takens_equals_cloud_route_and_device_twin(ctx):
    """One case per dim: the embedding made by the kernel and the embedding made in numpy and handed over as an explicit
    cloud give the same rows, and the device-tensor entry point gives what the host one gives."""
    import torch
    cases = apc.takens_cases()
    picked = [cases[i] for i in (0, 3, 10, 4)]
    assert [c[0] for c in picked] == [1, 2, 3, 4]
    dev = _dev(ctx)
    for dim, sub, n_t, tau, wins in picked:
        h0, h1, npts, st = engine.takens_rips_batch(wins, tau, dim=dim, subsample=sub, h1_cap=H1_CAP, ctx=ctx)
        clouds = np.stack([apc.takens_cloud(s, dim, tau, sub) for s in wins])
        c0, c1, cst = engine.cloud_rips_batch(clouds, normalise=True, h1_cap=H1_CAP, ctx=ctx)
        assert np.array_equal(st, cst) and np.all(npts == clouds.shape[1])
        out = engine.takens_rips_dev(torch.from_numpy(wins.copy()).to(dev), torch.full((len(wins),), tau, dtype=torch.int32, device=dev),
                                     dim=dim, subsample=sub, h1_cap=H1_CAP, ctx=ctx)
        torch.cuda.synchronize()
        d0, d1 = out.to_lists()
        assert np.array_equal(out.status.cpu().numpy(), st) and np.array_equal(out.n_points.cpu().numpy(), npts)
        for w in range(len(wins)):
            for a, b, c in ((h0[w], c0[w], d0[w]), (h1[w], c1[w], d1[w])):
                assert np.array_equal(brute.sort_rows(a), brute.sort_rows(b)), (dim, w)
                assert np.array_equal(brute.sort_rows(a), brute.sort_rows(c)), (dim, w)


# ------------------------------------------------------------------ explicit clouds
@pytest.mark.parametrize("normalise", [True, False])
def test_clouds_dim_1_2_4_equal_oracle(ctx, normalise):
    """Uniform and random-walk clouds of 3..128 points in 1, 2 and 4 dimensions, a quarter of them with every point twice;
    coordinates as given (threshold: twice the largest distance) or min-max normalised."""
    for kind, dim, P, pc in apc.cloud_cases():
        dm = port.cloud_dm(port.minmax_normalise(pc) if normalise else pc).astype(np.float32)
        th = 2.0 if normalise else float(np.float32(2.0) * dm.max())
        o = port.rips_f32(dm, thresh=th)
        h0, h1, st = engine.cloud_rips_batch(pc[None], normalise=normalise, thresh=th, h1_cap=H1_CAP, ctx=ctx)
        assert st[0] == 0, (kind, dim, P, st)
        assert _same_multiset(h0[0], o[0]) and _same_multiset(h1[0], o[1]), (kind, dim, P, normalise)


@pytest.mark.parametrize("normalise", [True, False])
def test_ragged_clouds_ignore_rows_past_n_pts(ctx, normalise):
    """Buffers (n_win, p_cap, dim) whose rows at and past n_pts[w] are NaN: valid windows equal the oracle on their own rows
    and hold no NaN, fewer than 3 points give [[0,0]],[[0,0]] (status 4), more than p_cap or 128 points status 16 and no
    rows, and every window gives what it gives alone in a buffer of exactly its size."""
    for p_cap, dim, buf, n_pts in apc.ragged_cloud_batches():
        h0, h1, st = engine.cloud_rips_batch(buf, n_pts=n_pts, normalise=normalise, h1_cap=H1_CAP, ctx=ctx)
        for w, n in enumerate(n_pts.tolist()):
            tag = (p_cap, dim, n, normalise)
            if n > min(p_cap, _lib.MAX_POINTS):
                assert st[w] == 16 and len(h0[w]) == 0 and len(h1[w]) == 0, tag
                continue
            if n < 3:
                assert st[w] == 4 and np.array_equal(h0[w], DEGENERATE) and np.array_equal(h1[w], DEGENERATE), tag
            else:
                pc = buf[w, :n]
                o = port.rips_f32(port.cloud_dm(port.minmax_normalise(pc) if normalise else pc).astype(np.float32))
                assert st[w] == 0, (tag, st[w])
                assert not np.isnan(h0[w]).any() and not np.isnan(h1[w]).any(), tag
                assert _same_multiset(h0[w], o[0]) and _same_multiset(h1[w], o[1]), tag
            if n >= 1:                                  # (a buffer without rows is not accepted: p_cap >= 1)
                a0, a1, ast = engine.cloud_rips_batch(buf[w:w + 1, :n], normalise=normalise, h1_cap=H1_CAP, ctx=ctx)
                assert ast[0] == st[w] and _same_multiset(a0[0], h0[w]) and _same_multiset(a1[0], h1[w]), tag


@pytest.mark.parametrize("words", [(2, 1), (2, 2)])
def test_lattice_in_four_dimensions_known_answer(ctx, words):
    """The k x k unit lattice (tests/test_oracle_golden.py has the argument) zero-padded to four coordinates: (k-1)^2 rows
    (1, sqrt 2) and k^2 H0 rows through the generic distance loop; k = 8: 49 classes alive at once (the 64-bit rung),
    k = 11: 121 points and 100 classes (the last rung, class vectors in HBM)."""
    from test_oracle_golden import lattice
    r2 = np.float64(np.float32(np.sqrt(2.0)))
    with _words(ctx, words):
        for k in (8, 11):
            pc = np.zeros((k * k, 4))
            pc[:, :2] = lattice(k)
            h0, h1, st = engine.cloud_rips_batch(pc[None], normalise=False, thresh=100.0, h1_cap=H1_CAP, ctx=ctx)
            assert st[0] == 0, (k, st)
            assert h1[0].shape == ((k - 1) ** 2, 2) and np.all(h1[0][:, 0] == 1.0) and np.all(h1[0][:, 1] == r2), k
            assert len(h0[0]) == k * k and np.all(h0[0][:-1, 1] == 1.0) and np.isinf(h0[0][-1, 1])


# ------------------------------------------------------------------ corr -> dist
def _corr_to_dist(corr, method):
    """nb2:105-120 in float64, one IEEE operation after the other: clip, the method's formula, max(., 0), zero diagonal."""
    with np.errstate(invalid="ignore"):
        r = np.minimum(np.maximum(corr, -1.0), 1.0)
        d = {"euclidean": lambda: np.sqrt(2.0 * (1.0 - r)),
             "abs": lambda: 1.0 - np.abs(r),
             "standard": lambda: 1.0 - r,
             "sqrt": lambda: np.sqrt(1.0 - r * r)}[method]()
        d = np.maximum(d, 0.0)
    i = np.arange(corr.shape[-1])
    d[..., i, i] = 0.0
    return d


def _same_bits(a, b):
    nan = np.isnan(b)
    return np.array_equal(a, b, equal_nan=True) and np.array_equal(np.signbit(a)[~nan], np.signbit(b)[~nan])


@pytest.mark.parametrize("method", list(engine.DIST_METHODS))
def test_corr_to_dist_every_method_bit_exact(ctx, method):
    """Pearson matrices of 1..129 channels, a stack of 500 (a second trip of the grid-stride loop, where the diagonal is
    found by idx % n^2) and a matrix of edge values: +-1 and the neighbours beyond, +-2, +-0, denormals, 1 - 2^-53 (whose
    square a contracted multiply-add would not round), NaN and +-inf, NaN and out-of-range values on the diagonal."""
    for name, corr in apc.corr_cases():
        got = engine.corr_to_dist_batch(corr, method, ctx=ctx)
        assert _same_bits(got, _corr_to_dist(corr, method)), (name, method)
        one = graphs.correlation_to_distance(corr[-1], method)
        assert _same_bits(one, got[-1]), (name, method)


def test_corr_to_dist_euclidean_reproduces_corr_dist(ctx):
    W = synth.eeg_windows(5, seed=3)
    W[1, 5] = 1.25                       # zero-variance channel: correlation NaN -> 0
    W[2, 11] = W[2, 7]                   # duplicated channel: correlation 1
    corr, dist = engine.corr_dist_batch(W, ctx=ctx)
    assert _same_bits(engine.corr_to_dist_batch(corr, "euclidean", ctx=ctx), dist)
