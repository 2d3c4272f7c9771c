"""
The sublevel-set persistence kernel (csrc/sublevel.hip) against tests/sublevel_ref.py.

Rows, counts, indices and status are compared as BYTES, whole buffers at once: the buffers go in filled with NaN / -1, the
reference leaves the same fill outside rows [0, cnt), so one comparison checks the rows, their order, the indices, the
counts, the status words and that nothing else was written.  Births and deaths are copies of input samples, so there is
no tolerance anywhere.
"""
import itertools

import numpy as np
import pytest

import sublevel_ref as ref
from tda_eeg_audio_amd import _lib, engine, utils

pytestmark = pytest.mark.gpu

# lane (63..65), wave (250..257: four samples per lane), layout (511..513: the wave kernels end at 512, a workgroup per
# signal from 513 on) and the two ends of the range
N_T = [1, 2, 3, 63, 64, 65, 250, 256, 257, 511, 512, 513, 4096]


def _dev(ctx):
    import torch
    return torch.device("cuda", ctx.device)


def _kinds(n_t, rng):
    """One signal of every kind the issue lists, (13, n_t): 13 signals do not fill the last workgroup of four."""
    i = np.arange(n_t, dtype=np.float64)
    plateau = rng.standard_normal(n_t)
    k = max(1, n_t // 5)
    plateau[:k] = plateau[k - 1]
    plateau[n_t - k:] = plateau[n_t - k]
    return np.stack([rng.standard_normal(n_t), rng.standard_normal(n_t), rng.standard_normal(n_t) * 1e-3 + 7.0,
                     rng.integers(0, 2, n_t).astype(np.float64), rng.integers(0, 2, n_t).astype(np.float64),
                     rng.integers(0, 3, n_t).astype(np.float64), rng.integers(0, 3, n_t).astype(np.float64),
                     np.full(n_t, -2.5), i * 0.5 - 3.0, -i * 0.25, (i % 2) + 1e-3 * i,      # the last: TDA_SL_ROWS rows
                     plateau, np.round(np.cumsum(rng.standard_normal(n_t)))])


def _run_dev(sigs, ctx, cap=None, n_ch=None, tables=None, want_index=True):
    """The _dev form on pre-filled buffers -> host (dgm, cnt, idx, status)."""
    import torch
    dev = _dev(ctx)
    if tables is None:
        sig_t = torch.from_numpy(np.ascontiguousarray(sigs)).to(dev)
        n_sig, n_t = int(np.prod(sigs.shape[:-1])), sigs.shape[-1]
        kw = {}
    else:
        start, ld, n_ch, n_t = tables
        sig_t = torch.from_numpy(np.ascontiguousarray(sigs).reshape(-1)).to(dev)
        n_sig = len(start) * n_ch
        kw = dict(n_t=n_t, n_ch=n_ch, win_start_t=torch.from_numpy(start).to(dev), win_ld_t=torch.from_numpy(ld).to(dev))
    cap = ref.rows_bound(n_t) if cap is None else cap
    dgm = torch.full((n_sig, cap, 2), float("nan"), dtype=torch.float64, device=dev)
    idx = torch.full((n_sig, cap, 2), -1, dtype=torch.int32, device=dev) if want_index else None
    cnt = torch.full((n_sig,), -5, dtype=torch.int32, device=dev)
    st = torch.full((n_sig,), -5, dtype=torch.int32, device=dev)
    engine.sublevel_dev(sig_t, dgm_t=dgm, cnt_t=cnt, idx_t=idx, status_t=st, cap=cap, ctx=ctx, **kw)
    torch.cuda.synchronize()
    return dgm.cpu().numpy(), cnt.cpu().numpy(), None if idx is None else idx.cpu().numpy(), st.cpu().numpy()


def _assert_bytes(got, want):
    for g, w, name in zip(got, want, ("dgm", "cnt", "idx", "status")):
        if g is None:
            continue
        assert g.shape == w.shape and g.dtype == w.dtype, name
        if g.tobytes() != w.tobytes():
            bad = np.flatnonzero([g[s].tobytes() != w[s].tobytes() for s in range(g.shape[0])])
            raise AssertionError(f"{name}: signals {bad[:8].tolist()} differ; first: got {g[bad[0]]!r} want {w[bad[0]]!r}")


@pytest.mark.parametrize("n_t", N_T)
def test_boundary_lengths_every_kind(ctx, n_t):
    sigs = _kinds(n_t, np.random.default_rng(100 + n_t))
    cap = ref.rows_bound(n_t) + 1                                   # a row more than the bound: it stays the fill
    _assert_bytes(_run_dev(sigs, ctx, cap=cap), ref.sublevel_batch(sigs, cap=cap))
    if n_t >= 3:
        assert ref.sublevel_batch(sigs[10:11])[1][0] == ref.rows_bound(n_t)      # the alternating signal fills the bound


@pytest.mark.parametrize("n_t", [3, 250, 513])
def test_47_channels(ctx, n_t):
    """(n_win, 47, n_t) stacked windows: signal w * 47 + c; 94 signals leave the last workgroup of four half empty."""
    rng = np.random.default_rng(47 + n_t)
    sigs = np.concatenate([_kinds(n_t, rng) for _ in range(8)])[:94].reshape(2, 47, n_t)
    _assert_bytes(_run_dev(sigs, ctx), ref.sublevel_batch(sigs.reshape(94, n_t)))


def test_rising_sawtooth_4096(ctx):
    """The quadratic worst case: every one of the 2,047 maxima scans back to sample 0.  Two signals only."""
    i = np.arange(4096, dtype=np.float64)
    sigs = np.stack([i + 2.0 * (i % 2), 0.5 * i + 3.0 * (i % 2)])
    want = ref.sublevel_batch(sigs)
    assert want[1].tolist() == [2048, 2048]
    _assert_bytes(_run_dev(sigs, ctx), want)


@pytest.mark.parametrize("n", range(1, 8))
def test_exhaustive_three_values(ctx, n):
    sigs = np.array(list(itertools.product((0.0, 1.0, 2.0), repeat=n)))
    _assert_bytes(_run_dev(sigs, ctx), ref.sublevel_batch(sigs))


@pytest.mark.parametrize("n_t", [250, 600])
@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_non_finite_sample_flags_its_signal_only(ctx, n_t, bad):
    sigs = _kinds(n_t, np.random.default_rng(7))[:9]
    clean = _run_dev(sigs, ctx)
    sigs[4, n_t - 1] = bad                                          # the last sample: the last lane's last load
    got = _run_dev(sigs, ctx)
    assert got[1][4] == 0 and got[3][4] == _lib.TDA_WIN_NOT_FINITE and np.isnan(got[0][4]).all() and (got[2][4] == -1).all()
    _assert_bytes(got, ref.sublevel_batch(sigs))
    for s in (3, 5):                                                # the neighbours: the bytes of the clean batch
        assert all(g[s].tobytes() == c[s].tobytes() for g, c in zip(got, clean))


@pytest.mark.parametrize("n_t", [250, 600])
def test_alone_and_in_batch_same_bytes(ctx, n_t):
    sigs = _kinds(n_t, np.random.default_rng(11))
    batch = _run_dev(sigs, ctx)
    for s in (0, 5, 12):
        alone = _run_dev(sigs[s:s + 1], ctx)
        assert all(a[0].tobytes() == b[s].tobytes() for a, b in zip(alone, batch))


def test_without_index_buffer(ctx):
    sigs = _kinds(250, np.random.default_rng(3))
    _assert_bytes(_run_dev(sigs, ctx, want_index=False), ref.sublevel_batch(sigs))


@pytest.mark.parametrize("n_ch, L", [(3, 700), (1, 1000)])
def test_table_addressing_reads_windows_in_place(ctx, n_ch, L):
    """Overlapping windows (step 62) of packed recordings of two lengths, rows win_ld = L_r != n_t apart, against the same
    windows stacked."""
    rng = np.random.default_rng(62)
    n_t, step, lens = 250, 62, [L, L + 131]
    recs = [np.round(rng.standard_normal((n_ch, l)), 1) for l in lens]
    flat = np.concatenate([r.reshape(-1) for r in recs])
    off = np.concatenate([[0], np.cumsum([n_ch * l for l in lens])])
    start, ld, stacked = [], [], []
    for r, l in enumerate(lens):
        for k in range((l - n_t) // step + 1):
            start.append(off[r] + k * step); ld.append(l)
            stacked.append(recs[r][:, k * step:k * step + n_t])
    start, ld, stacked = np.array(start, np.int64), np.array(ld, np.int64), np.stack(stacked)
    in_place = _run_dev(flat, ctx, tables=(start, ld, n_ch, n_t))
    _assert_bytes(in_place, _run_dev(stacked, ctx))
    _assert_bytes(in_place, ref.sublevel_batch(stacked.reshape(-1, n_t)))
    host = engine.sublevel_batch(flat, n_t=n_t, win_start=start, win_ld=ld, n_ch=n_ch, ctx=ctx)
    _assert_bytes(host, in_place)


def test_refusals_launch_nothing(ctx):
    import torch
    dev = _dev(ctx)
    ok = np.zeros((2, 3, 9))

    def refused(sig, **kw):
        n_sig = 6
        cap = kw.pop("cap", 5)
        bufs = dict(dgm_t=torch.full((n_sig, max(cap, 8), 2), float("nan"), dtype=torch.float64, device=dev),
                    idx_t=torch.full((n_sig, max(cap, 8), 2), -1, dtype=torch.int32, device=dev),
                    cnt_t=torch.full((n_sig,), -5, dtype=torch.int32, device=dev),
                    status_t=torch.full((n_sig,), -5, dtype=torch.int32, device=dev))
        with pytest.raises(_lib.TdaError):
            engine.sublevel_dev(torch.from_numpy(sig).to(dev), cap=cap, ctx=ctx, **bufs, **kw)
        torch.cuda.synchronize()
        assert torch.isnan(bufs["dgm_t"]).all() and (bufs["idx_t"] == -1).all()
        assert (bufs["cnt_t"] == -5).all() and (bufs["status_t"] == -5).all()
        with pytest.raises(_lib.TdaError):
            engine.sublevel_batch(sig, cap=cap, ctx=ctx)

    refused(ok, cap=ref.rows_bound(9) - 1)                          # cap < TDA_SL_ROWS(n_t)
    refused(np.zeros((2, 3, 0)))                                    # n_t < 1
    refused(np.zeros((1, 1, _lib.SL_MAX_SAMPLES + 1)), cap=_lib.SL_MAX_SAMPLES)          # n_t > TDA_SL_MAX_SAMPLES
    refused(np.zeros((2, 0, 9)))                                    # n_ch < 1
    # ... and through the tables, where the sizes are arguments of their own
    flat, tab = torch.zeros(64, dtype=torch.float64, device=dev), torch.zeros(2, dtype=torch.int64, device=dev)
    for n_ch, n_t, cap in ((0, 9, 5), (3, 0, 5), (3, _lib.SL_MAX_SAMPLES + 1, 4096), (3, 9, 4)):
        with pytest.raises(_lib.TdaError):
            engine.sublevel_dev(flat, n_t=n_t, win_start_t=tab, win_ld_t=tab, n_ch=n_ch, cap=cap, ctx=ctx)
    with pytest.raises(_lib.TdaError):                              # one table without the other
        ctx.check(ctx.lib.tda_sublevel_batch_dev(ctx.h, engine._tp(flat), engine._tp(tab), None, 2, 1, 9, engine._tp(flat), 5,
                                                 engine._tp(tab), None, engine._tp(tab), None))
    assert _lib.SL_MAX_SAMPLES == 4096 and engine.sublevel_rows(4096) == 2048
    # the limits themselves are accepted
    _assert_bytes(_run_dev(ok, ctx), ref.sublevel_batch(ok.reshape(6, 9)))


@pytest.mark.parametrize("n_t", [65, 250, 700])
def test_host_twin_equals_dev_form(ctx, n_t):
    sigs = _kinds(n_t, np.random.default_rng(5))
    sigs[2, 0] = np.nan
    cap = ref.rows_bound(n_t) + 2
    dgm = np.full((13, cap, 2), np.nan)
    idx = np.full((13, cap, 2), -1, np.int32)
    host = engine.sublevel_batch(sigs, cap=cap, dgm=dgm, idx=idx, ctx=ctx)
    _assert_bytes(host, _run_dev(sigs, ctx, cap=cap))
    _assert_bytes(host, ref.sublevel_batch(sigs, cap=cap))
    if n_t == 65:                                                   # idx = NULL: the rows, counts and status words alone
        p, s = engine.ptr, engine.f64(sigs)
        d2, c2, st2 = np.full((13, cap, 2), np.nan), np.zeros(13, np.int32), np.zeros(13, np.int32)
        ctx.check(ctx.lib.tda_sublevel_batch(ctx.h, p(s), None, None, 13, 1, n_t, p(d2), cap, p(c2), None, p(st2)))
        assert d2.tobytes() == host[0].tobytes() and c2.tobytes() == host[1].tobytes() and st2.tobytes() == host[3].tobytes()


def test_utils_compute_sublevel_persistence(ctx):
    inf = np.inf
    d, i = utils.compute_sublevel_persistence([3, 1, 4, 1, 5, 9, 2, 6], return_index=True)
    assert d.tolist() == [[1, 4], [2, 9], [1, inf]] and i.tolist() == [[3, 2], [6, 5], [1, -1]]
    assert d.dtype == np.float64 and i.dtype == np.int32
    assert utils.compute_sublevel_persistence([1, 0, 1, 0, 1]).tolist() == [[0, 1], [0, inf]]
    assert utils.compute_sublevel_persistence([2, 2, 2]).tolist() == [[2, inf]]
    assert utils.compute_sublevel_persistence([5]).tolist() == [[5, inf]]
    x = np.random.default_rng(9).standard_normal((5, 250))
    many = utils.compute_sublevel_persistence(x)
    assert isinstance(many, list) and len(many) == 5
    for s in range(5):
        want = ref.sublevel_union_find(x[s])
        assert many[s].tobytes() == want[0].tobytes()
        assert utils.compute_sublevel_persistence(-x[s]).tobytes() == ref.sublevel_union_find(-x[s])[0].tobytes()
    with pytest.raises(ValueError):
        utils.compute_sublevel_persistence([1.0, np.nan, 0.0])
    with pytest.raises(ValueError):
        utils.compute_sublevel_persistence(np.zeros((2, 2, 2)))
    with pytest.raises(_lib.TdaError):
        utils.compute_sublevel_persistence(np.zeros(_lib.SL_MAX_SAMPLES + 1))
