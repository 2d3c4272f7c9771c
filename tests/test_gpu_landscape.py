"""
The landscape kernel (csrc/landscape.hip) against tests/landscape_ref.py.  Every comparison is np.array_equal: the kernel
has to give the bits of the written definition (equal_nan only where a group without a kept diagram is NaN by
definition).
"""
import numpy as np
import pytest

import landscape_ref as lr
from tda_eeg_audio_amd import engine, utils
from tda_eeg_audio_amd._lib import TdaError

pytestmark = pytest.mark.gpu

GRID64 = np.linspace(0.0, 2.0, 64)
CONTENTS = ["f64", "f32", "inf", "all_inf", "dup", "zero", "h0"]


def _content(rng, k, what):
    if what == "f32":
        return lr.random_diagram(rng, k, kind="f32")
    if what == "inf":
        return lr.random_diagram(rng, k, kind="f32", n_inf=max(1, k // 4))
    if what == "all_inf":
        return lr.random_diagram(rng, k, n_inf=k)
    if what == "dup":                                               # tied tents: few distinct rows, repeated
        base = lr.random_diagram(rng, 3, kind="f32")
        return base[rng.integers(0, 3, k)]
    if what == "zero":                                              # zero-persistence rows among ordinary ones
        d = lr.random_diagram(rng, k)
        d[::2, 1] = d[::2, 0]
        return d
    if what == "h0":
        return lr.random_diagram(rng, k, kind="f32", h0=True, n_inf=1)
    return lr.random_diagram(rng, k)


def _pack(dgms, cap, over=()):
    """Diagram buffers of capacity cap; the diagrams in `over` report more rows than the buffer has."""
    rows = np.zeros((len(dgms), cap, 2)); cnt = np.zeros(len(dgms), np.int32)
    for i, d in enumerate(dgms):
        rows[i, :len(d)] = d
        cnt[i] = len(d) + (7 if i in over else 0)
    return rows, cnt


def _gpu(ctx, rows, cnt, grid, K, seg_off=None, status=None, mask=0, out=None):
    import torch
    dev = torch.device("cuda", ctx.device)
    t = lambda a, dt: None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)
    out_t = None if out is None else torch.from_numpy(out).to(dev)
    got = engine.landscape_mean_dev(t(rows, np.float64), t(cnt, np.int32), t(grid, np.float64), K, seg_off_t=t(seg_off, np.int32),
                                    status_t=t(status, np.int32), skip_mask=mask, out_t=out_t, ctx=ctx)
    torch.cuda.synchronize()
    return got.cpu().numpy()


@pytest.mark.parametrize("cap", [47, 128, 256])
@pytest.mark.parametrize("K", [1, 5, 8])
def test_row_counts_and_contents(ctx, cap, K):
    rng = np.random.default_rng(1000 * cap + K)
    counts = sorted({c for c in (0, 1, K - 1, K, K + 1, 63, 64, 65, cap) if 0 <= c <= cap})
    dgms = [_content(rng, k, what) if k else np.zeros((0, 2)) for k in counts for what in CONTENTS]
    dgms.append(lr.random_diagram(rng, cap, kind="f32"))            # full buffer whose count says cap + 7: cap rows
    rows, cnt = _pack(dgms, cap, over={len(dgms) - 1})
    assert cnt[-1] > cap
    got = _gpu(ctx, rows, cnt, GRID64, K)
    want = lr.landscape_mean(rows, cnt, GRID64, K)
    assert got.shape == (len(dgms), K + 1, 64)
    assert np.array_equal(got, want)
    assert want[:, :K].any() and want[:, K].any()


def _exact_grid():
    """Hits births, deaths and midpoints of the rows of _exact_rows exactly."""
    r = _exact_rows()
    fin = r[np.isfinite(r[:, 1])]
    return np.unique(np.concatenate([r[:, 0], fin[:, 1], (fin[:, 0] + fin[:, 1]) / 2]))


def _exact_rows():
    return np.array([[0.0, 1.0], [0.0, 2.0], [0.5, 1.5], [0.0, np.inf], [0.25, 0.75], [0.25, 0.75], [1.0, 1.0], [0.125, 1.875]])


GRIDS = {
    "n1": np.array([0.7]), "n63": np.linspace(0.0, 2.0, 63), "n64": GRID64, "n65": np.linspace(0.0, 2.0, 65),
    "n256": np.linspace(0.0, 2.0, 256), "exact": _exact_grid(),
    "nonuniform": np.sort(np.random.default_rng(9).uniform(-0.5, 2.5, 100)) ** 3,
    "descending": np.linspace(2.0, 0.0, 130),
}


@pytest.mark.parametrize("name", list(GRIDS))
def test_grids(ctx, name):
    grid = GRIDS[name]
    rng = np.random.default_rng(len(grid))
    dgms = [_exact_rows(), np.zeros((0, 2))] + [_content(rng, int(rng.integers(1, 128)), w) for w in CONTENTS]
    dgms.append(lr.random_diagram(rng, 1000, kind="f32"))           # the capacity of the large Rips buffers: 16 chunks
    for cap, some in ((128, dgms[:-1]), (1024, dgms[-3:])):
        rows, cnt = _pack(some, cap)
        for K in (5, 8):
            got = _gpu(ctx, rows, cnt, grid, K)
            assert got.shape == (len(some), K + 1, len(grid))
            assert np.array_equal(got, lr.landscape_mean(rows, cnt, grid, K)), (cap, K)


@pytest.fixture(scope="module")
def grouped():
    """Groups of 0, 1, 2, 15 and 89 diagrams in one call, and their reference vectors (computed once)."""
    rng = np.random.default_rng(77)
    sizes = [0, 1, 2, 15, 89, 0, 15]
    seg_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    n = int(seg_off[-1])
    ks = rng.integers(0, 100, n)
    dgms = [_content(rng, int(k), CONTENTS[i % len(CONTENTS)]) if k else np.zeros((0, 2)) for i, k in enumerate(ks)]
    rows, cnt = _pack(dgms, 128)
    return dict(rows=rows, cnt=cnt, seg_off=seg_off, n=n, sizes=sizes)


def test_groups(ctx, grouped):
    g = grouped
    K = 5
    got = _gpu(ctx, g["rows"], g["cnt"], GRID64, K, seg_off=g["seg_off"])
    want = lr.landscape_mean(g["rows"], g["cnt"], GRID64, K, seg_off=g["seg_off"])
    assert got.shape == (len(g["sizes"]), K + 1, 64)
    assert np.isnan(want[0]).all() and np.isnan(want[5]).all() and np.isfinite(want[[1, 2, 3, 4, 6]]).all()
    assert np.array_equal(got, want, equal_nan=True)
    assert np.isnan(got[0]).all() and np.isnan(got[5]).all()
    # a group of one diagram is the diagram's own vector
    w = int(g["seg_off"][1])
    assert np.array_equal(got[1], lr.diagram_vector(lr.cut(g["rows"][w], g["cnt"][w]), GRID64, K))


def test_status_mask(ctx, grouped):
    g = grouped
    K = 5
    rng = np.random.default_rng(78)
    status = np.where(rng.random(g["n"]) < 0.3, 4, 0).astype(np.int32)
    status[rng.random(g["n"]) < 0.1] |= 16
    status[rng.random(g["n"]) < 0.2] |= 1                           # a bit outside the mask removes nothing
    s0, s1 = g["seg_off"][3], g["seg_off"][4]
    status[s0:s1] = 4                                               # every window of the group of 15: NaN
    status[g["seg_off"][4]] = 16                                    # the first window of the group of 89
    mask = 4 | 16
    got = _gpu(ctx, g["rows"], g["cnt"], GRID64, K, seg_off=g["seg_off"], status=status, mask=mask)
    want = lr.landscape_mean(g["rows"], g["cnt"], GRID64, K, seg_off=g["seg_off"], status=status, skip_mask=mask)
    assert np.isnan(want[3]).all() and np.isfinite(want[4]).all()
    assert np.array_equal(got, want, equal_nan=True)
    unmasked = _gpu(ctx, g["rows"], g["cnt"], GRID64, K, seg_off=g["seg_off"], status=status, mask=0)
    assert np.array_equal(unmasked, lr.landscape_mean(g["rows"], g["cnt"], GRID64, K, seg_off=g["seg_off"]), equal_nan=True)


def test_null_seg_off_and_525_diagrams(ctx):
    rng = np.random.default_rng(525)
    dgms = [lr.random_diagram(rng, int(rng.integers(1, 47)), kind="f32", h0=i % 2 == 0) for i in range(525)]
    rows, cnt = _pack(dgms, 47)
    got = _gpu(ctx, rows, cnt, GRID64, 5)
    assert got.tobytes() == _gpu(ctx, rows, cnt, GRID64, 5, seg_off=np.arange(526)).tobytes()
    assert np.array_equal(got, lr.landscape_mean(rows, cnt, GRID64, 5))
    seg = np.array([0, 89, 200, 525], np.int32)
    assert np.array_equal(_gpu(ctx, rows, cnt, GRID64, 5, seg_off=seg), lr.landscape_mean(rows, cnt, GRID64, 5, seg_off=seg))


def test_row_order_does_not_matter(ctx):
    rng = np.random.default_rng(31)
    dgms = [_content(rng, k, w) for k, w in zip((5, 64, 100, 128, 77, 33, 90), CONTENTS)]
    rows, cnt = _pack(dgms, 128)
    perm = rows.copy()
    for i, d in enumerate(dgms):
        perm[i, :len(d)] = d[rng.permutation(len(d))]
    assert (perm != rows).any()
    for K in (1, 8):
        assert _gpu(ctx, rows, cnt, GRID64, K).tobytes() == _gpu(ctx, perm, cnt, GRID64, K).tobytes()


@pytest.mark.parametrize("cap,n_grid,K", [(47, 64, 0), (47, 64, 9), (47, 0, 5), (47, 257, 5), (0, 64, 5)])
def test_invalid_arguments_launch_nothing(ctx, cap, n_grid, K):
    import torch
    dev = torch.device("cuda", ctx.device)
    rows = torch.zeros((3, max(cap, 1), 2), dtype=torch.float64, device=dev)
    cnt = torch.ones(3, dtype=torch.int32, device=dev)
    grid = torch.zeros(n_grid, dtype=torch.float64, device=dev)
    out = torch.full((3, 10, 257), -7.0, dtype=torch.float64, device=dev)
    rc = ctx.lib.tda_landscape_mean_dev(ctx.h, engine._tp(rows), engine._tp(cnt), cap, 3, None, 3, None, 0, engine._tp(grid),
                                        n_grid, K, engine._tp(out), None)
    torch.cuda.synchronize()
    assert rc != 0
    with pytest.raises(TdaError):
        ctx.check(rc)
    assert bool((out == -7.0).all())
    if cap >= 1 and n_grid >= 1:
        with pytest.raises(TdaError):
            engine.landscape_batch(np.zeros((3, cap, 2)), np.ones(3, np.int32), np.zeros(n_grid), K, ctx=ctx)


def test_host_and_deferred_paths(ctx):
    rng = np.random.default_rng(12)
    dgms = [_exact_rows(), np.zeros((0, 2)), lr.random_diagram(rng, 40, kind="f32", n_inf=2), lr.random_diagram(rng, 7, h0=True)]
    rows, cnt = _pack(dgms, 40)
    grid = np.linspace(0.0, 2.0, 33)
    host = engine.landscape_batch(rows, cnt, grid, 5, ctx=ctx)
    assert np.array_equal(host, lr.landscape_mean(rows, cnt, grid, 5))
    now = []
    for d in dgms:
        lam, beta = utils.persistence_landscape(d, grid, levels=3), utils.betti_curve(d, grid)
        want = lr.diagram_vector(d, grid, 3)
        assert lam.shape == (3, 33) and beta.shape == (33,)
        assert np.array_equal(lam, want[:3]) and np.array_equal(beta, want[3])
        now.append((lam, beta))
    dflt = utils.persistence_landscape(dgms[0])
    assert dflt.shape == (5, 64) and np.array_equal(dflt, lr.diagram_vector(dgms[0], utils.default_landscape_grid(), 5)[:5])
    with utils.batch():
        later = [(utils.persistence_landscape(d, grid, levels=3), utils.betti_curve(d, grid)) for d in dgms]
        other = utils.persistence_landscape(dgms[2], levels=8)      # another grid, more levels: its own launch
        with pytest.raises(ValueError):
            utils.betti_curve(np.zeros((2, 3)), grid)
    for (lam, beta), (lam_d, beta_d) in zip(now, later):
        assert np.asarray(lam_d).tobytes() == lam.tobytes() and np.asarray(beta_d).tobytes() == beta.tobytes()
        assert lam_d.shape == (3, 33) and beta_d.shape == (33,)
    assert np.array_equal(np.asarray(other), lr.diagram_vector(dgms[2], utils.default_landscape_grid(), 8)[:8])
