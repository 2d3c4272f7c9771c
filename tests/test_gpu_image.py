"""
The persistence-image kernel (csrc/image.hip) against tests/image_ref.py (float64 numpy, scipy's erfc).  The kernel uses the
device library's erfc, so the comparison is

    |gpu - ref| <= (C * W_g + N_g * |ref|) * 2^-53                  (image_ref.tolerance, image_ref.C)

and np.array_equal where the definition demands the same bytes.  Every comparison prints q = max |gpu - ref| / (2^-53 W_g)
before it asserts: C is 4 x the largest q of this file on an MI355X, rounded up to a power of two (image_ref.C has the
figures).
"""
import numpy as np
import pytest

import image_ref as ir
from tda_eeg_audio_amd import engine, utils
from tda_eeg_audio_amd._lib import TdaError

pytestmark = pytest.mark.gpu

TDA_ERR_INVALID = 1                                                 # include/tdaeeg.h

CONTENTS = ["f64", "f32", "inf", "all_inf", "dup", "zero", "h0"]
XE20, YE20 = np.linspace(0.0, 2.0, 21), np.linspace(0.0, 0.7, 21)


def _content(rng, k, what):
    if what == "f32":
        return ir.random_diagram(rng, k, kind="f32")
    if what == "inf":
        return ir.random_diagram(rng, k, kind="f32", n_inf=max(1, k // 4))
    if what == "all_inf":
        return ir.random_diagram(rng, k, n_inf=k)
    if what == "dup":                                               # few distinct rows, repeated
        base = ir.random_diagram(rng, 3, kind="f32")
        return base[rng.integers(0, 3, k)]
    if what == "zero":                                              # zero-persistence rows among ordinary ones
        d = ir.random_diagram(rng, k)
        d[::2, 1] = d[::2, 0]
        return d
    if what == "h0":                                                # every birth 0, one essential class
        return ir.random_diagram(rng, k, kind="f32", h0=True, n_inf=1)
    return ir.random_diagram(rng, k)


def _pack(dgms, cap, over=()):
    """Diagram buffers of capacity cap; the diagrams in `over` report 7 rows more than they (and the buffer) have."""
    rows = np.zeros((len(dgms), cap, 2)); cnt = np.zeros(len(dgms), np.int32)
    for i, d in enumerate(dgms):
        rows[i, :len(d)] = d
        cnt[i] = len(d) + (7 if i in over else 0)
    return rows, cnt


def _gpu(ctx, rows, cnt, xe, ye, sigma, power, seg_off=None, status=None, mask=0):
    import torch
    dev = torch.device("cuda", ctx.device)
    t = lambda a, dt: None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)
    got = engine.image_mean_dev(t(rows, np.float64), t(cnt, np.int32), t(xe, np.float64), t(ye, np.float64), sigma, power,
                                seg_off_t=t(seg_off, np.int32), status_t=t(status, np.int32), skip_mask=mask, ctx=ctx)
    torch.cuda.synchronize()
    return got.cpu().numpy()


def _close(got, ref, what):
    """The tolerance of this file, q printed first.  ref = (mean, W, N) of image_ref; NaN (a group without a kept diagram)
    has to be NaN on both sides."""
    mean, W, N = ref
    assert got.shape == mean.shape, what
    nan = np.isnan(mean)
    assert np.array_equal(np.isnan(got), nan), what
    err = np.where(nan, 0.0, np.abs(got - mean))
    live = W > 0
    q = float((err[live].reshape(live.sum(), -1).max(axis=1) / (ir.EPS * W[live])).max()) if live.any() else 0.0
    print(f"q = {q:.3f}   [{what}]")
    tol = np.where(nan, 0.0, ir.tolerance(np.where(nan, 0.0, mean), W, N, ir.C))
    assert (err <= tol).all(), (what, q, float((err - tol).max()))
    return q


@pytest.mark.parametrize("cap", [47, 128])
@pytest.mark.parametrize("power", [0, 1, 2])
def test_row_counts_and_contents(ctx, cap, power):
    rng = np.random.default_rng(1000 * cap + power)
    counts = sorted({c for c in (0, 1, 63, 64, 65, cap) if c <= cap})
    dgms = [_content(rng, k, what) if k else np.zeros((0, 2)) for k in counts for what in CONTENTS]
    dgms.append(ir.random_diagram(rng, cap, kind="f32"))            # full buffer whose count says cap + 7: cap rows
    rows, cnt = _pack(dgms, cap, over={len(dgms) - 1})
    assert cnt[-1] == cap + 7
    got = _gpu(ctx, rows, cnt, XE20, YE20, 0.05, power)
    ref = ir.image_mean(rows, cnt, XE20, YE20, 0.05, power)
    _close(got, ref, f"cap {cap} power {power}")
    assert (got >= 0).all() and got.any()
    empty = [i for i, d in enumerate(dgms) if not np.isfinite(d).all(axis=1).any()]
    assert len(empty) >= 2 and not got[empty].any()                 # an empty F: all zeros, not NaN


def test_thousand_rows_in_a_1024_buffer(ctx):
    rng = np.random.default_rng(1024)
    dgms = [ir.random_diagram(rng, 1000, kind="f32"), _content(rng, 1000, "inf"), _content(rng, 33, "h0")]
    rows, cnt = _pack(dgms, 1024)
    for power in (0, 2):
        _close(_gpu(ctx, rows, cnt, XE20, YE20, 0.05, power), ir.image_mean(rows, cnt, XE20, YE20, 0.05, power),
               f"1000 rows power {power}")


def _edges(name):
    rng = np.random.default_rng(17)
    if name == "nonuniform":                                        # 13 x 9, irregular widths
        return np.sort(rng.uniform(-0.2, 1.8, 14)), np.concatenate([[0.0], np.sort(rng.uniform(0.001, 0.7, 9))])
    n_x, n_y = name
    return np.linspace(-0.1, 1.7, n_x + 1), np.linspace(0.0, 0.7, n_y + 1)


@pytest.fixture(scope="module")
def mixed():
    """One diagram of every content, 1 to 127 rows, and an empty one, in buffers of 128 rows."""
    rng = np.random.default_rng(4)
    dgms = [np.zeros((0, 2))] + [_content(rng, int(rng.integers(1, 128)), w) for w in CONTENTS]
    return _pack(dgms, 128)


@pytest.mark.parametrize("sides", [(1, 1), (1, 32), (32, 1), (32, 32), (20, 20), (7, 5), "nonuniform"], ids=str)
def test_image_sides_and_edges(ctx, mixed, sides):
    rows, cnt = mixed
    xe, ye = _edges(sides)
    for power, sigma in ((1, 0.05), (0, 0.2)):
        got = _gpu(ctx, rows, cnt, xe, ye, sigma, power)
        assert got.shape == (len(cnt), len(ye) - 1, len(xe) - 1)
        _close(got, ir.image_mean(rows, cnt, xe, ye, sigma, power), f"sides {sides} power {power} sigma {sigma}")


def test_axes(ctx):
    """7 x 5: a point of large birth and small persistence lights row 0 (persistence), column 6 (birth)."""
    xe, ye = np.linspace(0.0, 1.4, 8), np.linspace(0.0, 0.5, 6)
    rows, cnt = _pack([np.array([[1.3, 1.35]]), np.array([[0.1, 0.55]])], 4)
    got = _gpu(ctx, rows, cnt, xe, ye, 0.02, 1)
    assert got.shape == (2, 5, 7)
    assert np.unravel_index(np.argmax(got[0]), (5, 7)) == (0, 6) and np.unravel_index(np.argmax(got[1]), (5, 7)) == (4, 0)


def test_edges_far_from_every_point(ctx, mixed):
    """No mass there: every pixel is at most the tolerance (the reference is 0 or a denormal-sized tail)."""
    rows, cnt = mixed
    xe, ye = np.linspace(50.0, 60.0, 8), np.linspace(40.0, 45.0, 6)
    ref = ir.image_mean(rows, cnt, xe, ye, 0.05, 1)
    got = _gpu(ctx, rows, cnt, xe, ye, 0.05, 1)
    _close(got, ref, "far edges")
    assert (np.abs(got) <= ir.tolerance(ref[0], ref[1], ref[2], ir.C)).all()


@pytest.mark.parametrize("sigma", [0.001, 0.05, 5.0])
@pytest.mark.parametrize("power", [0, 1, 2])
def test_width_and_weight(ctx, mixed, sigma, power):
    """sigma 0.001: the mass of a point sits in single pixels; sigma 5: nearly flat."""
    rows, cnt = mixed
    got = _gpu(ctx, rows, cnt, XE20, YE20, sigma, power)
    _close(got, ir.image_mean(rows, cnt, XE20, YE20, sigma, power), f"sigma {sigma} power {power}")


@pytest.fixture(scope="module")
def grouped():
    """Groups of 0, 1, 2, 15, 89, 0 and 15 diagrams in one call."""
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
    got = _gpu(ctx, g["rows"], g["cnt"], XE20, YE20, 0.05, 1, seg_off=g["seg_off"])
    ref = ir.image_mean(g["rows"], g["cnt"], XE20, YE20, 0.05, 1, seg_off=g["seg_off"])
    assert got.shape == (len(g["sizes"]), 20, 20)
    assert np.isnan(ref[0][[0, 5]]).all() and np.isfinite(ref[0][[1, 2, 3, 4, 6]]).all()
    _close(got, ref, "groups")
    assert np.isnan(got[0]).all() and np.isnan(got[5]).all()
    # byte equality: the same call twice; a group of one against the seg_off = NULL call; a group inside the batch against
    # that group alone
    assert _gpu(ctx, g["rows"], g["cnt"], XE20, YE20, 0.05, 1, seg_off=g["seg_off"]).tobytes() == got.tobytes()
    each = _gpu(ctx, g["rows"], g["cnt"], XE20, YE20, 0.05, 1)
    assert each.shape == (g["n"], 20, 20)
    assert np.array_equal(each[int(g["seg_off"][1])], got[1])
    for grp in (3, 4):
        s0, s1 = int(g["seg_off"][grp]), int(g["seg_off"][grp + 1])
        alone = _gpu(ctx, g["rows"][s0:s1], g["cnt"][s0:s1], XE20, YE20, 0.05, 1, seg_off=np.array([0, s1 - s0]))
        assert np.array_equal(alone[0], got[grp]), grp


def test_status_mask(ctx, grouped):
    g = grouped
    rng = np.random.default_rng(78)
    status = np.where(rng.random(g["n"]) < 0.3, 4, 0).astype(np.int32)
    status[rng.random(g["n"]) < 0.1] |= 16
    status[rng.random(g["n"]) < 0.2] |= 1                           # a bit outside the mask removes nothing
    s0, s1 = g["seg_off"][3], g["seg_off"][4]
    status[s0:s1] = 4                                               # every window of the group of 15: NaN
    status[g["seg_off"][4]] = 16                                    # the first window of the group of 89
    mask = 4 | 16
    got = _gpu(ctx, g["rows"], g["cnt"], XE20, YE20, 0.05, 2, seg_off=g["seg_off"], status=status, mask=mask)
    ref = ir.image_mean(g["rows"], g["cnt"], XE20, YE20, 0.05, 2, seg_off=g["seg_off"], status=status, skip_mask=mask)
    assert np.isnan(ref[0][3]).all() and np.isfinite(ref[0][4]).all() and np.isfinite(ref[0][6]).all()
    _close(got, ref, "status mask")                                 # NaN exactly in the groups 0, 3 and 5
    unmasked = _gpu(ctx, g["rows"], g["cnt"], XE20, YE20, 0.05, 2, seg_off=g["seg_off"], status=status, mask=0)
    _close(unmasked, ir.image_mean(g["rows"], g["cnt"], XE20, YE20, 0.05, 2, seg_off=g["seg_off"]), "mask 0")


def test_seg_off_entries_outside_the_buffer(ctx, grouped):
    g = grouped
    n = g["n"]
    seg = np.array([-5, 3, 10, n + 40, n + 50], np.int32)           # clamped to [0, n]: [0,3) [3,10) [10,n) and none
    got = _gpu(ctx, g["rows"], g["cnt"], XE20, YE20, 0.05, 1, seg_off=seg)
    ref = ir.image_mean(g["rows"], g["cnt"], XE20, YE20, 0.05, 1, seg_off=seg)
    assert np.isnan(ref[0][3]).all() and np.isfinite(ref[0][:3]).all()
    _close(got, ref, "seg_off outside")
    assert np.array_equal(got[:3], _gpu(ctx, g["rows"], g["cnt"], XE20, YE20, 0.05, 1, seg_off=np.array([0, 3, 10, n])))


@pytest.mark.parametrize("power", [0, 1, 2])
def test_mass_is_conserved(ctx, power):
    """Edges reaching 8 sigma past every point: the pixels sum to W within N * 2^-52 * W, the bound of the reference."""
    rng = np.random.default_rng(5 + power)
    d = ir.random_diagram(rng, 50, kind="f32")
    rows, cnt = _pack([d], 64)
    sigma = 0.05
    xe, ye = np.linspace(0.0 - 8 * sigma, 1.5 + 8 * sigma, 21), np.linspace(0.0 - 8 * sigma, 0.6 + 8 * sigma, 14)
    got = _gpu(ctx, rows, cnt, xe, ye, sigma, power)
    ref = ir.image_mean(rows, cnt, xe, ye, sigma, power)
    _close(got, ref, f"mass power {power}")
    W, N = ref[1][0], ref[2][0]
    print(f"mass: |sum - W| / (2^-52 W) = {abs(got.sum() - W) / (2.0 ** -52 * W):.3f} of {N} allowed")
    assert abs(got.sum() - W) <= N * 2.0 ** -52 * W


INVALID = [dict(n_x=0), dict(n_x=33), dict(n_y=0), dict(n_y=33), dict(sigma=0.0), dict(sigma=-0.1), dict(sigma=float("nan")),
           dict(sigma=float("inf")), dict(power=3), dict(cap=0)]


@pytest.mark.parametrize("bad", INVALID, ids=lambda b: "%s=%s" % next(iter(b.items())))
def test_invalid_arguments_launch_nothing(ctx, bad):
    import torch
    dev = torch.device("cuda", ctx.device)
    a = dict(n_x=20, n_y=20, sigma=0.05, power=1, cap=47)
    a.update(bad)
    rows = torch.zeros((3, max(a["cap"], 1), 2), dtype=torch.float64, device=dev)
    cnt = torch.ones(3, dtype=torch.int32, device=dev)
    xe = torch.linspace(0, 2, 34, dtype=torch.float64, device=dev)
    ye = torch.linspace(0, 1, 34, dtype=torch.float64, device=dev)
    out = torch.full((3, 33, 33), -7.0, dtype=torch.float64, device=dev)
    rc = ctx.lib.tda_image_mean_dev(ctx.h, engine._tp(rows), engine._tp(cnt), a["cap"], 3, None, 3, None, 0, engine._tp(xe),
                                    a["n_x"], engine._tp(ye), a["n_y"], a["sigma"], a["power"], engine._tp(out), None)
    torch.cuda.synchronize()
    assert rc == TDA_ERR_INVALID
    with pytest.raises(TdaError):
        ctx.check(rc)
    assert bool((out == -7.0).all())
    if a["cap"] >= 1 and a["n_x"] >= 1 and a["n_y"] >= 1:           # the host twin: the same answer
        with pytest.raises(TdaError):
            engine.image_batch(np.zeros((3, a["cap"], 2)), np.ones(3, np.int32), np.linspace(0, 2, a["n_x"] + 1),
                               np.linspace(0, 1, a["n_y"] + 1), a["sigma"], a["power"], ctx=ctx)


def test_host_twin_rejects_bad_edges(ctx):
    rows, cnt = np.zeros((2, 4, 2)), np.ones(2, np.int32)
    for xe in ([0.0, 1.0, 1.0], [0.0, np.nan, 2.0], [0.0, np.inf], [1.0, 0.5]):
        with pytest.raises(TdaError):
            engine.image_batch(rows, cnt, xe, [0.0, 1.0], 0.1, 1, ctx=ctx)
        with pytest.raises(TdaError):
            engine.image_batch(rows, cnt, [0.0, 1.0], xe, 0.1, 1, ctx=ctx)


def test_host_and_deferred_paths(ctx):
    rng = np.random.default_rng(12)
    dgms = [np.array([[0.0, 1.0], [0.25, 0.75], [0.0, np.inf]]), np.zeros((0, 2)), ir.random_diagram(rng, 40, kind="f32", n_inf=2),
            ir.random_diagram(rng, 7, h0=True)]
    rows, cnt = _pack(dgms, 40)
    xe, ye = utils.default_image_edges(12, 9, pers_range=(0.0, 1.0))
    host = engine.image_batch(rows, cnt, xe, ye, 0.07, 1, ctx=ctx)
    _close(host, ir.image_mean(rows, cnt, xe, ye, 0.07, 1), "host twin")
    assert host.tobytes() == _gpu(ctx, rows, cnt, xe, ye, 0.07, 1).tobytes()
    now = [utils.persistence_image(d, xe, ye, 0.07) for d in dgms]
    for i, im in enumerate(now):
        assert im.shape == (9, 12) and np.array_equal(im, host[i])  # the same rows in a buffer of their own: the same bytes
    with utils.batch():
        later = [utils.persistence_image(d, xe, ye, 0.07) for d in dgms]
        other = utils.persistence_image(dgms[2], xe, ye, 0.07, power=2)         # other parameters: a launch of its own
        with pytest.raises(ValueError):
            utils.persistence_image(np.zeros((2, 3)), xe, ye, 0.07)
    for a, b in zip(now, later):
        assert b.shape == (9, 12) and np.asarray(b).tobytes() == a.tobytes()
    _close(np.asarray(other)[None], ir.image_mean(rows[2:3], cnt[2:3], xe, ye, 0.07, 2), "deferred power 2")
