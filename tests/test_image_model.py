"""
Persistence images on the CPU: the numpy reference (image_ref) against a 40-digit evaluation of the same definition, the
known answers, the group semantics, and the presence of the entry points and of the argument checks of the wrappers.
"""
import os

import numpy as np
import pytest

import image_ref as ir

EPS = 2.0 ** -53
P1 = 0.3413447460685429                                            # Phi(1) - Phi(0) of the standard normal


def _exact_images(rows, xe, ye, sigma):
    """The images of the three powers in 40-digit arithmetic.  p_i = d_i - b_i and s = sigma * 1.4142135623730951 are the
    float64 values the definition names (one IEEE operation each); everything after them -- the quotient, erfc, the
    differences, the products and the sums -- is exact to 40 digits."""
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 40
    b, p, _ = ir.weights(rows, 1)
    s = mp.mpf(float(np.float64(sigma) * ir.SQRT2))
    half = mp.mpf(1) / 2

    def factors(edges, centres):
        out = []
        for c in centres:
            cdf = [half * mp.erfc(-((mp.mpf(float(e)) - mp.mpf(float(c))) / s)) for e in edges]
            out.append([cdf[k + 1] - cdf[k] for k in range(len(edges) - 1)])
        return out

    fx, fy = factors(xe, b), factors(ye, p)
    imgs = []
    for power in (0, 1, 2):
        w = [mp.mpf(float(v)) ** power for v in p]
        imgs.append([[mp.fsum(w[i] * fy[i][r] * fx[i][c] for i in range(len(b))) for c in range(len(xe) - 1)]
                     for r in range(len(ye) - 1)])
    return mp, imgs


@pytest.mark.parametrize("n_x,n_y,n_rows,sigma", [(20, 20, 60, 0.05), (32, 32, 30, 0.01), (8, 5, 120, 0.3), (16, 16, 10, 0.1),
                                                  (32, 7, 90, 0.02)])
def test_reference_against_exact_arithmetic(n_x, n_y, n_rows, sigma):
    """Required: worst |ref - exact| <= 1.0 * 2^-53 * W, for every power."""
    rng = np.random.default_rng(1000 * n_x + n_y)
    rows = ir.random_diagram(rng, n_rows, kind="f32")
    xe, ye = np.linspace(-0.1, 1.7, n_x + 1), np.linspace(0.0, 0.7, n_y + 1)
    mp, exact = _exact_images(rows, xe, ye, sigma)
    for power in (0, 1, 2):
        ref, W, N = ir.diagram_image(rows, xe, ye, sigma, power)
        assert N == n_rows and W > 0
        worst = max(abs(mp.mpf(float(ref[r, c])) - exact[power][r][c]) for r in range(n_y) for c in range(n_x))
        ratio = float(worst / (mp.mpf(EPS) * mp.mpf(W)))
        print(f"sides ({n_x},{n_y}) rows {n_rows} sigma {sigma} power {power}: |ref - exact| / (2^-53 W) = {ratio:.3f}")
        assert ratio <= 1.0, (power, ratio)


@pytest.mark.parametrize("power", [0, 1, 2])
def test_one_point_four_equal_pixels(power):
    b, p, sigma = 0.5, 0.25, 0.125                                  # b + p, b - sigma, ... are exact in float64
    img, W, N = ir.diagram_image([[b, b + p]], [b - sigma, b, b + sigma], [p - sigma, p, p + sigma], sigma, power)
    want = p ** power * P1 ** 2
    assert img.shape == (2, 2) and N == 1 and W == p ** power
    assert np.abs(img - want).max() <= 1e-15 * want


@pytest.mark.parametrize("power", [0, 1, 2])
def test_mass_is_conserved(power):
    """Edges reaching 8 sigma past every point: the pixels sum to W within N * 2^-52 * W."""
    rng = np.random.default_rng(5 + power)
    rows = ir.random_diagram(rng, 50, kind="f32")
    sigma = 0.05
    xe, ye = np.linspace(0.0 - 8 * sigma, 1.5 + 8 * sigma, 21), np.linspace(0.0 - 8 * sigma, 0.6 + 8 * sigma, 14)
    img, W, N = ir.diagram_image(rows, xe, ye, sigma, power)
    assert N == 50 and abs(img.sum() - W) <= N * 2.0 ** -52 * W


def test_inf_row_changes_nothing():
    rng = np.random.default_rng(8)
    rows = ir.random_diagram(rng, 20)
    xe, ye = np.linspace(0, 2, 11), np.linspace(0, 1, 9)
    with_inf = np.concatenate([rows[:7], [[0.3, np.inf]], rows[7:], [[0.0, np.inf]]])
    for power in (0, 1, 2):
        a, b = ir.diagram_image(rows, xe, ye, 0.1, power), ir.diagram_image(with_inf, xe, ye, 0.1, power)
        assert a[0].tobytes() == b[0].tobytes() and a[1:] == b[1:]
    only = ir.diagram_image([[0.2, np.inf]], xe, ye, 0.1, 1)
    assert not only[0].any() and only[1:] == (0.0, 0)
    empty = ir.diagram_image(np.zeros((0, 2)), xe, ye, 0.1, 2)
    assert empty[0].shape == (8, 10) and not empty[0].any()


def test_axes_are_not_swapped():
    """7 x 5: n_x = 7 birth pixels, n_y = 5 persistence pixels; a point of large birth and small persistence lights
    row 0, column 6."""
    xe, ye = np.linspace(0.0, 1.4, 8), np.linspace(0.0, 0.5, 6)
    img, _, _ = ir.diagram_image([[1.3, 1.35]], xe, ye, 0.02, 1)
    assert img.shape == (5, 7)
    assert np.unravel_index(np.argmax(img), img.shape) == (0, 6)
    img, _, _ = ir.diagram_image([[0.1, 0.55]], xe, ye, 0.02, 1)
    assert np.unravel_index(np.argmax(img), img.shape) == (4, 0)


def test_group_semantics():
    rng = np.random.default_rng(7)
    dg = [ir.random_diagram(rng, 5) for _ in range(6)]
    rows = np.zeros((6, 8, 2)); cnt = np.full(6, 5, np.int32)
    for i, d in enumerate(dg):
        rows[i, :5] = d
    cnt[5] = 11                                                     # truncated: the 8 rows of the buffer
    xe, ye = np.linspace(0, 2, 8), np.linspace(0, 1, 6)
    out, W, N = ir.image_mean(rows, cnt, xe, ye, 0.1, 1, seg_off=[0, 2, 2, 6], status=[0, 4, 0, 0, 16, 0], skip_mask=4 | 16)
    one = ir.diagram_image(dg[0], xe, ye, 0.1, 1)
    assert out[0].tobytes() == one[0].tobytes() and W[0] == one[1] and N[0] == 5       # a group of one: x / 1
    assert np.isnan(out[1]).all() and W[1] == 0 and N[1] == 0                          # an empty group
    kept = [ir.diagram_image(d, xe, ye, 0.1, 1) for d in (dg[2], dg[3], rows[5])]
    assert np.array_equal(out[2], (kept[0][0] + kept[1][0] + kept[2][0]) / 3.0)
    assert N[2] == 5 + 5 + 8 and W[2] == (kept[0][1] + kept[1][1] + kept[2][1]) / 3.0
    masked, _, _ = ir.image_mean(rows, cnt, xe, ye, 0.1, 1, seg_off=[0, 2], status=[4, 16, 0, 0, 0, 0], skip_mask=4 | 16)
    assert np.isnan(masked).all()                                                      # the mask empties the group
    each, _, _ = ir.image_mean(rows, cnt, xe, ye, 0.1, 1)                              # seg_off = None
    assert each.shape == (6, 5, 7) and each[0].tobytes() == one[0].tobytes()
    lists, _, _ = ir.lists_mean([ir.cut(rows[w], cnt[w]) for w in range(6)], xe, ye, 0.1, 1, [0, 2, 2, 6])
    assert np.array_equal(lists[2], ir.image_mean(rows, cnt, xe, ye, 0.1, 1, seg_off=[0, 2, 2, 6])[0][2])


def test_entry_points_exist():
    from tda_eeg_audio_amd import _lib, drivers, engine, utils
    lib = _lib.load()                                               # torch's HIP runtime first, as the package loads it
    for name in ("tda_image_mean_dev", "tda_image_batch"):
        assert name in _lib.SYMBOLS
        assert hasattr(lib, name)
    assert len(_lib.SYMBOLS["tda_image_mean_dev"][1]) == 17 and len(_lib.SYMBOLS["tda_image_batch"][1]) == 12
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "tdaeeg.h")).read()
    assert "tda_image_mean_dev(" in header and "tda_image_batch(" in header
    assert "#define TDA_MAX_IMAGE_SIDE 32" in header and _lib.MAX_IMAGE_SIDE == 32
    for f in (engine.image_batch, engine.image_mean_dev, utils.persistence_image, utils.default_image_edges,
              drivers.images_from_distances, drivers.image_names):
        assert callable(f)
    xe, ye = utils.default_image_edges(20, 12)
    assert np.array_equal(xe, np.linspace(0.0, 2.0, 21)) and np.array_equal(ye, np.linspace(0.0, 2.0, 13))
    xe, ye = utils.default_image_edges(4, 2, birth_range=(0.5, 1.5), pers_range=(0.0, 0.25))
    assert np.array_equal(xe, np.linspace(0.5, 1.5, 5)) and np.array_equal(ye, np.linspace(0.0, 0.25, 3))
    names = drivers.image_names(["alpha", "beta"], n_x=3, n_y=2)
    assert len(names) == 2 * 2 * 2 * 3 and names[0] == "alpha_h0_image_r0_c0" and names[-1] == "beta_h1_image_r1_c2"


BAD = [
    dict(dgm=np.zeros((3, 3))), dict(dgm=[1.0, 2.0]),
    dict(xe=[0.0, 1.0, 1.0]), dict(xe=[1.0, 0.0]), dict(xe=[0.0, np.inf]), dict(xe=[0.0, np.nan, 1.0]), dict(xe=[0.0]),
    dict(xe=np.linspace(0, 1, 34)), dict(xe=np.zeros((2, 2))), dict(ye=[0.0, 0.5, 0.25]), dict(ye=np.linspace(0, 1, 34)),
    dict(sigma=0.0), dict(sigma=-0.1), dict(sigma=np.nan), dict(sigma=np.inf), dict(power=3), dict(power=-1), dict(power=0.5),
]


@pytest.mark.parametrize("bad", BAD, ids=lambda b: next(iter(b)))
def test_wrappers_raise_value_error_without_a_gpu(bad, monkeypatch):
    """A bad diagram, bad edges, sigma or power is a ValueError before any GPU call, immediate or inside utils.batch()."""
    from tda_eeg_audio_amd import engine, utils

    def no_gpu(*a, **k):
        raise AssertionError("a GPU entry point was reached")
    monkeypatch.setattr(engine, "image_batch", no_gpu)
    monkeypatch.setattr(engine, "get_ctx", no_gpu)
    kw = dict(dgm=np.array([[0.0, 1.0]]), xe=np.linspace(0, 2, 5), ye=np.linspace(0, 1, 4), sigma=0.1, power=1)
    kw.update(bad)
    with pytest.raises(ValueError):
        utils.persistence_image(**kw)
    with pytest.raises(ValueError):
        with utils.batch():
            utils.persistence_image(**kw)
    with pytest.raises(ValueError):
        engine.image_args(kw["xe"], kw["ye"], kw["sigma"], kw["power"]) if "dgm" not in bad else utils.persistence_image(**kw)


def test_no_cpu_fallback():
    """Without a GPU the image of a diagram is an error, never a host computation."""
    from tda_eeg_audio_amd import _lib, utils
    from tda_eeg_audio_amd._lib import TdaError
    rows = np.array([[0.0, 1.0], [0.25, 0.75], [0.0, np.inf]])
    xe, ye = utils.default_image_edges(6, 4)
    try:
        got = utils.persistence_image(rows, xe, ye, 0.1)
    except TdaError:
        return                                                      # no GPU: an error, not a host computation
    assert _lib._ctx, "a value without a HIP context: something computed it on the host"
    ref, W, N = ir.diagram_image(rows, xe, ye, 0.1, 1)
    assert got.shape == (4, 6) and np.abs(got - ref).max() <= (ir.C * W + N * ref.max()) * EPS
