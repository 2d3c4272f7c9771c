"""
The definition of the generators and representative cycles (include/tdaeeg.h) against the textbook reduction, on the CPU:
tests/generators_ref.py states it three times -- (a) reduction, (b) definition, (c) the kernel's mask route -- and this file
holds them against each other and against known answers.  No GPU.
"""
import numpy as np
import pytest

import euler_ref as er
import generators_ref as gr
from oracle import port


def _corr_keys(n, seed):
    rng = np.random.default_rng(seed)
    return er.keys_dm(port.corr_dist(rng.standard_normal((n, 250)))[1])


def _circle_keys(n, seed, loops=1):
    rng = np.random.default_rng(seed)
    th = rng.random(n) * 2 * np.pi
    pc = np.stack([np.cos(th), np.sin(th)], 1) * (1 + (np.arange(n) % loops)[:, None] * 2.5)
    pc += rng.standard_normal(pc.shape) * 0.05
    return er.keys_cloud(pc, True)


def _quantised_keys(n, seed, steps):
    rng = np.random.default_rng(seed)
    d = rng.random((n, n)) * 1.8 + 0.1
    d = np.round((d + d.T) / 2 * steps) / steps
    return er.keys_dm(d)


GENERIC = [("corr", n, s) for n, s in ((4, 1), (5, 2), (9, 3), (16, 4), (30, 5), (47, 6))] + \
          [("circle", n, s) for n, s in ((6, 1), (12, 2), (24, 3), (40, 4), (47, 5))]
QUANTISED = [(n, s, q) for n, s, q in ((4, 1, 2), (6, 2, 3), (9, 3, 4), (13, 4, 5), (20, 5, 8), (30, 6, 12), (47, 7, 16))]


def _keys(kind, n, seed):
    return _corr_keys(n, seed) if kind == "corr" else _circle_keys(n, seed, 2 if n >= 24 else 1)


def _check_window(keys, thresh, generic):
    """Every statement of the issue on one window; returns (rows, flagged rows)."""
    n = keys.shape[0]
    p0, p1, comps = gr.reduce_pairs(keys, thresh)
    h0, h1 = gr.diagrams_of(p0, p1, comps)
    cls = gr.classify(keys, thresh)
    B = {(a, b): w for w, a, b, kind, _ in cls if kind == "B"}
    K = {(a, b): w for w, a, b, kind, _ in cls if kind == "K"}
    F = [(w, (a, b)) for w, a, b, kind, _ in cls if kind == "F"]
    # every positive-persistence pair's edge is in B, its death edge in K with the row's death; F is Kruskal's forest
    for b_, d_, be, de in p1:
        assert be in B and B[be] == b_
        if de is not None:
            assert de in K and K[de] == d_
    assert [e for w, e in F if w != 0.0] == [e for _, e in p0] and len(F) == n - comps
    b = gr.generators(keys, h0, len(h0), h1, len(h1), thresh)
    c = gr.generators_masks(keys, h0, len(h0), h1, len(h1), thresh)
    for name in b:
        assert b[name].tobytes() == c[name].tobytes(), name
    # the forest edge of every finite H0 row, exact under ties as well
    fin = [e for w, e in F if w != 0.0]
    assert b["h0_edge"][:len(fin)].tolist() == [list(e) for e in fin] and (b["h0_edge"][len(fin):] == -1).all()
    by_row = {}
    for b_, d_, be, de in p1:
        by_row.setdefault((b_, d_), []).append((be, de))
    before = {(a, b_): i for i, (_, a, b_, _, _) in enumerate(cls)}
    flagged = 0
    for r in range(len(h1)):
        fl = int(b["h1_flag"][r])
        assert not fl & (gr.NO_EDGE | gr.CYCLE_TRUNCATED)           # the diagram is this input's, cyc_cap = 128
        if generic:
            assert fl == 0
        if fl:
            flagged += 1
            continue
        ba, bb, da, db = (int(x) for x in b["h1_gen"][r])
        pairs = by_row[(h1[r, 0], h1[r, 1])]
        assert (ba, bb) in [p[0] for p in pairs]
        assert ((da, db) if da >= 0 else None) in [p[1] for p in pairs]
        if len(pairs) == 1:
            assert pairs[0] == ((ba, bb), (da, db) if da >= 0 else None)
        # the cycle: a closed walk in G_e plus e, at least 4 vertices, e its youngest edge
        L = int(b["cyc_len"][r])
        walk = [int(v) for v in b["cyc"][r, :L]]
        assert L >= 4 and walk[0] == ba and walk[-1] == bb and len(set(walk)) == L and (b["cyc"][r, L:] == -1).all()
        pe = before[(ba, bb)]
        for u, v in zip(walk, walk[1:]):
            assert before[(max(u, v), min(u, v))] < pe
    # participation: the definition once more with numpy
    part = np.zeros(n)
    for r in range(len(h1)):
        if b["h1_flag"][r] == 0 and np.isfinite(h1[r, 1]):
            part[b["cyc"][r, :b["cyc_len"][r]]] += h1[r, 1] - h1[r, 0]
    assert np.allclose(b["part"], part, rtol=1e-12, atol=0)
    return len(h1), flagged


@pytest.mark.parametrize("kind,n,seed", GENERIC)
def test_generic_inputs_definition_is_the_reduction(kind, n, seed):
    rows, flagged = _check_window(_keys(kind, n, seed), 2.0, True)
    assert flagged == 0
    if n >= 12:
        assert rows > 0


@pytest.mark.parametrize("n,seed,steps", QUANTISED)
def test_quantised_inputs(n, seed, steps):
    _check_window(_quantised_keys(n, seed, steps), 2.0, False)


def test_quantised_inputs_do_flag():
    """The tie-heavy cases reach the flags (or the test above shows nothing about them)."""
    seen = 0
    for n, seed, steps in QUANTISED[3:6]:
        keys = _quantised_keys(n, seed, steps)
        p0, p1, comps = gr.reduce_pairs(keys)
        h0, h1 = gr.diagrams_of(p0, p1, comps)
        seen |= int(np.bitwise_or.reduce(gr.generators(keys, h0, len(h0), h1, len(h1))["h1_flag"], initial=0))
    assert seen & gr.BIRTH_TIED and seen & gr.DEATH_TIED


def test_small_threshold_gives_essential_rows():
    keys = _circle_keys(16, 9)
    full = gr.diagrams_of(*gr.reduce_pairs(keys))[1]
    loop = full[np.argmax(full[:, 1] - full[:, 0])]
    thresh = float(loop.mean())                                   # the circle's loop is born and not yet dead
    p0, p1, comps = gr.reduce_pairs(keys, thresh)
    h0, h1 = gr.diagrams_of(p0, p1, comps)
    assert np.isinf(h1[:, 1]).any()
    _check_window(keys, thresh, True)
    b = gr.generators(keys, h0, len(h0), h1, len(h1), thresh)
    ess = np.isinf(h1[:, 1])
    assert (b["h1_gen"][ess, 2:] == -1).all() and (b["h1_gen"][ess, :2] >= 0).all() and not b["h1_flag"][ess].any()


def _poly_keys(pts):
    pts = np.asarray(pts, dtype=np.float64)
    d = np.sqrt(((pts[:, None] - pts[None]) ** 2).sum(-1))
    return er.keys_dm(d)


def _run(keys, thresh=2.0, cyc_cap=128):
    p0, p1, comps = gr.reduce_pairs(keys, thresh)
    h0, h1 = gr.diagrams_of(p0, p1, comps)
    return h0, h1, gr.generators(keys, h0, len(h0), h1, len(h1), thresh, cyc_cap)


def test_unit_square():
    h0, h1, g = _run(_poly_keys([[0, 0], [1, 0], [1, 1], [0, 1]]))
    assert h1.tolist() == [[1.0, float(np.float32(np.sqrt(2.0)))]]
    assert g["h1_gen"][0].tolist() == [3, 2, 2, 0]                # the last side closes the loop, the first diagonal kills
    assert g["cyc"][0, :4].tolist() == [3, 0, 1, 2] and g["cyc_len"][0] == 4 and g["h1_flag"][0] == gr.DEATH_TIED
    assert g["h0_edge"].tolist() == [[1, 0], [2, 1], [3, 0], [-1, -1]]
    assert g["part"].tolist() == [0.0] * 4                        # the row is death-tied: flagged rows add nothing


def test_hexagon():
    th = np.arange(6) * np.pi / 3
    h0, h1, g = _run(_poly_keys(np.stack([np.cos(th), np.sin(th)], 1) * [1.0, 1.0]))
    assert len(h1) == 1 and g["cyc_len"][0] == 6 and sorted(g["cyc"][0, :6].tolist()) == list(range(6))
    a, b = g["h1_gen"][0, :2]
    assert g["cyc"][0, 0] == a and g["cyc"][0, 5] == b
    # cyc_cap below the cycle: flag, true length, prefix
    _, _, t = _run(_poly_keys(np.stack([np.cos(th), np.sin(th)], 1)), cyc_cap=4)
    assert t["h1_flag"][0] & gr.CYCLE_TRUNCATED and t["cyc_len"][0] == 6 and t["cyc"][0].tolist() == g["cyc"][0, :4].tolist()
    assert not t["part"].any()


def test_two_squares_sharing_a_vertex():
    pts = [[0, 0], [1, 0], [1, 1], [0, 1], [2, 1], [2, 2], [1, 2]]
    rng = np.random.default_rng(5)
    pts = np.asarray(pts, float) + rng.standard_normal((7, 2)) * 0.01       # generic: no ties
    h0, h1, g = _run(_poly_keys(pts))
    assert len(h1) == 2 and not g["h1_flag"][:2].any()
    cycles = sorted(sorted(g["cyc"][r, :g["cyc_len"][r]].tolist()) for r in range(2))
    assert cycles == [[0, 1, 2, 3], [2, 4, 5, 6]]
    pers = {tuple(sorted(g["cyc"][r, :4].tolist())): h1[r, 1] - h1[r, 0] for r in range(2)}
    assert g["part"][2] == (h1[0, 1] - h1[0, 0]) + (h1[1, 1] - h1[1, 0])
    assert g["part"][0] == pers[(0, 1, 2, 3)] and g["part"][5] == pers[(2, 4, 5, 6)]


def test_constant_matrix():
    n = 9
    keys = er.keys_dm(np.full((n, n), 0.75))
    h0, h1, g = _run(keys)
    assert len(h1) == 0 and len(h0) == n
    assert g["h0_edge"][:n - 1].tolist() == [[v, 0] for v in range(1, n)]    # a star forest
    m = gr.MaskRoute(keys, 2.0)
    assert m.forest(np.float64(np.float32(0.75))) == [(v, 0) for v in range(1, n)]
    assert m.searches == n - 1                                    # every other edge has a common neighbour


def test_foreign_diagram_has_no_edge():
    keys, other = _circle_keys(12, 1), _circle_keys(12, 2)
    p0, p1, comps = gr.reduce_pairs(other)
    h0, h1 = gr.diagrams_of(p0, p1, comps)
    assert len(h1)
    g = gr.generators(keys, h0, len(h0), h1, len(h1))
    assert (g["h1_flag"][:len(h1)] & gr.NO_EDGE).all() and (g["h1_gen"] == -1).all() and (g["cyc"] == -1).all()
    assert not g["cyc_len"].any() and not g["part"].any() and (g["h0_edge"] == -1).all()


def test_mean_part():
    rng = np.random.default_rng(3)
    part = rng.random((6, 5))
    seg = np.array([0, 0, 2, 6], np.int32)
    st = np.array([0, 4, 0, 16, 0, 0], np.int32)
    m = gr.mean_part(part, seg, st, 4 | 16)
    assert np.isnan(m[0]).all() and m[1].tolist() == part[0].tolist()
    assert m[2].tolist() == (((part[2] + part[4]) + part[5]) / 3.0).tolist()
    assert gr.mean_part(part).tolist() == part.tolist()
