"""
The network curves on the CPU (include/tdaeeg.h, "Network curves"; tests/network_ref.py): the two evaluations of the contract
agree byte for byte, the identities between the rows hold, the known graphs give the answers worked out by hand, and the
written float64 definitions stay within the reordering bound of networkx's.  No GPU.
"""
import numpy as np
import pytest

import euler_ref as er
import network_cases as nc
import network_ref as nr

GRID7 = np.array([1.1, 0.1, 0.2, 0.3, 0.5, 0.9, 0.15])


def _sym_random(n, seed, hi=2.2):
    rng = np.random.default_rng(seed)
    d = rng.random((n, n)) * hi
    return (d + d.T) / 2


@pytest.fixture(scope="module")
def blocks():
    """n -> (keys, the level-set evaluation on GRID7), computed once."""
    out = {}
    for n in (1, 2, 3, 47, 65, 128):
        keys = er.keys_dm(_sym_random(n, 7000 + n))
        out[n] = (keys, nr.curves(keys, GRID7))
    return out


@pytest.mark.parametrize("n", [1, 2, 3, 47, 65, 128])
def test_two_evaluations_agree(blocks, n):
    keys, (cnt, mea, nod) = blocks[n]
    c2, m2, v2 = nr.curves_csgraph(keys, GRID7)
    assert cnt.dtype == np.int32 and cnt.shape == (nr.ROWS, 7) and mea.shape == (nr.MEASURES, 7) and nod.shape == (nr.NODAL, 7, n)
    assert cnt.tobytes() == c2.tobytes() and mea.tobytes() == m2.tobytes() and nod.tobytes() == v2.tobytes()


@pytest.mark.parametrize("n", [1, 2, 3, 47, 65, 128])
def test_identities(blocks, n):
    _, (cnt, mea, nod) = blocks[n]
    row = dict(zip(nr.COUNT_NAMES, cnt.astype(np.int64)))
    deg, tri, reach, far, ecc = nod.astype(np.int64)
    assert (deg.sum(1) == 2 * row["edges"]).all() and (tri.sum(1) == 3 * row["triangles"]).all()
    assert (reach.sum(1) == 2 * row["pairs"]).all() and (far.sum(1) == 2 * row["hops"]).all()
    assert (ecc.max(1) == row["diameter"]).all() and (deg.max(1) == row["max_degree"]).all()
    assert ((deg == 0).sum(1) == row["isolated"]).all()
    assert (row["largest"] == reach.max(1) + 1).all() and (row["components"] >= 1).all()
    assert ((mea >= 0.0) & np.isfinite(mea)).all() and (mea[:3] <= 1.0).all()
    if n >= 47:
        # both regimes of the grid: many components with long paths at the small scales, one component at the large ones
        assert row["components"][1:4].min() > 1 and row["components"][[0, 4, 5]].tolist() == [1, 1, 1]
        assert row["diameter"].max() >= 4


@pytest.mark.parametrize("name", sorted(nc.known()))
def test_known_answers(name):
    A, cnt, mea = nc.known()[name]
    for graph in (nr.graph_levels, nr.graph_csgraph):
        c, m, v = nr.curves_of_adjacency(A, graph)
        assert c.tolist() == cnt, (name, graph.__name__)
        assert m.tobytes() == np.array(mea, np.float64).tobytes(), (name, m, mea)
    # ... and through the keys of the distance matrix that realises the graph
    c, m, _ = nr.block_dm(nc.dm_of_graph(A), [nc.SCALE])
    assert c[:, 0].tolist() == cnt and m[:, 0].tobytes() == np.array(mea, np.float64).tobytes()


def test_small_graphs():
    # n = 1: one component of one vertex; n = 2 with its edge: one pair at one hop
    c, m, v = nr.curves_of_adjacency(nc.empty(1))
    assert c.tolist() == [0, 1, 0, 0, 0, 1, 1, 0, 0, 0] and m.tolist() == [0.0] * 4 and v.tolist() == [[0]] * 5
    c, m, v = nr.curves_of_adjacency(nc.complete(2))
    assert c.tolist() == [1, 0, 1, 0, 0, 1, 2, 1, 1, 1] and m.tolist() == [0.0, 0.0, 1.0, 1.0]
    c, m, v = nr.curves_of_adjacency(nc.complete(3))
    assert c.tolist() == [3, 0, 2, 3, 1, 1, 3, 3, 3, 1] and m.tolist() == [1.0, 1.0, 1.0, 1.0]
    assert v.tolist() == [[2] * 3, [1] * 3, [2] * 3, [2] * 3, [1] * 3]


def test_presence_rule_is_eulers():
    """edges and triangles are rows f_1 and f_2 of the Euler reference on the same keys, NaNs and thresh included."""
    d = _sym_random(13, 14)
    d[7, 3] = d[3, 7] = np.nan
    keys = er.keys_dm(d)
    grid = np.array([2.5, 1.4, np.nan, 0.9, 0.3])
    for thresh in (3.0, 1.0):
        cnt, _, _ = nr.curves(keys, grid, thresh)
        f = er.counts_mat(keys, grid, thresh, 2)
        assert cnt[0].tolist() == f[1].tolist() and cnt[4].tolist() == f[2].tolist()


def test_mean_seq_is_the_sequential_sum():
    rng = np.random.default_rng(5)
    b = rng.random((6, 4, 3))
    seg = np.array([0, 0, 4, 6], np.int32)
    st = np.array([0, 4, 0, 0, 16, 16], np.int32)
    m = nr.mean_seq(b, seg, st, 4 | 16)
    assert np.isnan(m[0]).all() and np.isnan(m[2]).all()
    assert m[1].tobytes() == ((((0.0 + b[0]) + b[2]) + b[3]) / 3.0).tobytes()
    assert nr.mean_seq(b).tobytes() == b.tobytes()


def test_networkx_agrees_within_the_reordering_bound():
    nx = pytest.importorskip("networkx")
    for n in (47, 65, 128):
        keys = er.keys_dm(_sym_random(n, 7000 + n))
        _, mea, _ = nr.curves(keys, GRID7)
        tol = n * (n - 1) * 2.0 ** -52                             # at most n (n - 1) terms of size at most 1, reordered
        for g, t in enumerate(GRID7):
            G = nx.from_numpy_array(er.adjacency(keys, t, 2.0))
            ref = [nx.transitivity(G), nx.average_clustering(G), nx.global_efficiency(G)]
            for k in range(3):
                assert abs(mea[k, g] - ref[k]) <= tol, (n, t, nr.MEASURE_NAMES[k], mea[k, g], ref[k])
