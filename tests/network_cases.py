"""
Graphs with known network curves, shared by tests/test_network_model.py (CPU) and tests/test_gpu_network.py: boolean
adjacency matrices, the distance matrix that realises one at a scale, and the answers worked out by hand.  Test
infrastructure only.
"""
import numpy as np

IN, OUT, SCALE = 0.5, 1.5, 1.0            # an edge has distance IN, a non-edge OUT; the graph is read at SCALE


def _sym(n, pairs):
    A = np.zeros((n, n), bool)
    for a, b in pairs:
        A[a, b] = A[b, a] = True
    return A


def empty(n):
    return np.zeros((n, n), bool)


def complete(n):
    return ~np.eye(n, dtype=bool)


def path(n):
    return _sym(n, [(v, v + 1) for v in range(n - 1)])


def cycle(n):
    return _sym(n, [(v, (v + 1) % n) for v in range(n)])


def star(n, hub):
    return _sym(n, [(hub, v) for v in range(n) if v != hub])


def two_cliques_blocks(n):
    """K_{n/2} on the vertices below n / 2 and K_{n/2} on the rest."""
    half = np.arange(n) < n // 2
    return (half[:, None] == half[None, :]) & ~np.eye(n, dtype=bool)


def two_cliques_interleaved(n):
    """K_{n/2} on the even vertices and K_{n/2} on the odd ones: each component spans both mask words at n = 128."""
    par = np.arange(n) % 2
    return (par[:, None] == par[None, :]) & ~np.eye(n, dtype=bool)


def dm_of_graph(A):
    """A symmetric distance matrix whose graph at SCALE is A."""
    d = np.where(A, IN, OUT).astype(np.float64)
    np.fill_diagonal(d, 0.0)
    return d


def c2(m):
    return m * (m - 1) // 2


# name -> (adjacency, the ten counts in row order, the four measures); the arithmetic is in the comments
def known():
    out = {}
    n = 128
    out["empty_128"] = (empty(n), [0, n, 0, 0, 0, n, 1, 0, 0, 0], [0.0, 0.0, 0.0, 0.0])
    # K_n: every pair at one hop; wedges n C(n - 1, 2), triangles C(n, 3)
    tri = n * (n - 1) * (n - 2) // 6
    out["K_128"] = (complete(n), [c2(n), 0, n - 1, n * c2(n - 1), tri, 1, n, c2(n), c2(n), 1], [1.0, 1.0, 1.0, 1.0])
    # P_n: p_d = n - d; hops = sum d (n - d) = (n - 1) n (n + 1) / 6
    hops = (n - 1) * n * (n + 1) // 6
    eff = 0.0
    for d in range(1, n):
        eff += float(n - d) / float(d)
    out["P_128"] = (path(n), [n - 1, 0, 2, n - 2, 0, 1, n, c2(n), hops, n - 1], [0.0, 0.0, eff / float(c2(n)), float(hops) / float(c2(n))])
    assert hops == 349504
    # C_65: p_d = 65 for d = 1..32
    m = 65
    eff = 0.0
    for d in range(1, 33):
        eff += float(m) / float(d)
    hops = m * sum(range(1, 33))
    out["C_65"] = (cycle(m), [m, 0, 2, m, 0, 1, m, c2(m), hops, 32], [0.0, 0.0, eff / float(c2(m)), float(hops) / float(c2(m))])
    # stars: n - 1 pairs at one hop, C(n - 1, 2) at two
    for hub in (0, 64, 127):
        p1, p2 = n - 1, c2(n - 1)
        eff = (0.0 + float(p1) / 1.0) + float(p2) / 2.0
        out[f"star_128_hub{hub}"] = (star(n, hub), [n - 1, 0, n - 1, c2(n - 1), 0, 1, n, c2(n), p1 + 2 * p2, 2],
                                     [0.0, 0.0, eff / float(c2(n)), float(p1 + 2 * p2) / float(c2(n))])
    # two K_64, in blocks and interleaved
    h = 64
    cnt = [2 * c2(h), 0, h - 1, n * c2(h - 1), 2 * (h * (h - 1) * (h - 2) // 6), 2, h, 2 * c2(h), 2 * c2(h), 1]
    mea = [1.0, 1.0, float(2 * c2(h)) / float(c2(n)), 1.0]
    out["two_K_64_blocks"] = (two_cliques_blocks(n), cnt, mea)
    out["two_K_64_interleaved"] = (two_cliques_interleaved(n), cnt, mea)
    return out
