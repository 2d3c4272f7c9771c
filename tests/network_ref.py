"""
CPU statement of the network curves (include/tdaeeg.h, "Network curves"): the graph measures of the thresholded graph of a
window at every scale of a grid.  The keys and the presence rule are euler_ref's.  The integers are evaluated twice,
independently: level sets of a breadth-first search on boolean matrices (curves), and scipy.sparse.csgraph's shortest
paths and connected components (curves_csgraph).  The four float64 measures are the written functions of those integers,
in Python floats (IEEE doubles, one operation at a time).  The group means: euler_ref.mean_exact for the integer blocks,
mean_seq (the sequential sum) for the measures.  Test infrastructure only.
"""
import numpy as np

import euler_ref as er

ROWS, MEASURES, NODAL = 10, 4, 5
COUNT_NAMES = ("edges", "isolated", "max_degree", "wedges", "triangles", "components", "largest", "pairs", "hops", "diameter")
MEASURE_NAMES = ("transitivity", "clustering", "efficiency", "path_length")
NODAL_NAMES = ("degree", "triangles", "reach", "farness", "eccentricity")


def _c2(m):
    return m * (m - 1) // 2


def measures_of(n, deg, tri, p):
    """The float64 rows from the integers: deg[v], tri[v] and p[d] = unordered pairs at hop distance d (p[0] unused)."""
    wedges = sum(_c2(int(d)) for d in deg)
    triangles = sum(int(t) for t in tri) // 3
    pairs = sum(int(x) for x in p[1:])
    hops = sum(d * int(p[d]) for d in range(1, len(p)))
    trans = float(3 * triangles) / float(wedges) if wedges else 0.0
    S = 0.0
    for v in range(n):
        S += 0.0 if deg[v] < 2 else float(int(tri[v])) / float(_c2(int(deg[v])))
    clus = S / float(n)
    E = 0.0
    for d in range(1, len(p)):
        E += float(int(p[d])) / float(d)
    eff = 0.0 if n < 2 else E / float(_c2(n))
    path = float(hops) / float(pairs) if pairs else 0.0
    return [trans, clus, eff, path]


def _block(n, deg, tri, reach, far, ecc, p, comps, largest):
    pairs = sum(int(x) for x in p[1:])
    hops = sum(d * int(p[d]) for d in range(1, len(p)))
    diam = max([d for d in range(1, len(p)) if p[d]], default=0)
    assert sum(int(t) for t in tri) % 3 == 0
    cnt = [int(deg.sum()) // 2, int((deg == 0).sum()), int(deg.max(initial=0)), sum(_c2(int(d)) for d in deg),
           sum(int(t) for t in tri) // 3, comps, largest, pairs, hops, diam]
    return cnt, measures_of(n, deg, tri, p), np.stack([deg, tri, reach, far, ecc])


def graph_levels(A):
    """One graph by level sets: next = (frontier . A) & ~visited from every source at once."""
    n = A.shape[0]
    Ai = A.astype(np.int64)
    deg = Ai.sum(1)
    tri = ((Ai @ Ai) * Ai).sum(1) // 2
    visited = np.eye(n, dtype=bool)
    frontier = visited.copy()
    reach, far, ecc = (np.zeros(n, np.int64) for _ in range(3))
    p = [0]
    for d in range(1, n):
        nxt = ((frontier.astype(np.int64) @ Ai) > 0) & ~visited
        c = nxt.sum(1)
        if not c.any():
            break
        reach += c
        far += d * c
        ecc[c > 0] = d
        assert int(c.sum()) % 2 == 0
        p.append(int(c.sum()) // 2)
        visited |= nxt
        frontier = nxt
    comps = sum(1 for s in range(n) if int(np.argmax(visited[s])) == s)
    return _block(n, deg, tri, reach, far, ecc, p, comps, int(visited.sum(1).max()))


def graph_csgraph(A):
    """The same graph by scipy.sparse.csgraph: hop distances and component labels."""
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import connected_components, shortest_path
    n = A.shape[0]
    Ai = A.astype(np.int64)
    deg = np.array([int(A[v].sum()) for v in range(n)], np.int64)
    tri = np.diagonal(Ai @ Ai @ Ai) // 2
    h = shortest_path(csr_matrix(Ai), directed=False, unweighted=True)
    ok = np.isfinite(h) & ~np.eye(n, dtype=bool)
    hi = np.where(ok, h, 0).astype(np.int64)
    reach, far, ecc = ok.sum(1).astype(np.int64), hi.sum(1), hi.max(1, initial=0)
    p = np.bincount(hi[np.triu(ok, 1)], minlength=1).tolist()
    p[0] = 0
    n_comp, labels = connected_components(csr_matrix(Ai), directed=False)
    return _block(n, deg, tri, reach, far, ecc, p, int(n_comp), int(np.bincount(labels).max()))


def curves(keys, grid, thresh=2.0, graph=graph_levels, n_node=None):
    """(counts (ROWS, n_grid) int32, measures (MEASURES, n_grid) float64, nodal (NODAL, n_grid, n_node) int32) of the keys
    of one window; the nodal columns at and above n are 0."""
    n = np.asarray(keys).shape[0]
    n_node = n if n_node is None else n_node
    grid = np.asarray(grid, dtype=np.float64)
    cnt = np.zeros((ROWS, len(grid)), np.int64)
    mea = np.zeros((MEASURES, len(grid)), np.float64)
    nod = np.zeros((NODAL, len(grid), n_node), np.int64)
    for g, t in enumerate(grid):
        c, m, v = graph(er.adjacency(keys, t, thresh))
        cnt[:, g], mea[:, g], nod[:, g, :n] = c, m, v
    assert max(cnt.max(initial=0), nod.max(initial=0)) < 2 ** 31
    return cnt.astype(np.int32), mea, nod.astype(np.int32)


def curves_csgraph(keys, grid, thresh=2.0, n_node=None):
    return curves(keys, grid, thresh, graph_csgraph, n_node)


def curves_of_adjacency(A, graph=graph_levels):
    """The blocks of one given graph (a boolean symmetric matrix with a False diagonal) at a single grid point."""
    c, m, v = graph(np.asarray(A, dtype=bool))
    return np.array(c, np.int64), np.array(m), v


def stack(blocks):
    """A list of (counts, measures, nodal) per window -> the three batch arrays."""
    return tuple(np.stack([b[k] for b in blocks]) for k in range(3))


def zeros(n_grid, n_node):
    return np.zeros((ROWS, n_grid), np.int32), np.zeros((MEASURES, n_grid)), np.zeros((NODAL, n_grid, n_node), np.int32)


# ---------------------------------------------------------------- blocks of the input forms, with their status words
def block_dm(dist, grid, thresh=2.0, symmetrise=True, graph=graph_levels):
    return curves(er.keys_dm(dist, symmetrise), grid, thresh, graph)


def block_cloud(pc, n_pts, grid, thresh=2.0, normalise=True):
    """((counts, measures, nodal with p_cap columns), status) of one window of the cloud form."""
    p_cap = pc.shape[0]
    if n_pts > min(p_cap, er.MAX_POINTS):
        return zeros(len(grid), p_cap), er.TDA_WIN_TOO_LARGE
    if n_pts < 3:
        return zeros(len(grid), p_cap), er.TDA_WIN_DEGENERATE
    return curves(er.keys_cloud(pc[:n_pts], normalise), grid, thresh, n_node=p_cap), 0


def block_takens(sig, tau, grid, thresh=2.0, dim=3, subsample=2):
    """The same of one Takens window; nodal has MAX_POINTS columns."""
    P = er.takens_points(len(sig), tau, dim, subsample)
    if tau < 1 or P > er.MAX_POINTS:
        return zeros(len(grid), er.MAX_POINTS), er.TDA_WIN_TOO_LARGE
    if P < 3:
        return zeros(len(grid), er.MAX_POINTS), er.TDA_WIN_DEGENERATE
    return curves(er.keys_takens(sig, tau, dim, subsample), grid, thresh, n_node=er.MAX_POINTS), 0


# ---------------------------------------------------------------- group means
mean_exact = er.mean_exact                                          # the integer blocks


def mean_seq(blocks, seg_off=None, status_in=None, skip_mask=0):
    """The float64 blocks: S = 0.0, S += the kept windows in ascending order, S / (double)m; NaN for an empty group."""
    blocks = np.asarray(blocks, dtype=np.float64)
    groups = er._groups(len(blocks), seg_off)
    out = np.full((len(groups),) + blocks.shape[1:], np.nan)
    for g, (w0, w1) in enumerate(groups):
        kept = er._kept(w0, w1, status_in, skip_mask)
        if kept:
            S = np.zeros(blocks.shape[1:])
            for w in kept:
                S = S + blocks[w]
            out[g] = S / np.float64(len(kept))
    return out
