"""
CPU statement of the generators and representative cycles of Rips persistence pairs (include/tdaeeg.h, "Generators and
representative cycles"), three times and independently:
  (a) ``reduce_pairs``    the textbook reduction of oracle/brute.py's kind, extended to keep each pair's edge and the
                          youngest edge of its killing triangle;
  (b) ``generators``      the definition of the header, with sets, labels and a queue;
  (c) ``generators_masks`` the kernel's route: every candidate found by key equality in flat-index order, adjacency at the
                          edge's own time as bit masks (Python ints), breadth-first search on masks, parent = ctz.
Test infrastructure only.  Keys are handed round as a symmetric (n, n) float32 matrix; only k[a][b], a > b, is the contract
(euler_ref.keys_dm / keys_cloud / keys_takens make them).
"""
from collections import deque

import numpy as np

BIRTH_TIED, DEATH_TIED, CYCLE_TRUNCATED, NO_EDGE = 1, 2, 4, 8
TDA_WIN_DEGENERATE = 4
TDA_WIN_TOO_LARGE = 16
MAX_POINTS = 128


def tri(a):
    return a * (a - 1) // 2


def sorted_edges(keys, thresh=2.0):
    """The edges with k <= (float)thresh in the order (key, a, b), a > b: the order of the flat index tri(a) + b among
    equal keys.  A NaN key is no edge."""
    k = np.asarray(keys, dtype=np.float32)
    n = k.shape[0]
    th = np.float32(thresh)
    return sorted((float(k[a, b]), a, b) for a in range(n) for b in range(a) if k[a, b] <= th)


# ---------------------------------------------------------------- (a) the reduction
def reduce_pairs(keys, thresh=2.0):
    """Z/2 reduction of the triangle boundary matrix with the edges in the order above and every triangle entering with
    its youngest edge.  Returns (h0, h1, the number of components): h0 = [(death, (a, b))] in the order the forest edges
    arrive (zero keys dropped);
    h1 = [(birth, death, birth_edge, death_edge)] with death = inf and death_edge = None for essential classes; pairs of
    zero persistence dropped."""
    edges = sorted_edges(keys, thresh)
    n = np.asarray(keys).shape[0]
    pos = {(a, b): p for p, (_, a, b) in enumerate(edges)}
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    h0, negative = [], set()
    for p, (w, a, b) in enumerate(edges):
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[ra] = rb
            negative.add(p)
            if w != 0.0:
                h0.append((w, (a, b)))
    tris = []
    for i in range(n):
        for j in range(i):
            if (i, j) not in pos:
                continue
            for k in range(j):
                if (i, k) in pos and (j, k) in pos:
                    ps = (pos[(i, j)], pos[(i, k)], pos[(j, k)])
                    tris.append((max(ps), i, j, k, (1 << ps[0]) | (1 << ps[1]) | (1 << ps[2])))
    tris.sort(key=lambda t: t[:4])
    low2col, killer = {}, {}
    for young, _, _, _, col in tris:
        while col:
            low = col.bit_length() - 1
            other = low2col.get(low)
            if other is None:
                low2col[low] = col
                killer[low] = young
                break
            col ^= other
    h1 = []
    for p, (w, a, b) in enumerate(edges):
        if p in negative:
            continue
        if p in killer:
            q = killer[p]
            if edges[q][0] > w:
                h1.append((w, edges[q][0], (a, b), edges[q][1:]))
        else:
            h1.append((w, np.inf, (a, b), None))
    return h0, h1, n - len(negative)


def diagrams_of(h0_pairs, h1_pairs, n_components):
    """The rows as the Rips kernels order them: H0 ascending death then the essential rows, H1 descending birth."""
    h0 = [(0.0, d) for d, _ in sorted(h0_pairs, key=lambda p: p[0])] + [(0.0, np.inf)] * n_components
    h1 = sorted(((b, d) for b, d, _, _ in h1_pairs), key=lambda r: (-r[0], r[1]))
    return np.array(h0, dtype=np.float64).reshape(-1, 2), np.array(h1, dtype=np.float64).reshape(-1, 2)


# ---------------------------------------------------------------- (b) the definition
def bfs_cycle(adj, a, b):
    """Breadth-first from b in level sets; the parent of a vertex is the lowest-numbered adjacent vertex of the previous
    level.  Returns a, parent(a), ..., b, or None when a is not reached."""
    parent = {b: None}
    level = deque([b])
    while level and a not in parent:
        prev = set(level)
        nxt = deque()
        for v in range(len(adj)):
            if v not in parent:
                c = adj[v] & prev
                if c:
                    nxt.append((v, min(c)))
        for v, p in nxt:
            parent[v] = p
        level = deque(v for v, _ in nxt)
    if a not in parent:
        return None
    walk = [a]
    while walk[-1] != b:
        walk.append(parent[walk[-1]])
    return walk


def classify(keys, thresh=2.0):
    """Every edge in order with its kind: 'F' (!conn), 'B' (conn and !cn), 'K' (cn), judged in the graph G_e of the edges
    before it.  Returns [(key, a, b, kind, cycle or None)]."""
    n = np.asarray(keys).shape[0]
    adj = [set() for _ in range(n)]
    label = list(range(n))
    out = []
    for w, a, b in sorted_edges(keys, thresh):
        cn = bool(adj[a] & adj[b])
        conn = label[a] == label[b]
        kind = "K" if cn else ("B" if conn else "F")
        out.append((w, a, b, kind, bfs_cycle(adj, a, b) if kind == "B" else None))
        adj[a].add(b)
        adj[b].add(a)
        if not conn:
            la, lb = label[a], label[b]
            label = [lb if x == la else x for x in label]
    return out


def _runs(vals):
    r = 0
    while r < len(vals):
        r1 = r + 1
        while r1 < len(vals) and vals[r1] == vals[r]:
            r1 += 1
        yield r, r1
        r = r1


def _empty(h1_cap, h0_cap, cyc_cap, part_ld):
    return dict(h1_gen=np.full((h1_cap, 4), -1, np.int16), h1_flag=np.zeros(h1_cap, np.int32),
                cyc=np.full((h1_cap, cyc_cap), -1, np.int16), cyc_len=np.zeros(h1_cap, np.int32),
                part=np.zeros(part_ld, np.float64), h0_edge=np.full((h0_cap, 2), -1, np.int16))


def _assemble(n, h0, c0, h1, c1, cyc_cap, part_ld, births_of, deaths_of, forest_of):
    """The rules that turn the candidate lists into the outputs; births_of(x) = [(a, b, cycle)] of B with key x in order,
    deaths_of(x) = [(a, b)] of K, forest_of(x) = [(a, b)] of F."""
    h0 = np.asarray(h0, dtype=np.float64).reshape(-1, 2)
    h1 = np.asarray(h1, dtype=np.float64).reshape(-1, 2)
    h0_cap, h1_cap = h0.shape[0], h1.shape[0]
    out = _empty(h1_cap, h0_cap, cyc_cap, part_ld)
    R = min(max(int(c1), 0), h1_cap)
    for r0, r1 in _runs(list(h1[:R, 0])):
        cands = births_of(h1[r0, 0])
        for r in range(r0, r1):
            d = h1[r, 1]
            flag = BIRTH_TIED if len(cands) != r1 - r0 else 0
            if r - r0 >= len(cands):
                flag |= NO_EDGE
            death = (-1, -1)
            if d != np.inf:
                kc = deaths_of(d)
                if not kc:
                    flag |= NO_EDGE
                else:
                    death = kc[0]
                    if len(kc) > 1:
                        flag |= DEATH_TIED
            if not flag & NO_EDGE:
                a, b, walk = cands[r - r0]
                out["h1_gen"][r] = [a, b, death[0], death[1]]
                out["cyc_len"][r] = len(walk)
                out["cyc"][r, :min(len(walk), cyc_cap)] = walk[:cyc_cap]
                if len(walk) > cyc_cap:
                    flag |= CYCLE_TRUNCATED
            out["h1_flag"][r] = flag
    R0 = min(max(int(c0), 0), h0_cap)
    for r0, r1 in _runs(list(h0[:R0, 1])):
        cands = forest_of(h0[r0, 1]) if h0[r0, 1] != np.inf else []      # an essential row has no edge
        for r in range(r0, min(r1, r0 + len(cands))):
            out["h0_edge"][r] = cands[r - r0]
    for v in range(min(n, part_ld)):
        s = np.float64(0.0)
        for r in range(R):
            if out["h1_flag"][r] == 0 and np.isfinite(h1[r, 1]) and v in out["cyc"][r, :out["cyc_len"][r]]:
                s = s + (h1[r, 1] - h1[r, 0])
        out["part"][v] = s
    return out


def generators(keys, h0, c0, h1, c1, thresh=2.0, cyc_cap=128, part_ld=None):
    """(b): the outputs of one window as the header defines them, from the classified edge list."""
    k = np.asarray(keys, dtype=np.float32)
    n = k.shape[0]
    by = {"F": {}, "B": {}, "K": {}}                              # kind -> key (the float32 value, exactly) -> edges in order
    for w, a, b, kind, walk in classify(k, thresh):
        by[kind].setdefault(w, []).append((a, b, walk))

    def pick(kind, x):
        return by[kind].get(float(x), [])                         # (a NaN is equal to no key)

    return _assemble(n, h0, c0, h1, c1, cyc_cap, n if part_ld is None else part_ld,
                     lambda x: pick("B", x),
                     lambda x: [(a, b) for a, b, _ in pick("K", x)],
                     lambda x: [(a, b) for a, b, _ in pick("F", x)])


# ---------------------------------------------------------------- (c) the kernel's route
def _ctz(m):
    return (m & -m).bit_length() - 1


class MaskRoute:
    """Lookups by key equality over the flat triangle; every judgement from the keys alone, at the edge's own time."""

    def __init__(self, keys, thresh):
        self.k = np.asarray(keys, dtype=np.float32)
        self.n = self.k.shape[0]
        self.th = np.float32(thresh)
        self.searches = 0
        self.levels = 0

    def flat(self, x, y):
        return tri(x) + y if x > y else tri(y) + x

    def before(self, x, y, ke, fe):
        kk = self.k[max(x, y), min(x, y)]
        return bool(kk <= self.th and (kk < ke or (kk == ke and self.flat(x, y) < fe)))

    def row(self, v, ke, fe):
        m = 0
        for u in range(self.n):
            if u != v and self.before(v, u, ke, fe):
                m |= 1 << u
        return m

    def matches(self, x):
        for a in range(1, self.n):
            for b in range(a):
                kk = self.k[a, b]
                if kk <= self.th and np.float64(kk) == x:
                    yield a, b

    def cn(self, a, b):
        ke, fe = self.k[a, b], self.flat(a, b)
        return bool(self.row(a, ke, fe) & self.row(b, ke, fe) & ~((1 << a) | (1 << b)))

    def search(self, a, b):
        """Returns the walk a .. b, or None."""
        self.searches += 1
        ke, fe = self.k[a, b], self.flat(a, b)
        adj = [self.row(v, ke, fe) for v in range(self.n)]
        vis = fr = 1 << b
        par = [-1] * self.n
        for _ in range(self.n):
            nf = 0
            for v in range(self.n):
                if not (vis >> v) & 1 and adj[v] & fr:
                    par[v] = _ctz(adj[v] & fr)
                    nf |= 1 << v
            if not nf:
                break
            self.levels += 1
            vis |= nf
            fr = nf
            if (nf >> a) & 1:
                walk = [a]
                while walk[-1] != b:
                    walk.append(par[walk[-1]])
                return walk
        return None

    def births(self, x):
        out = []
        for a, b in self.matches(x):
            if not self.cn(a, b):
                walk = self.search(a, b)
                if walk is not None:
                    out.append((a, b, walk))
        return out

    def deaths(self, x):
        return [(a, b) for a, b in self.matches(x) if self.cn(a, b)]

    def forest(self, x):
        return [(a, b) for a, b in self.matches(x) if not self.cn(a, b) and self.search(a, b) is None]


def generators_masks(keys, h0, c0, h1, c1, thresh=2.0, cyc_cap=128, part_ld=None):
    m = MaskRoute(keys, thresh)
    return _assemble(m.n, h0, c0, h1, c1, cyc_cap, m.n if part_ld is None else part_ld, m.births, m.deaths, m.forest)


# ---------------------------------------------------------------- windows of the cloud forms, fill values, group means
def fill(h1_cap, h0_cap, cyc_cap, part_ld):
    """What a skipped, degenerate or refused window gets."""
    return _empty(h1_cap, h0_cap, cyc_cap, part_ld)


def mean_part(part, seg_off=None, status_in=None, skip_mask=0):
    """Per group and vertex: the parts of the kept windows added in window order from +0.0, divided by their number; NaN
    for a group without a kept window."""
    part = np.asarray(part, dtype=np.float64)
    n_win = part.shape[0]
    groups = ([(w, w + 1) for w in range(n_win)] if seg_off is None else
              [(max(int(seg_off[g]), 0), min(int(seg_off[g + 1]), n_win)) for g in range(len(seg_off) - 1)])
    out = np.full((len(groups), part.shape[1]), np.nan)
    for g, (w0, w1) in enumerate(groups):
        kept = [w for w in range(w0, w1) if status_in is None or not (int(status_in[w]) & skip_mask)]
        if kept:
            s = np.zeros(part.shape[1])
            for w in kept:
                s = s + part[w]
            out[g] = s / np.float64(len(kept))
    return out
