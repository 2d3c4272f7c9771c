"""
numpy reference of the sublevel-set persistence of a 1-D signal (include/tdaeeg.h, "Sublevel-set persistence of time
series"): the union-find definition, and the per-maximum form the kernel evaluates, restated independently of it.  Both
return (rows (m, 2) float64, idx (m, 2) int32), the essential row (x[g], inf), (g, -1) last.  No GPU, no project code.
"""
import numpy as np


def rows_bound(n):
    """TDA_SL_ROWS(n)."""
    return (n + 1) // 2


def _finish(finite, x, g):
    """Finite rows (birth, death, birth index, death index) into (death, birth, death index) order + the essential row."""
    finite.sort(key=lambda r: (r[1], r[0], r[3]))
    finite.append((x[g], np.inf, g, -1))
    rows = np.array([[r[0], r[1]] for r in finite], dtype=np.float64).reshape(-1, 2)
    idx = np.array([[r[2], r[3]] for r in finite], dtype=np.int32).reshape(-1, 2)
    return rows, idx


def sublevel_union_find(x):
    """The definition: vertices in (x[i], i) order, union-find, elder rule."""
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[0]
    assert x.ndim == 1 and n >= 1 and np.isfinite(x).all()
    order = sorted(range(n), key=lambda i: (x[i], i))
    pos = np.empty(n, np.int64)
    pos[order] = np.arange(n)                     # rank in the total order
    parent = [-1] * n                             # -1: not entered yet
    low = list(range(n))                          # root -> the minimum of its component

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i

    finite = []
    for v in order:
        parent[v] = v
        for u in (v - 1, v + 1):
            if 0 <= u < n and parent[u] != -1:
                a, b = find(u), find(v)
                if a == b:
                    continue
                if pos[low[a]] > pos[low[b]]:     # a's minimum is the larger one: a dies
                    a, b = b, a
                dying = low[b]
                if x[dying] != x[v]:
                    finite.append((x[dying], x[v], dying, v))
                parent[b] = a
    return _finish(finite, x, order[0])


def sublevel_per_maximum(x):
    """The equivalent form: one row per interior vertex above both neighbours in the total order."""
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[0]
    assert x.ndim == 1 and n >= 1 and np.isfinite(x).all()

    def below(a, b):                              # a before b in the total order
        return (x[a], a) < (x[b], b)

    finite = []
    for p in range(1, n - 1):
        if not (below(p - 1, p) and below(p + 1, p)):
            continue
        q = p - 1
        while q - 1 >= 0 and below(q - 1, p):
            q -= 1
        ml = min(range(q, p), key=lambda i: (x[i], i))
        q = p + 1
        while q + 1 < n and below(q + 1, p):
            q += 1
        mr = min(range(p + 1, q + 1), key=lambda i: (x[i], i))
        y = mr if below(ml, mr) else ml
        if x[y] != x[p]:
            finite.append((x[y], x[p], y, p))
    g = min(range(n), key=lambda i: (x[i], i))
    return _finish(finite, x, g)


def sublevel_batch(sigs, cap=None, fill=np.nan, fill_idx=-1):
    """What tda_sublevel_batch leaves in pre-filled buffers for stacked signals (n_sig, n_t): (dgm (n_sig, cap, 2), cnt, idx
    (n_sig, cap, 2), status).  A signal with a non-finite sample: cnt 0, status 64, its block still the fill."""
    sigs = np.asarray(sigs, dtype=np.float64)
    n_sig, n_t = sigs.shape
    cap = rows_bound(n_t) if cap is None else cap
    dgm = np.full((n_sig, cap, 2), fill, dtype=np.float64)
    idx = np.full((n_sig, cap, 2), fill_idx, dtype=np.int32)
    cnt = np.zeros(n_sig, np.int32)
    status = np.zeros(n_sig, np.int32)
    for s in range(n_sig):
        if not np.isfinite(sigs[s]).all():
            status[s] = 64
            continue
        r, i = sublevel_union_find(sigs[s])
        cnt[s] = r.shape[0]
        dgm[s, :cnt[s]] = r
        idx[s, :cnt[s]] = i
    return dgm, cnt, idx, status
