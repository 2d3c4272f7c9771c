"""
numpy model of the class-bit cuts of the Rips sweep (csrc/rips.hip, phase b of rips_sweep), shared by
tests/test_chunk_cut_model.py and tests/test_gpu_chunk_cuts.py.

The sweep takes the filtration a chunk of edges at a time (512 edges in the point-cloud kernels, 256 in the
distance-matrix kernels).  Phase b gives a class bit to EVERY birth of a chunk before any kill of it has freed one,
so with `bits` class bits a chunk that starts at rank s with A(s) classes alive closes just before its
(bits - A(s) + 1)-th birth: a CUT.  The kills of the shortened chunk free bits and the next chunk starts AT the cut.  A
cut at the first edge of a chunk means that more than `bits` classes are alive at once: the window is flagged for the
next wider pass.  A STRETCH below is a run of chunks each of which starts at the cut of the one before: the edges of
one full-length chunk that had to be taken in pieces.

What the model needs:
  * births by rank: exact, from the filtration alone -- a birth is an edge without a common neighbour among the earlier
    edges (`quiet_tail_model.first_cover`) that joins two vertices Kruskal has already connected;
  * deaths by rank: from the oracle's H1 rows.  A row gives the LENGTH of the killing edge, not its rank, and a class
    of zero persistence gives no row at all, so every class gets an interval [lo, hi] of ranks for its death: the ranks
    of the edges of that length (for a class without a row: behind its birth, up to the last edge of its own length).
    The walk is done twice, every class dying at `lo` and every class dying at `hi`; a window counts for a case only if
    both walks agree on all its cuts.  Lengths are float32 values of continuous data: ties are rare, and where there is
    none the two walks are the same walk;
  * chunk starts: chunks follow each other, except behind a quiet chunk (nothing alive, nothing born), where the
    coverage scan moves the start to the next true candidate (an edge still without a common neighbour at its own rank;
    tests/quiet_tail_model.py).
"""
import numpy as np

import quiet_tail_model as Q


def births(n, a, b):
    """(candidate, birth) per rank: candidate = no common neighbour among the earlier edges; birth = a candidate whose
    ends Kruskal has joined already."""
    E = len(a)
    cand = Q.first_cover(n, a, b) >= np.arange(E)
    comp = np.arange(n)
    birth = np.zeros(E, dtype=bool)
    for r in np.nonzero(cand)[0]:
        ca, cb = comp[a[r]], comp[b[r]]
        if ca == cb:
            birth[r] = True
        else:
            comp[comp == cb] = ca
    return cand, birth


def death_intervals(key, birth, h1):
    """(rb, lo, hi) per class in birth order: it dies at a rank in [lo, hi] (E: never)."""
    E = len(key)
    rows = {}
    for kb, kd in np.asarray(h1, dtype=np.float64).reshape(-1, 2):
        rows.setdefault(np.float32(kb), []).append(kd)
    for v in rows.values():
        v.sort()
    out = []
    for rb in np.nonzero(birth)[0]:
        ds = rows.get(key[rb])
        if ds:                                       # ties of birth lengths: the rows in order of their deaths
            kd = ds.pop(0)
            if not np.isfinite(kd):
                out.append((rb, E, E))
                continue
            at = np.nonzero(key == np.float32(kd))[0]
            out.append((rb, int(max(at.min(), rb + 1)), int(max(at.max(), rb + 1))))
        else:                                        # zero persistence: killed by an edge of its own length
            at = np.nonzero(key == key[rb])[0]
            out.append((rb, rb + 1, int(max(at.max(), rb + 1))))
    return out


def walk(n, a, b, key, h1, chunk, bits, late=False):
    """The chunks of the first pass with `bits` class bits.  Returns a list of dicts, one per chunk: r0, end, cut (the
    chunk closed early, at `end`), after_cut (it starts at the cut of the chunk before), lonely (after_cut and no other
    candidate in it than the edge at the cut), overflow (a cut at its first edge: the pass flags the window and stops)."""
    E = len(a)
    cand, birth = births(n, a, b)
    iv = death_intervals(key, birth, h1)
    rb = np.array([x[0] for x in iv], dtype=np.int64)
    rd = np.array([x[2] if late else x[1] for x in iv], dtype=np.int64)
    brank = np.nonzero(birth)[0]
    cand_rank = np.nonzero(cand)[0]
    out = []
    r0, after_cut = 0, False
    while r0 < E:
        end = min(r0 + chunk, E)
        alive = int(np.count_nonzero((rb < r0) & (rd >= r0)))
        inside = brank[(brank >= r0) & (brank < end)]
        rec = dict(r0=r0, end=end, cut=False, after_cut=after_cut, overflow=False,
                   lonely=after_cut and int(np.count_nonzero((cand_rank >= r0) & (cand_rank < end))) == 1)
        out.append(rec)
        if len(inside) > bits - alive:
            q = int(inside[bits - alive])
            if q == r0:
                rec["overflow"] = True
                break
            rec["cut"], rec["end"] = True, q
            r0, after_cut = q, True
            continue
        after_cut = False
        if alive == 0 and len(inside) == 0:          # quiet: the coverage scan moves on to the next true candidate
            nxt = cand_rank[cand_rank >= end]
            if len(nxt) == 0:
                break
            r0 = int(nxt[0])
        else:
            r0 = end
    return out


def cuts(n, a, b, key, h1, chunk, bits):
    """The walk, if it is the same whichever end of its interval every class dies at; else None."""
    early, late_ = walk(n, a, b, key, h1, chunk, bits), walk(n, a, b, key, h1, chunk, bits, late=True)
    return early if early == late_ else None


def cases(chunks):
    """The cases of a window, a set of names: first (the first chunk is cut), later (a later one), double (a chunk that
    starts at a cut is cut again: one stretch of edges in three pieces or more), lonely (a chunk that starts at a cut
    and holds no other candidate), overflow, none (no cut at all).  Empty for a window the model cannot decide."""
    if chunks is None:
        return set()
    out = set()
    for i, c in enumerate(chunks):
        if c["overflow"]:
            out.add("overflow")
        if c["cut"]:
            out.add("first" if i == 0 else "later")
            if c["after_cut"]:
                out.add("double")
        if c["lonely"]:
            out.add("lonely")
    return out or {"none"}


# ---------------------------------------------------------------------------------------------------------------
# inputs shared by the model test (which proves that they cut where it says) and the GPU test (which runs them)
# ---------------------------------------------------------------------------------------------------------------
CLOUD_THRESH = Q.CLOUD_THRESH


def ladder(n, seed, rails=2, grow=0.004, height=1.0, jitter=1e-4):
    """A ladder of `rails` rails, `height` apart, and n // rails rungs whose rectangles grow in width along it:
    the rails - 1 rectangles of step k are born when their long sides enter (1.5 height (1 + k grow)) and die at their
    diagonal, step after step, a number of them alive at once that falls with `grow`.  Points that are left over are put
    on the first rung, between the rails (apparent edges only: they change no class)."""
    rng = np.random.default_rng(seed)
    m = n // rails
    w = 1.5 * height * (1.0 + grow * np.arange(m - 1))
    x = np.concatenate([[0.0], np.cumsum(w)])
    pts = np.concatenate([np.stack([x, np.full(m, height * k), np.zeros(m)], 1) for k in range(rails)])
    extra = n - rails * m
    if extra:
        pts = np.concatenate([pts, [[0.0, height * (k + 0.5), 0.0] for k in range(extra)]])
    return pts + jitter * rng.standard_normal(pts.shape)


def cloud_filtration(pts, thresh=CLOUD_THRESH):
    from oracle import port
    dm = port.cloud_dm(np.asarray(pts, dtype=np.float64)).astype(np.float32)
    return (len(pts),) + Q.filtration(dm, thresh), port.rips_f32(dm, thresh=thresh)


AUDIO_BANDS = Q.AUDIO_BANDS
LADDERS = {                        # name: (points, rails, grow) -- 60 points: one vertex word; 122 to 124: two
    "ladder60": (60, 3, 0.03),
    "ladder122": (122, 4, 0.03),
    "ladder123": (123, 4, 0.03),
    "ladder124": (124, 4, 0.03),
}


def ladder_clouds(name, copies=8):
    """copies of one ladder that differ in their jitter: (copies, n, 3)"""
    n, rails, grow = LADDERS[name]
    return np.stack([ladder(n, 100 + k, rails=rails, grow=grow) for k in range(copies)])


def audio_cases(bits, chunk=512, bands=AUDIO_BANDS):
    """{band: [cases of window 0, ...]} for the 64 windows per band of quiet_tail_model.audio_sample()"""
    from oracle import port
    out = {}
    for band, (wins, tau) in Q.audio_sample().items():
        if band not in bands:
            continue
        out[band] = []
        for w in wins:
            dm = Q.audio_dm(w, tau)
            a, b, key = Q.filtration(dm)
            out[band].append(cases(cuts(dm.shape[0], a, b, key, port.audio_persistence(w, tau)[0][1], chunk, bits)))
    return out


def ladder_cases(name, bits, chunk, copies=8):
    out = []
    for pts in ladder_clouds(name, copies):
        (n, a, b, key), dg = cloud_filtration(pts)
        out.append(cases(cuts(n, a, b, key, dg[1], chunk, bits)))
    return out
