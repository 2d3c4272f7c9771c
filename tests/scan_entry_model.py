"""
numpy model of the entry into the coverage scan of the Rips sweep (csrc/rips.hip, the `if (calm)` block of rips_sweep),
shared by tests/test_scan_entry_model.py and tests/test_gpu_scan_entry.py.

The scan (tests/quiet_tail_model.py) needs two things: adjacency rows that hold exactly the edges below the rank it
starts from, and no class alive, so that every class vector is zero and an edge it passes over needs nothing but its
adjacency bits.

  * rule "today":  the scan is entered from a QUIET chunk only (nothing alive, nothing born).  The busy chunk in which
                   the last class dies is followed by one more regular chunk, which finds nothing and scans at its end;
  * rule "direct": the scan is entered from every chunk that ends CALM, i.e. with no class alive, busy or not -- the
                   state is the same.  A chunk that phase b cut short for class bits does not scan: it ends just before
                   a known candidate (tests/chunk_cut_model.py).

Two models: `tail` sets the two rules side by side behind the last busy chunk of a window, with the scan of
quiet_tail_model; `walk` is the chunk walk of chunk_cut_model with the calm rule, for inputs that end calm in the MIDDLE
of their filtration (the lull clouds below) and for the class-bit ladders.
"""
import numpy as np

import chunk_cut_model as C
import quiet_tail_model as Q


def tail(n, a, b, key, h1, chunk):
    """Both rules from Q.tail_start on.  Returns a dict: start; today / direct = (chunks behind the last busy one, scan
    rounds); passed = the ranks the direct rule passes over without a chunk; starts = where it starts chunks."""
    Ev = len(a)
    start = Q.tail_start(key, h1, chunk)
    if start >= Ev:                                  # the last busy chunk is the last chunk: one round that finds nothing
        return dict(start=start, today=(0, 1), direct=(0, 1), passed=[], starts=[])
    direct = Q.quiet_tail(n, a, b, start, chunk, retest=True)
    today = Q.quiet_tail(n, a, b, min(start + chunk, Ev), chunk, retest=True)
    return dict(start=start, today=(1 + len(today["starts"]), max(today["rounds"], 1)),
                direct=(len(direct["starts"]), direct["rounds"]), passed=direct["skipped"], starts=direct["starts"])


def oracle_ranks(key, h1):
    """[ranks of the edges whose length is the birth, or the finite death, of a row of the oracle's H1 diagram]: one
    array per value (more than one rank only where lengths tie)."""
    h1 = np.asarray(h1, dtype=np.float64).reshape(-1, 2)
    vals = np.concatenate([h1[:, 0], h1[np.isfinite(h1[:, 1]), 1]])
    return [np.nonzero(key == np.float32(v))[0] for v in np.unique(vals)]


def walk(n, a, b, key, h1, chunk, bits, direct, late=False):
    """The chunks of a pass with `bits` class bits, as chunk_cut_model.walk, with the scan entered from a quiet chunk
    (direct=False) or from every chunk that ends calm and was not cut (direct=True).  One dict per chunk: r0, end, cut,
    overflow, busy (a class alive at its start or born in it), calm (no class alive behind it), scanned (its end entered
    the scan), next (the rank the next chunk starts at; E: none)."""
    E = len(a)
    cand, birth = C.births(n, a, b)
    iv = C.death_intervals(key, birth, h1)
    rb = np.array([x[0] for x in iv], dtype=np.int64)
    rd = np.array([x[2] if late else x[1] for x in iv], dtype=np.int64)
    brank = np.nonzero(birth)[0]
    cand_rank = np.nonzero(cand)[0]
    out = []
    r0 = 0
    while r0 < E:
        end = min(r0 + chunk, E)
        alive = int(np.count_nonzero((rb < r0) & (rd >= r0)))
        inside = brank[(brank >= r0) & (brank < end)]
        rec = dict(r0=r0, end=end, cut=False, overflow=False, busy=alive > 0 or len(inside) > 0, calm=False,
                   scanned=False, next=E)
        out.append(rec)
        if len(inside) > bits - alive:
            q = int(inside[bits - alive])
            if q == r0:
                rec["overflow"] = True
                break
            rec["cut"], rec["end"], rec["next"] = True, q, q
            r0 = q
            continue
        rec["calm"] = int(np.count_nonzero((rb < end) & (rd >= end))) == 0
        if rec["calm"] and (direct or not rec["busy"]):
            rec["scanned"] = True
            nxt = cand_rank[cand_rank >= end]
            rec["next"] = int(nxt[0]) if len(nxt) else E
            r0 = rec["next"]
        else:
            rec["next"] = end
            r0 = end
    return out


def walks(n, a, b, key, h1, chunk, bits, direct):
    """The walk, if it is the same whichever end of its interval every class dies at; else None."""
    early, late_ = walk(n, a, b, key, h1, chunk, bits, direct), walk(n, a, b, key, h1, chunk, bits, direct, late=True)
    return early if early == late_ else None


def busy_entries(chunks):
    """The chunks whose end entered the scan though they were busy: what the direct rule adds."""
    return [c for c in chunks if c["busy"] and c["scanned"]]


# ---------------------------------------------------------------------------------------------------------------
# inputs shared by the model test (which proves that they take the new path) and the GPU test (which runs them)
# ---------------------------------------------------------------------------------------------------------------
CLOUD_THRESH = Q.CLOUD_THRESH
LULLS = {                         # name: (circles, points per circle, radius, chunk of the kernel the cloud is meant for)
    "lull96": (8, 12, 0.25, 512),
    "lull120": (10, 12, 0.20, 512),
    "lull45": (3, 15, 0.30, 256),
    "lull60": (5, 12, 0.25, 256),
}
LULL_SEEDS = (0, 1, 2)


def lull_cloud(k, m, r, seed, jitter=0.01):
    """k small circles of m points, radius r, in the plane z = 0, their centres on a circle of radius 3, a random phase
    per circle, Gaussian jitter.  The small loops are born and die among the k m (m - 1) / 2 edges inside the circles;
    the edges between neighbouring circles come much later: k - 1 merges and the birth of the large loop.  In between
    lies a chunk end with no class alive -- a lull in the middle of the filtration."""
    rng = np.random.default_rng(seed)
    phase = rng.random(k) * 2.0 * np.pi
    cang = 2.0 * np.pi * np.arange(k) / k
    ang = phase[:, None] + 2.0 * np.pi * np.arange(m)[None, :] / m
    x = 3.0 * np.cos(cang)[:, None] + r * np.cos(ang)
    y = 3.0 * np.sin(cang)[:, None] + r * np.sin(ang)
    pts = np.stack([x.ravel(), y.ravel(), np.zeros(k * m)], 1)
    return pts + jitter * rng.standard_normal(pts.shape)


def lull_clouds(name, copies=8):
    """copies of one lull cloud that differ in their jitter (and share their phases): (copies, k m, 3)"""
    k, m, r, _ = LULLS[name]
    base = lull_cloud(k, m, r, LULL_SEEDS[0], jitter=0.0)
    return Q.jittered(base, copies, 40 + k)


def lull(n, a, b, key, h1, chunk, bits=64):
    """The lull of a filtration: (end, birth, start) = the first chunk end of the direct walk that is busy, calm and has
    a birth behind it; the rank of that birth; the rank at which the direct rule starts its next chunk.  None: no lull."""
    chunks = walks(n, a, b, key, h1, chunk, bits, direct=True)
    if chunks is None:
        return None
    _, birth = C.births(n, a, b)
    brank = np.nonzero(birth)[0]
    for c in busy_entries(chunks):
        later = brank[brank >= c["end"]]
        if len(later):
            return c["end"], int(later[0]), c["next"]
    return None


def ring_windows_ending_in_the_last_chunk(chunk=512):
    """[(name, w)]: copies of the ring clouds of quiet_tail_model whose last class dies in the last chunk before the end
    of the filtration, so that the scan of the direct rule starts at or behind that end."""
    from oracle import port
    out = []
    for name, (clouds, n_pts) in Q.explicit_clouds().items():
        if not name.startswith("ring"):
            continue
        for w in range(len(clouds)):
            pc = Q.cloud_points(clouds, n_pts, w)
            dm = port.cloud_dm(pc).astype(np.float32)
            a, b, key = Q.filtration(dm, CLOUD_THRESH)
            chunks = walks(len(pc), a, b, key, port.rips_f32(dm, thresh=CLOUD_THRESH)[1], chunk, 32, direct=True)
            if chunks and chunks[-1]["busy"] and chunks[-1]["scanned"] and chunks[-1]["end"] >= len(a):
                out.append((name, w))
    return out
