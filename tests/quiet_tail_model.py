"""
numpy model of the quiet tail of the Rips sweep (csrc/rips.hip, the `if (quiet)` block of rips_sweep), shared by
tests/test_quiet_tail_model.py and tests/test_gpu_quiet_tail.py.

In the quiet state (no H1 class alive, none born) a chunk ends with a coverage scan: the first remaining edge without
a common neighbour in the adjacency rows.  The rows hold the edges up to the END OF THE CHUNK only, so they are stale
for that edge; the edges in front of it join the rows, and

  * rule "now":     a chunk of `chunk` edges starts at the hit, whatever it is;
  * rule "re-test": the hit is tested again against rows that now hold every edge before it.  Covered: a false alarm,
                    the scan goes on from it.  Still uncovered: a true candidate (a merge or a birth), a chunk starts.

The model keeps the rows as a boolean matrix and knows nothing about ranks; `first_cover` is the independent check (the
rank at which an edge gets its first common neighbour, from the rank matrix alone).
"""
import numpy as np

BIG = np.iinfo(np.int64).max


def filtration(dm_f32, thresh=2.0):
    """Edges (a > b) of a float32 distance matrix ordered by (length, a, b), cut at min(thresh, enclosing radius)."""
    dm = np.asarray(dm_f32, dtype=np.float32)
    a, b = np.tril_indices(dm.shape[0], -1)
    key = dm[a, b]
    cut = min(np.float32(thresh), dm.max(axis=1).min())
    keep = key <= cut
    a, b, key = a[keep], b[keep], key[keep]
    o = np.lexsort((b, a, key))
    return a[o], b[o], key[o]


def first_cover(n, a, b):
    """first_cover[r]: the smallest rank s such that the edges of rank <= s give edge r a common neighbour (BIG: never).
    Edge r has a common neighbour among the strictly earlier edges iff first_cover[r] < r."""
    R = np.full((n, n), BIG, dtype=np.int64)
    R[a, b] = R[b, a] = np.arange(len(a))
    return np.maximum(R[a], R[b]).min(axis=1)


def tail_start(key, h1, chunk):
    """First multiple of `chunk` behind the last finite H1 death (behind the first chunk if there is none)."""
    fin = h1[np.isfinite(h1[:, 1]), 1] if len(h1) else np.zeros(0)
    if len(fin) == 0:
        return chunk
    last = int(np.nonzero(key == np.float32(fin.max()))[0].max())
    return (last // chunk + 1) * chunk


def quiet_tail(n, a, b, start, chunk, retest, max_rounds=32):
    """Walk the tail from rank `start` on, the sweep quiet all the way.  Returns a dict:
    starts: ranks at which regular chunks start; skipped: ranks that only joined the rows; alarms: scan hits that were
    passed over without a chunk; stops: scan hits in all; rounds: scan rounds in all; scans: chunk ends that scanned."""
    Ev = len(a)
    adj = np.zeros((n, n), dtype=bool)

    def add(lo, hi):
        adj[a[lo:hi], b[lo:hi]] = True
        adj[b[lo:hi], a[lo:hi]] = True

    pos = min(start, Ev)
    add(0, pos)
    out = dict(starts=[], skipped=[], alarms=[], stops=0, rounds=0, scans=0)
    while pos < Ev:
        out["scans"] += 1
        hit = pos
        for rnd in range(max_rounds):
            out["rounds"] += 1
            unc = ~(adj[a[pos:]] & adj[b[pos:]]).any(axis=1)
            prev, hit = hit, (pos + int(np.argmax(unc)) if unc.any() else Ev)
            if rnd and hit != prev:
                out["alarms"].append(prev)
            if hit < Ev and (rnd == 0 or hit != prev):
                out["stops"] += 1
            if hit >= Ev or hit == pos:              # nothing left / the rows were exact for the hit: a true candidate
                break
            add(pos, hit)
            out["skipped"] += list(range(pos, hit))
            pos = hit
            if not retest:
                break
        if hit >= Ev:
            out["skipped"] += list(range(pos, Ev))
            break
        out["starts"].append(pos)
        end = min(pos + chunk, Ev)
        add(pos, end)
        pos = end
    return out


# ---------------------------------------------------------------------------------------------------------------
# inputs shared by the model test (which proves that they take the new path) and the GPU test (which runs them)
# ---------------------------------------------------------------------------------------------------------------
AUDIO_BANDS = ("delta", "theta", "alpha", "beta", "gamma")
CLOUD_THRESH = 100.0                 # explicit clouds: coordinates as given, the enclosing radius is the only cut


def audio_sample():
    """{band: (64 windows, tau)}: windows 0, 2, ..., 14 of each recording of synth.corpus_audio(8, 15); tau of the
    first window, as the pipeline takes it per recording."""
    from oracle import port
    from tda_eeg_audio_amd import synth
    x = synth.corpus_audio(8, 15)
    out = {}
    for band in AUDIO_BANDS:
        wins = np.ascontiguousarray(x[band][:, 0:15:2].reshape(64, -1))
        out[band] = (wins, port.compute_tau(wins[0], 125))
    return out


def audio_dm(window, tau):
    from oracle import port
    return port.cloud_dm(port.minmax_normalise(port.takens(window, 3, tau, 2))).astype(np.float32)


def _ball(rng, k):
    v = rng.standard_normal((k, 3))
    v /= np.linalg.norm(v, axis=1)[:, None]
    return v * (rng.random(k) ** (1.0 / 3.0))[:, None]


def blob_far(n, seed):
    """A blob (unit ball: its H1 classes die below 0.8, its long edges are the quiet tail) and one point at distance
    2.5 from its centre: the merge of that point is a TRUE candidate late in the tail, behind false alarms."""
    rng = np.random.default_rng(seed)
    return np.concatenate([[[2.5, 0.0, 0.0]], _ball(rng, n - 1)])


def blob_ring(n, seed):
    """A blob and, five units away, a sparse ring: four points on a square of side 1.3.  The ring closes at 1.3 -- a
    late BIRTH in the blob's quiet tail, behind false alarms --, dies at its diagonal (1.84), and the tail goes on with
    the blob's longest edges and, from 3.5 on, the edges between blob and ring (a late merge)."""
    rng = np.random.default_rng(seed)
    sq = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]], float) * 1.3 + [5.0, 0.0, 0.0]
    return np.concatenate([sq, _ball(rng, n - 4)])


def control_cloud(seed=2):
    """40 points of a tight blob: after the first chunk every remaining edge is covered at the first scan."""
    return 0.05 * np.random.default_rng(seed).standard_normal((40, 3))


def jittered(base, copies, seed, sigma=0.01):
    rng = np.random.default_rng(seed)
    return np.stack([base + sigma * rng.standard_normal(base.shape) for _ in range(copies)])


def explicit_clouds():
    """{name: (clouds (32, p_cap, 3), n_pts (32,))}: each construction at 60 points (one vertex word) and at 122, 123
    and 124 points (two vertex words), 32 jittered copies."""
    out = {}
    for name, make in (("far", blob_far), ("ring", blob_ring)):
        out[name + "60"] = (jittered(make(60, 1), 32, 7), np.full(32, 60, np.int32))
        big = jittered(make(124, 3), 32, 9)
        out[name + "124"] = (big, (122 + np.arange(32) % 3).astype(np.int32))    # (the far point / the ring come first)
    return out


def cloud_points(clouds, n_pts, w):
    """The points of copy w: its first n_pts[w] rows, as the kernels read them."""
    return clouds[w][:int(n_pts[w])]
