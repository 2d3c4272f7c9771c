"""
Phase d of the Rips sweep lists the triangles it has to test as a work list in owner order and tests one per lane, NT per
trip; the entries are placed by prefix sums, so the list stands in the order of the killing edges.  The inputs here are
the smallest at which that can go wrong: more triangles in a chunk than one trip holds (owners whose triangles straddle
two trips), all of them trivial or thousands of them not, lists that overflow their capacity, more than one class word
(the reduction that takes the list in any order), and no triangle at all -- through every kernel that inlines the sweep.

Bar: H0 and H1 rows bit-equal to the oracle as sorted multisets, counts and status words equal.
"""
import numpy as np
import pytest

from oracle import brute, port
from tda_eeg_audio_amd import engine, synth

pytestmark = pytest.mark.gpu

CLOUD_THRESH = 100.0                 # explicit clouds: coordinates as given, the enclosing radius is the only cut
DM_WORDS = ((1, 1), (2, 1))          # distance matrices: one class word (ordered reduction), two (min-reduction)
CLOUD_WIDTHS = ((1, 1), (1, 2))      # first pass of the point-cloud kernel: narrow layout (32 class bits), wide (64)


def _same(a, b):
    return np.array_equal(brute.sort_rows(a), brute.sort_rows(b))


def _check_dm(ctx, d, thresh, words, tag):
    """d: (n_win, n, n) -> diagrams of rips_dm_kernel under every class width of `words`, against the oracle"""
    ref = [port.rips_dm(x, thresh=thresh) for x in d]
    out = None
    try:
        for w in words:
            ctx.set_class_words(*w)
            h0, h1, st = engine.rips_dm_batch(d, thresh=thresh, h1_cap=1024, ctx=ctx)
            assert not st.any(), (tag, w, st)
            for k in range(len(d)):
                assert _same(h0[k], ref[k][0]) and _same(h1[k], ref[k][1]), (tag, w, k)
            out = (h0, h1)
    finally:
        ctx.set_class_words(2, 1)
    return out


# ---- more triangles than one trip, all vectors zero ----

@pytest.mark.parametrize("n", [24, 47])
def test_equal_lengths_many_trivial_triangles(ctx, n):
    """Every off-diagonal entry equal: ties fall in flat-index order, an edge (a, b) has the common neighbours below b and,
    with empty adjacency rows at the start of chunk 0, b - 1 triangles to test (24 points: C(22,3) = 1,540 in a chunk of
    256 edges).  n - 1 rows at that length, the essential one, no H1 row."""
    d = np.ones((1, n, n)) - np.eye(n)
    h0, h1 = _check_dm(ctx, d, 2.0, DM_WORDS, ("equal", n))
    assert len(h1[0]) == 0 and len(h0[0]) == n
    assert np.all(h0[0][:-1] == [0.0, 1.0]) and np.isinf(h0[0][-1, 1])


@pytest.mark.parametrize("n", [24, 47])
def test_equal_lengths_with_a_class_alive(ctx, n):
    """The same cluster beside a square of four points whose class (born at 0.5, its diagonals beyond the threshold) is
    alive while the cluster's edges are swept: a chunk in which nothing is alive and nothing is born tests no triangle, so
    this is the variant in which the trips are taken for certain -- every vector is still zero."""
    m = n + 4
    d = np.full((m, m), 1.8)
    d[:n, :n] = 1.0
    for k in range(4):
        d[n + k, n + (k + 1) % 4] = d[n + (k + 1) % 4, n + k] = 0.5
    np.fill_diagonal(d, 0.0)
    h0, h1 = _check_dm(ctx, d[None], 1.5, DM_WORDS, ("equal+square", n))
    assert len(h1[0]) == 1 and h1[0][0, 0] == 0.5 and np.isinf(h1[0][0, 1])
    assert len(h0[0]) == m


def test_fused_eeg_kernel_nearly_equal_correlations(ctx):
    """The fused EEG kernel (256 threads, 47 points) on windows whose correlations all lie within 1e-3 of one value: the
    edges come in an arbitrary order, classes are born among them and nearly every edge has dozens of triangles to test."""
    import torch
    dev = torch.device("cuda", ctx.device)
    rng = np.random.default_rng(11)
    G = np.full((47, 47), 0.2) + rng.uniform(-1e-3, 1e-3, (47, 47))
    G = (G + G.T) / 2
    np.fill_diagonal(G, 1.0)
    ev, U = np.linalg.eigh(G)
    assert ev.min() > 0
    L = (U * np.sqrt(ev)) @ U.T
    W = np.empty((4, 47, 250))
    for k in range(4):
        Z = rng.standard_normal((250, 47))
        Z -= Z.mean(axis=0)
        Q, _ = np.linalg.qr(Z)
        W[k] = L @ Q.T
    out = engine.eeg_window_dev(torch.from_numpy(W).to(dev), h1_cap=1024, ctx=ctx)
    torch.cuda.synchronize()
    assert int(out.status.max()) == 0 and int(out.status.min()) == 0
    a0, a1 = out.to_lists()
    for w in range(len(W)):
        o = port.rips_dm(port.corr_dist(W[w])[1])
        assert _same(a0[w], o[0]) and _same(a1[w], o[1]), w


# ---- the same in the 512-thread kernels ----

def _ball_and_circle(circle_radius, centre):
    """40 points within a ball of radius 0.02 and 60 on a circle"""
    rng = np.random.default_rng(7)
    v = rng.standard_normal((40, 3))
    v *= (0.02 * rng.random(40) ** (1.0 / 3.0) / np.linalg.norm(v, axis=1))[:, None]
    ang = 2.0 * np.pi * np.arange(60) / 60.0
    ring = circle_radius * np.stack([np.cos(ang), np.sin(ang), np.zeros(60)], 1) + np.asarray(centre)
    return np.concatenate([v, ring])


@pytest.mark.parametrize("name", ["unit circle", "small circle"])
def test_ball_and_circle_cloud_both_first_pass_widths(ctx, name):
    """The 780 short edges of the ball fill the first chunks of 512 and carry thousands of triangles.  "unit circle": the
    circle of radius 1 around the ball.  "small circle": radius 0.005, three units away -- its class is born before most
    of the short edges and dies among them, and its own 1,200 chords below that length give lists of non-zero vectors
    that overflow."""
    pc = _ball_and_circle(1.0, (0, 0, 0)) if name == "unit circle" else _ball_and_circle(0.005, (3, 0, 0))
    ref = port.rips_f32(port.cloud_dm(pc).astype(np.float32), thresh=CLOUD_THRESH)
    try:
        for words in CLOUD_WIDTHS:
            ctx.set_class_words(*words)
            h0, h1, st = engine.cloud_rips_batch(pc[None], normalise=False, thresh=CLOUD_THRESH, h1_cap=1024, ctx=ctx)
            assert st[0] == 0, (name, words, st)
            assert _same(h0[0], ref[0]) and _same(h1[0], ref[1]), (name, words)
    finally:
        ctx.set_class_words(2, 1)


# ---- lists that overflow their capacity ----

@pytest.mark.parametrize("band", ["alpha", "delta"])
def test_audio_windows_with_overflowing_lists(ctx, band):
    """256 synthetic audio windows of a band: 0.40 (alpha) and 0.13 (delta) list rounds per window find more entries
    than the list holds, process the earliest alone and list the chunk again."""
    wins = synth.audio_windows(256, band, seed=1)
    tau = int(engine.tau_batch(wins[:1], 125, ctx=ctx)[0])
    ref = [port.audio_persistence(w, tau)[0] for w in wins]
    try:
        for words in CLOUD_WIDTHS:
            ctx.set_class_words(*words)
            h0, h1, npts, st = engine.takens_rips_batch(wins, tau, h1_cap=1024, ctx=ctx)
            assert not st.any(), (band, words, np.flatnonzero(st))
            for w in range(len(wins)):
                assert _same(h0[w], ref[w][0]) and _same(h1[w], ref[w][1]), (band, words, w)
    finally:
        ctx.set_class_words(2, 1)


# ---- more than one class word: the reduction that takes the list in any order ----

def _bipartite_matrix(seed):
    """K(23,24) at distance 1, everything else at distance 2, ties broken: 506 classes alive at once"""
    n = 47
    side = np.arange(n) < 23
    d = np.where(side[:, None] != side[None, :], 1.0, 2.0)
    d = d + np.random.default_rng(seed).random((n, n)) * 1e-3
    d = (d + d.T) / 2
    np.fill_diagonal(d, 0)
    return d


def _bipartite_windows(n_rep, seed):
    """47-channel windows whose correlation graph is K(23,24) (cross-group correlation 0.23, within-group 0.20)"""
    rng = np.random.default_rng(seed)
    G = np.full((47, 47), 0.20)
    G[:23, 23:] = 0.23; G[23:, :23] = 0.23
    np.fill_diagonal(G, 1.0)
    ev, U = np.linalg.eigh(G)
    assert ev.min() > 0
    L = (U * np.sqrt(ev)) @ U.T
    out = np.empty((n_rep, 47, 250))
    for k in range(n_rep):
        Z = rng.standard_normal((250, 47))
        Z -= Z.mean(axis=0)
        Q, _ = np.linalg.qr(Z)
        out[k] = (L @ Q.T) * rng.uniform(0.5, 2.0, size=(47, 1))
    return out


def _lattice(k):
    g = np.arange(k, dtype=np.float64)
    return np.stack(np.meshgrid(g, g, indexing="ij"), -1).reshape(-1, 2)


def test_bipartite_matrices_through_the_widening_kernels(ctx):
    """Every window flagged by hand and redone by the widening passes alone (TDA_RETRY_ONLY: 128 to 512 class bits; the
    ladder of a 47-point matrix has no last rung), and the whole ladder from the first pass."""
    import torch
    dev = torch.device("cuda", ctx.device)
    d = np.stack([_bipartite_matrix(s) for s in range(3)])
    ref = [port.rips_dm(x, thresh=3.0) for x in d]
    dm = torch.from_numpy(d).to(dev)
    out = engine.DeviceDiagrams(len(d), 47, 1024, dev)
    out.status.fill_(2); out.c0.fill_(-5); out.c1.fill_(-5)
    ctx.set_retry_policy(ctx.RETRY_ONLY)
    try:
        engine.rips_dm_dev(dm, out, thresh=3.0, ctx=ctx)
    finally:
        ctx.set_retry_policy(ctx.RETRY_AUTO)
    auto = engine.rips_dm_dev(dm, thresh=3.0, h1_cap=1024, ctx=ctx)
    torch.cuda.synchronize()
    for res in (out, auto):
        assert int(res.status.max()) == 0 and int(res.status.min()) == 0
        a0, a1 = res.to_lists()
        for w in range(len(d)):
            assert _same(a0[w], ref[w][0]) and _same(a1[w], ref[w][1]), w


def test_bipartite_windows_through_the_fused_kernels_ladder(ctx):
    import torch
    dev = torch.device("cuda", ctx.device)
    W = _bipartite_windows(3, seed=5)
    out = engine.eeg_window_dev(torch.from_numpy(W).to(dev), h1_cap=1024, ctx=ctx)
    torch.cuda.synchronize()
    assert int(out.status.max()) == 0 and int(out.status.min()) == 0
    a0, a1 = out.to_lists()
    for w in range(len(W)):
        o = port.rips_dm(port.corr_dist(W[w])[1])
        assert _same(a0[w], o[0]) and _same(a1[w], o[1]), w


@pytest.mark.parametrize("route", ["matrix", "cloud"])
def test_lattice_11x11_with_and_without_the_last_rung(ctx, route):
    """100 classes alive at once on 121 points.  TDA_RETRY_ONE_STEP launches the first pass and one widening pass and
    never the last rung: the window comes back exact or flagged for it (class overflow, nothing else), never wrong.  The
    whole ladder gives the 100 rows (1, sqrt 2)."""
    P = _lattice(11)
    d = np.sqrt(((P[:, None] - P[None]) ** 2).sum(-1))
    ref = port.rips_dm(d, thresh=100.0) if route == "matrix" else port.rips_f32(port.cloud_dm(P).astype(np.float32), thresh=100.0)
    assert len(ref[1]) == 100

    def run():
        if route == "matrix":
            return engine.rips_dm_batch(d[None], thresh=100.0, h1_cap=1024, ctx=ctx)
        return engine.cloud_rips_batch(P[None], normalise=False, thresh=100.0, h1_cap=1024, ctx=ctx)
    ctx.set_retry_policy(ctx.RETRY_ONE_STEP)
    try:
        h0, h1, st = run()
    finally:
        ctx.set_retry_policy(ctx.RETRY_AUTO)
    assert st[0] in (0, 2), st
    if st[0] == 0:
        assert _same(h0[0], ref[0]) and _same(h1[0], ref[1])
    h0, h1, st = run()
    assert st[0] == 0
    assert _same(h0[0], ref[0]) and _same(h1[0], ref[1])


# ---- no triangle at all ----

@pytest.mark.parametrize("thresh", [1.5, 2.0])
def test_path_metric_has_no_triangle_to_test(ctx, thresh):
    """d(i, j) = |i - j| on 30 points: below 2 no edge has a common neighbour; at 2 the edges (i, i + 2) have exactly one,
    the apex itself, and nothing is left to test."""
    i = np.arange(30, dtype=np.float64)
    d = np.abs(i[:, None] - i[None])
    h0, h1 = _check_dm(ctx, d[None], thresh, DM_WORDS, ("path", thresh))
    assert len(h1[0]) == 0 and len(h0[0]) == 30 and np.all(h0[0][:-1, 1] == 1.0)


def test_window_of_two_points(ctx):
    d = np.array([[[0.0, 1.0], [1.0, 0.0]]])
    h0, h1 = _check_dm(ctx, d, 2.0, DM_WORDS, "two points")
    assert len(h1[0]) == 0 and len(h0[0]) == 2 and h0[0][0, 1] == 1.0
