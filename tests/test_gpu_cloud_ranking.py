"""
The ranking of the NARROW first pass of the point-cloud kernel (csrc/rips.hip: rank_edges_narrow -- keys beside the
bucket members, ranks counted in slot order): diagrams compared exactly with the CPU oracle, as tests/test_gpu_parity.py
does, with 32 class bits (ctx.set_class_words(1, 1)) so that the narrow pass is the one that answers.  The counter of
the widening passes (ctx.set_retry_counter) says whether it did: a window that a widening pass redid was not ranked
by the code under test.
"""
import numpy as np
import pytest

from oracle import port
from tda_eeg_audio_amd import engine

pytestmark = pytest.mark.gpu


def _same_multiset(a, b):
    from oracle import brute
    return np.array_equal(brute.sort_rows(a), brute.sort_rows(b))


def _narrow(ctx, clouds, n_pts=None, normalise=False, thresh=100.0):
    """One launch through the narrow first pass: diagrams, status words, windows redone by a widening pass."""
    import torch
    ctr = torch.zeros(4, dtype=torch.int64, device=torch.device("cuda", 0))
    ctx.set_class_words(1, 1)
    ctx.set_retry_counter(ctr.data_ptr())
    try:
        h0, h1, st = engine.cloud_rips_batch(clouds, n_pts=n_pts, normalise=normalise, thresh=thresh, h1_cap=1024, ctx=ctx)
        torch.cuda.synchronize()
    finally:
        ctx.set_retry_counter(None)
        ctx.set_class_words(2, 1)
    return h0, h1, st, int(ctr.sum())


def _oracle(pc, normalise, thresh):
    x = port.minmax_normalise(pc) if normalise else pc
    return port.rips_f32(port.cloud_dm(x).astype(np.float32), thresh=thresh)


def _polygon3(n):
    ang = 2.0 * np.pi * np.arange(n) / n
    return np.stack([np.cos(ang), np.sin(ang), np.zeros(n)], axis=1)


def _check(ctx, pcs, normalise, thresh, redone_cap):
    """Clouds of one size or several (padded to the largest, the sizes in n_pts) in ONE launch, each against the oracle."""
    p_cap = max(len(p) for p in pcs)
    batch = np.zeros((len(pcs), p_cap, 3))
    for i, p in enumerate(pcs):
        batch[i, :len(p)] = p
    h0, h1, st, redone = _narrow(ctx, batch, n_pts=[len(p) for p in pcs], normalise=normalise, thresh=thresh)
    print(f"{len(pcs)} clouds of {min(map(len, pcs))}..{p_cap} points: {redone} redone by a widening pass")
    assert redone <= redone_cap, f"{redone} of {len(pcs)} windows were redone by a widening pass: not a test of the narrow pass"
    assert not (st & ~4).any(), st
    for i, p in enumerate(pcs):
        o = _oracle(p, normalise, thresh)
        assert _same_multiset(h0[i], o[0]) and _same_multiset(h1[i], o[1]), (i, len(p))
    return h0, h1


def _polygon_answer(n, h0, h1):
    """Known answer (tests/test_oracle_golden.py: polygon_h1): ONE class, from the side to the chord of ceil(n / 3) steps."""
    from test_oracle_golden import polygon_h1
    b, d = polygon_h1(n)
    assert h1.shape == (1, 2), h1
    assert abs(h1[0, 0] - b) < 2e-7 * b and abs(h1[0, 1] - d) < 2e-7 * d, (n, h1)
    assert len(h0) == n and np.all(np.abs(h0[:-1, 1] - b) < 2e-7 * b) and np.isinf(h0[-1, 1])


@pytest.mark.parametrize("n", list(range(6, 14)))
def test_regular_polygons_every_bucket_a_tie(ctx, n):
    """n evenly spaced points on the unit circle (z = 0, coordinates as given): every bucket of the ranking is one chord
    length with n (or n / 2) tied keys -- n = 6..13 has bucket sizes of every residue mod 4, the tie path and the read
    into the next bucket.  No widening pass."""
    h0, h1 = _check(ctx, [_polygon3(n)], False, 10.0, 0)
    _polygon_answer(n, h0[0], h1[0])


def test_every_edge_ranked_padding_at_the_end_of_the_arrays(ctx):
    """Ev = E = 7,626 = NARROW_EMAX: the padding of the walk sits at the very end of skey, in front of sidx.
    * The 124-gon.  Its one class lives from rank 124 to rank ~5,100 (the chords of 42 steps), and the narrow layout hands
      a window with a class alive in a chunk that starts beyond rank ~4,600 to the wide pass (csrc/rips.hip, the comment
      above rips_sweep: class vectors and `ord` share a region).  So this window IS redone by a widening pass, with this
      ranking and with the one before it (measured: 1 of 1 on both): the narrow ranking runs on it, its padding at the
      end of the arrays, and the diagram checked here is the wide pass's.
    * 124 lattice points of the sphere x^2 + y^2 + z^2 = 89, 62 antipodal pairs: the 62 diameters are equal to the bit
      and are the enclosing radius, so again Ev = E, with heavy ties throughout (integer squared lengths) -- and every
      class is dead by rank ~2,100 (CPU oracle), so the narrow pass answers alone: no widening pass."""
    h0, h1 = _check(ctx, [_polygon3(124)], False, 10.0, 1)
    _polygon_answer(124, h0[0], h1[0])
    m = 9
    pts = [(x, y, z) for x in range(-m, m + 1) for y in range(-m, m + 1) for z in range(-m, m + 1) if x * x + y * y + z * z == 89]
    half = [p for p in pts if p > (0, 0, 0)][:62]
    sphere = np.array(half + [tuple(-c for c in p) for p in half], dtype=np.float64)
    assert sphere.shape == (124, 3)
    _check(ctx, [sphere], False, 1000.0, 0)


def test_zero_keys_one_bucket_and_three_points(ctx):
    """P = 3 (three edges: fewer slots than lanes); the regular tetrahedron (six equal keys: kmin == teff, one bucket,
    every rank decided by the flat index); coincident points (zero keys, kmin = 0): every vertex of the 9-gon twice,
    and a random cloud whose second half repeats the first.  No window may need a widening pass."""
    rng = np.random.default_rng(3)
    tri = rng.random((3, 3))
    tetra = np.array([[1.0, 1.0, 1.0], [1.0, -1.0, -1.0], [-1.0, 1.0, -1.0], [-1.0, -1.0, 1.0]])
    twice = np.repeat(_polygon3(9), 2, axis=0)
    dup = rng.random((14, 3)); dup[7:] = dup[:7]
    for pcs in ([tri], [tetra], [twice], [dup], [tri, tetra, twice, dup]):
        h0, h1 = _check(ctx, pcs, False, 10.0, 0)
    assert len(h1[1]) == 0 and len(h0[1]) == 4 and np.all(np.abs(h0[1][:-1, 1] - np.sqrt(8.0)) < 2e-7 * np.sqrt(8.0))
    assert h1[2].shape == (1, 2) and len(h0[2]) == 9          # zero-length merges are dropped


# Seed 20261 for all three cases below.  What the parent of the commit that added this file gave with it (windows
# redone by a widening pass): 0 of 20 clouds of 64 points, 0 of 20 of 65 points, 0 of 200 in the mixed launch.
SEED = 20261


def _curve_cloud(rng, P):
    """A random cloud of the kind the narrow pass is built for: P points along a random closed curve (three harmonics)
    with jitter -- few classes alive at once, as the Takens clouds of band-limited windows."""
    t = np.sort(rng.random(P)) * 2.0 * np.pi
    amp = rng.standard_normal((3, 3)) / np.array([1.0, 2.0, 3.0])[:, None]
    ph = rng.random((3, 3)) * 2.0 * np.pi
    pc = sum(amp[k][None, :] * np.sin((k + 1) * t[:, None] + ph[k][None, :]) for k in range(3))
    return pc + 0.05 * rng.standard_normal((P, 3))


@pytest.mark.parametrize("P", [64, 65])
def test_random_clouds_at_the_vertex_word_boundary(ctx, P):
    """20 random clouds of 64 and of 65 points (one and two vertex words in the sweep behind the ranking), min-max
    normalised as the audio route does; at most 1 in 20 may have needed a widening pass."""
    rng = np.random.default_rng(SEED + P)
    _check(ctx, [_curve_cloud(rng, P) for _ in range(20)], True, 2.0, 1)


def test_mixed_sizes_in_one_launch(ctx):
    """200 random clouds with P mixed over 3..124 in one launch (every workgroup its own E, Ev and slot count, the
    largest at NARROW_EMAX); at most 1 in 20 may have needed a widening pass."""
    rng = np.random.default_rng(SEED)
    sizes = np.concatenate([[3, 4, 5, 123, 124, 124], rng.integers(3, 125, 194)])
    _check(ctx, [_curve_cloud(rng, int(P)) for P in sizes], True, 2.0, 10)
