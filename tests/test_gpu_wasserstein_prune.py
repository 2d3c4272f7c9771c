"""
The pruning of the Wasserstein solver (tda_set_wasserstein_pruning) against the full computation, in one process on one
context: dead rows and columns trimmed off the equal-birth recurrence, and the all-diagonal short cut of the general
solver, must leave every output and every status word as it was, bit for bit.

Bars: `out` and `status` with pruning on and off identical as raw bytes (also across the three launch schemes); values
with pruning on within 1e-10 of brute.safe_wasserstein_oracle; the counter (tda_set_wasserstein_counter) shows that the
short cut was taken on exactly the pairs built far apart, that at least the points built dead were trimmed (both built a
factor 2 beyond the cut), and that nothing is pruned with the switch off.  Under 300 pairs in all, diagrams of at most
128 rows.
"""
import numpy as np
import pytest

from oracle import brute
from tda_eeg_audio_amd import engine

pytestmark = pytest.mark.gpu

CP = 0.7071067811865476
CUT = (1.0 - CP) / (1.0 + CP)                 # q / p below which a column can only go to the diagonal: 1 / (3 + 2 sqrt 2)


class Batch:
    """Pairs (A_i, B_i) in buffers of the given capacities; `dead` = points built to be trimmed, `far` = pairs built far apart."""

    def __init__(self, cap_a, cap_b):
        self.cap = (cap_a, cap_b)
        self.A, self.B, self.dead, self.far = [], [], 0, 0

    def add(self, a, b, dead=0, far=0):
        self.A.append(np.asarray(a, float).reshape(-1, 2))
        self.B.append(np.asarray(b, float).reshape(-1, 2))
        self.dead += dead
        self.far += far

    def arrays(self):
        out = []
        for dgms, cap in ((self.A, self.cap[0]), (self.B, self.cap[1])):
            rows = np.full((len(dgms), cap, 2), 7.25)               # stale rows behind the count
            cnt = np.zeros(len(dgms), np.int32)
            for i, d in enumerate(dgms):
                assert len(d) <= cap
                rows[i, :len(d)] = d
                cnt[i] = len(d)
            out += [rows, cnt]
        return out


def _h0(b0, pers):
    p = np.sort(np.asarray(pers, float))
    return np.stack([np.full(len(p), b0), b0 + p], 1)


def equal_birth_batch():
    rng = np.random.default_rng(21)
    B = Batch(128, 128)
    # (persistences up to 1.4: a total of 128 of them stays near 100, where the order of a sum moves it by 1e-12, not 1e-10)
    live = lambda n: rng.uniform(0.05, 0.1, n)                      # ratios < 2: always live against each other
    low = lambda n: rng.uniform(1e-4, 0.05 * CUT / 2, n)            # a factor 2 below the cut of 0.05
    high = lambda n: rng.uniform(0.1 * 2.0 / CUT, 1.4, n)           # a factor 2 above the cut of 0.1
    for R, C in [(46, 121), (64, 128), (13, 64), (30, 65), (64, 64), (5, 128)]:
        B.add(_h0(0, live(R)), _h0(0, live(C)))                                             # no dead column
        B.add(_h0(0, live(R)), _h0(0, np.r_[low(C // 2), live(C - C // 2)]), dead=C // 2)  # dead prefix
        B.add(_h0(0, np.r_[live(C - C // 3), high(C // 3)]), _h0(0, live(R)), dead=C // 3)  # dead suffix, A the larger
        B.add(_h0(0, live(R)), _h0(0, np.r_[low(C // 4), live(C - 2 * (C // 4)), high(C // 4)]), dead=2 * (C // 4))
        B.add(_h0(0, live(R)), _h0(0, low(C)), dead=R + C)                                  # every column dead
        B.add(_h0(0, live(R)), _h0(0, high(C)), dead=R + C)
        if R >= 4:                                                                          # dead rows around live ones
            B.add(_h0(0, np.r_[low(2), live(R - 4), high(2)]), _h0(0, live(C)), dead=4)
    # R = 1, C = 1
    for p, q in [(0.7, 0.8), (0.7, 0.01), (0.01, 0.7), (0.7, 0.7)]:
        B.add(_h0(0, [p]), _h0(0, [q]), dead=2 if min(p, q) < 0.1 else 0)
    B.add(_h0(0, [0.07]), _h0(0, np.r_[low(40), live(40)]), dead=40)
    B.add(_h0(0, np.r_[live(20), high(20)]), _h0(0, [0.09]), dead=20)
    # empty diagrams (-> {(0, 0)}), rows that are not finite
    B.add(np.zeros((0, 2)), _h0(0, live(9)))
    B.add(_h0(0, live(9)), np.zeros((0, 2)))
    B.add(np.zeros((0, 2)), np.zeros((0, 2)))
    B.add([[0.0, np.inf]] * 3, _h0(0, live(5)))
    B.add(np.r_[_h0(0, live(10)), [[0.0, np.inf]], _h0(0, low(10))], _h0(0, live(40)))      # unsorted: the general solver
    inf_mid = _h0(0, np.r_[low(10), live(10)])
    B.add(np.insert(inf_mid, 5, [0.0, np.inf], axis=0), _h0(0, live(40)), dead=10)                      # sorted once the row is dropped
    # tied deaths
    for R, C in [(20, 50), (64, 100)]:
        B.add(_h0(0, rng.integers(4, 9, R) / 80.0), _h0(0, rng.integers(1, 600, C) / 640.0))
        B.add(_h0(0, np.full(R, 0.75)), _h0(0, np.r_[np.full(C // 2, 0.01), np.full(C - C // 2, 0.75)]), dead=C // 2)
    # births != 0, one of them far larger than the persistences
    for b0 in (0.3, -0.75, 1.25):
        B.add(_h0(b0, live(30)), _h0(b0, np.r_[low(25), live(50), high(25)]), dead=50)
        # (persistences >= 0.01: next to a birth of 1.25 the expansion's cancellation moves a cost |p - q| by about
        # ulp(3) / 2|p - q|, which for persistences of 1e-4 is 2e-12 per matched pair, for these 2e-14;
        # births of 1e3 and more: test_large_common_birth_bits)
        B.add(_h0(b0, 10.0 ** rng.uniform(-2, 0, 40)), _h0(b0, 10.0 ** rng.uniform(-2, 0, 90)))
    # ratios within an ulp of the cut, and on either side of the margin
    for p0 in (1.0, 0.7310585786300049):
        for side in (CUT, 1.0 / CUT):
            base = p0 * side
            qs = [np.nextafter(base, -np.inf), base, np.nextafter(base, np.inf)]
            qs += [base * (1.0 + s * r) for r in (5e-7, 9.9e-7, 1.01e-6, 2e-6, 1e-4) for s in (-1.0, 1.0)]
            for q in qs:
                B.add(_h0(0, [p0, p0]), _h0(0, [q, q, p0]))
    # more than 64 rows: the general solver, with and without pruning
    B.add(_h0(0, live(65)), _h0(0, np.r_[low(30), live(36)]))
    B.add(_h0(0, low(65)), _h0(0, rng.uniform(0.50, 0.52, 70)), far=1)      # |d - d'| > 0.49 against s + t < 0.38
    return B


def large_birth_batch():
    """A common birth far larger than the persistences: the cancellation in the expansion is what the margin is for."""
    rng = np.random.default_rng(24)
    B = Batch(64, 128)
    for b0 in (1000.0, 1e6, -4e4):
        for R, C in [(30, 100), (64, 128), (1, 50)]:
            B.add(_h0(b0, rng.uniform(0.5, 1.0, R)), _h0(b0, 10.0 ** rng.uniform(-6, 2, C)))
            B.add(_h0(b0, 10.0 ** rng.uniform(-6, 2, R)), _h0(b0, 10.0 ** rng.uniform(-6, 2, C)))
    return B


def _h1(rng, n, b_lo, b_hi, p_lo, p_hi):
    b = rng.uniform(b_lo, b_hi, n)
    return np.stack([b, b + rng.uniform(p_lo, p_hi, n)], 1)


SIZES = [(35, 41), (20, 100), (64, 64), (64, 65), (65, 64), (1, 128), (63, 2), (128, 128), (3, 3)]   # both sides of 64 x 64


def general_batches():
    """far apart / one live cell / overlapping, in buffers of 256 rows: the small first launch and the wide one."""
    rng = np.random.default_rng(22)
    far, one_live, overlap = Batch(256, 256), Batch(256, 256), Batch(256, 256)
    eeg = lambda n: _h1(rng, n, 1.0, 1.1, 0.05, 0.3)                # s <= 0.22
    aud = lambda n: _h1(rng, n, 0.1, 0.2, 0.005, 0.02)              # t <= 0.015; the boxes are > 1.1 apart: > 2 (s + t)
    for M, N in SIZES:
        far.add(eeg(M), aud(N), far=1)
        far.add(aud(M), eeg(N), far=1)
        # the bounding boxes overlap, every point is far from the other diagram's box all the same
        Mt = min(M, 80)
        two = np.r_[_h1(rng, Mt, 0.0, 0.1, 0.005, 0.01), _h1(rng, Mt // 2, 10.0, 10.1, 0.005, 0.01)]
        far.add(two, _h1(rng, max(N, len(two)), 5.0, 5.1, 0.005, 0.01), far=1)
        # one live cell just inside: a long-lived point of each diagram next to each other
        a, b = eeg(M), aud(N)
        a[M // 2], b[N // 3] = (0.6, 1.6), (0.61, 1.61)
        one_live.add(a, b)
        overlap.add(_h1(rng, M, 0.0, 1.0, 0.0, 1.0), _h1(rng, N, 0.0, 1.0, 0.0, 1.0))
        overlap.add(_h1(rng, M, 0.0, 1.0, 0.0, 0.2), _h1(rng, N, 0.3, 1.2, 0.0, 0.2))
    far.add(np.zeros((0, 2)), aud(30), far=1)                        # {(0, 0)} against short-lived points
    return far, one_live, overlap


@pytest.fixture(scope="module")
def counter(ctx):
    import torch
    c = torch.zeros(3, dtype=torch.int64, device=torch.device("cuda", ctx.device))
    ctx.set_wasserstein_counter(c.data_ptr())
    yield c
    ctx.set_wasserstein_counter(None)
    ctx.set_wasserstein_pruning(True)
    ctx.set_launch_scheme(ctx.SCHEME_LISTS)


def _run(ctx, counter, arrays, prune, scheme=None):
    import torch
    ctx.set_wasserstein_pruning(prune)
    ctx.set_launch_scheme(ctx.SCHEME_LISTS if scheme is None else scheme)
    counter.zero_()
    torch.cuda.synchronize()
    out, st = engine.wasserstein_batch(*arrays, ctx=ctx, want_status=True)
    torch.cuda.synchronize()
    return out, st, counter.cpu().numpy().copy()


def _oracle(batch):
    return np.array([brute.safe_wasserstein_oracle(a, b) for a, b in zip(batch.A, batch.B)])


def test_equal_birth_trimming(ctx, counter):
    batch = equal_birth_batch()
    arrays = batch.arrays()
    n = len(batch.A)
    on, st_on, c_on = _run(ctx, counter, arrays, True)
    off, st_off, c_off = _run(ctx, counter, arrays, False)
    print(f"equal birth: {n} pairs, counters on {c_on.tolist()} off {c_off.tolist()}, points built dead {batch.dead}")
    assert on.tobytes() == off.tobytes() and st_on.tobytes() == st_off.tobytes()
    assert (st_on == 0).all()
    err = np.abs(on - _oracle(batch))
    print("equal birth: max |gpu - oracle| =", err.max())
    assert err.max() < 1e-10
    assert c_on[2] == n and c_off[2] == n
    assert c_on[1] >= batch.dead > 0 and c_on[0] == batch.far
    assert c_off[0] == 0 and c_off[1] == 0


def test_large_common_birth_bits(ctx, counter):
    """Bits only: at births of 1e3 .. 1e6 the reference's own expansion is off by more than 1e-10."""
    batch = large_birth_batch()
    arrays = batch.arrays()
    on, st_on, c_on = _run(ctx, counter, arrays, True)
    off, st_off, c_off = _run(ctx, counter, arrays, False)
    print(f"large birth: {len(batch.A)} pairs, counters on {c_on.tolist()} off {c_off.tolist()}")
    assert on.tobytes() == off.tobytes() and st_on.tobytes() == st_off.tobytes()
    assert (st_on == 0).all() and c_on[1] > 0 and c_off[1] == 0


def test_general_short_cut(ctx, counter):
    far, one_live, overlap = general_batches()
    total = 0
    for name, batch in (("far", far), ("one live cell", one_live), ("overlap", overlap)):
        arrays = batch.arrays()
        n = len(batch.A)
        total += n
        ref = _oracle(batch)
        runs = {}
        for scheme in (ctx.SCHEME_LISTS, ctx.SCHEME_GRID, ctx.SCHEME_ONE):
            for prune in (True, False):
                runs[scheme, prune] = _run(ctx, counter, arrays, prune, scheme)
        out0, st0, _ = runs[ctx.SCHEME_LISTS, True]
        assert (st0 == 0).all()
        for key, (out, st, c) in runs.items():
            assert out.tobytes() == out0.tobytes() and st.tobytes() == st0.tobytes(), (name, key)
            assert c[2] == n, (name, key, c)
            if key[1]:
                if name == "far":
                    assert c[0] == batch.far == n, (name, key, c)
                elif name == "one live cell":
                    assert c[0] == 0, (name, key, c)
                assert c[1] == 0
            else:
                assert c[0] == 0 and c[1] == 0, (name, key, c)
        err = np.abs(out0 - ref)
        print(f"{name}: {n} pairs, short cuts {runs[ctx.SCHEME_LISTS, True][2][0]}, max |gpu - oracle| = {err.max()}")
        assert err.max() < 1e-10
    assert total <= 300


def _dev(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def test_cross_and_matrix_entry_points(ctx, counter):
    """One call each through tda_wasserstein_cross_dev and tda_wasserstein_matrix_dev: the same solver, its options from
    the same context.  Two A groups of three diagrams against two B groups; H1-like, far apart and overlapping."""
    import torch
    dev = torch.device("cuda", ctx.device)
    rng = np.random.default_rng(23)
    b = Batch(256, 256)
    for k in range(6):                  # A 1, 3, 5 meet B 4, 0, 2: far apart; the other three pairs overlap
        b.add(_h1(rng, 30 + k, 1.0, 1.1, 0.05, 0.3) if k % 2 else _h1(rng, 30 + k, 0.0, 1.0, 0.0, 1.0),
              _h1(rng, 40 + 10 * k, 0.0, 1.0, 0.0, 1.0) if k % 2 else _h1(rng, 40 + 10 * k, 0.1, 0.2, 0.005, 0.02))
    ra, ca, rb, cb = (_dev(x, dev) for x in b.arrays())
    seg = _dev(np.array([0, 3, 6], np.int32), dev)
    status_b = torch.zeros(6, dtype=torch.int32, device=dev)
    partner = _dev(np.array([1, 0], np.int32), dev)
    cls_a = _dev(np.array([0, 0], np.int32), dev)
    got = {}
    for prune in (True, False):
        ctx.set_wasserstein_pruning(prune)
        counter.zero_()
        w, st = engine.wasserstein_cross_dev(ra, ca, seg, rb, cb, seg, status_b, partner, ctx=ctx)
        torch.cuda.synchronize()
        c_cross = counter.cpu().numpy().copy()
        counter.zero_()
        out, pairs, flags = engine.wasserstein_matrix_dev(ra, ca, seg, cls_a, rb, cb, seg, status_b, 2, ctx=ctx)
        torch.cuda.synchronize()
        c_mat = counter.cpu().numpy().copy()
        got[prune] = [t.cpu().numpy() for t in (w, st, out, pairs, flags)]
        assert c_cross[2] == 6 and c_mat[2] == 12
        if prune:
            assert c_cross[0] >= 3 and c_mat[0] >= 3
        else:
            assert c_cross[0] == 0 and c_mat[0] == 0
    for x, y in zip(got[True], got[False]):
        assert x.tobytes() == y.tobytes()
    w, st = got[True][:2]
    assert (st == 0).all()
    # A diagram i of group g against B diagram i of the partner group
    ref = np.array([brute.safe_wasserstein_oracle(b.A[i], b.B[(i + 3) % 6]) for i in range(6)])
    assert np.abs(w - ref).max() < 1e-10
