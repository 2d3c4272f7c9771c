"""
The Wasserstein distances of order 1 and 2 with the L2 or the L-infinity ground metric (csrc/wasserstein_q.hip) against
the CPU reference tests/wasserstein_q_ref.py, all four variants unless a test says otherwise.

Bar: every status 0 and, with S the sum of all diagonal costs of the pair and V_gpu = out (order 1) or out * out
(order 2), |V_gpu - V_ref| <= 1e-10 * max(1, S) -- the bar the order-1 kernel is held to against the same kind of
reference (test_gpu_parity.py), placed on V so that the root of a tiny V does not blow it up.  Every test prints the
largest deviation it saw, in units of max(1, S).  Known answers are `==`; pruning on against off, a pair alone against
the same pair in a batch, and index arrays against gathered buffers are bytes.  A few hundred pairs per variant, the
references computed once per test.
"""
import numpy as np
import pytest

import wasserstein_q_ref as wq
from tda_eeg_audio_amd import _lib, engine, pipeline, synth, utils

pytestmark = pytest.mark.gpu

VARIANTS = wq.VARIANTS
BAR = 1e-10


def _pack(dgms, cap, fill=7.25):
    """Diagrams in a buffer of `cap` rows with stale rows (fill) behind the count."""
    rows = np.full((len(dgms), cap, 2), fill)
    cnt = np.zeros(len(dgms), np.int32)
    for i, d in enumerate(dgms):
        d = np.asarray(d, float).reshape(-1, 2)
        assert len(d) <= cap
        rows[i, :len(d)] = d
        cnt[i] = len(d)
    return rows, cnt


def _gpu(ctx, A, B, cap_a, cap_b, order, ground, **kw):
    ra, ca = _pack(A, cap_a)
    rb, cb = _pack(B, cap_b)
    return engine.wasserstein_q_batch(ra, ca, rb, cb, order=order, ground=ground, ctx=ctx, want_status=True, **kw)


def _refs(A, B, order, ground):
    """(V_ref, S) per pair."""
    return (np.array([wq.value_ref(a, b, order, ground) for a, b in zip(A, B)]),
            np.array([wq.diag_sum(a, b, order, ground) for a, b in zip(A, B)]))


def _held(out, st, ref, S, order, what):
    """The bar; returns the largest deviation in units of max(1, S)."""
    assert (st == 0).all(), (what, np.flatnonzero(st != 0)[:5], st[st != 0][:5])
    V = out if order == 1 else out * out
    dev = np.abs(V - ref) / np.maximum(1.0, S)
    k = int(np.argmax(dev))
    print(f"{what}: {len(out)} pairs, max |V_gpu - V_ref| / max(1, S) = {dev[k]:.3g}")
    assert dev[k] <= BAR, (what, k, V[k], ref[k], S[k])
    return float(dev[k])


def _check(ctx, A, B, cap_a, cap_b, order, ground, what, ref=None):
    ref = _refs(A, B, order, ground) if ref is None else ref
    out, st = _gpu(ctx, A, B, cap_a, cap_b, order, ground)
    _held(out, st, ref[0], ref[1], order, f"{what} ({order}, {ground})")
    return out, st, ref


def test_known_answers(ctx):
    for order, ground in VARIANTS:
        known = [(a, b, want[order, ground]) for a, b, want in wq.KNOWN if (order, ground) in want]
        out, st = _gpu(ctx, [k[0] for k in known], [k[1] for k in known], 8, 8, order, ground)
        assert (st == 0).all() and out.tolist() == [k[2] for k in known], (order, ground, out.tolist())
        out, st = _gpu(ctx, [k[1] for k in known], [k[0] for k in known], 8, 8, order, ground)
        assert (st == 0).all() and out.tolist() == [k[2] for k in known], (order, ground, out.tolist())


@pytest.mark.parametrize("order,ground", VARIANTS)
def test_brute_forceable_pairs_with_ties(ctx, order, ground):
    pairs = wq.small_pairs(200, seed=41)
    A, B = [p[0] for p in pairs], [p[1] for p in pairs]
    _, _, (ref, S) = _check(ctx, A, B, 4, 4, order, ground, "small pairs")
    for k in range(0, 200, 5):                                     # the reference itself against exhaustive search
        assert abs(ref[k] - wq.value_brute(A[k], B[k], order, ground)) <= 1e-13 * max(1.0, S[k])


SIZES = {128: [(1, 1), (46, 122), (63, 64), (64, 65), (65, 128), (5, 128), (128, 128)],
         256: [(130, 250), (256, 256)], 512: [(300, 512)]}


@pytest.fixture(scope="module")
def sized():
    """Random float32-exact diagrams at the sizes where the kernel changes path (rows in one or more lanes' slots, 2 / 4 /
    8 column slots per lane), half of them with ties."""
    rng = np.random.default_rng(42)
    out = {}
    for cap, sizes in SIZES.items():
        A = [wq.random_diagram(rng, R, ties=i % 2 == 1) for i, (R, C) in enumerate(sizes)]
        B = [wq.random_diagram(rng, C, ties=i % 2 == 1) for i, (R, C) in enumerate(sizes)]
        out[cap] = (A, B)
    return out


@pytest.mark.parametrize("order,ground", VARIANTS)
@pytest.mark.parametrize("cap", sorted(SIZES))
def test_sizes_both_ways_round(ctx, sized, cap, order, ground):
    A, B = sized[cap]
    _, _, ref = _check(ctx, A, B, cap, cap, order, ground, f"sizes, capacity {cap}")               # B the larger
    _check(ctx, B, A, cap, cap, order, ground, f"sizes reversed, capacity {cap}", ref)             # A the larger
    if cap == 128:                                                 # buffers of different capacities, the small side first / second
        sub = (ref[0][:2], ref[1][:2])
        _check(ctx, A[:2], B[:2], 47, 128, order, ground, "capacities 47 x 128", sub)
        _check(ctx, B[:2], A[:2], 128, 47, order, ground, "capacities 128 x 47", sub)


def _equal_birth_pairs():
    rng = np.random.default_rng(43)
    f32 = lambda x: np.float32(x).astype(float)
    h0 = wq.h0_diagram
    A, B = [], []
    for R, C in [(46, 122), (64, 128), (1, 50), (65, 66)]:          # (65, 66) falls off the 64-row path
        A.append(h0(0.0, f32(rng.uniform(0.01, 1.0, R)))); B.append(h0(0.0, f32(rng.uniform(0.01, 1.0, C))))
        A.append(h0(0.0, f32(rng.uniform(0.01, 1.0, R)), sort=False)); B.append(h0(0.0, f32(rng.uniform(0.01, 1.0, C)), sort=False))
        A.append(h0(0.0, rng.integers(1, 9, R) / 8.0)); B.append(h0(0.0, rng.integers(1, 17, C) / 16.0))      # tied deaths
        A.append(h0(0.375, f32(rng.uniform(0.01, 1.0, R)))); B.append(h0(0.375, f32(rng.uniform(0.01, 1.0, C))))   # shifted births
        A.append(h0(-0.75, f32(rng.uniform(0.01, 1.0, R)))); B.append(h0(0.25, f32(rng.uniform(0.01, 1.0, C))))    # two different births
        A.append(h0(0.0, np.full(R, 0.75))); B.append(h0(0.0, np.full(C, 0.75)))                               # all persistences equal
        A.append(h0(0.0, np.full(R, 0.75))); B.append(h0(0.0, np.full(C, 0.5)))
        # the workload's shape: long-lived rows, half of the columns far below the cut
        A.append(h0(0.0, rng.uniform(0.48, 1.04, R)))
        B.append(h0(0.0, np.where(rng.random(C) < 0.5, rng.uniform(1e-4, 0.04, C), rng.uniform(0.08, 0.9, C))))
    return A, B


@pytest.mark.parametrize("order,ground", VARIANTS)
def test_equal_birth_pairs(ctx, order, ground):
    A, B = _equal_birth_pairs()
    _, _, ref = _check(ctx, A, B, 128, 128, order, ground, "equal births")
    _check(ctx, B, A, 128, 128, order, ground, "equal births reversed", ref)


def _hygiene_batches():
    """The batches of test_buffer_hygiene, built once per call: name -> (A, B or None, (ra, ca, rb, cb), idx keywords).
    A / B are the diagrams the reference sees (None: the test has its own assertion)."""
    rng = np.random.default_rng(44)
    d = lambda n: wq.random_diagram(rng, n)
    inf_mid = np.insert(d(20), 7, [0.25, np.inf], axis=0)
    nan_mid = np.insert(d(9), 3, [np.nan, 0.5], axis=0)
    all_inf = np.array([[0.0, np.inf]] * 3)
    none = np.zeros((0, 2))
    out = {}
    # stale rows of 7.25 behind every count, inf / NaN rows in the middle, diagrams without a finite row, empty diagrams
    A = [d(10), inf_mid, nan_mid, all_inf, d(6), all_inf, none, none, d(5)]
    B = [d(30), d(40), inf_mid, d(12), all_inf, all_inf, none, d(7), none]
    out["rows"] = (A, B, _pack(A, 64) + _pack(B, 64), {})
    # count 0 with capacity 1
    rows = np.full((2, 1, 2), 7.25)
    out["capacity 1"] = (None, None, (rows, np.zeros(2, np.int32), rows, np.array([0, 1], np.int32)), {})
    # counts beyond the capacity and below zero are clamped, as in the Wasserstein entry points
    ra, _ = _pack([d(8)], 8)
    rb, _ = _pack([d(8)], 8)
    out["clamped counts"] = ([ra[0]], [none], (ra, np.array([100], np.int32), rb, np.array([-3], np.int32)), {})
    # index arrays
    A = [wq.random_diagram(rng, int(n)) for n in rng.integers(0, 40, 12)]
    B = [wq.random_diagram(rng, int(n)) for n in rng.integers(0, 90, 9)]
    ia, ib = rng.integers(0, 12, 30).astype(np.int32), rng.integers(0, 9, 30).astype(np.int32)
    out["index arrays"] = ([A[i] for i in ia], [B[j] for j in ib], _pack(A, 64) + _pack(B, 128), dict(idx_a=ia, idx_b=ib))
    return out


@pytest.mark.parametrize("order,ground", VARIANTS)
def test_buffer_hygiene(ctx, order, ground):
    kw = dict(order=order, ground=ground, ctx=ctx, want_status=True)
    got = {}
    for name, (A, B, arrays, idx) in _hygiene_batches().items():
        out, st = engine.wasserstein_q_batch(*arrays, **idx, **kw)
        got[name] = (out, st)
        if A is not None:
            _held(out, st, *_refs(A, B, order, ground), order, f"hygiene, {name} ({order}, {ground})")
    out, st = got["rows"]
    assert out[5] == 0.0 and out[6] == 0.0
    out, st = got["capacity 1"]
    assert (st == 0).all() and out[0] == 0.0 and out[1] == 0.0
    # index arrays against gathered buffers: bytes
    (ra, ca, rb, cb), idx = _hygiene_batches()["index arrays"][2:]
    ia, ib = idx["idx_a"], idx["idx_b"]
    out, st = got["index arrays"]
    ident, st2 = engine.wasserstein_q_batch(ra[ia], ca[ia], rb[ib], cb[ib], **kw)
    assert (st2 == 0).all() and out.tobytes() == ident.tobytes()
    # a pair alone and the same pair inside the batch: the same bytes
    for k in (0, 7, 29):
        alone, st1 = engine.wasserstein_q_batch(ra[ia[k]][None], ca[ia[k]][None], rb[ib[k]][None], cb[ib[k]][None], **kw)
        assert st1[0] == 0 and alone.tobytes() == out[k:k + 1].tobytes()


def _capacity_batch():
    """513 finite rows in buffers of 600: A too large, B too large, a pair that fits."""
    rng = np.random.default_rng(45)
    big, small = wq.random_diagram(rng, 513), wq.random_diagram(rng, 10)
    return big, small, _pack([big, small, small], 600) + _pack([small, big, small], 600)


def test_pair_above_the_capacity_limit_is_a_status(ctx):
    big, small, arrays = _capacity_batch()
    for order, ground in VARIANTS:
        out, st = engine.wasserstein_q_batch(*arrays, order=order, ground=ground, ctx=ctx, want_status=True)
        assert st.tolist() == [_lib.TDA_WIN_NOT_CONVERGED, _lib.TDA_WIN_NOT_CONVERGED, 0], (order, ground)
        assert np.isnan(out[:2]).all() and out[2] == 0.0
    fin = np.vstack([big[:512], [[0.0, np.inf]] * 8])              # 520 rows, 512 of them finite: fits
    _check(ctx, [fin], [small], 600, 600, 2, "l2", "512 finite rows of 520")


def test_bad_parameters_are_rejected_by_the_library(ctx):
    """The C entry points themselves: TDA_ERR_INVALID (1) and nothing launched -- out keeps its bytes."""
    ra, ca = _pack([[[0, 1]]], 2)
    out, st = np.full(1, 123.0), np.full(1, 77, np.int32)
    P = _lib.ptr
    for order, ground in [(0, 0), (3, 0), (2, 2), (1, -1)]:
        rc = ctx.lib.tda_wasserstein_q_batch(ctx.h, P(ra), P(ca), 1, 2, P(ra), P(ca), 1, 2, None, None, 1, order, ground, P(out), P(st))
        assert rc == 1 and out[0] == 123.0 and st[0] == 77, (order, ground, rc)
    for order, ground in [(3, "l2"), (2, "l1")]:
        with pytest.raises(_lib.TdaError):
            engine.wasserstein_q_batch(ra, ca, ra, ca, order=order, ground=ground, ctx=ctx)


def test_order_1_l2_against_the_existing_distance(ctx):
    """The same quantity, not the same float: within the bound of the margin comment in csrc/wasserstein.hip."""
    rng = np.random.default_rng(46)
    A = [wq.random_diagram(rng, int(n), ties=k % 3 == 0) for k, n in enumerate(rng.integers(0, 100, 40))]
    B = [wq.random_diagram(rng, int(n), ties=k % 3 == 0) for k, n in enumerate(rng.integers(0, 128, 40))]
    eb = _equal_birth_pairs()
    A, B = A + eb[0], B + eb[1]
    ra, ca = _pack(A, 128)
    rb, cb = _pack(B, 128)
    new, st = engine.wasserstein_q_batch(ra, ca, rb, cb, order=1, ground="l2", ctx=ctx, want_status=True)
    old, st_o = engine.wasserstein_batch(ra, ca, rb, cb, ctx=ctx, want_status=True)
    assert (st == 0).all() and (st_o == 0).all()
    X = np.array([max(np.abs(wq.clean(a)).max(), np.abs(wq.clean(b)).max()) for a, b in zip(A, B)])
    n = np.array([min(len(wq.clean(a)), len(wq.clean(b))) for a, b in zip(A, B)])
    bound = 1e-7 * X * (n + 1)
    diff = np.abs(new - old)
    print(f"(1, l2) against tda_wasserstein_batch: max |difference| = {diff.max():.3g}, smallest bound {bound.min():.3g}")
    assert (diff <= bound).all(), (int(np.argmax(diff - bound)), diff.max())


# ---- pruning on against off -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def counter(ctx):
    import torch
    c = torch.zeros(3, dtype=torch.int64, device=torch.device("cuda", ctx.device))
    ctx.set_wasserstein_counter(c.data_ptr())
    yield c
    ctx.set_wasserstein_counter(None)
    ctx.set_wasserstein_pruning(True)


def _on_off(ctx, counter, arrays, order, ground, **idx):
    """out / status with pruning on and off: identical bytes (NaN payloads included); the counters of the run with pruning
    on.  Every pair of a batch is counted once, also one that ends with a status."""
    import torch
    got = {}
    for prune in (True, False):
        ctx.set_wasserstein_pruning(prune)
        counter.zero_()
        torch.cuda.synchronize()
        out, st = engine.wasserstein_q_batch(*arrays, order=order, ground=ground, ctx=ctx, want_status=True, **idx)
        torch.cuda.synchronize()
        got[prune] = (out, st, counter.cpu().numpy().copy())
    ctx.set_wasserstein_pruning(True)
    on, off = got[True], got[False]
    assert on[0].tobytes() == off[0].tobytes() and on[1].tobytes() == off[1].tobytes(), (order, ground)
    n = len(on[0])
    assert on[2][2] == n and off[2][2] == n and off[2][0] == 0 and off[2][1] == 0, (on[2], off[2])
    return on[0], on[1], on[2]


def _h1(rng, n, b_lo, b_hi, p_lo, p_hi):
    b = rng.uniform(b_lo, b_hi, n)
    return np.stack([b, b + rng.uniform(p_lo, p_hi, n)], 1)


@pytest.mark.parametrize("order,ground", VARIANTS)
def test_pruning_leaves_every_byte(ctx, counter, sized, order, ground):
    rng = np.random.default_rng(47)
    # every batch of the tests above, in every orientation and capacity they run it in
    known = [(a, b) for a, b, want in wq.KNOWN if (order, ground) in want]
    KA, KB = [k[0] for k in known], [k[1] for k in known]
    _on_off(ctx, counter, _pack(KA, 8) + _pack(KB, 8), order, ground)
    _on_off(ctx, counter, _pack(KB, 8) + _pack(KA, 8), order, ground)
    pairs = wq.small_pairs(200, seed=41)
    _on_off(ctx, counter, _pack([p[0] for p in pairs], 4) + _pack([p[1] for p in pairs], 4), order, ground)
    for cap, (A, B) in sized.items():
        _on_off(ctx, counter, _pack(A, cap) + _pack(B, cap), order, ground)
        _on_off(ctx, counter, _pack(B, cap) + _pack(A, cap), order, ground)
    A, B = sized[128]
    _on_off(ctx, counter, _pack(A[:2], 47) + _pack(B[:2], 128), order, ground)
    _on_off(ctx, counter, _pack(B[:2], 128) + _pack(A[:2], 47), order, ground)
    for name, (_, _, arrays, idx) in _hygiene_batches().items():
        _on_off(ctx, counter, arrays, order, ground, **idx)
    out, st, c = _on_off(ctx, counter, _capacity_batch()[2], order, ground)        # the statuses, and the NaNs, as bytes
    assert st.tolist() == [_lib.TDA_WIN_NOT_CONVERGED, _lib.TDA_WIN_NOT_CONVERGED, 0]
    A, B = _equal_birth_pairs()
    out, st, c = _on_off(ctx, counter, _pack(A, 128) + _pack(B, 128), order, ground)
    assert c[1] > 0, c                                             # the workload-shaped pairs lose their dead columns
    _on_off(ctx, counter, _pack(B, 128) + _pack(A, 128), order, ground)
    # equal-birth pairs with persistence ratios within an ulp of the cut, and on either side of the rule's margin
    cut = wq.CUTS[order, ground]
    A, B = [], []
    for p0 in (1.0, 0.7310585786300049):
        for side in (1.0 / cut, cut):
            base = p0 * side
            qs = [np.nextafter(base, -np.inf), base, np.nextafter(base, np.inf)]
            qs += [base * (1.0 + s * r) for r in (1e-12, 5e-10, 9.9e-10, 1.01e-9, 2e-9, 1e-4) for s in (-1.0, 1.0)]
            for q in qs:
                A.append(wq.h0_diagram(0, [p0, p0])); B.append(wq.h0_diagram(0, [q, q, p0]))
                A.append(wq.h0_diagram(0.5, [q] * 3)); B.append(wq.h0_diagram(0.5, [p0]))
    out, st, c = _on_off(ctx, counter, _pack(A, 8) + _pack(B, 8), order, ground)
    _held(out, st, *_refs(A, B, order, ground), order, f"ratios at the cut ({order}, {ground})")
    assert c[1] > 0, c
    # H1-like pairs: far apart (the short cut), one live cell, overlapping
    eeg = lambda n: _h1(rng, n, 1.0, 1.1, 0.05, 0.3)
    aud = lambda n: _h1(rng, n, 0.1, 0.2, 0.005, 0.02)
    far_a, far_b, live_a, live_b, over_a, over_b = [], [], [], [], [], []
    for M, N in [(35, 41), (20, 100), (64, 65), (1, 128), (128, 128), (3, 3)]:
        far_a += [eeg(M), aud(M)]; far_b += [aud(N), eeg(N)]
        a, b = eeg(M), aud(N)
        a[M // 2], b[N // 3] = (0.6, 1.6), (0.61, 1.61)              # one live cell: a long-lived point of each, side by side
        live_a.append(a); live_b.append(b)
        over_a.append(_h1(rng, M, 0.0, 1.0, 0.0, 1.0)); over_b.append(_h1(rng, N, 0.0, 1.0, 0.0, 1.0))
    far_a.append(np.zeros((0, 2))); far_b.append(aud(30))          # {(0, 0)} against short-lived points
    out, st, c = _on_off(ctx, counter, _pack(far_a, 256) + _pack(far_b, 256), order, ground)
    assert c[0] == len(far_a) and c[1] == 0, c                     # every pair took the short cut
    _held(out, st, *_refs(far_a, far_b, order, ground), order, f"far apart ({order}, {ground})")
    out, st, c = _on_off(ctx, counter, _pack(live_a, 256) + _pack(live_b, 256), order, ground)
    assert c[0] == 0 and c[1] == 0, c                              # a live cell: the solver runs as it is
    _held(out, st, *_refs(live_a, live_b, order, ground), order, f"live cells ({order}, {ground})")
    out, st, c = _on_off(ctx, counter, _pack(over_a, 256) + _pack(over_b, 256), order, ground)
    _held(out, st, *_refs(over_a, over_b, order, ground), order, f"overlapping ({order}, {ground})")


# ---- through the step ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def step(ctx):
    """A small Workspace step on synthetic windows with wasserstein_q=(2, "l2") and the bottleneck distance; its diagrams."""
    import torch
    dev = torch.device("cuda", ctx.device)
    n_win, per = 60, 4                                             # 3 groups x 5 bands x 4 windows
    seg_off = np.arange(0, n_win + 1, per, dtype=np.int32)
    eeg = torch.from_numpy(synth.eeg_windows(n_win, seed=3, windows_per_recording=per)).to(dev)
    aud = torch.from_numpy(synth.audio_windows_all_bands(n_win // 5, seed=4)[0]).to(dev)
    plain = pipeline.Workspace(n_win, seg_off, dev)
    want = pipeline.run_step(eeg, aud, plain, ctx=ctx).cpu().numpy().copy()
    ws = pipeline.Workspace(n_win, seg_off, dev, bottleneck=True, wasserstein_q=(2, "l2"))
    got = pipeline.run_step(eeg, aud, ws, ctx=ctx).cpu().numpy().copy()
    torch.cuda.synchronize()
    return dict(ws=ws, want=want, got=got, eeg=eeg, aud=aud, seg_off=seg_off, n_win=n_win, per=per)


def test_run_step_with_wasserstein_q(ctx, step):
    ws, seg_off, n_win, per = step["ws"], step["seg_off"], step["n_win"], step["per"]
    assert step["got"].tobytes() == step["want"].tobytes()         # the rows are what they are without the option
    e0, e1 = ws.eeg.to_lists()
    a0, a1 = ws.aud.to_lists()
    q0, q1 = ws.q0.cpu().numpy(), ws.q1.cpu().numpy()
    _held(q0, ws.qs0.cpu().numpy(), *_refs(e0, a0, 2, "l2"), 2, "step H0 pairs (2, l2)")
    _held(q1, ws.qs1.cpu().numpy(), *_refs(e1, a1, 2, "l2"), 2, "step H1 pairs (2, l2)")
    keep = (ws.aud.status.cpu().numpy() & (_lib.TDA_WIN_DEGENERATE | _lib.TDA_WIN_TOO_LARGE)) == 0
    wqm = ws.wq.cpu().numpy()
    assert wqm.shape == (n_win // per, 2)
    for g in range(n_win // per):
        sl = slice(seg_off[g], seg_off[g + 1])
        assert wqm[g, 0] == np.nanmean(q0[sl][keep[sl]]) and wqm[g, 1] == np.nanmean(q1[sl][keep[sl]])
    # a view over the first groups computes the same values
    v = ws.view(seg_off[:7])
    pipeline.run_step(step["eeg"][:24], step["aud"][:24], v, ctx=ctx)
    assert np.array_equal(v.wq.cpu().numpy(), wqm[:6]) and v.q0.shape[0] == 24


def test_ordering_chain_and_counters_on_the_step(ctx, step, counter):
    """Per pair of the step: bottleneck <= W2(linf) <= W1(linf) <= W1(l2) and W2(l2) <= W1(l2), each with 1e-9 of slack;
    pruning on and off give the same bytes on these diagrams, with the short cut taken on H1 pairs and columns trimmed on
    H0 pairs."""
    import torch
    ws = step["ws"]
    legs = {"h0": (ws.eeg.h0, ws.eeg.c0, ws.aud.h0, ws.aud.c0, ws.b0), "h1": (ws.eeg.h1, ws.eeg.c1, ws.aud.h1, ws.aud.c1, ws.b1)}
    for name, (ra, ca, rb, cb, bott) in legs.items():
        arrays = [t.cpu().numpy() for t in (ra, ca, rb, cb)]
        w = {}
        for order, ground in VARIANTS:
            out, st, c = _on_off(ctx, counter, arrays, order, ground)
            assert (st == 0).all()
            w[order, ground] = out
            print(f"step {name} ({order}, {ground}): counters {c.tolist()}")
            assert (c[0] > 0) if name == "h1" else (c[1] > 0), (name, order, ground, c)
            dev_out, dev_st = engine.wasserstein_q_dev(ra, ca, rb, cb, order=order, ground=ground, ctx=ctx)
            torch.cuda.synchronize()
            assert dev_out.cpu().numpy().tobytes() == out.tobytes() and (dev_st.cpu().numpy() == 0).all()
        b = bott.cpu().numpy()
        eps = 1e-9
        assert (b <= w[2, "linf"] + eps).all() and (w[2, "linf"] <= w[1, "linf"] + eps).all()
        assert (w[1, "linf"] <= w[1, "l2"] + eps).all() and (w[2, "l2"] <= w[1, "l2"] + eps).all()


def test_safe_wasserstein_q_immediate_and_batched(ctx):
    rng = np.random.default_rng(48)
    pairs = [(wq.random_diagram(rng, int(m)), wq.random_diagram(rng, int(n))) for m, n in rng.integers(0, 50, (8, 2))]
    pairs[2] = (np.array([[0.0, np.inf], [0.125, 0.5]]), pairs[2][1])
    pairs[4] = (np.zeros(3), pairs[4][1])                          # not 2-D: the empty diagram
    bad = 5
    pairs[bad] = (np.zeros((4, 3)), pairs[bad][1])                 # malformed: three columns
    good = [k for k in range(8) if k != bad]
    for order, ground in VARIANTS:
        now = np.array([utils.safe_wasserstein_q(a, b, order, ground) for a, b in pairs])
        assert np.isnan(now[bad])
        A, B = [wq.clean(pairs[k][0]) for k in good], [wq.clean(pairs[k][1]) for k in good]
        _held(now[good], np.zeros(7, int), *_refs(A, B, order, ground), order, f"safe_wasserstein_q ({order}, {ground})")
        with utils.batch():
            later = [utils.safe_wasserstein_q(a, b, order=order, ground=ground) for a, b in pairs]
            other = utils.safe_wasserstein_q(*pairs[0], order=3 - order, ground=ground)
            w = utils.safe_wasserstein(*pairs[0])
        assert all(isinstance(x, utils.DeferredScalar) for x in later)
        vals = np.array([float(x) for x in later])
        assert np.isnan(vals[bad]) and vals[good].tobytes() == now[good].tobytes()
        assert float(other) == utils.safe_wasserstein_q(*pairs[0], order=3 - order, ground=ground)
        assert float(w) == utils.safe_wasserstein(*pairs[0])
    assert utils.safe_wasserstein_q(*pairs[0]) == utils.safe_wasserstein_q(*pairs[0], order=2, ground="l2")
