"""
The launch schemes of the finishing pass and of the Wasserstein launches (tda_set_launch_scheme) against each other, in
one process on the same buffers: the packed finishing kernel (eight lanes per diagram) and the list-driven second
launches must give what the one-wave-per-diagram kernel and the launches over the whole batch give, bit for bit.

Bars: rows and features of the schemes identical as raw bytes (NaNs compared as bits); mean / std / sum / max of the
default scheme bit-equal to np.mean / np.std / np.sum / np.max on the same rows, the entropy (OCML's log) within 1e-12
relative; Wasserstein outputs and status words of the schemes identical.
"""
import numpy as np
import pytest

from tda_eeg_audio_amd import engine

pytestmark = pytest.mark.gpu

LARGE_K = (65, 66, 72, 100, 128, 129, 200, 255, 256, 300)
KINDS = ("random", "ties", "some_inf", "all_inf", "one_finite", "zero_persistence", "some_pn_zero")


def _diagram(kind, k, rng):
    """k rows in emission order (any order): births on a coarse grid where ties are wanted."""
    if kind == "ties":
        b = rng.integers(0, 4, k) / 4.0                          # equal births ...
        d = b + rng.integers(1, 4, k) / 8.0                      # ... with equal and with unequal deaths
    else:
        b = rng.random(k)
        d = b + rng.random(k)
    if kind == "some_inf":
        d[rng.random(k) < 0.3] = np.inf
    elif kind == "all_inf":
        d[:] = np.inf                                            # m = 0
    elif kind == "one_finite" and k:
        keep = int(rng.integers(0, k))
        d[np.arange(k) != keep] = np.inf                         # m = 1
    elif kind == "zero_persistence":
        d = b.copy()                                             # total persistence 0: the tot > 0 guard
    elif kind == "some_pn_zero":
        z = rng.random(k) < 0.5
        d[z] = b[z]                                              # pn == 0 for these rows
    return np.stack([b, d], 1).reshape(-1, 2)


def _diagram_set(cap, seed):
    """Every row count 0..64 and counts in 65..300 for every kind; 525 diagrams: not a multiple of 8, so the last wave of
    a set of the packed kernel has idle groups.  A count above the capacity is clamped by the kernels."""
    rng = np.random.default_rng(seed)
    ks = [(kind, k) for kind in KINDS for k in list(range(65)) + list(LARGE_K)]
    order = rng.permutation(len(ks))                             # large and small diagrams share waves
    rows = np.zeros((len(ks), cap, 2))
    cnt = np.zeros(len(ks), np.int32)
    for at, i in enumerate(order):
        kind, k = ks[i]
        kk = min(k, cap)
        rows[at, :kk] = _diagram(kind, kk, rng)
        cnt[at] = k
    assert len(ks) % 8 != 0
    return rows, cnt


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _run(ctx, scheme, host_sets, torch, dev):
    """The finishing pass under `scheme` on fresh copies of the sets -> [(rows, feat or None)] on the host."""
    ctx.set_launch_scheme(scheme)
    try:
        sets = []
        for rows, cnt, order, want_feat in host_sets:
            rows_t = torch.from_numpy(rows).to(dev)
            cnt_t = torch.from_numpy(cnt).to(dev)
            feat_t = torch.full((rows.shape[0], 11), -7.0, dtype=torch.float64, device=dev) if want_feat else None
            sets.append((rows_t, cnt_t, order, feat_t))
        engine.diagram_finish_dev(sets, ctx=ctx)
        torch.cuda.synchronize()
    finally:
        ctx.set_launch_scheme(ctx.SCHEME_LISTS)
    return [(r.cpu().numpy(), None if f is None else f.cpu().numpy()) for r, _, _, f in sets]


def _ripser_order(d):
    """Descending birth; ties: descending death, then emission order."""
    idx = sorted(range(len(d)), key=lambda i: (-d[i, 0], -d[i, 1], i))
    return d[idx]


def _numpy_features(d):
    """extract_features (scripts/utils.py:144-177) with numpy, on rows in the order given."""
    out = np.zeros(11)
    fin = np.isfinite(d).all(axis=1)
    f = d[fin]
    out[1] = len(d) - len(f)
    if len(f) == 0:
        return out
    p = f[:, 1] - f[:, 0]
    out[0] = len(f)
    out[2], out[3] = np.mean(f[:, 0]), np.std(f[:, 0])
    out[4], out[5] = np.mean(f[:, 1]), np.std(f[:, 1])
    out[6], out[7] = np.mean(p), np.std(p)
    out[8], out[9] = np.max(p), np.sum(p)
    if len(f) > 1 and out[9] > 0:
        pn = p / out[9]
        pn = pn[pn > 0]
        out[10] = -np.sum(pn * np.log(pn + 1e-10)) / np.log(len(f) + 1e-10)
    return out


def _host_sets(n_sets):
    # the sets of a step: EEG H0 (47 rows, emission order kept), EEG H1 and audio H1 (256 rows, ripser's order); a fourth
    # set that is only put in order
    specs = [(47, False, True), (256, True, True), (256, True, True), (64, True, False)][:n_sets]
    return [(*_diagram_set(cap, 100 + i), order, feat) for i, (cap, order, feat) in enumerate(specs)]


@pytest.mark.parametrize("n_sets", [3, 4])
def test_packed_finish_identical_to_wave_per_diagram(ctx, n_sets):
    import torch
    dev = torch.device("cuda", 0)
    host_sets = _host_sets(n_sets)
    new = _run(ctx, ctx.SCHEME_LISTS, host_sets, torch, dev)
    for scheme in (ctx.SCHEME_GRID, ctx.SCHEME_ONE):
        old = _run(ctx, scheme, host_sets, torch, dev)
        for s, ((r_new, f_new), (r_old, f_old)) in enumerate(zip(new, old)):
            assert np.array_equal(_bits(r_new), _bits(r_old)), (scheme, s)
            if f_new is not None:
                bad = np.nonzero((_bits(f_new) != _bits(f_old)).any(axis=1))[0]
                assert bad.size == 0, (scheme, s, bad[:8], host_sets[s][1][bad[:8]], f_new[bad[:1]], f_old[bad[:1]])
    # a second call on the same stream finds its list empty again: same bytes
    again = _run(ctx, ctx.SCHEME_LISTS, host_sets, torch, dev)
    for (r_new, f_new), (r2, f2) in zip(new, again):
        assert np.array_equal(_bits(r_new), _bits(r2))
        assert f_new is None or np.array_equal(_bits(f_new), _bits(f2))


def test_packed_finish_against_numpy(ctx):
    import torch
    dev = torch.device("cuda", 0)
    host_sets = _host_sets(4)
    got = _run(ctx, ctx.SCHEME_LISTS, host_sets, torch, dev)
    for s, ((rows_in, cnt, order, want_feat), (rows, feat)) in enumerate(zip(host_sets, got)):
        cap = rows_in.shape[1]
        for i in range(rows_in.shape[0]):
            k = min(int(cnt[i]), cap)
            want = _ripser_order(rows_in[i, :k]) if order else rows_in[i, :k]
            assert np.array_equal(_bits(rows[i, :k]), _bits(want)), (s, i, k)
            assert np.array_equal(_bits(rows[i, k:]), _bits(rows_in[i, k:])), (s, i, k)
            if not want_feat:
                continue
            ref = _numpy_features(want)
            assert np.array_equal(feat[i, :10], ref[:10]), (s, i, k, feat[i], ref)      # counts, mean, std, max, sum: bit-equal
            assert np.isclose(feat[i, 10], ref[10], rtol=1e-12, atol=0), (s, i, k, feat[i, 10], ref[10])


def test_wasserstein_list_launch_identical(ctx):
    """Pairs on both sides of the 64 x 64 limit in one batch (as test_wasserstein_vs_persim_restatement_and_bruteforce),
    many times over so that the list-driven launch has more entries than workgroups; twice on one stream and once on a
    second one: a list left uncleared would show as a pair solved twice or not at all."""
    import torch
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(8)
    sizes = [(0, 0), (1, 64), (64, 64), (65, 3), (64, 65), (100, 100), (3, 250), (200, 130), (40, 41), (63, 64)] * 61
    As = [np.sort(rng.random((m, 2)), axis=1) for m, _ in sizes]
    Bs = [np.sort(rng.random((n, 2)), axis=1) for _, n in sizes]
    ra, ca = engine.pack_diagrams(As, cap=256); rb, cb = engine.pack_diagrams(Bs, cap=256)
    ca[7] = 300; cb[7] = 400                                     # counts above the capacity are clamped
    t = [torch.from_numpy(x).to(dev) for x in (ra, ca, rb, cb)]

    def run(scheme):
        ctx.set_launch_scheme(scheme)
        try:
            out = torch.full((len(sizes),), -7.0, dtype=torch.float64, device=dev)
            st = torch.full((len(sizes),), -7, dtype=torch.int32, device=dev)
            engine.wasserstein_dev(t[0], t[1], t[2], t[3], out_t=out, status_t=st, ctx=ctx)
            torch.cuda.current_stream().synchronize()
        finally:
            ctx.set_launch_scheme(ctx.SCHEME_LISTS)
        return out.cpu().numpy(), st.cpu().numpy()

    ref_out, ref_st = run(ctx.SCHEME_ONE)
    assert not ref_st.any()
    results = [run(ctx.SCHEME_GRID), run(ctx.SCHEME_LISTS), run(ctx.SCHEME_LISTS)]
    torch.cuda.synchronize()
    with torch.cuda.stream(torch.cuda.Stream(device=dev)):
        results.append(run(ctx.SCHEME_LISTS))
    results.append(run(ctx.SCHEME_LISTS))
    for n, (out, st) in enumerate(results):
        assert np.array_equal(_bits(out), _bits(ref_out)), (n, np.nonzero(_bits(out) != _bits(ref_out))[0][:8])
        assert np.array_equal(st, ref_st), n
