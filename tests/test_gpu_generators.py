"""
GPU tests of the generators and representative cycles (csrc/generators.hip; include/tdaeeg.h, "Generators and
representative cycles"): every output as bytes against the definition in tests/generators_ref.py ((b), `generators`), fed
with the keys of the oracle and the rows the Rips kernels themselves wrote.  The shapes are the smallest that can break
the kernel: the mask word boundary (63, 64, 65, 127, 128), the one- and two-word templates, fewer and more runs than waves,
tied births and deaths, every capacity below its demand, the three input forms with their status words (clouds of dimension
1 to 4, three Takens embeddings: the key pass is the one the Euler kernels share), batches, means and the refusals.
"""
import ctypes as C

import numpy as np
import pytest

import euler_ref as er
import generators_ref as gr

pytestmark = pytest.mark.gpu

SENT = -7
NAMES = ("h1_gen", "h1_flag", "cyc", "cyc_len", "part", "h0_edge")


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda", 0))


def _sym_random(n_win, n, seed, hi=2.2):
    rng = np.random.default_rng(seed)
    d = rng.random((n_win, n, n)) * hi
    return (d + d.transpose(0, 2, 1)) / 2


def _circles(n_win, n, seed):
    """Distance matrices of noisy double circles: few H1 rows, long cycles, many search levels."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n_win):
        th = rng.random(n) * 2 * np.pi
        pc = np.stack([np.cos(th), np.sin(th)], 1) * (0.35 + 0.25 * (np.arange(n) % 2)[:, None])
        pc += rng.standard_normal(pc.shape) * 0.02
        out.append(np.sqrt(((pc[:, None] - pc[None]) ** 2).sum(-1)))
    return np.stack(out)


def _quantised(n_win, n, seed, steps):
    d = _sym_random(n_win, n, seed, 1.8) + 0.1
    return np.round(d * steps) / steps


def _rows(dgm):
    return [t.cpu().numpy() for t in (dgm.h0, dgm.c0, dgm.h1, dgm.c1)]


def _ref_windows(keys_list, h0, c0, h1, c1, thresh=2.0, cyc_cap=128, part_ld=None, ref=gr.generators):
    out = [ref(k, h0[w], c0[w], h1[w], c1[w], thresh, cyc_cap, part_ld) for w, k in enumerate(keys_list)]
    return {name: np.stack([o[name] for o in out]) for name in NAMES}


def _same(got, ref, names=NAMES, where=""):
    for name in names:
        g = got[name]
        assert g.dtype == ref[name].dtype and g.shape == ref[name].shape, (where, name, g.dtype, g.shape, ref[name].shape)
        assert g.tobytes() == ref[name].tobytes(), (where, name, np.argwhere(g != ref[name])[:5])


def _dm_case(ctx, dms, thresh=2.0, cyc_cap=128, h1_cap=256, symmetrise=True):
    """Rips on the device, the generators on its DeviceDiagrams, the reference on the same rows."""
    from tda_eeg_audio_amd import engine
    dm_t = _dev(dms)
    dgm = engine.rips_dm_dev(dm_t, thresh=thresh, symmetrise=symmetrise, h1_cap=h1_cap, ctx=ctx)
    out = engine.generators_dm_dev(dm_t, dgm, thresh, symmetrise, cyc_cap, ctx=ctx).to_host()
    h0, c0, h1, c1 = _rows(dgm)
    ref = _ref_windows([er.keys_dm(d, symmetrise) for d in dms], h0, c0, h1, c1, thresh, cyc_cap)
    _same(out, ref)
    assert not out["status"].any()
    return out, (h0, c0, h1, c1), dgm


# (n, windows, kind)
DM_CASES = [(3, 2, "random"), (4, 3, "random"), (5, 3, "random"), (47, 2, "random"), (47, 2, "circles"), (63, 1, "circles"),
            (64, 2, "circles"), (65, 1, "circles"), (127, 1, "circles"), (128, 1, "circles"), (70, 1, "random")]


@pytest.mark.parametrize("n,n_win,kind", DM_CASES)
def test_distance_matrices(ctx, n, n_win, kind):
    dms = _sym_random(n_win, n, 1000 + n) if kind == "random" else _circles(n_win, n, 2000 + n)
    out, (h0, c0, h1, c1), _ = _dm_case(ctx, dms, h1_cap=2048 if kind == "random" else 256)
    assert (c1 <= h1.shape[1]).all()
    rows = int(c1.sum())
    if n >= 47:
        assert rows > 4 and not out["h1_flag"].any()               # more runs than waves, generic: nothing flagged
        assert out["cyc_len"].max() >= (6 if kind == "circles" else 4) and out["part"].max() > 0
        assert (out["h0_edge"][:, :n - 1] >= 0).all()
    if n >= 65:
        assert out["h0_edge"].max() == n - 1                       # the second mask word is in use
    if n >= 127:
        assert out["cyc"].max() >= 64 and out["h1_gen"][..., 1].max() >= 64
    # the mask route gives the same bytes where it is cheap enough to run
    if n <= 47:
        _same(out, _ref_windows([er.keys_dm(d) for d in dms], h0, c0, h1, c1, ref=gr.generators_masks))


def test_known_answers(ctx):
    sq = np.array([[0, 0], [1, 0], [1, 1], [0, 1]], float)
    d = np.sqrt(((sq[:, None] - sq[None]) ** 2).sum(-1))
    out, (h0, c0, h1, c1), _ = _dm_case(ctx, d[None])
    assert c1.tolist() == [1] and out["h1_gen"][0, 0].tolist() == [3, 2, 2, 0] and out["cyc"][0, 0, :4].tolist() == [3, 0, 1, 2]
    assert out["h1_flag"][0, 0] == gr.DEATH_TIED and out["h0_edge"][0].tolist() == [[1, 0], [2, 1], [3, 0], [-1, -1]]
    # a constant matrix: no H1 row, a star forest, and only n - 1 searches however many keys tie
    from tda_eeg_audio_amd import engine
    n = 40
    dm_t = _dev(np.full((1, n, n), 0.75))
    dgm = engine.rips_dm_dev(dm_t, ctx=ctx)
    g = engine.generators_dm_dev(dm_t, dgm, work=True, ctx=ctx).to_host()
    assert dgm.c1.cpu().numpy().tolist() == [0]
    assert g["h0_edge"][0, :n - 1].tolist() == [[v, 0] for v in range(1, n)] and (g["h0_edge"][0, n - 1:] == -1).all()
    assert g["work"][0, :, 0].sum() == n - 1 and not g["part"].any()


@pytest.mark.parametrize("n,steps", [(13, 5), (20, 8), (30, 12), (66, 40)])
def test_tied_births_and_deaths(ctx, n, steps):
    dms = _quantised(3, n, 300 + n, steps)
    out, (h0, c0, h1, c1), _ = _dm_case(ctx, dms, h1_cap=1024)
    R = int(c1[0])
    births, deaths = h1[0, :R, 0], h1[0, :R, 1]
    assert len(set(births.tolist())) < R and len(set(deaths.tolist())) < R       # runs of equal births, of equal deaths
    seen = int(np.bitwise_or.reduce(out["h1_flag"].ravel()))
    assert seen & gr.BIRTH_TIED and seen & gr.DEATH_TIED and not seen & gr.NO_EDGE
    assert (out["h0_edge"][0, :int(np.isfinite(h0[0, :c0[0], 1]).sum())] >= 0).all()


def test_capacities_below_demand(ctx):
    from tda_eeg_audio_amd import engine
    dms = _circles(2, 47, 77)
    full, (h0, c0, h1, c1), _ = _dm_case(ctx, dms)
    assert full["cyc_len"].max() > 6
    # cyc_cap smaller than a cycle: flag, true length, prefix; the flagged rows leave the participation
    small, _, _ = _dm_case(ctx, dms, cyc_cap=5)
    long = full["cyc_len"] > 5
    assert long.any() and ((small["h1_flag"] & gr.CYCLE_TRUNCATED) != 0).tolist() == long.tolist()
    assert small["cyc_len"].tobytes() == full["cyc_len"].tobytes() and small["cyc"].tobytes() == full["cyc"][..., :5].tobytes()
    assert small["part"].sum() < full["part"].sum()
    # h1_cap smaller than the count: the rows the Rips kernel kept
    cut = int(c1.min()) - 2
    out, (_, _, h1c, c1c), dgm = _dm_case(ctx, dms, h1_cap=cut)
    assert (c1c > cut).all() and (dgm.status.cpu().numpy() & 1).all() and out["h1_gen"].shape == (2, cut, 4)
    # fewer rows than the buffers hold: the fill values above the counts
    R = int(c1[0])
    assert (full["h1_gen"][0, R:] == -1).all() and (full["cyc"][0, R:] == -1).all() and not full["cyc_len"][0, R:].any()
    assert not full["h1_flag"][0, R:].any()
    assert engine.generators_args(np.int64(4)) == 4


def test_small_threshold_gives_essential_rows(ctx):
    dms = _circles(2, 30, 88)
    full, (_, _, h1, c1), _ = _dm_case(ctx, dms)
    rows = h1[0, :c1[0]]
    loop = rows[np.argmax(rows[:, 1] - rows[:, 0])]
    thresh = float(loop.mean())
    out, (h0, c0, h1t, c1t), _ = _dm_case(ctx, dms, thresh=thresh)
    ess = np.isinf(h1t[0, :c1t[0], 1])
    assert ess.any() and (out["h1_gen"][0, :c1t[0]][ess, 2:] == -1).all() and (out["h1_gen"][0, :c1t[0]][ess, :2] >= 0).all()
    assert not out["h1_flag"][0, :c1t[0]][ess].any()
    assert np.isinf(h0[0, :c0[0], 1]).sum() >= 1 and (out["h0_edge"][0, c0[0] - 1] == -1).all()
    # symmetrise = 0 on a matrix that is not symmetric
    raw = np.random.default_rng(5).random((2, 21, 21)) * 2.4 - 0.4
    _dm_case(ctx, raw, symmetrise=False, h1_cap=512)
    _dm_case(ctx, raw, symmetrise=True, h1_cap=512)


def test_foreign_diagram_and_skipped_windows(ctx):
    import torch
    from tda_eeg_audio_amd import engine
    dms = _circles(3, 24, 99)
    dm_t = _dev(dms)
    dgm = engine.rips_dm_dev(dm_t, ctx=ctx)
    h0, c0, h1, c1 = _rows(dgm)
    # the rows of the next window: nothing matches
    rolled = (dgm.h0.roll(1, 0).contiguous(), dgm.c0.roll(1, 0).contiguous(), dgm.h1.roll(1, 0).contiguous(),
              dgm.c1.roll(1, 0).contiguous())
    out = engine.generators_dm_dev(dm_t, rolled, ctx=ctx).to_host()
    rh0, rc0, rh1, rc1 = (np.roll(x, 1, 0) for x in (h0, c0, h1, c1))
    _same(out, _ref_windows([er.keys_dm(d) for d in dms], rh0, rc0, rh1, rc1))
    for w in range(3):
        assert (out["h1_flag"][w, :rc1[w]] & gr.NO_EDGE).all()
    assert (out["h1_gen"] == -1).all() and (out["cyc"] == -1).all() and not out["part"].any() and (out["h0_edge"] == -1).all()
    # a skipped window gets the fill values only; the others are what they are alone
    rs = _dev(np.array([0, 2, 1], np.int32))
    sk = engine.generators_dm_dev(dm_t, dgm, rips_status=rs, skip_mask=2, ctx=ctx).to_host()
    ref = _ref_windows([er.keys_dm(d) for d in dms], h0, c0, h1, c1)
    fill = gr.fill(h1.shape[1], h0.shape[1], 128, 24)
    for name in NAMES:
        ref[name][1] = fill[name]
    _same(sk, ref)
    assert not sk["status"].any()
    # h0_edge off, by the switch and by rows without H0: the other outputs do not move
    for dg, kw in ((dgm, dict(h0_edge=False)), ((None, None, dgm.h1, dgm.c1), {})):
        o = engine.generators_dm_dev(dm_t, dg, **kw, ctx=ctx)
        assert o.h0_edge is None
        _same(o.to_host(), _ref_windows([er.keys_dm(d) for d in dms], h0, c0, h1, c1), NAMES[:5])
    o = engine.generators_dm_dev(dm_t, dgm, part=False, ctx=ctx)
    assert o.part is None
    _same(o.to_host(), _ref_windows([er.keys_dm(d) for d in dms], h0, c0, h1, c1),
          ("h1_gen", "h1_flag", "cyc", "cyc_len", "h0_edge"))
    # without the cycle buffer: the edges, lengths and flags as with it (cyc_cap still decides the truncation flag)
    bare = engine.DeviceGenerators(3, h0.shape[1], h1.shape[1], 5, 24, dm_t.device, part=False, cyc=False)
    engine.generators_dm_dev(dm_t, dgm, cyc_cap=5, out=bare, ctx=ctx)
    assert bare.cyc is None
    _same(bare.to_host(), _ref_windows([er.keys_dm(d) for d in dms], h0, c0, h1, c1, cyc_cap=5),
          ("h1_gen", "h1_flag", "cyc_len", "h0_edge"))
    torch.cuda.synchronize()


# ---------------------------------------------------------------- cloud forms
CLOUD_P = [2, 3, 64, 65, 128, 129]


def _clouds(dim, seed, p_cap=129):
    rng = np.random.default_rng(seed)
    pc = rng.random((len(CLOUD_P) + 1, p_cap, dim)) * 3.0 - 1.0
    n_pts = np.array(CLOUD_P + [40], np.int32)
    pc[-1, :, 0] = 0.25                                           # a constant column: range 0 -> 1
    return pc, n_pts


def _ref_clouds(pc, n_pts, h0, c0, h1, c1, normalise, cyc_cap=128):
    p_cap = pc.shape[1]
    out, st = [], []
    for w, P in enumerate(n_pts):
        if P > min(p_cap, 128) or P < 3:
            out.append(gr.fill(h1.shape[1], h0.shape[1], cyc_cap, p_cap))
            st.append(16 if P > min(p_cap, 128) else 4)
        else:
            out.append(gr.generators(er.keys_cloud(pc[w, :P], normalise), h0[w], c0[w], h1[w], c1[w], 2.0, cyc_cap, p_cap))
            st.append(0)
    return {name: np.stack([o[name] for o in out]) for name in NAMES}, st


@pytest.mark.parametrize("dim,normalise", [(2, True), (3, False), (1, True), (4, True)])
def test_clouds(ctx, dim, normalise):
    from tda_eeg_audio_amd import engine
    pc, n_pts = _clouds(dim, 20 + dim)
    h0, c0, h1, c1, rst = engine.cloud_rips_batch(pc, n_pts, normalise, h1_cap=512, ctx=ctx, raw=True)
    assert rst.tolist() == [4, 0, 0, 0, 0, 16, 0]
    dgm = (_dev(h0), _dev(c0), _dev(h1), _dev(c1))
    out = engine.generators_cloud_dev(_dev(pc), _dev(n_pts), dgm, normalise, ctx=ctx).to_host()
    ref, st = _ref_clouds(pc, n_pts, h0, c0, h1, c1, normalise)
    _same(out, ref)
    assert out["status"].tolist() == st == [4, 0, 0, 0, 0, 16, 0]
    assert out["part"].shape == (7, 129) and not out["part"][4, 128:].any() and (out["h1_gen"][[0, 5]] == -1).all()
    if dim > 1:
        assert out["part"][4].max() > 0 and out["cyc"][4].max() >= 64
    else:                                                         # points of a line: a path of 127 forest edges
        assert out["h0_edge"][4].max() == 127 and (out["h0_edge"][4, :127] >= 0).all()
    # the host twin
    host = engine.generators_cloud_batch(pc, h0, c0, h1, c1, n_pts, normalise, ctx=ctx)
    _same(host, ref)
    assert host["status"].tolist() == st
    # the one-word template on the same clouds: p_cap = 64
    sub, n_sub = np.ascontiguousarray(pc[[1, 2, 6], :64]), np.array([3, 64, 40], np.int32)
    rows = tuple(_dev(x[[1, 2, 6]]) for x in (h0, c0, h1, c1))
    o64 = engine.generators_cloud_dev(_dev(sub), _dev(n_sub), rows, normalise, ctx=ctx).to_host()
    for name in NAMES:
        want = ref[name][[1, 2, 6]]
        assert o64[name].tobytes() == (want[:, :64] if name == "part" else want).tobytes(), name
    assert not o64["status"].any()


def test_takens_windows(ctx):
    import torch
    from tda_eeg_audio_amd import engine, synth
    taus = np.array([102, 2, 0, 125, 124, 40, -3], np.int32)        # P = 23, 123, refused, 0, 1, 85, refused
    sig = synth.audio_windows(len(taus), "alpha", seed=3)
    sig_t, tau_t = _dev(sig), _dev(taus)
    dgm = engine.takens_rips_dev(sig_t, tau_t, h1_cap=512, ctx=ctx)
    npts_t = torch.full((len(taus),), SENT, dtype=torch.int32, device="cuda:0")
    out = engine.generators_takens_dev(sig_t, tau_t, dgm, n_points_t=npts_t, ctx=ctx).to_host()
    h0, c0, h1, c1 = _rows(dgm)
    ref = []
    for w, tau in enumerate(taus):
        P = er.takens_points(sig.shape[1], int(tau), 3, 2)
        if tau < 1 or P > 128 or P < 3:
            ref.append(gr.fill(512, 128, 128, 128))
        else:
            ref.append(gr.generators(er.keys_takens(sig[w], tau), h0[w], c0[w], h1[w], c1[w], 2.0, 128, 128))
    _same(out, {name: np.stack([o[name] for o in ref]) for name in NAMES})
    assert out["status"].tolist() == [0, 0, 16, 4, 4, 0, 16] == dgm.status.cpu().numpy().tolist()
    npts = npts_t.cpu().numpy()
    assert npts[:2].tolist() == [23, 123] and npts[3:6].tolist() == [0, 1, 85]
    assert c1[1] > 4 and not out["h1_flag"][1].any() and out["part"][1].max() > 0
    # other embeddings: dim 4 with subsample 3 (P = 83) and dim 2 with subsample 2 (P = 122)
    for dim, sub, tau in ((4, 3, 1), (2, 2, 7)):
        t = _dev(np.full(2, tau, np.int32))
        d2 = engine.takens_rips_dev(sig_t[:2].contiguous(), t, dim=dim, subsample=sub, h1_cap=512, ctx=ctx)
        o2 = engine.generators_takens_dev(sig_t[:2].contiguous(), t, d2, dim=dim, subsample=sub, ctx=ctx).to_host()
        r0, q0, r1, q1 = _rows(d2)
        ref2 = [gr.generators(er.keys_takens(sig[w], tau, dim, sub), r0[w], q0[w], r1[w], q1[w], 2.0, 128, 128) for w in range(2)]
        _same(o2, {name: np.stack([o[name] for o in ref2]) for name in NAMES}, where=(dim, sub, tau))
        assert not o2["status"].any() and q1.min() > 0
    # the host twin
    host = engine.generators_takens_batch(sig, taus, h0, c0, h1, c1, ctx=ctx)
    _same(host, out)
    assert host["status"].tolist() == out["status"].tolist() and host["n_points"][:2].tolist() == [23, 123]
    # ... with n_points = NULL
    o, rows, outs = engine._gen_host(len(taus), 128, h0, c0, h1, c1, 128, None, True, True, False)
    w = engine.f64(sig)
    ctx.check(ctx.lib.tda_generators_takens_batch(ctx.h, engine.ptr(w), engine.ptr(taus), len(taus), sig.shape[1], 3, 2, 2.0,
                                                  *rows, 0, *outs, None, engine.ptr(o["status"])))
    _same(o, out, names=NAMES + ("status",))


# ---------------------------------------------------------------- batches, host forms, means
def test_batch_behaviour(ctx):
    import torch
    from tda_eeg_audio_amd import engine
    dms = np.concatenate([_circles(20, 47, 40), _sym_random(4, 47, 41)])
    dm_t = _dev(dms)
    dgm = engine.rips_dm_dev(dm_t, h1_cap=512, ctx=ctx)
    # oversized outputs: the tail is not touched
    big = engine.DeviceGenerators(27, 47, 512, 16, 47, dm_t.device)
    for t in (big.h1_gen, big.h1_flag, big.cyc, big.cyc_len, big.status, big.part, big.h0_edge):
        t.fill_(SENT)
    engine.generators_dm_dev(dm_t, dgm, cyc_cap=16, out=big, ctx=ctx)
    out = big.to_host()
    for name in NAMES + ("status",):
        assert (out[name][24:] == SENT).all(), name
    assert not out["status"][:24].any()
    h0, c0, h1, c1 = _rows(dgm)
    pick = [0, 19, 23]
    ref = _ref_windows([er.keys_dm(dms[w]) for w in pick], h0[pick], c0[pick], h1[pick], c1[pick], cyc_cap=16)
    _same({k: v[pick] for k, v in out.items()}, ref)
    # a window alone and inside the batch
    for w in pick:
        one = tuple(t[w:w + 1].contiguous() for t in (dgm.h0, dgm.c0, dgm.h1, dgm.c1))
        alone = engine.generators_dm_dev(dm_t[w:w + 1].contiguous(), one, cyc_cap=16, ctx=ctx).to_host()
        for name in NAMES:
            assert alone[name][0].tobytes() == out[name][w].tobytes(), (w, name)
    # the host twin, from the raw rows of the host Rips call
    rh0, rc0, rh1, rc1, _ = engine.rips_dm_batch(dms, h1_cap=512, ctx=ctx, raw=True)
    host = engine.generators_dm_batch(dms, rh0, rc0, rh1, rc1, cyc_cap=16, ctx=ctx)
    _same(host, {k: v[:24] for k, v in out.items()})
    # ... its other branches: no H0 rows, the Rips status words, no part, no h0_edge, the work counters
    lean = dict(cyc_cap=16, part=False, h0_edge=False, work=True, ctx=ctx)
    lean_d = engine.generators_dm_dev(dm_t, (None, None, dgm.h1, dgm.c1), rips_status=dgm.status, **lean).to_host()
    lean_h = engine.generators_dm_batch(dms, None, None, rh1, rc1, rips_status=dgm.status.cpu().numpy(), **lean)
    assert sorted(lean_h) == sorted(lean_d) == ["cyc", "cyc_len", "h1_flag", "h1_gen", "status", "work"]
    _same(lean_h, lean_d, names=sorted(lean_d))
    # ... and cyc = NULL: edges, flags and lengths only
    o, rows, outs = engine._gen_host(24, 47, rh0, rc0, rh1, rc1, 16, None, False, True, False)
    d = engine.f64(dms)
    ctx.check(ctx.lib.tda_generators_dm_batch(ctx.h, engine.ptr(d), 24, 47, 2.0, 1, *rows, 0, *outs[:3], None, *outs[4:],
                                              engine.ptr(o["status"])))
    bare = engine.DeviceGenerators(24, 47, 512, 16, 47, dm_t.device, part=False, cyc=False)
    engine.generators_dm_dev(dm_t, dgm, cyc_cap=16, part=False, out=bare, ctx=ctx)
    _same(o, bare.to_host(), names=("h1_gen", "h1_flag", "cyc_len", "h0_edge", "status"))
    torch.cuda.synchronize()


def test_eeg_windows_composition(ctx):
    from oracle import port
    from tda_eeg_audio_amd import engine, synth
    win = synth.eeg_windows(6, seed=60, windows_per_recording=3)
    assert win.shape == (6, 47, 250)
    seg = np.array([0, 3, 3, 6], np.int32)
    dgm, gen = engine.generators_eeg_windows_dev(_dev(win), h1_cap=512, seg_off_t=_dev(seg), ctx=ctx)
    out = gen.to_host()
    h0, c0, h1, c1 = _rows(dgm)
    keys = [er.keys_dm(port.corr_dist(w)[1]) for w in win]
    ref = _ref_windows(keys, h0, c0, h1, c1)
    _same(out, ref)
    assert c1.min() > 4 and not out["h1_flag"].any() and not out["status"].any()
    assert out["mean"].tobytes() == gr.mean_part(ref["part"], seg).tobytes() and np.isnan(out["mean"][1]).all()
    # the fused kernel's diagrams are the matrix route's
    d2 = engine.rips_dm_dev(engine.corr_dist_dev(_dev(win), ctx=ctx), h1_cap=512, ctx=ctx)
    assert d2.h1.cpu().numpy()[0, :c1[0]].tobytes() == h1[0, :c1[0]].tobytes()


def test_group_means(ctx):
    from tda_eeg_audio_amd import engine
    dms = _circles(7, 24, 50)
    dm_t = _dev(dms)
    dgm = engine.rips_dm_dev(dm_t, ctx=ctx)
    seg = np.array([0, 0, 1, 6, 7], np.int32)                       # sizes 0, 1 (skipped alone), 5, 1
    st = np.array([4, 0, 0, 16, 0, 0, 0], np.int32)
    gen = engine.generators_dm_dev(dm_t, dgm, seg_off_t=_dev(seg), status_in=_dev(st), mean_skip=4 | 16, ctx=ctx)
    part, mean = gen.part.cpu().numpy(), gen.mean.cpu().numpy()
    ref = gr.mean_part(part, seg, st, 4 | 16)
    assert mean.shape == (4, 24) and mean.tobytes() == ref.tobytes()
    assert np.isnan(mean[0]).all() and np.isnan(mean[1]).all() and not np.isnan(mean[2:]).any() and mean[2].max() > 0
    # nothing skipped, and every window its own group
    m0 = engine.generators_mean_dev(gen.part, 7, 24, seg_off_t=_dev(seg), ctx=ctx).cpu().numpy()
    assert m0.tobytes() == gr.mean_part(part, seg).tobytes()
    own = engine.generators_mean_dev(gen.part, 7, 24, ctx=ctx).cpu().numpy()
    assert own.tobytes() == part.tobytes()
    # the host form
    mh = np.full((4, 24), -1.0)
    hp = lambda a: a.ctypes.data_as(C.c_void_p)                   # noqa: E731
    ctx.check(ctx.lib.tda_generators_mean(ctx.h, hp(part), 7, 24, hp(seg), 4, hp(st), 4 | 16, hp(mh)))
    assert mh.tobytes() == ref.tobytes()
    mo = np.full((7, 24), -1.0)                                   # seg_off = NULL, status_in = NULL
    ctx.check(ctx.lib.tda_generators_mean(ctx.h, hp(part), 7, 24, None, 7, None, 0, hp(mo)))
    assert mo.tobytes() == own.tobytes()


def _msg(ctx):
    buf = C.create_string_buffer(512)
    ctx.lib.tda_last_error(ctx.h, buf, 512)
    return buf.value.decode()


def test_refusals(ctx):
    import torch
    from tda_eeg_audio_amd import engine
    dev = torch.device("cuda", 0)
    p = engine._tp
    lib, h = ctx.lib, ctx.h
    dm = torch.zeros((2, 129, 129), dtype=torch.float64, device=dev)
    rows = torch.zeros((2, 8, 2), dtype=torch.float64, device=dev)
    cnt = torch.zeros(2, dtype=torch.int32, device=dev)
    gen = torch.full((2, 8, 4), SENT, dtype=torch.int16, device=dev)
    flag = torch.full((2, 8), SENT, dtype=torch.int32, device=dev)
    cyc = torch.full((2, 8, 128), SENT, dtype=torch.int16, device=dev)
    st = torch.full((2,), SENT, dtype=torch.int32, device=dev)
    mean = torch.full((2, 9), -7.0, dtype=torch.float64, device=dev)

    def tail(cyc_cap=8, h1_cap=8, h0=rows, h0_cap=8, h0_edge=gen):
        return (p(h0), h0_cap, p(cnt) if h0 is not None else None, p(rows), h1_cap, p(cnt), None, 0, cyc_cap, p(gen), p(flag),
                p(cyc), p(flag), None, p(h0_edge), None)

    calls = [
        lambda: lib.tda_generators_dm_batch_dev(h, p(dm), 2, 129, 2.0, 1, *tail(), p(st), None),               # n
        lambda: lib.tda_generators_dm_batch_dev(h, p(dm), 2, 0, 2.0, 1, *tail(), p(st), None),
        lambda: lib.tda_generators_dm_batch_dev(h, p(dm), 2, 9, 2.0, 1, *tail(cyc_cap=3), p(st), None),        # cyc_cap
        lambda: lib.tda_generators_dm_batch_dev(h, p(dm), 2, 9, 2.0, 1, *tail(cyc_cap=129), p(st), None),
        lambda: lib.tda_generators_dm_batch_dev(h, p(dm), 2, 9, 2.0, 1, *tail(h1_cap=0), p(st), None),         # h1_cap
        lambda: lib.tda_generators_dm_batch_dev(h, p(dm), 2, 9, 2.0, 1, *tail(h0=None), p(st), None),          # h0_edge, no rows
        lambda: lib.tda_generators_dm_batch_dev(h, p(dm), 2, 9, 2.0, 1, *tail(h0_cap=0), p(st), None),
        lambda: lib.tda_generators_cloud_batch_dev(h, p(dm), p(cnt), 2, 8, 5, 1, 2.0, *tail(), p(st), None),   # dim
        lambda: lib.tda_generators_cloud_batch_dev(h, p(dm), p(cnt), 2, 8, 0, 1, 2.0, *tail(), p(st), None),
        lambda: lib.tda_generators_cloud_batch_dev(h, p(dm), p(cnt), 2, 0, 3, 1, 2.0, *tail(), p(st), None),   # p_cap
        lambda: lib.tda_generators_takens_batch_dev(h, p(dm), p(cnt), 2, 250, 5, 2, 2.0, *tail(), None, p(st), None),
        lambda: lib.tda_generators_takens_batch_dev(h, p(dm), p(cnt), 2, 0, 3, 2, 2.0, *tail(), None, p(st), None),
        lambda: lib.tda_generators_takens_batch_dev(h, p(dm), p(cnt), 2, 250, 3, 2, 2.0, *tail(cyc_cap=2), None, p(st), None),
        lambda: lib.tda_generators_dm_batch_dev(h, None, 2, 9, 2.0, 1, *tail(), p(st), None),                  # a null pointer
        lambda: lib.tda_generators_dm_batch_dev(h, p(dm), 2, 9, 2.0, 1, *(tail()[:11] + (None, p(flag), p(mean), None, None)),
                                                p(st), None),                                                  # part, no cyc
        lambda: lib.tda_generators_mean_dev(h, p(mean), 2, 9, None, 1, None, 0, p(mean), None),                # n_seg != n_win
        lambda: lib.tda_generators_mean_dev(h, p(mean), 2, 0, None, 2, None, 0, p(mean), None),                # n
    ]
    for k, call in enumerate(calls):
        assert call() == 1, k                                      # TDA_ERR_INVALID
        assert _msg(ctx), k
    torch.cuda.synchronize()
    assert (gen == SENT).all() and (flag == SENT).all() and (cyc == SENT).all() and (st == SENT).all() and (mean == -7.0).all()
    # the host forms refuse before anything is staged or written
    hp = lambda a: a.ctypes.data_as(C.c_void_p)                   # noqa: E731
    dmh, rh, ch = np.zeros((2, 9, 9)), np.zeros((2, 8, 2)), np.zeros(2, np.int32)
    gh, fh, cyh, sh = np.full((2, 8, 4), SENT, np.int16), np.full((2, 8), SENT, np.int32), np.full((2, 8, 8), SENT, np.int16), \
        np.full(2, SENT, np.int32)

    def htail(cyc_cap=8):
        return (hp(rh), 8, hp(ch), hp(rh), 8, hp(ch), None, 0, cyc_cap, hp(gh), hp(fh), hp(cyh), hp(fh), None, None, None)

    assert lib.tda_generators_dm_batch(h, hp(dmh), 2, 9, 2.0, 1, *htail(3), hp(sh)) == 1
    assert lib.tda_generators_dm_batch(h, hp(dmh), 2, 129, 2.0, 1, *htail(), hp(sh)) == 1
    assert lib.tda_generators_mean(h, hp(dmh), 2, 9, None, 1, None, 0, hp(np.zeros(18))) == 1
    assert (gh == SENT).all() and (fh == SENT).all() and (cyh == SENT).all() and (sh == SENT).all()
    # the Python front end refuses with ValueError before any call
    dgm = (None, None, rows, cnt)
    for bad in (3, 129, 8.0, True, None):
        with pytest.raises(ValueError):
            engine.generators_dm_dev(dm[:, :9, :9].contiguous(), dgm, cyc_cap=bad, ctx=ctx)
    with pytest.raises(ValueError):
        engine.generators_dm_batch(dmh, None, None, rh[:, :0], ch, ctx=ctx)
    # an empty batch is no error and touches nothing
    assert lib.tda_generators_dm_batch_dev(h, None, 0, 9, 2.0, 1, *((None, 0, None, None, 8, None, None, 0, 8) + (None,) * 7),
                                           None, None) == 0
