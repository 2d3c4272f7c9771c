"""
The assignment solver shared by csrc/wasserstein.hip and csrc/wasserstein_q.hip (csrc/assign_dev.h) against the bytes the
two private copies of it gave before they were merged.

tests/golden/assign_parent_bytes.npz (written once by tools/make_assign_parent_bytes.py, on the MI355X, at the last
commit with two solvers) holds ragged input diagrams, the pairs of four launches (buffers of 128, 256, 512 and 600 rows)
and the `out` / `status` words of every entry point: tda_wasserstein_batch, the four tda_wasserstein_q_batch variants,
tda_wasserstein_cross_dev and tda_wasserstein_matrix_dev, each with pruning on and off, the order-1 ones under the
list-driven and the grid-driven second launch.  Bar: equal bytes, NaN payloads included.  The pairs are the smallest
that reach every instantiation (1, 2, 4, 8 column slots per lane) and every exit: see the generator.
"""
import os

import numpy as np
import pytest

from tda_eeg_audio_amd import engine

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "assign_parent_bytes.npz")
GROUPS = {"c128": 128, "c256": 256, "c512": 512, "c600": 600}       # launch -> rows of both diagram buffers
ORDER1_MAX = 512                    # tda_wasserstein_batch refuses larger buffers; c600 is for tda_wasserstein_q_batch
VARIANTS = [(1, "l2"), (2, "l2"), (1, "linf"), (2, "linf")]


def pack(points, off, idx, cap, fill=7.25):
    """Diagrams idx of the ragged table in a buffer of `cap` rows, stale rows (fill) behind the count."""
    rows = np.full((len(idx), cap, 2), fill)
    cnt = np.zeros(len(idx), np.int32)
    for i, d in enumerate(idx):
        p = points[off[d]:off[d + 1]]
        assert len(p) <= cap
        rows[i, :len(p)] = p
        cnt[i] = len(p)
    return rows, cnt


def tables(n):
    """The group tables of n pairs: three A groups (none above 64 diagrams); for the cross launch B is grouped alike and
    group g meets group g, so pair i is (A_i, B_i); for the matrix every A group is its own class with two columns: the
    B group itself, and the B group without its first diagram (A_i meets B_{i+1}, the last position has no pair)."""
    cuts = [0, (n + 2) // 3, (2 * n + 2) // 3, n]
    seg = np.array(cuts, np.int32)
    gather, seg_m = [], [0]
    for g in range(3):
        own = list(range(cuts[g], cuts[g + 1]))
        for col in (own, own[1:]):
            gather += col
            seg_m.append(len(gather))
    return seg, np.arange(3, dtype=np.int32), np.array(gather, np.int64), np.array(seg_m, np.int32)


def run_group(ctx, fx, g):
    """{key: array} of every entry point on the pairs of launch g."""
    import torch
    cap = GROUPS[g]
    dev = torch.device("cuda", ctx.device)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    points, off = fx["points"], fx["off"]
    ra, ca = pack(points, off, fx[g + "_a"], cap)
    rb, cb = pack(points, off, fx[g + "_b"], cap)
    n = len(ca)
    got = {}
    try:
        for prune in (1, 0):
            ctx.set_wasserstein_pruning(bool(prune))
            for order, ground in VARIANTS:
                out, st = engine.wasserstein_q_batch(ra, ca, rb, cb, order=order, ground=ground, ctx=ctx, want_status=True)
                got[f"{g}/q{order}{ground}/p{prune}/out"], got[f"{g}/q{order}{ground}/p{prune}/status"] = out, st
            if cap > ORDER1_MAX:
                continue
            seg, cls_a, gather, seg_m = tables(n)
            dra, dca, drb, dcb = t(ra), t(ca), t(rb), t(cb)
            drm, dcm = t(rb[gather]), t(cb[gather])
            zeros = torch.zeros(len(gather), dtype=torch.int32, device=dev)
            for scheme in (ctx.SCHEME_LISTS, ctx.SCHEME_GRID):
                ctx.set_launch_scheme(scheme)
                key = f"{g}/%s/s{scheme}/p{prune}/%s"
                out, st = engine.wasserstein_batch(ra, ca, rb, cb, ctx=ctx, want_status=True)
                got[key % ("batch", "out")], got[key % ("batch", "status")] = out, st
                w, st = engine.wasserstein_cross_dev(dra, dca, t(seg), drb, dcb, t(seg), zeros, t(cls_a), ctx=ctx)
                got[key % ("cross", "out")], got[key % ("cross", "status")] = w.cpu().numpy(), st.cpu().numpy()
                o, p, f = engine.wasserstein_matrix_dev(dra, dca, t(seg), t(cls_a), drm, dcm, t(seg_m), zeros, 2, ctx=ctx)
                for name, x in (("out", o), ("pairs", p), ("flags", f)):
                    got[key % ("matrix", name)] = x.cpu().numpy()
    finally:
        ctx.set_wasserstein_pruning(True)
        ctx.set_launch_scheme(ctx.SCHEME_LISTS)
    return got


@pytest.fixture(scope="module")
def fx():
    return np.load(FIXTURE)


@pytest.mark.parametrize("g", sorted(GROUPS))
def test_bytes_of_the_two_solvers(ctx, fx, g):
    got = run_group(ctx, fx, g)
    want = sorted(k for k in fx.files if k.startswith(g + "/"))
    assert sorted(got) == want and len(want) >= 16
    for k in want:
        assert got[k].dtype == fx[k].dtype and got[k].tobytes() == fx[k].tobytes(), k
