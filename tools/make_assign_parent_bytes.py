#!/usr/bin/env python3
"""Writes tests/golden/assign_parent_bytes.npz: the inputs of tests/test_gpu_assign_bytes.py and what the library of the
checked-out tree answers.  Run once on the MI355X at the last commit with a private solver in each of wasserstein.hip
and wasserstein_q.hip; the test then holds every later tree to those bytes.

    python tools/make_assign_parent_bytes.py [--out tests/golden/assign_parent_bytes.npz]

The pairs, by what they reach (rows x columns are finite points; "general" = distinct births):
  general 3 x 5, 40 x 64, 64 x 65 (at 256 rows: deferred by the small first launch), 70 x 130 (4 column slots per lane),
  130 x 260 (8), each also with the larger diagram first; equal births 1 x 1, 20 x 64, 64 x 200 (the recurrence, with dead
  prefixes and suffixes), equal births with 65 rows (falls through to the general solver); an empty diagram against a
  full one; NaN / inf rows interleaved; every cell dead; exactly one live cell; 520 finite points in a buffer of 600
  rows (TDA_WIN_NOT_CONVERGED under tda_wasserstein_q_batch).
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import test_gpu_assign_bytes as T      # noqa: E402
import wasserstein_q_ref as wq         # noqa: E402


def build_inputs():
    rng = np.random.default_rng(20261019)
    f32 = lambda x: np.float32(x).astype(float)
    dgms, names = [], {}

    def add(name, d):
        names[name] = len(dgms)
        dgms.append(np.asarray(d, float).reshape(-1, 2))

    def general(n, exact32):                    # float32-exact coordinates tie in the sums, float64 ones do not
        b = rng.uniform(0.0, 1.0, n)
        p = rng.uniform(0.01, 0.5, n)
        if exact32:
            b, p = f32(b), f32(p)
        return np.stack([b, b + p], 1)

    def h0(n):                                  # persistences over three decades: dead prefixes and suffixes
        return wq.h0_diagram(0.0, f32(10.0 ** rng.uniform(-3.0, 0.0, n)))

    for i, n in enumerate([3, 5, 40, 64, 65, 70, 130, 260, 30]):
        add(f"g{n}", general(n, i % 2 == 0))
    add("g64b", general(64, False))
    add("g130b", general(130, True))
    for n in [20, 64, 65, 80, 200]:
        add(f"h{n}", h0(n))
    add("h1a", wq.h0_diagram(0.0, [0.7]))
    add("h1b", wq.h0_diagram(0.0, [0.8]))
    add("empty", np.zeros((0, 2)))
    bad = [[np.nan, 1.0], [0.5, np.inf], [-np.inf, 0.0], [np.nan, np.nan], [0.25, np.nan], [np.inf, np.inf]]
    for name, src, at in (("nan40", "g40", [0, 7, 8, 43]), ("nan64", "g64b", [3, 4, 5, 30, 68, 69])):
        d = dgms[names[src]]
        rows, k = [], 0
        for r in range(len(d) + len(at)):
            if r in at:
                rows.append(bad[at.index(r)])
            else:
                rows.append(d[k]); k += 1
        add(name, rows)
    # far apart and near the diagonal: no cell has a negative gain; one more point each that meet: exactly one has
    dead_a = np.array([[0.1 * i, 0.1 * i + 0.01] for i in range(6)])
    dead_b = np.array([[10.0 + 0.1 * j, 10.0 + 0.1 * j + 0.02] for j in range(9)])
    add("dead_a", dead_a); add("dead_b", dead_b)
    add("live_a", np.r_[dead_a[:3], [[5.0, 7.0]], dead_a[3:]])
    add("live_b", np.r_[dead_b[:5], [[5.1, 7.1]], dead_b[5:]])
    for a, b, n_live in (("dead_a", "dead_b", 0), ("live_a", "live_b", 1)):
        for order, ground in T.VARIANTS:
            C, s, t = wq.costs(dgms[names[a]], dgms[names[b]], order, ground)
            assert int((wq.gains(C, s, t) < 0.0).sum()) == n_live, (a, b, order, ground)
    add("g520", general(520, False))

    small = [("g3", "g5"), ("g40", "g64"), ("g64", "g65"), ("h1a", "h1b"), ("h20", "h64"), ("h65", "h80"), ("empty", "g30"),
             ("nan40", "nan64"), ("dead_a", "dead_b"), ("live_a", "live_b"), ("g40", "h64")]
    wide = [("g70", "g130"), ("h64", "h200"), ("g64b", "g130b")]
    rev = lambda ps: [(b, a) for a, b in ps]
    pairs = {
        "c128": small + rev(small[:3] + small[4:8]) + [("empty", "empty")],
        "c256": small + wide + rev(small[1:3] + small[4:7] + wide),
        "c512": [("g130", "g260"), ("g260", "g130"), ("g64", "g65"), ("h64", "h200"), ("live_b", "live_a"), ("h200", "h64")],
        "c600": [("g520", "g5"), ("g3", "g5"), ("g5", "g520")],
    }
    fx = {"points": np.concatenate(dgms), "off": np.cumsum([0] + [len(d) for d in dgms]).astype(np.int64)}
    for g, ps in pairs.items():
        fx[g + "_a"] = np.array([names[a] for a, _ in ps], np.int32)
        fx[g + "_b"] = np.array([names[b] for _, b in ps], np.int32)
    return fx


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "assign_parent_bytes.npz"))
    args = ap.parse_args()
    from tda_eeg_audio_amd import _lib
    ctx = _lib.get_ctx(0)
    fx = build_inputs()
    n_pairs = 0
    for g in sorted(T.GROUPS):
        got = T.run_group(ctx, fx, g)
        n_pairs += len(fx[g + "_a"])
        for k, v in got.items():
            if k.endswith("/status"):
                print(f"{k:32s} {np.bincount(v.astype(np.int64) & 0xff).nonzero()[0].tolist()}")
        fx.update(got)
    np.savez_compressed(args.out, **fx)
    print(f"{n_pairs} pairs, {len(fx['points'])} points, {len(fx)} arrays, {os.path.getsize(args.out)} bytes -> {args.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
