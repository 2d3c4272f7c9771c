"""
The Wasserstein distances of order 1 and 2 (L2 / L-infinity ground metric) on the CPU: the assignment reference against
exhaustive search, the recurrence of the kernel's equal-birth path against the assignment, the live-range rule of that
path (csrc/wasserstein_q.hip, restated in tests/wasserstein_q_ref.py) at the four cuts, and the `wq` record of
pipeline.step_outputs.  No GPU.

Bars.  Reference against exhaustive search: both sum the same float64 costs with math.fsum, so they differ only where two
matchings tie within rounding: 1e-13 * max(1, S), S the sum of the pair's diagonal costs (a few ulps of sums below 10).
Recurrence against assignment: 1e-12 * max(1, S) -- the recurrence sums gains C - s - t, each a few ulps of S off, over
at most 64 matched pairs.  Live-range rule: the same BITS with and without it, and every trimmed cell has a computed
gain of exactly 0.
"""
import math
import types

import numpy as np
import pytest

import wasserstein_q_ref as wq
from tda_eeg_audio_amd import _lib, engine, pipeline, utils

VARIANTS = wq.VARIANTS


def test_known_answers_of_the_reference():
    for A, B, want in wq.KNOWN:
        for (order, ground), w in want.items():
            assert wq.distance_ref(A, B, order, ground) == w, (A, B, order, ground)
            assert wq.distance_ref(B, A, order, ground) == w
            v = wq.value_line(A, B, order, ground)
            assert v is None or wq.distance(v, order) == w


@pytest.mark.parametrize("order,ground", VARIANTS)
def test_reference_against_exhaustive_search(order, ground):
    worst = 0.0
    for a, b in wq.small_pairs(200, seed=31):
        ref, brute = wq.value_ref(a, b, order, ground), wq.value_brute(a, b, order, ground)
        S = wq.diag_sum(a, b, order, ground)
        worst = max(worst, abs(ref - brute) / max(1.0, S))
        assert abs(ref - brute) <= 1e-13 * max(1.0, S), (a, b, ref, brute)
    print(f"order {order} {ground}: max |ref - brute| / max(1, S) = {worst:.3g}")


def _line_pairs(rng, n):
    out = []
    for k in range(n):
        R, C = int(rng.integers(1, 65)), int(rng.integers(1, 129))
        kind = k % 5
        b0 = 0.0
        if kind == 0:                                        # the workload: EEG deaths 0.48 .. 1.04, half the audio < 0.08
            p = rng.uniform(0.48, 1.04, R)
            q = np.where(rng.random(C) < 0.5, rng.uniform(1e-4, 0.08, C), rng.uniform(0.08, 0.9, C))
        elif kind == 1:                                      # log-uniform over four decades: prefix, suffix, dead rows
            p, q = 10.0 ** rng.uniform(-2, 2, R), 10.0 ** rng.uniform(-2, 2, C)
        elif kind == 2:                                      # tied deaths on a coarse grid
            p, q = rng.integers(1, 40, R) / 8.0, rng.integers(1, 400, C) / 64.0
        elif kind == 3:                                      # a common birth != 0
            b0 = float(rng.choice([0.3, -2.0, 37.5]))
            p, q = 10.0 ** rng.uniform(-3, 1, R), 10.0 ** rng.uniform(-3, 1, C)
        else:                                                # near each other: (almost) everything live
            p, q = rng.uniform(0.5, 1.0, R), rng.uniform(0.4, 1.2, C)
        out.append((wq.h0_diagram(b0, p), wq.h0_diagram(b0, q)))
    return out


@pytest.mark.parametrize("order,ground", VARIANTS)
def test_recurrence_against_assignment(order, ground):
    rng = np.random.default_rng(32)
    worst = 0.0
    for a, b in _line_pairs(rng, 150):
        line, ref = wq.value_line(a, b, order, ground), wq.value_ref(a, b, order, ground)
        assert line is not None
        S = wq.diag_sum(a, b, order, ground)
        worst = max(worst, abs(line - ref) / max(1.0, S))
        assert abs(line - ref) <= 1e-12 * max(1.0, S), (len(a), len(b), line, ref)
    print(f"order {order} {ground}: max |recurrence - assignment| / max(1, S) = {worst:.3g}")
    # what the kernel does not take this way
    assert wq.value_line(wq.h0_diagram(0, [0.5, 0.25], sort=False), wq.h0_diagram(0, [1.0, 2.0]), order, ground) is None
    assert wq.value_line([[0, 1], [0.5, 1]], [[0, 1], [0, 2]], order, ground) is None
    assert wq.value_line(wq.h0_diagram(0, np.arange(1, 66)), wq.h0_diagram(0, np.arange(1, 67)), order, ground) is None


def _check_rule(b0, pr, qc, order, ground, min_trim=0):
    """Bits with and without the live-range rule; every trimmed cell has a computed gain of exactly 0."""
    R, Cn = wq.h0_diagram(b0, pr), wq.h0_diagram(b0, qc)
    if len(R) > len(Cn):
        R, Cn = Cn, R
    g = wq.line_gains(R, Cn, order, ground)
    ilo, ihi, jlo, jhi = wq.live_ranges(b0, R[:, 1], Cn[:, 1], order, ground)
    dead = np.ones(g.shape, bool)
    dead[ilo:ihi, jlo:jhi] = False
    assert (g[dead] == 0.0).all(), ("a trimmed cell has a computed gain != 0", order, ground, b0)
    full, trimmed = wq.recurrence(g), wq.recurrence(g[ilo:ihi, jlo:jhi])
    assert np.float64(full).tobytes() == np.float64(trimmed).tobytes(), (full, trimmed, order, ground)
    n_trim = len(R) - (ihi - ilo) + len(Cn) - (jhi - jlo)
    assert n_trim >= min_trim, (n_trim, min_trim, order, ground)
    return n_trim, int((~dead).sum())


@pytest.mark.parametrize("order,ground", VARIANTS)
def test_live_range_rule_random(order, ground):
    rng = np.random.default_rng(33)
    trimmed = live = 0
    for a, b in _line_pairs(rng, 150):
        t, l = _check_rule(a[0, 0], a[:, 1] - a[0, 0], b[:, 1] - b[0, 0], order, ground)
        trimmed, live = trimmed + t, live + l
    assert trimmed > 0 and live > 0
    cut = wq.CUTS[order, ground]
    for R, C in [(1, 1), (1, 128), (64, 128), (7, 90)]:
        p = rng.uniform(0.5, 1.0, R)
        t, _ = _check_rule(0.0, p, rng.uniform(0.55, 0.95, C), order, ground)       # ratios < 2: nothing may go
        assert t == 0
        _check_rule(0.0, p, rng.uniform(1e-3, 0.5 / cut / 2, C), order, ground, min_trim=R + C)    # a factor 2 beyond the cut
        _check_rule(0.0, p, rng.uniform(2 * cut, 40.0, C), order, ground, min_trim=R + C)
        nd = C // 3
        q = np.concatenate([rng.uniform(1e-3, 0.2 / cut, nd), rng.uniform(0.5, 1.0, C - 2 * nd), rng.uniform(2.5 * cut, 20.0, nd)])
        _check_rule(0.0, p, q, order, ground, min_trim=2 * nd)
        _check_rule(0.25, p, q, order, ground, min_trim=2 * nd)


@pytest.mark.parametrize("order,ground", VARIANTS)
def test_ratios_at_the_cut(order, ground):
    """Persistence ratios within ulps of the cut, and on either side of the rule's margin: whichever side they fall on,
    the same bits; and the cut itself is where the computed gain changes sign."""
    cut = wq.CUTS[order, ground]
    rel = [0.0, 1e-12, 5e-10, 9.9e-10, 1e-9, 1.01e-9, 2e-9, 1e-6, 1e-3]
    for p0 in (1.0, 0.7310585786300049, 3.0, 1e-3):
        for side in (1.0 / cut, cut):
            base = p0 * side
            qs = [np.nextafter(base, -np.inf), base, np.nextafter(base, np.inf)]
            qs += [base * (1.0 + s * r) for r in rel for s in (-1.0, 1.0)]
            for q in qs:
                _check_rule(0.0, [p0], [q], order, ground)
                _check_rule(0.0, [p0, p0], [q, p0], order, ground)
                _check_rule(0.5, [p0] * 3, [q] * 2 + [p0] * 2, order, ground)
    # the table of cuts: a cell 1e-6 inside has a gain < 0, a cell 1e-6 outside a gain of 0
    for r, live in ((cut * (1 - 1e-6), True), (cut * (1 + 1e-6), False)):
        for R, Cn in ((wq.h0_diagram(0, [1.0]), wq.h0_diagram(0, [r])), (wq.h0_diagram(0, [r]), wq.h0_diagram(0, [1.0]))):
            assert (wq.line_gains(R, Cn, order, ground)[0, 0] < 0.0) == live
    # huge coordinates switch the rule off instead of overflowing
    assert wq.live_ranges(0.0, np.array([1e200]), np.array([1.0, 1e200]), order, ground) == (0, 1, 0, 2)
    # persistences whose squares underflow are never trimmed against each other
    assert wq.live_ranges(0.0, np.array([1e-160]), np.array([1e-170, 1e-160]), order, ground) == (0, 1, 0, 2)


# ---- the table of optional outputs ------------------------------------------------------------------------------------
GRID, LEVELS = np.linspace(0.0, 2.0, 16), 2
IMAGES = (np.linspace(0.0, 1.0, 5), np.linspace(0.0, 1.0, 4), 0.1, 1)
DIRS = utils.default_directions(4)


def test_step_outputs_wq_alone():
    (o,) = pipeline.step_outputs(wasserstein_q=(2, "l2"))
    assert o.name == "wq" and o.shape == (pipeline.WQ_COLS,) == (2,) and o.params == (2, "l2")
    assert pipeline.step_outputs(wasserstein_q=None) == []
    for order, ground in VARIANTS:
        assert pipeline.step_outputs(wasserstein_q=(order, ground))[0].params == (order, ground)
    assert pipeline.step_outputs(wasserstein_q=[1, "linf"])[0].params == (1, "linf")


def test_step_outputs_all_six_in_the_fixed_order():
    outs = pipeline.step_outputs(correlations=True, bottleneck=True, landscapes=(GRID, LEVELS), images=IMAGES, sliced=DIRS,
                                 wasserstein_q=(1, "linf"))
    assert [o.name for o in outs] == ["corr", "bott", "land", "img", "slc", "wq"]
    assert outs[-1].shape == (2,) and outs[-1].params == (1, "linf")
    # whatever the order of the keywords, and with outputs left out
    assert [o.name for o in pipeline.step_outputs(wasserstein_q=(2, "linf"), sliced=DIRS, bottleneck=True)] == ["bott", "slc", "wq"]
    # the first five are what they are without the sixth
    five = pipeline.step_outputs(correlations=True, bottleneck=True, landscapes=(GRID, LEVELS), images=IMAGES, sliced=DIRS)
    assert [(o.name, o.shape) for o in five] == [(o.name, o.shape) for o in outs[:5]]


@pytest.mark.parametrize("bad", [(3, "l2"), (0, "l2"), (2, "L2"), (2, "l1"), (2, 0), (1.5, "l2"), (True, "l2"), 2, "l2", (2,),
                                 (2, "l2", 0), ("2", "l2"), (2, None)])
def test_step_outputs_invalid_tuples(bad):
    with pytest.raises(ValueError):
        pipeline.step_outputs(wasserstein_q=bad)


def test_bad_parameters_raise_before_any_launch(monkeypatch):
    """engine rejects a bad order or ground before it asks for a context or marshals a call; utils.safe_wasserstein_q turns
    that into NaN, immediately and queued.  Context, marshalling and library loading are replaced by recorders here, so
    "before any launch" is what is asserted, not what a machine without a GPU happens to do."""
    reached = []
    fake = types.SimpleNamespace(lib=types.SimpleNamespace(tda_wasserstein_q_batch=None, tda_wasserstein_q_batch_dev=None))
    monkeypatch.setattr(engine, "get_ctx", lambda *a, **k: reached.append("get_ctx") or fake)
    monkeypatch.setattr(engine, "_pair_batch", lambda *a, **k: reached.append("_pair_batch"))
    monkeypatch.setattr(engine, "_pair_dev", lambda *a, **k: reached.append("_pair_dev"))
    monkeypatch.setattr(_lib, "load", lambda *a, **k: reached.append("load"))
    rows, cnt = np.zeros((1, 2, 2)), np.zeros(1, np.int32)
    for order, ground in [(3, "l2"), (2, "l3"), (0, "linf"), (True, "l2"), (2, 1)]:
        with pytest.raises(_lib.TdaError, match="wasserstein_q"):
            engine.wasserstein_q_batch(rows, cnt, rows, cnt, order=order, ground=ground)
        with pytest.raises(_lib.TdaError, match="wasserstein_q"):
            engine.wasserstein_q_dev(None, None, None, None, order=order, ground=ground)
        assert math.isnan(utils.safe_wasserstein_q([[0, 1]], [[0, 2]], order=order, ground=ground))
        with utils.batch():
            later = utils.safe_wasserstein_q([[0, 1]], [[0, 2]], order=order, ground=ground)
        assert math.isnan(float(later))
        assert reached == [], (order, ground, reached)
    # the recorders do see a well-formed call: the check above is not vacuous
    engine.wasserstein_q_batch(rows, cnt, rows, cnt, order=2, ground="linf")
    assert reached == ["get_ctx", "_pair_batch"]


def test_abi_is_declared_bound_and_exported():
    import os
    for name in ("tda_wasserstein_q_batch", "tda_wasserstein_q_batch_dev"):
        assert name in _lib.SYMBOLS
    # the arguments of tda_wasserstein_batch[_dev] with (order, ground) before out / status
    for name in ("tda_wasserstein_batch", "tda_wasserstein_batch_dev"):
        res, args = _lib.SYMBOLS[name]
        k = args.index(_lib._I, 9 if name.endswith("_dev") else 11) + 1           # behind n_pairs
        q = _lib.SYMBOLS[name.replace("wasserstein", "wasserstein_q")]
        assert q == (res, args[:k] + [_lib._I, _lib._I] + args[k:])
    assert (_lib.TDA_GROUND_L2, _lib.TDA_GROUND_LINF) == (0, 1) and engine.GROUNDS == {"l2": 0, "linf": 1}
    assert callable(utils.safe_wasserstein_q) and callable(engine.wasserstein_q_batch) and callable(engine.wasserstein_q_dev)
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "tdaeeg.h")).read()
    assert "tda_wasserstein_q_batch_dev(" in header and "tda_wasserstein_q_batch(" in header
    assert "#define TDA_GROUND_L2   0" in header and "#define TDA_GROUND_LINF 1" in header
