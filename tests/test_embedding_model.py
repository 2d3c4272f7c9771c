"""
The CPU statement of the delay and dimension selection against itself (tests/embedding_ref.py): the two statements agree --
as bytes for every integer, for nn, dim and frac, to the measured bar for the mutual information --, the inputs with answers
worked out by hand give them, the four named signals give the delays and dimensions the literature's rules give, and the
error of the numpy statement of the mutual information against the 50-digit evaluation is measured again.  No GPU.
"""
import math

import numpy as np
import pytest

import embedding_cases as ec
import embedding_ref as er


def _same(a, b, keys, what):
    for k in keys:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), (what, k)


@pytest.mark.parametrize("name", [c[0] for c in ec.ami_cases()])
def test_ami_statements_agree(name):
    _, wins, max_lag, n_bins = next(c for c in ec.ami_cases() if c[0] == name)
    ref = ec.reference("ami", name)
    for w, x in enumerate(wins):
        a, b = er.ami_loops(x, max_lag, n_bins), er.ami_np(x, max_lag, n_bins)
        _same(a, b, ("joint", "status"), (name, w))
        assert a["ami"].shape == b["ami"].shape == (er.resolve_max_lag(len(x), max_lag) + 1,)
        if a["status"] == er.TDA_WIN_NOT_FINITE:
            assert np.isnan(a["ami"]).all() and np.isnan(b["ami"]).all() and a["tau"] == b["tau"] == 0
            continue
        err = np.abs(a["ami"] - b["ami"]).max()
        assert err <= er.AMI_BAR, (name, w, err)
        # tau is a function of the row it comes with
        assert a["tau"] == er.first_minimum(a["ami"]) and b["tau"] == er.first_minimum(b["ami"])
        assert ref["tau"][w] == b["tau"] and ref["joint"][w].tobytes() == b["joint"].tobytes()
        if a["status"] == 0:
            # the bins are bytes; row and column sums of every table are the bin counts of the two ends
            assert er.bins_loops(x, n_bins) == er.bins_np(x, n_bins).tolist()
            bn = er.bins_np(x, n_bins)
            assert bn.max() == n_bins - 1 and bn[np.argmax(x)] == n_bins - 1 and bn[np.argmin(x)] == 0
            for L, J in enumerate(a["joint"]):
                N = len(x) - L
                assert J.sum() == N
                assert (J.sum(1) == np.bincount(bn[:N], minlength=n_bins)).all()
                assert (J.sum(0) == np.bincount(bn[L:], minlength=n_bins)).all()
            assert (a["ami"] >= -er.AMI_BAR).all() and a["ami"][0] >= a["ami"].max() - er.AMI_BAR


@pytest.mark.parametrize("name", [c[0] for c in ec.fnn_cases()])
def test_fnn_statements_agree(name):
    _, wins, taus, d_max, theiler = next(c for c in ec.fnn_cases() if c[0] == name)
    for w, (x, tau) in enumerate(zip(wins, np.broadcast_to(taus, (len(wins),)))):
        a, b = er.fnn_loops(x, tau, d_max, theiler), er.fnn_np(x, tau, d_max, theiler)
        _same(a, b, ("counts", "frac", "nn", "status"), (name, w))
        assert a["dim"] == b["dim"]
        c = a["counts"]
        assert (c[:, 3] <= c[:, 1] + c[:, 2]).all() and (c[:, 3] >= np.maximum(c[:, 1], c[:, 2])).all() and (c[:, 3] <= c[:, 0]).all()
        for d in range(1, d_max + 1):
            M = len(x) - d * int(tau)
            row = a["nn"][d - 1]
            assert (row[max(M, 0):] == -1).all() and c[d - 1, 0] == (row >= 0).sum()
            i = np.nonzero(row >= 0)[0]
            assert (np.abs(i - row[i]) >= theiler).all() and (row[i] < M).all()
    _same(ec.reference("fnn", name), er.fnn_batch(wins, taus, d_max, theiler, route=er.fnn_loops),
          ("counts", "frac", "dim", "nn", "status"), name)


def test_known_alternating():
    """A strictly alternating two-valued signal on two bins: J_1 is off-diagonal only, J_2 diagonal only, and I(0) = log 2
    for an even length."""
    for n_t in (8, 66):
        for route in (er.ami_loops, er.ami_np):
            r = route(ec.alternating(n_t), 6, 2)
            assert r["status"] == 0 and r["joint"][1].tolist() == [[0, n_t // 2], [(n_t - 1) // 2, 0]]
            assert r["joint"][0].tolist() == [[n_t // 2, 0], [0, n_t // 2]] and r["joint"][2][0, 1] == r["joint"][2][1, 0] == 0
            assert abs(r["ami"][0] - math.log(2.0)) <= er.AMI_BAR
        assert np.float64(er.ami_loops(ec.alternating(n_t), 6, 2)["ami"][0]).tobytes() == np.float64(math.log(2.0)).tobytes()


def test_known_repeated_integers():
    """x = [0, 1, 2, 3] * 8: every point has neighbours at distance zero, and the tie goes to the smallest j."""
    x = ec.repeated_integers()
    for route in (er.fnn_loops, er.fnn_np):
        r = route(x, 1, 3, 1)
        assert r["status"] == 0
        for d in (1, 2, 3):
            M = 32 - d
            want = [i + 4 if i < 4 else i % 4 for i in range(M)] + [-1] * d
            assert r["nn"][d - 1].tolist() == want, d
        # a period-4 signal continues the same way from every copy: no false neighbour, except where the size bound bites
        assert r["counts"][:, 0].tolist() == [31, 30, 29] and not r["counts"][:, 1].any()
        assert r["dim"] == 1 and r["frac"].tolist() == [0.0, 0.0, 0.0]
    # four bins, one per value: I(L) = log 4 at the multiples of 4 up to the rounding, and the first minimum is L = 1
    a = er.ami_np(x, None, 4)
    assert abs(a["ami"][0] - math.log(4.0)) <= er.AMI_BAR and abs(a["ami"][4] - math.log(4.0)) <= er.AMI_BAR


def test_known_refusals():
    for route in (er.ami_loops, er.ami_np):
        r = route(np.full(20, 1.25), None, 8)
        assert r["status"] == er.TDA_WIN_DEGENERATE and r["tau"] == 0 and not r["ami"].any() and not r["joint"].any()
        assert r["ami"].shape == (6,)
        x = np.arange(20.0)
        x[7] = -np.inf
        r = route(x, 3, 8)
        assert r["status"] == er.TDA_WIN_NOT_FINITE and r["tau"] == 0 and np.isnan(r["ami"]).all() and not r["joint"].any()
    for route in (er.fnn_loops, er.fnn_np):
        x = np.arange(12.0) ** 2
        for tau, want in ((0, er.TDA_WIN_TOO_LARGE), (-3, er.TDA_WIN_TOO_LARGE), (11, er.TDA_WIN_DEGENERATE), (10, 0)):
            r = route(x, tau, 2, 1)
            assert r["status"] == want, tau
            if want:
                assert not r["counts"].any() and not r["frac"].any() and r["dim"] == 0 and (r["nn"] == -1).all()
        x[3] = np.nan
        assert route(x, 2, 2, 1)["status"] == er.TDA_WIN_NOT_FINITE
    assert er.resolve_max_lag(250) == 62 and er.resolve_max_lag(250, 125) == 125 and er.resolve_max_lag(4) == 1
    assert er.resolve_max_lag(67, 1000) == 65 and er.resolve_max_lag(5, -3) == 1
    assert er.fallback_tau(0, 250) == 6 and er.fallback_tau(0, 250, 125) == 12 and er.fallback_tau(0, 20) == 1
    assert er.fallback_tau(5, 250) == 5


def test_named_signals():
    """The delays and dimensions of the four signals, by both statements.  The margins of the AMI decisions (how far the
    minimum lies below its neighbours) are some twelve orders of magnitude above the rounding of log, so the delays are
    compared exactly."""
    for name, (x, tau, dim) in ec.named().items():
        a, b = er.ami_np(x), er.ami_loops(x)
        assert a["tau"] == b["tau"] == tau, (name, a["tau"], b["tau"])
        row = a["ami"]
        margin = min(row[tau - 1] - row[tau], row[tau + 1] - row[tau]) if row[tau + 1] > row[tau] else row[tau - 1] - row[tau]
        assert margin > 1e-3, (name, margin)
        for L in range(1, tau):                                  # and no earlier lag is within reach of a minimum
            assert not (row[L] < row[L - 1] + 1e-9 and row[L] <= row[L + 1] + 1e-9), (name, L)
        if dim is not None:
            assert er.fnn_np(x, tau, 5, 1)["dim"] == dim, name
    x = ec.sine()
    for route in (er.fnn_np, er.fnn_loops):
        r = route(x, 7, 5, 1)
        assert tuple(r["counts"][:3, 3]) == ec.SINE_EITHER and tuple(r["counts"][:3, 0]) == ec.SINE_VALID
        assert r["dim"] == 2 and r["frac"][1] == 5.0 / 236.0
    assert er.fnn_np(ec.lorenz(), 6, 5, 6)["dim"] == 3           # theiler = tau, the default of utils
    assert er.fnn_np(x, 7, 5, 7)["dim"] == 2


def test_ami_error_of_the_numpy_statement():
    """The bar of the GPU tests is 8 times the error measured here: against the 50-digit evaluation, on the inputs of the
    GPU tests, never against the kernel."""
    worst = 0.0
    for name, wins, max_lag, n_bins in ec.ami_cases():
        ref = ec.reference("ami", name)
        for w in range(len(wins)):
            if ref["status"][w] == 0:
                worst = max([worst] + er.ami_errors(ref["joint"][w], ref["ami"][w]))
    print(f"ami: largest |numpy statement - 50 digits| = {worst:.3e} = 2^{np.log2(worst):.2f}; "
          f"written {er.AMI_REF_ERR:.3e}, bar {er.AMI_BAR:.3e}")
    assert 0.0 < worst <= er.AMI_REF_ERR
    assert er.AMI_BAR == 8 * er.AMI_REF_ERR
