"""
GPU: the utils twins and the driver of the delay and dimension selection (utils.compute_ami, compute_tau_ami,
false_nearest_neighbours, estimate_embedding_dimension; drivers.embedding_parameters_from_windows) against the CPU
statement (tests/embedding_ref.py).  The driver's group values are the statement's, evaluated here from the kernels' own
per-window outputs: integers and sums in window order, so bytes.
"""
import numpy as np
import pytest

import embedding_cases as ec
import embedding_ref as er

pytestmark = pytest.mark.gpu


def test_utils_on_the_named_signals(ctx):
    from tda_eeg_audio_amd import _lib, utils
    for name, (x, tau, dim) in ec.named().items():
        ami = utils.compute_ami(x)
        ref = er.ami_np(x)
        assert ami.shape == ref["ami"].shape and np.abs(ami - ref["ami"]).max() <= er.AMI_BAR, name
        assert utils.compute_tau_ami(x) == tau, name
        fnn = utils.false_nearest_neighbours(x, tau)                       # theiler = tau
        want = er.fnn_np(x, tau, 5, tau)
        for k, key in enumerate(_lib.FNN_COUNT_NAMES):
            assert fnn[key].tobytes() == want["counts"][:, k].tobytes(), (name, key)
        assert fnn["fraction"].tobytes() == want["frac"].tobytes() and fnn["dim"] == want["dim"]
        if dim is not None:
            assert utils.estimate_embedding_dimension(x, tau, theiler=1) == dim, name
            assert utils.estimate_embedding_dimension(x, tau) == dim, name
    x = ec.sine()
    assert tuple(utils.false_nearest_neighbours(x, 7, theiler=1)["false_either"][:3]) == ec.SINE_EITHER
    assert utils.estimate_embedding_dimension(x, 7, max_dim=1) == 0         # one dimension is not enough for a sine
    assert utils.estimate_embedding_dimension(x, 7, max_dim=1, frac_tol=1.0) == 1


def test_utils_fallback_and_errors(ctx):
    from tda_eeg_audio_amd import utils
    from tda_eeg_audio_amd._lib import TdaError
    ramp = np.arange(250.0)
    assert er.ami_np(ramp, 5, 2)["tau"] == 0 and utils.compute_tau_ami(ramp, 5, 2) == 1
    assert utils.compute_tau_ami(ramp, 40, 2) == er.fallback_tau(er.ami_np(ramp, 40, 2)["tau"], 250, 40)
    assert utils.compute_tau_ami(np.full(250, 2.0)) == 6                  # compute_tau's max(62 // 10, 1)
    assert utils.compute_tau_ami(np.full(250, 2.0), 125) == 12
    assert not utils.compute_ami(np.full(50, 2.0)).any()
    bad = ramp.copy()
    bad[17] = np.nan
    for call in (lambda: utils.compute_ami(bad), lambda: utils.compute_tau_ami(bad),
                 lambda: utils.false_nearest_neighbours(bad, 3)):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(TdaError):
        utils.false_nearest_neighbours(ramp, 0)
    assert utils.estimate_embedding_dimension(ramp, 249) == 0              # no point has a second coordinate


def _group_rows(wins, seg, tau_seg, max_lag, n_bins, max_dim, theiler, frac_tol, ctx):
    """The driver's rows by the header's rules, from the per-window outputs of the kernels."""
    from tda_eeg_audio_amd import engine
    n_lag = er.resolve_max_lag(wins.shape[1], max_lag) + 1
    ami, _, _, ast = engine.ami_batch(wins, max_lag, n_bins, ctx=ctx)
    rows = np.full((len(seg) - 1, 2 + n_lag + max_dim), np.nan)
    for g in range(len(seg) - 1):
        a, b = seg[g], seg[g + 1]
        rows[g, 0] = tau_seg[g]
        th = max(int(tau_seg[g]), 1) if theiler is None else theiler
        cnt, frac, _, _, fst = engine.fnn_batch(wins[a:b], int(tau_seg[g]), max_dim, min(th, wins.shape[1]), frac_tol=frac_tol,
                                                ctx=ctx) if b > a else (np.zeros((0, max_dim, 4), np.int32), None, None, None, [])
        tot = np.zeros((max_dim, 4), np.int64)
        S, m = np.zeros(max_dim), 0
        for w in range(b - a):
            if fst[w] == 0:
                tot += cnt[w]
                S = S + frac[w]
                m += 1
        rows[g, 2 + n_lag:] = S / np.float64(m) if m else np.nan
        rows[g, 1] = 0
        for d in range(max_dim):
            if tot[d, 0] > 0 and float(tot[d, 3]) <= frac_tol * float(tot[d, 0]):
                rows[g, 1] = d + 1
                break
        S, m = np.zeros(n_lag), 0
        for w in range(a, b):
            if ast[w] == 0:
                S = S + ami[w]
                m += 1
        rows[g, 2:2 + n_lag] = S / np.float64(m) if m else np.nan
    return rows


@pytest.mark.parametrize("theiler", [None, 2])
def test_embedding_parameters_from_windows(ctx, theiler):
    from tda_eeg_audio_amd import drivers
    nm = ec.named()
    bad = nm["henon"][0].copy()
    bad[100] = np.inf
    groups = [np.stack([nm["sine"][0], nm["sine"][0][::-1], nm["white_noise"][0]]),
              np.zeros((0, 250)),
              np.stack([nm["henon"][0], bad, np.full(250, 1.0)]),
              np.stack([np.arange(250.0), nm["henon"][0]]),
              np.stack([bad])]
    wins = np.concatenate(groups)
    seg = np.concatenate([[0], np.cumsum([len(g) for g in groups])])
    for max_lag, n_bins, max_dim, frac_tol in ((None, 16, 5, 0.05), (5, 2, 3, 0.3)):
        out = drivers.embedding_parameters_from_windows(groups, max_lag, n_bins, max_dim, theiler, frac_tol=frac_tol)
        lag = er.resolve_max_lag(250, max_lag)
        assert out.shape == (5, 2 + lag + 1 + max_dim)
        # the delay of a group: the first minimum of its first window, compute_tau's fallback without one, 0 when empty
        first = [er.ami_np(g[0], max_lag, n_bins)["tau"] if len(g) else None for g in groups]
        tau_seg = [0 if f is None else er.fallback_tau(f, 250, max_lag) for f in first]
        assert out[:, 0].tolist() == tau_seg
        want = _group_rows(wins, seg, tau_seg, max_lag, n_bins, max_dim, theiler, frac_tol, ctx)
        # exact values (a NaN is a NaN whatever its sign bit)
        assert np.array_equal(out, want, equal_nan=True), (max_lag, np.argwhere(~((out == want) | (np.isnan(out) & np.isnan(want)))))
        assert np.isnan(out[1, 2:]).all() and out[1, 1] == 0             # the empty group
        assert np.isnan(out[4, 2:]).all() and out[4, 1] == 0             # its only window is not finite
    names = drivers.embedding_names(lag + 1, max_dim)
    assert len(names) == len(drivers.BANDS) * out.shape[1]
