"""The CPU oracle's generic branches (any length and max_lag of compute_tau, dim 1..4 and any subsample of the Takens
embedding and the cloud distances) against plain restatements, on the inputs of tests/audio_param_cases.py: what
tests/test_gpu_audio_params.py then holds the kernels against.  No GPU."""
import math

import numpy as np

import audio_param_cases as apc
from oracle import brute, port


def _exact_in_float64(s):
    """Integer samples whose mean is a half-integer and whose lag sums stay below 2^52: centring, every product and every
    partial sum are exact in float64, so the oracle's signs are the true ones whatever the margin."""
    s = np.asarray(s)
    return bool(np.array_equal(s, np.round(s)) and (2.0 * s.sum()) % len(s) == 0 and len(s) * np.abs(s).max() ** 2 < 2.0 ** 52)


def test_oracle_tau_equals_extended_precision_on_every_decided_case():
    """port.compute_tau == tau_longdouble wherever the sign that decides is at least 1e-9 of ac[0] away from zero: double
    rounding of a sum of up to 2048 products is below 1e-12 of ac[0].  Only the constant signals (no variance: every
    autocorrelation is 0) are left out.  A lag sum that is exactly zero (the ramp 0, 1, 2: (-1)(0) + (0)(1)) has no margin
    either, but there float64 is exact and the case is compared all the same.  Every lag chunk of tau_kernel occurs
    among the compared delays."""
    n_cases = compared = 0
    chunks = [0] * len(apc.LAG_CHUNKS)
    for n_t, max_lag, sig in apc.tau_cases():
        for name, s in zip(apc.TAU_SIGNALS, sig):
            n_cases += 1
            tau, margin = apc.tau_longdouble(s, max_lag)
            if margin < 1e-9 and not _exact_in_float64(s):
                assert name == "constant", (n_t, max_lag, name, margin)
                continue
            assert port.compute_tau(s, max_lag) == tau, (n_t, max_lag, name, margin)
            compared += name != "constant"
            chunks[apc.lag_chunk(tau)] += 1
    assert n_cases == 864
    assert compared == n_cases - len(apc.tau_cases()) == 720      # every signal but the 144 constant ones
    assert all(chunks), chunks
    print("compared delays per lag chunk", chunks)


def test_oracle_takens_is_the_index_rule():
    for dim, sub, n_t, tau, wins in apc.takens_cases():
        n = n_t - (dim - 1) * tau
        for s in wins:
            pc = port.takens(s, dim, tau, sub)
            assert np.array_equal(pc, apc.takens_cloud(s, dim, tau, sub)), (dim, sub, n_t, tau)
            assert len(pc) == math.ceil(n / sub) == apc.takens_points(n_t, dim, tau, sub)
    m = apc.MIXED_TAU
    got = tuple(apc.takens_points(m["n_t"], m["dim"], t, m["subsample"]) if t else m["n_t"] for t in m["tau"])
    assert got == apc.MIXED_P


def test_oracle_cloud_distances_within_1e7_of_extended_precision():
    """Components of a normalised cloud lie in [0, 1], so |x|^2 <= 4: the three roundings of |x|^2 - 2 x.y + |y|^2 leave a
    few 1e-15 in d^2, at most ~6e-8 in d where d is about 0 -- 1e-7 absolute for dim 1..4."""
    clouds = [(dim, pc) for _, dim, _, pc in apc.cloud_cases()]
    clouds += [(dim, apc.takens_cloud(s, dim, tau, sub)) for dim, sub, _, tau, wins in apc.takens_cases() for s in wins]
    assert {d for d, _ in clouds} == {1, 2, 3, 4}
    for dim, pc in clouds:
        x = port.minmax_normalise(pc)
        assert x.min() >= 0.0 and x.max() <= 1.0
        xl = x.astype(np.longdouble)
        ref = np.sqrt(((xl[:, None, :] - xl[None, :, :]) ** 2).sum(-1))
        assert np.abs(port.cloud_dm(x).astype(np.longdouble) - ref).max() <= 1e-7, (dim, len(pc))


def test_oracle_audio_persistence_equals_brute_force_on_small_clouds():
    n = 0
    for dim, sub, n_t, tau, wins in apc.takens_cases():
        if apc.takens_points(n_t, dim, tau, sub) > apc.BRUTE_P:
            continue
        n += 1
        for s in wins:
            (o0, o1), P = port.audio_persistence(s, tau, dim, sub)
            dm = port.cloud_dm(port.minmax_normalise(port.takens(s, dim, tau, sub))).astype(np.float32)
            b = brute.rips_brute(dm.astype(np.float64), 2.0)
            assert np.array_equal(brute.sort_rows(o1), brute.sort_rows(b[1])), (dim, sub, n_t, tau)
    assert n == 3
