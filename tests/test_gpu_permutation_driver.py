"""
drivers.two_sample_from_diagrams: the matrix between recordings built on the device by the existing Gram calls and tested
without leaving it, against the same matrix fetched to the host and fed through utils.two_sample_permutation_test.
"""
import numpy as np
import pytest

from tda_eeg_audio_amd import drivers, engine, utils

pytestmark = pytest.mark.gpu

N_REC = 12
Y = np.array([0, 0, 0, 0, 0, 1, 1, 1, 1, 1, 1, 1], np.uint8)
SUBJECTS = np.array(["a", "a", "b", "c", "d", "e", "e", "f", "g", "h", "i", "i"])


def _diagram(rng, shift):
    k = int(rng.integers(3, 9))
    b = rng.uniform(0.0, 0.6, k) + shift
    return np.stack([b, b + rng.uniform(0.05, 0.8, k)], axis=1)


def _recordings(per_rec):
    rng = np.random.default_rng(3)
    recs = [[_diagram(rng, 0.3 * Y[r]) for _ in range(per_rec)] for r in range(N_REC)]
    return recs if per_rec > 1 else [r[0] for r in recs]


def _host_matrix(ctx, dgms, metric):
    import torch
    dev = torch.device("cuda", ctx.device)
    kind, par = metric
    flat = [d for rec in dgms for d in rec] if kind == "kernel" else dgms
    rows, cnt = engine.pack_diagrams(flat)
    rows_t, cnt_t = torch.from_numpy(rows).to(dev), torch.from_numpy(cnt).to(dev)
    if kind == "sliced":
        G = engine.sliced_wasserstein_gram_dev(rows_t, cnt_t, torch.from_numpy(engine._directions(par)).to(dev), ctx=ctx)
    elif kind == "fisher":
        G = engine.persistence_fisher_gram_dev(rows_t, cnt_t, par, ctx=ctx)
    else:
        off = np.concatenate([[0], np.cumsum([len(rec) for rec in dgms])]).astype(np.int32)
        G = engine.diagram_kernel_gram_dev(rows_t, cnt_t, par, seg_off_a=torch.from_numpy(off).to(dev), ctx=ctx)
    return G.cpu().numpy()


@pytest.mark.parametrize("metric", [("sliced", utils.default_directions(16)), ("fisher", 0.5), ("kernel", ("pss", 0.1))],
                         ids=["sliced", "fisher", "kernel"])
def test_driver_equals_the_host_route(ctx, metric):
    dgms = _recordings(3 if metric[0] == "kernel" else 1)
    got = drivers.two_sample_from_diagrams(dgms, Y, subjects=SUBJECTS, metric=metric, n_permutations=199, ctx=ctx)
    G = _host_matrix(ctx, dgms, metric)
    assert G.shape == (N_REC, N_REC) and np.isfinite(G).all()
    name = "mmd" if metric[0] == "kernel" else "joint_loss"
    assert got["statistic"] == name
    want = utils.two_sample_permutation_test(G, Y, subjects=SUBJECTS, n_permutations=199, statistic=name, ctx=ctx)
    for key in ("observed", "null", "p", "p_family", "n1"):
        assert got[key].tobytes() == want[key].tobytes(), key
    assert got["null"].shape == (1, 199) and 1 / 200 <= got["p"][0] <= 1
    # the statistic can be chosen, and an unknown metric is refused
    if metric[0] == "fisher":
        e = drivers.two_sample_from_diagrams(dgms, Y, subjects=SUBJECTS, metric=metric, n_permutations=199, statistic="energy",
                                             ctx=ctx)
        assert e["statistic"] == "energy" and e["observed"].tobytes() == utils.two_sample_permutation_test(
            G, Y, subjects=SUBJECTS, n_permutations=199, statistic="energy", ctx=ctx)["observed"].tobytes()
        with pytest.raises(ValueError):
            drivers.two_sample_from_diagrams(dgms, Y, metric=("euclid", None), ctx=ctx)
