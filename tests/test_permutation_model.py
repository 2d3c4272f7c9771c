"""
The two-sample permutation test without a GPU: the written order of the sums (tests/permutation_ref.py) against exactly
rounded sums, the relabellings, the statistics and the p-values.  The kernel is held against the same reference, bit for
bit, in tests/test_gpu_permutation.py.
"""
import numpy as np
import pytest

import permutation_ref as ref
from tda_eeg_audio_amd import utils

STATS = ("joint_loss", "energy", "mmd")


def _matrix(n, n_mat=1, seed=0, ld=None):
    rng = np.random.default_rng(seed)
    d = rng.uniform(-1.0, 3.0, (n_mat, n, ld or n))
    return d


def _labels(P, n, seed=1):
    return (np.random.default_rng(seed).random((P, n)) < 0.4).astype(np.uint8)


@pytest.mark.parametrize("n", [2, 3, 63, 65, 129])
def test_written_order_within_the_bound_of_any_order(n):
    D, lab = _matrix(n, 2, seed=n), _labels(9, n, seed=n + 1)
    lab[0], lab[1] = 0, 1
    got, n1 = ref.perm_sums(D, lab)
    exact, terms, mass = ref.perm_sums_fsum(D, lab)
    assert np.array_equal(n1, lab.sum(axis=1))
    assert terms.sum(axis=0).tolist() == [n * (n - 1) // 2] * lab.shape[0]
    bound = terms[None] * 2.0 ** -53 * mass               # m * 2^-53 * sum |d|: any summation order of m terms
    assert (np.abs(got - exact) <= bound).all()
    assert (got[:, 1:, 0] == 0).all() and (got[:, [0, 2], 1] == 0).all()      # all 0: only S00; all 1: only S11


def test_row_block_changes_the_order_not_the_sets():
    D, lab = _matrix(70, 1, seed=3), _labels(5, 70, seed=4)
    a, _ = ref.perm_sums(D, lab)
    b, _ = ref.perm_sums(D, lab, row_block=7)
    exact, terms, mass = ref.perm_sums_fsum(D, lab)
    assert not np.array_equal(a, b)                        # the block size is part of the written order
    assert (np.abs(b - exact) <= terms[None] * 2.0 ** -53 * mass).all()


def test_leading_dimension_and_lower_triangle_are_not_read():
    D, lab = _matrix(20, 2, seed=5, ld=27), _labels(6, 20, seed=6)
    want, _ = ref.perm_sums(D, lab)
    D2 = D.copy()
    D2[:, :, 20:] = np.nan
    il = np.tril_indices(20)
    D2[:, il[0], il[1]] = np.nan
    got, _ = ref.perm_sums(D2, lab)
    assert np.array_equal(got, want)


def test_subject_permutations_are_the_helpers_draws():
    rng0 = np.random.default_rng(7)
    subjects = np.array([f"s{rng0.integers(0, 9):02d}" for _ in range(40)])
    per_subject = {s: int(rng0.integers(0, 2)) for s in np.unique(subjects)}
    y = np.array([per_subject[s] for s in subjects], dtype=np.int64)
    got = utils.subject_permutations(y, subjects, n_permutations=25, seed=11)
    assert got.shape == (26, 40) and got.dtype == np.uint8 and np.array_equal(got[0], y)
    rng = np.random.default_rng(11)
    for k in range(1, 26):
        assert np.array_equal(got[k], utils.permute_labels_by_subject(y, subjects, rng)), k
    # the helper itself, against the plain statement of what it does: the sorted subjects' labels, shuffled by ONE
    # rng.permutation call, handed back to every recording of the subject
    rng_a, rng_b = np.random.default_rng(5), np.random.default_rng(5)
    for _ in range(4):
        names = sorted(set(subjects))
        shuffled = rng_b.permutation(np.array([y[list(subjects).index(s)] for s in names]))
        want = np.array([shuffled[names.index(s)] for s in subjects], dtype=y.dtype)
        out = utils.permute_labels_by_subject(y, subjects, rng_a)
        assert out.dtype == y.dtype and np.array_equal(out, want)
    # without subjects: rng.permutation(y) per row
    got = utils.subject_permutations(y, None, n_permutations=8, seed=3)
    rng = np.random.default_rng(3)
    assert all(np.array_equal(got[k], rng.permutation(y)) for k in range(1, 9))
    assert (got.sum(axis=1) == y.sum()).all()


def test_two_clusters_exhaustive_p_is_two_in_seventy():
    D, y = ref.two_clusters(4, 4, seed=2)
    lab = ref.all_labellings(8, 4)
    assert lab.shape == (70, 8)
    sums, n1 = ref.perm_sums(D[None], lab)
    t = utils.two_sample_statistic(sums, n1, 8, "joint_loss")[0]
    obs = int(np.flatnonzero((lab == y).all(axis=1))[0])
    comp = int(np.flatnonzero((lab == 1 - y).all(axis=1))[0])
    assert t[obs].tobytes() == t[comp].tobytes()
    others = np.delete(t, [obs, comp])
    assert (others > t[obs]).all()                         # the strict minimum, shared with the complement only
    assert int((t <= t[obs]).sum()) == 2                   # exact p = 2 / 70
    e = utils.two_sample_statistic(sums, n1, 8, "energy")[0]
    assert int((e >= e[obs]).sum()) == 2


@pytest.mark.parametrize("name", STATS)
def test_complement_gives_the_same_bytes(name):
    D, lab = _matrix(67, 2, seed=8), _labels(12, 67, seed=9)
    a, n1a = ref.perm_sums(D, lab)
    b, n1b = ref.perm_sums(D, 1 - lab)
    assert a[:, 0].tobytes() == b[:, 1].tobytes() and a[:, 1].tobytes() == b[:, 0].tobytes()
    assert a[:, 2].tobytes() == b[:, 2].tobytes() and np.array_equal(n1a + n1b, np.full(12, 67))
    ta, tb = utils.two_sample_statistic(a, n1a, 67, name), utils.two_sample_statistic(b, n1b, 67, name)
    assert ta.tobytes() == tb.tobytes()


def test_statistics_are_the_references_and_energy_is_minus_mmd():
    D, lab = _matrix(31, 3, seed=10), _labels(40, 31, seed=12)
    sums, n1 = ref.perm_sums(D, lab)
    for name in STATS:
        assert utils.two_sample_statistic(sums, n1, 31, name).tobytes() == ref.statistic(sums, n1, 31, name).tobytes()
    e, k = utils.two_sample_statistic(sums, n1, 31, "energy"), utils.two_sample_statistic(sums, n1, 31, "mmd")
    assert np.array_equal(e, -k) and np.isfinite(e).all()
    with pytest.raises(ValueError):
        utils.two_sample_statistic(sums, n1, 31, "t")


def test_a_group_of_one_is_nan():
    D = _matrix(6, 1, seed=13)
    lab = np.array([[1, 0, 0, 0, 0, 0], [1, 1, 1, 1, 1, 0], [0, 0, 0, 0, 0, 0], [1, 1, 0, 0, 0, 0]], np.uint8)
    sums, n1 = ref.perm_sums(D, lab)
    for name in STATS:
        t = utils.two_sample_statistic(sums, n1, 6, name)[0]
        assert np.isnan(t[:3]).all() and np.isfinite(t[3])


@pytest.mark.parametrize("name", STATS)
def test_p_values(name):
    D, y = ref.two_clusters(10, 12, seed=4, gap=1.5)
    D = np.stack([D, _matrix(22, 1, seed=14)[0] + 2.0, D ** 2])
    if name == "mmd":
        D = np.exp(-D)
    lab = utils.subject_permutations(y, None, n_permutations=199, seed=5)
    sums, n1 = ref.perm_sums(D, lab)
    stat = utils.two_sample_statistic(sums, n1, 22, name)
    p, pf = utils.permutation_p_values(stat, np.ones(3, bool), name)
    rp, rpf = ref.p_values(stat, np.ones(3, bool), name)
    assert p.tobytes() == rp.tobytes() and pf.tobytes() == rpf.tobytes()
    assert ((p >= 1 / 200) & (p <= 1)).all() and ((pf >= 1 / 200) & (pf <= 1)).all()
    assert (pf >= p).all()                                  # the family-wise value never beats the matrix' own
    assert p[0] < 0.05 < p[1]                               # clusters against noise
    for m in range(3):                                      # one matrix: the correction has nothing to correct
        p1, pf1 = utils.permutation_p_values(stat[m:m + 1], np.ones(1, bool), name)
        assert p1.tobytes() == pf1.tobytes() == p[m:m + 1].tobytes()
    # a matrix marked non-finite has NaN and leaves the family
    p2, pf2 = utils.permutation_p_values(stat, np.array([True, False, True]), name)
    assert np.isnan(p2[1]) and np.isnan(pf2[1]) and p2[0] == p[0] and pf2[0] <= pf[0]
