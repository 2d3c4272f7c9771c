"""
The permutation-sums kernel against the written order of include/tdaeeg.h ("Two-sample permutation sums") as
tests/permutation_ref.py evaluates it: bit for bit, at every size at which the kernel takes another path (the row block
R = TDA_PT_ROW_BLOCK = 64: R - 1, R, R + 1, 2R + 1 are 63, 64, 65, 129; the eight-entry inner step; partial and several
label words; more than one wave and workgroup), and the test built on it end to end.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import permutation_ref as ref
from tda_eeg_audio_amd import _lib, engine, utils

pytestmark = pytest.mark.gpu

FILL = -7.25
SIZES = [2, 3, 63, 64, 65, 129]
PERMS = [1, 63, 64, 65, 257]
assert ref.ROW_BLOCK == _lib.PT_ROW_BLOCK == 64


def _dev(ctx):
    import torch
    return torch.device("cuda", ctx.device)


def _labels(P, n, seed):
    """Random labellings; the last rows (as far as P allows) are all 0, all 1, alternating and a single 1."""
    lab = (np.random.default_rng(seed).random((P, n)) < 0.45).astype(np.uint8)
    single = np.zeros(n, np.uint8)
    single[n // 2] = 1
    for k, s in enumerate((np.zeros(n, np.uint8), np.ones(n, np.uint8), (np.arange(n) & 1).astype(np.uint8), single)):
        if k + 1 < P:
            lab[P - 1 - k] = s
    return lab


@functools.lru_cache(maxsize=None)
def _case(n, P, n_mat):
    """(D with ld = n + 3, everything outside the strict upper triangle NaN; labels; the reference's sums and n1)."""
    rng = np.random.default_rng(1000 * n + 10 * P + n_mat)
    D = np.full((n_mat, n, n + 3), np.nan)
    iu = np.triu_indices(n, 1)
    D[:, iu[0], iu[1]] = rng.uniform(-1.0, 3.0, (n_mat, len(iu[0])))
    lab = _labels(P, n, seed=n + P)
    sums, n1 = ref.perm_sums(D, lab)
    for a in (D, lab, sums, n1):
        a.setflags(write=False)
    return D, lab, sums, n1


def _run(D, lab, ctx, n_perm=None):
    """permutation_sums_dev into pre-filled buffers."""
    import torch
    dev = _dev(ctx)
    P = lab.shape[0] if n_perm is None else n_perm
    D_t = torch.from_numpy(np.array(D)).to(dev)
    lab_t = torch.from_numpy(engine.pack_labels(lab).view(np.int64)).to(dev)
    out = torch.full((D.shape[0], 3, P), FILL, dtype=torch.float64, device=dev)
    n1 = torch.full((P,), -5, dtype=torch.int32, device=dev)
    engine.permutation_sums_dev(D_t, lab_t, out_t=out, n1_t=n1, ctx=ctx)
    torch.cuda.synchronize()
    return out.cpu().numpy(), n1.cpu().numpy()


@pytest.mark.parametrize("n_mat", [1, 3])
@pytest.mark.parametrize("P", PERMS)
@pytest.mark.parametrize("n", SIZES)
def test_bytes_of_the_written_order(ctx, n, P, n_mat):
    D, lab, want, want_n1 = _case(n, P, n_mat)
    got, n1 = _run(D, lab, ctx)
    assert np.isfinite(got).all()                        # the diagonal, the lower triangle and the padding are NaN
    assert got.tobytes() == want.tobytes()
    assert np.array_equal(n1, want_n1)
    host, host_n1 = engine.permutation_sums_batch(D, lab, ctx=ctx)
    assert host.tobytes() == want.tobytes() and np.array_equal(host_n1, want_n1)


def test_a_relabelling_alone_and_a_matrix_alone(ctx):
    D, lab, want, want_n1 = _case(129, 257, 3)
    for k in (0, 64, 200, 256):
        got, n1 = _run(D, lab[k:k + 1], ctx)
        assert got.tobytes() == want[:, :, k:k + 1].tobytes() and n1[0] == want_n1[k]
    got, _ = _run(D, lab[190:], ctx)                     # another place in the batch, another lane and word
    assert got.tobytes() == want[:, :, 190:].tobytes()
    for m in range(3):
        got, _ = _run(D[m:m + 1], lab, ctx)
        assert got.tobytes() == want[m:m + 1].tobytes()
    # fewer relabellings than the packed words hold: the rest is not computed into the outputs
    got, n1 = _run(D, lab, ctx, n_perm=70)
    assert got.tobytes() == want[:, :, :70].tobytes() and np.array_equal(n1, want_n1[:70])
    # the host form without n1, and with n1 alone (no matrix)
    p, d, packed = engine.ptr, engine.f64(D), engine.pack_labels(lab)
    out, n1 = np.empty((3, 3, 257)), np.empty(257, np.int32)
    ctx.check(ctx.lib.tda_perm_sums_batch(ctx.h, p(d), 3, 129, d.shape[2], p(packed), 257, p(out), None))
    ctx.check(ctx.lib.tda_perm_sums_batch(ctx.h, None, 0, 129, 129, p(packed), 257, None, p(n1)))
    assert out.tobytes() == want.tobytes() and np.array_equal(n1, want_n1)


def test_complement_swaps_the_within_sums(ctx):
    D, lab, want, want_n1 = _case(129, 65, 3)
    got, n1 = _run(D, 1 - lab, ctx)
    assert got[:, 0].tobytes() == want[:, 1].tobytes() and got[:, 1].tobytes() == want[:, 0].tobytes()
    assert got[:, 2].tobytes() == want[:, 2].tobytes() and np.array_equal(n1, 129 - want_n1)


@pytest.mark.parametrize("ij", [(0, 1), (10, 64), (63, 64), (64, 128), (127, 128), (5, 9)])
def test_one_nan_reaches_the_sums_of_its_class_only(ctx, ij):
    D, lab, want, _ = _case(129, 65, 1)
    i, j = ij
    D = np.array(D)
    D[0, i, j] = np.nan
    got, _ = _run(D, lab, ctx)
    cls = np.where(lab[:, i] != lab[:, j], 2, lab[:, i])           # the sum that holds the pair: S00 0, S11 1, S01 2
    hit = np.arange(3)[:, None] == cls[None, :]
    assert np.array_equal(np.isnan(got[0]), hit)
    assert got[0][~hit].tobytes() == want[0][~hit].tobytes()
    inf = np.array(D)
    inf[0, i, j] = np.inf
    got, _ = _run(inf, lab, ctx)
    assert np.array_equal(np.isinf(got[0]), hit) and got[0][~hit].tobytes() == want[0][~hit].tobytes()


def test_accuracy_against_exactly_rounded_sums(ctx):
    D, lab, _, _ = _case(129, 65, 1)
    got, _ = _run(D, lab, ctx)
    exact, terms, mass = ref.perm_sums_fsum(np.nan_to_num(np.array(D)), lab)
    bound = terms[None] * 2.0 ** -53 * mass               # m * 2^-53 * sum |d|
    err = np.abs(got - exact)
    assert (err[bound == 0] == 0).all()
    q = float((err[bound > 0] / bound[bound > 0]).max())
    print(f"q = max |gpu - fsum| / (m 2^-53 sum|d|) = {q:.3e}")
    assert q <= 1.0


def _call_dev(ctx, n_mat, n, ld, n_perm, work_doubles=None):
    """tda_perm_sums_batch_dev with pre-filled buffers sized for a small valid call; returns (status, message, untouched)."""
    import torch
    dev = _dev(ctx)
    D = torch.zeros(4096, dtype=torch.float64, device=dev)
    lab = torch.zeros(4096, dtype=torch.int64, device=dev)
    work = torch.full((4096,), FILL, dtype=torch.float64, device=dev)
    out = torch.full((4096,), FILL, dtype=torch.float64, device=dev)
    n1 = torch.full((4096,), -5, dtype=torch.int32, device=dev)
    tp = lambda t: C.c_void_p(t.data_ptr())
    rc = ctx.lib.tda_perm_sums_batch_dev(ctx.h, tp(D), n_mat, n, ld, tp(lab), n_perm, tp(work),
                                         4096 if work_doubles is None else work_doubles, tp(out), tp(n1), None)
    torch.cuda.synchronize()
    buf = C.create_string_buffer(512)
    ctx.lib.tda_last_error(ctx.h, buf, 512)
    untouched = bool((out == FILL).all() and (n1 == -5).all() and (work == FILL).all())
    return rc, buf.value.decode(), untouched


@pytest.mark.parametrize("args, word", [((1, 1, 1, 4), "TDA_PT_MAX_ITEMS"), ((1, _lib.PT_MAX_ITEMS + 1, _lib.PT_MAX_ITEMS + 1, 4),
                                                                              "TDA_PT_MAX_ITEMS"),
                                        ((1, 8, 8, 0), "TDA_PT_MAX_PERM"), ((1, 8, 8, _lib.PT_MAX_PERM + 1), "TDA_PT_MAX_PERM"),
                                        ((1, 8, 7, 4), "ld"), ((_lib.PT_MAX_MATRICES + 1, 8, 8, 4), "TDA_PT_MAX_MATRICES")])
def test_limits_are_errors_and_write_nothing(ctx, args, word):
    rc, msg, untouched = _call_dev(ctx, *args)
    assert rc == 1 and word in msg and untouched
    n_mat, n, ld, n_perm = args
    if n <= 8 and n_mat == 1:                             # the host form: the same refusal before anything is staged
        out, n1 = np.full((1, 3, 8), FILL), np.full(8, -5, np.int32)
        rc = ctx.lib.tda_perm_sums_batch(ctx.h, _lib.ptr(np.zeros((1, 8, 8))), n_mat, n, ld, _lib.ptr(np.zeros((1, 8), np.uint64)),
                                         n_perm, _lib.ptr(out), _lib.ptr(n1))
        assert rc == 1 and (out == FILL).all() and (n1 == -5).all()


def test_small_work_space_is_an_error(ctx):
    rc, msg, untouched = _call_dev(ctx, 1, 8, 8, 4, work_doubles=_lib.pt_work_doubles(1, 8, 4) - 1)
    assert rc == 1 and "TDA_PT_WORK_DOUBLES" in msg and untouched
    rc, _, untouched = _call_dev(ctx, 1, 8, 8, 4, work_doubles=_lib.pt_work_doubles(1, 8, 4))
    assert rc == 0 and not untouched
    with pytest.raises(_lib.TdaError):
        engine.permutation_sums_batch(np.zeros((1, 1, 1)), np.zeros((3, 1), np.uint8), ctx=ctx)
    with pytest.raises(_lib.TdaError):
        engine.permutation_sums_batch(np.zeros((1, 5, 5)), np.zeros((0, 5), np.uint8), ctx=ctx)


@functools.lru_cache(maxsize=None)
def _forty():
    """Three 40 x 40 matrices (two clusters 17 + 23, noise, the clusters squared) and 1 + 999 labellings."""
    D, y = ref.two_clusters(17, 23, seed=6, gap=3.0)
    noise = np.random.default_rng(7).uniform(1.0, 2.0, (40, 40))
    stack = np.stack([D, noise, D ** 2])
    lab = utils.subject_permutations(y, None, n_permutations=999, seed=42)
    return stack, y, lab


def _same_dict(got, want):
    for key in ("observed", "null", "p", "p_family"):
        assert got[key].shape == want[key].shape and got[key].tobytes() == want[key].tobytes(), key


@pytest.mark.parametrize("name", ["joint_loss", "energy", "mmd"])
def test_two_sample_permutation_test_end_to_end(ctx, name):
    import torch
    stack, y, lab = _forty()
    D = np.exp(-stack) if name == "mmd" else stack
    want = ref.permutation_test(D, lab, name)
    got = utils.two_sample_permutation_test(D, y, n_permutations=999, statistic=name, seed=42, ctx=ctx)
    _same_dict(got, want)
    assert got["null"].shape == (3, 999) and np.array_equal(got["n1"], np.full(1000, 23))
    assert got["p"][0] <= 0.01 and got["p"][1] > 0.01 and (got["p_family"] >= got["p"]).all()
    # the matrices on the device, the labellings handed in: the same dict
    dev_got = utils.two_sample_permutation_test(torch.from_numpy(D).to(_dev(ctx)), y, statistic=name, labels=lab, ctx=ctx)
    _same_dict(dev_got, want)
    # one 2-D matrix is one matrix, and its family-wise value is its own
    one = utils.two_sample_permutation_test(D[0], y, n_permutations=999, statistic=name, ctx=ctx)
    _same_dict(one, ref.permutation_test(D[0], lab, name))
    assert one["p"].shape == (1,) and one["p"].tobytes() == one["p_family"].tobytes() == got["p"][:1].tobytes()


def test_a_non_finite_matrix_has_nan_p(ctx):
    stack, y, lab = _forty()
    D = np.array(stack)
    D[1, 3, 30] = np.nan                                  # a between-group pair: the joint loss of y itself never sees it
    got = utils.two_sample_permutation_test(D, y, n_permutations=999, ctx=ctx)
    _same_dict(got, ref.permutation_test(D, lab, "joint_loss"))
    assert np.isfinite(got["observed"]).all() and np.isnan(got["p"][1]) and np.isnan(got["p_family"][1])
    assert np.isfinite(got["p"][[0, 2]]).all() and np.isfinite(got["p_family"][[0, 2]]).all()
    D[1] = np.tril(np.full((40, 40), np.nan)) + np.triu(stack[1], 1)     # NaN outside the upper triangle: not read
    clean = utils.two_sample_permutation_test(D, y, n_permutations=999, ctx=ctx)
    _same_dict(clean, ref.permutation_test(stack, lab, "joint_loss"))
