"""The two-sample permutation sums on the corpus shape: n = 1,416 recordings, n_mat = 10 matrices (5 bands x {H0, H1}),
10,000 subject-level relabellings and the observed labelling, in ONE run; HIP events around whole calls, medians of `reps`
calls with their spread:
  kernel        engine.permutation_sums_dev alone (both launches, buffers made once), with the conditional additions per
                second of the definition (one per pair, matrix and relabelling) and of what the kernel issues (two v_add_f64
                per pair, one of them kept) beside the chip's vector float64 addition rate
  torch         the obvious route on the same GPU: S11 = ((U @ Z) * Z).sum(0) and S00 with 1 - Z in float64 through torch, U
                the strict upper triangle and Z the (n, n_perm) 0 / 1 label matrix; S01 = total - S00 - S11.  Its sums are
                in the order of the BLAS, not a written one; the largest difference from the kernel's is reported
  numpy         the same products in numpy on `numpy_perms` relabellings of one matrix, scaled to the whole job
  test          the whole utils.two_sample_permutation_test call on the resident matrices: relabellings drawn, packed and
                uploaded, the kernel, the sums fetched, statistics and p-values (host clock around a call that ends with
                the results on the host)
Writes profiles/permutation_bench.json (or the path given last).
    python tools/permutation_bench.py [n] [n_perm] [reps] [out.json]"""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tda_eeg_audio_amd import _lib, engine, utils      # noqa: E402

N_MAT = 10
FP64_VECTOR_TFLOPS = 78.6        # MI355X data sheet: vector float64, a fused multiply-add counted as two
FP64_VECTOR_TADDS = FP64_VECTOR_TFLOPS / 2


def timed(fn, reps):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(round(a.elapsed_time(b), 4))
    return ts


def summary(ts, **kw):
    return dict(ms_all=ts, ms_median=float(np.median(ts)), ms_min=min(ts), ms_max=max(ts),
                spread=round((max(ts) - min(ts)) / float(np.median(ts)), 4), **kw)


def corpus(n, seed=0):
    """n recordings of n // 24 subjects (24 recordings each, the rest to the last), half of the subjects in each group,
    and N_MAT Euclidean distance matrices of point clouds whose groups differ slightly in one of them."""
    rng = np.random.default_rng(seed)
    n_sub = max(n // 24, 4)
    subjects = np.minimum(np.arange(n) // 24, n_sub - 1)
    y = (subjects % 2).astype(np.uint8)
    D = np.empty((N_MAT, n, n))
    for m in range(N_MAT):
        x = rng.standard_normal((n, 4))
        if m == 0:
            x[y == 1, 0] += 0.25
        D[m] = np.sqrt(((x[:, None, :] - x[None, :, :]) ** 2).sum(-1))
    return D, y, subjects


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 1416
    n_perm = int(sys.argv[2]) if len(sys.argv) > 2 else 10000
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 7
    out_path = sys.argv[4] if len(sys.argv) > 4 else os.path.join(ROOT, "profiles", "permutation_bench.json")
    numpy_perms = 4
    ctx = _lib.get_ctx(0)
    dev = torch.device("cuda", 0)
    D, y, subjects = corpus(n)
    t0 = time.perf_counter()
    lab = utils.subject_permutations(y, subjects, n_perm, seed=42)
    t_draw = time.perf_counter() - t0
    P = lab.shape[0]
    pairs = n * (n - 1) // 2
    res = dict(tool="permutation_bench", lib=os.path.basename(_lib.LIB_PATH), n=n, n_mat=N_MAT, relabellings=P, reps=reps,
               pairs_per_matrix=pairs, conditional_additions=pairs * N_MAT * P, fp64_vector_tadds=FP64_VECTOR_TADDS,
               draw_relabellings_ms=round(1e3 * t_draw, 2))

    D_t = torch.from_numpy(D).to(dev)
    lab_t = torch.from_numpy(engine.pack_labels(lab).view(np.int64)).to(dev)
    out_t = torch.empty((N_MAT, 3, P), dtype=torch.float64, device=dev)
    n1_t = torch.empty(P, dtype=torch.int32, device=dev)
    work_t = torch.empty(_lib.pt_work_doubles(N_MAT, n, P), dtype=torch.float64, device=dev)
    ts = timed(lambda: engine.permutation_sums_dev(D_t, lab_t, out_t, n1_t, ctx=ctx, work_t=work_t), reps)
    ms = float(np.median(ts))
    adds = pairs * N_MAT * P
    res["kernel"] = summary(ts, tadds=round(adds / ms / 1e9, 3), fraction_of_vector_fp64_adds=round(adds / ms / 1e9 / FP64_VECTOR_TADDS, 4),
                            tadds_issued=round(2 * adds / ms / 1e9, 3),
                            fraction_of_vector_fp64_adds_issued=round(2 * adds / ms / 1e9 / FP64_VECTOR_TADDS, 4),
                            work_bytes=int(work_t.numel()) * 8, bytes_read=int(D_t.numel() + lab_t.numel()) * 8)
    sums = out_t.cpu().numpy().copy()
    # the same call again gives the same bytes
    engine.permutation_sums_dev(D_t, lab_t, out_t, n1_t, ctx=ctx, work_t=work_t)
    res["kernel"]["repeatable_bytes"] = bool(out_t.cpu().numpy().tobytes() == sums.tobytes())

    U_t = torch.triu(D_t, 1)
    Z_t = torch.from_numpy(lab.T.astype(np.float64)).to(dev).contiguous()         # (n, P)
    Zc_t = 1.0 - Z_t
    tot_t = U_t.sum(dim=(1, 2))
    tor = torch.empty((N_MAT, 3, P), dtype=torch.float64, device=dev)

    def torch_route():
        for m in range(N_MAT):
            tor[m, 1] = ((U_t[m] @ Z_t) * Z_t).sum(0)
            tor[m, 0] = ((U_t[m] @ Zc_t) * Zc_t).sum(0)
            tor[m, 2] = tot_t[m] - tor[m, 0] - tor[m, 1]
    ts = timed(torch_route, reps)
    diff = float(np.abs(tor.cpu().numpy() - sums).max())
    res["torch"] = summary(ts, max_abs_difference_from_kernel=diff, largest_sum=float(np.abs(sums).max()),
                           gemm_tflops=round(2 * 2.0 * n * n * P * N_MAT / float(np.median(ts)) / 1e9, 3))
    del U_t, Z_t, Zc_t, tor
    torch.cuda.empty_cache()

    U = np.triu(D[0], 1)
    Z = lab[:numpy_perms].T.astype(np.float64)
    t0 = time.perf_counter()
    s11 = ((U @ Z) * Z).sum(0)
    s00 = ((U @ (1.0 - Z)) * (1.0 - Z)).sum(0)
    s01 = U.sum() - s00 - s11
    t_np = time.perf_counter() - t0
    assert np.allclose(np.stack([s00, s11, s01]), sums[0][:, :numpy_perms], rtol=1e-9)
    res["numpy"] = dict(relabellings=numpy_perms, matrices=1, ms=round(1e3 * t_np, 3),
                        ms_scaled_to_job=round(1e3 * t_np * P / numpy_perms * N_MAT, 1))

    def whole():
        return utils.two_sample_permutation_test(D_t, y, subjects, n_permutations=n_perm, seed=42, ctx=ctx)
    whole()
    ts = []
    for _ in range(max(reps // 2, 2)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = whole()
        ts.append(round(1e3 * (time.perf_counter() - t0), 2))
    res["test"] = summary(ts, p=[float(v) for v in r["p"]], p_family=[float(v) for v in r["p_family"]])
    res["speedup_kernel_over_torch"] = round(res["torch"]["ms_median"] / res["kernel"]["ms_median"], 3)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({k: (v["ms_median"] if isinstance(v, dict) and "ms_median" in v else v) for k, v in res.items()
                      if k in ("kernel", "torch", "numpy", "test", "speedup_kernel_over_torch")}))
    print(json.dumps({k: res["kernel"][k] for k in ("tadds", "fraction_of_vector_fp64_adds", "tadds_issued",
                                                    "fraction_of_vector_fp64_adds_issued", "spread", "repeatable_bytes")}))


if __name__ == "__main__":
    main()
