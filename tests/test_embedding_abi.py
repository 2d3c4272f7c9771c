"""
The C ABI of the delay and dimension selection on the built library, and the argument refusals of engine.ami_args and
engine.fnn_args, which hold the limits of the header and refuse before any GPU call.  No GPU: nothing here creates a
context (the C entry points need one to leave their message in; tests/test_gpu_embedding.py::test_refusals calls them with
every bad argument).
"""
import os
import re

import numpy as np
import pytest

from tda_eeg_audio_amd import _lib, drivers, engine, utils

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASES = ("tda_ami_batch", "tda_fnn_batch")


def _header():
    return open(os.path.join(ROOT, "include", "tdaeeg.h")).read()


def _header_args(name):
    m = re.search(r"tda_status\s+" + name + r"\s*\(([^;]*?)\)\s*;", _header(), re.S)
    assert m, name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_symbols_exported_and_bound():
    lib = _lib.load()
    for name in [b + s for b in BASES for s in ("_dev", "")] + ["tda_ami_segments_dev"]:
        assert hasattr(lib, name), name
        res, args = _lib.SYMBOLS[name]
        decl = _header_args(name)
        assert res is _lib.C.c_int and len(args) == len(decl), name
        for a, d in zip(args, decl):                 # double <-> c_double, int <-> c_int, every pointer <-> void*
            want = _lib.c_vp if "*" in d else _lib.C.c_double if d.startswith("double") else _lib.C.c_int
            assert a is want, (name, d)
    for base in BASES:                               # the _dev form takes the host form's arguments and a stream
        assert _header_args(base + "_dev")[:-1] == _header_args(base) and _header_args(base + "_dev")[-1] == "void* stream"
    # the segments form is tda_tau_segments_dev with n_bins behind max_lag
    seg = _header_args("tda_tau_segments_dev")
    k = seg.index("int max_lag") + 1
    assert _header_args("tda_ami_segments_dev") == seg[:k] + ["int n_bins"] + seg[k:]


def test_macros_are_the_headers():
    for macro, const, want in (("TDA_AMI_MAX_SAMPLES", _lib.AMI_MAX_SAMPLES, 8192), ("TDA_AMI_MAX_BINS", _lib.AMI_MAX_BINS, 32),
                               ("TDA_FNN_MAX_SAMPLES", _lib.FNN_MAX_SAMPLES, 2048), ("TDA_FNN_MAX_DIM", _lib.FNN_MAX_DIM, 8),
                               ("TDA_FNN_COLS", _lib.FNN_COLS, 4)):
        m = re.search(r"#define\s+" + macro + r"\s+(\d+)\b", _header())
        assert m and int(m.group(1)) == const == want, macro
    assert len(_lib.FNN_COUNT_NAMES) == _lib.FNN_COLS
    text = _header()
    sec = text[text.index("Delay and dimension selection: mutual information"):text.index("#define TDA_AMI_MAX_SAMPLES")]
    for k, name in enumerate(_lib.FNN_COUNT_NAMES):  # the columns are named in the header's order
        assert re.search(r"\*\s+%d %s\b" % (k, name), sec), name
    # the kernels keep to the determinism the header promises: LDS integer atomics only, in the histogram
    src = open(os.path.join(ROOT, "tda_eeg_audio_amd", "csrc", "embedding.hip")).read()
    code = "\n".join(line.split("//")[0] for line in src.splitlines())
    assert code.count("atomic") == 1 and "atomicAdd(&h[" in code
    assert "embedding.hip" in open(os.path.join(ROOT, "tda_eeg_audio_amd", "csrc", "Makefile")).read()


def test_ami_args():
    assert engine.ami_args(250) == (62, 16) and engine.ami_args(250, 125, 8) == (125, 8)
    assert engine.ami_args(250, -5) == (62, 16) and engine.ami_args(67, 1000, 32) == (65, 32)
    assert engine.ami_args(4, None, 2) == (1, 2) and engine.ami_args(np.int64(8192), np.int32(0)) == (0, 16)
    for n_t in (3, 0, -1, _lib.AMI_MAX_SAMPLES + 1, 250.0, None):
        with pytest.raises(ValueError):
            engine.ami_args(n_t)
    for n_bins in (1, 0, -4, _lib.AMI_MAX_BINS + 1, 16.0, True, None, "16"):
        with pytest.raises(ValueError):
            engine.ami_args(250, None, n_bins)
    for max_lag in (2.0, "3", True):
        with pytest.raises(ValueError):
            engine.ami_args(250, max_lag)


def test_fnn_args():
    assert engine.fnn_args(250) == (5, 1, 10.0, 2.0, 0.05)
    assert engine.fnn_args(2048, 8, 2048, 1, np.float32(0.5), 1) == (8, 2048, 1.0, 0.5, 1.0)
    assert engine.fnn_args(4, 1, 4, 1e-300, 1e300, 0.0) == (1, 4, 1e-300, 1e300, 0.0)
    bad = [dict(n_t=3), dict(n_t=_lib.FNN_MAX_SAMPLES + 1), dict(d_max=0), dict(d_max=_lib.FNN_MAX_DIM + 1), dict(d_max=2.0),
           dict(theiler=0), dict(theiler=251), dict(theiler=-1), dict(theiler=True), dict(r_tol=0.0), dict(r_tol=-1.0),
           dict(r_tol=float("nan")), dict(a_tol=0.0), dict(a_tol=float("nan")), dict(a_tol=None), dict(frac_tol=-1e-9),
           dict(frac_tol=1.0 + 1e-9), dict(frac_tol=float("nan")), dict(frac_tol="0.1")]
    for kw in bad:
        with pytest.raises(ValueError):
            engine.fnn_args(**{"n_t": 250, **kw})


def test_front_ends_refuse_before_any_gpu_call():
    sig = np.sin(np.arange(250) * 0.2)
    with pytest.raises(ValueError):
        engine.ami_batch(sig[None], n_bins=1)
    with pytest.raises(ValueError):
        engine.ami_batch(sig[None, :3])
    with pytest.raises(ValueError):
        engine.ami_batch(sig)
    with pytest.raises(ValueError):
        engine.fnn_batch(sig[None], 7, d_max=9)
    with pytest.raises(ValueError):
        engine.fnn_batch(sig[None], 7, theiler=251)
    with pytest.raises(ValueError):
        engine.fnn_batch(np.zeros((1, 2049)), 7)
    with pytest.raises(ValueError):
        utils.compute_ami(sig, n_bins=33)
    with pytest.raises(ValueError):
        utils.compute_ami(sig[None])
    with pytest.raises(ValueError):
        utils.compute_tau_ami(sig, max_lag=1.5)
    with pytest.raises(ValueError):
        utils.false_nearest_neighbours(sig, 7.0)
    with pytest.raises(ValueError):
        utils.false_nearest_neighbours(sig, 7, max_dim=0)
    with pytest.raises(ValueError):
        utils.estimate_embedding_dimension(sig, 7, frac_tol=2.0)
    with pytest.raises(ValueError):
        drivers.embedding_parameters_from_windows([np.zeros((2, 50)), np.zeros((2, 60))])
    with pytest.raises(ValueError):
        drivers.embedding_parameters_from_windows([np.zeros((2, 50))], n_bins=40)
    with pytest.raises(ValueError):
        drivers.embedding_parameters_from_windows([np.zeros((2, 50))], theiler=1.5)
    with pytest.raises(ValueError):
        drivers.embedding_parameters_from_windows([np.zeros((2, 50))], max_dim=9)
    # groups without a window need no GPU
    out = drivers.embedding_parameters_from_windows([np.zeros((0, 50))] * 2, max_lag=12, max_dim=3)
    assert out.shape == (2, 2 + 13 + 3) and not out[:, :2].any() and np.isnan(out[:, 2:]).all()


def test_embedding_names():
    names = drivers.embedding_names(13, 3, ["alpha", "beta"])
    assert len(names) == 2 * (2 + 13 + 3) == len(set(names))
    assert names[:3] == ["alpha_tau_ami", "alpha_dim_fnn", "alpha_ami_L0"] and names[-1] == "beta_fnn_frac_d3"
    assert len(drivers.embedding_names(63)) == len(drivers.BANDS) * (2 + 63 + 5)
