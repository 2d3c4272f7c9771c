"""
The C ABI of the Euler characteristic curves on the built library, and the argument refusals of engine.euler_args.  No GPU:
nothing here creates a context.
"""
import os
import re

import numpy as np
import pytest

from tda_eeg_audio_amd import _lib, drivers, engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASES = ("tda_euler_dm_batch", "tda_euler_cloud_batch", "tda_euler_takens_batch", "tda_euler_mean")


def _header():
    return open(os.path.join(ROOT, "include", "tdaeeg.h")).read()


def _header_args(name):
    m = re.search(r"tda_status\s+" + name + r"\s*\(([^;]*?)\)\s*;", _header(), re.S)
    assert m, name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_symbols_exported_and_bound():
    lib = _lib.load()
    for base in BASES:
        for name in (base + "_dev", base):
            assert hasattr(lib, name), name
            res, args = _lib.SYMBOLS[name]
            decl = _header_args(name)
            assert res is _lib.C.c_int and len(args) == len(decl), name
            for a, d in zip(args, decl):             # double <-> c_double, int <-> c_int, every pointer <-> void*
                want = _lib.c_vp if "*" in d else _lib.C.c_double if d.startswith("double") else _lib.C.c_int
                assert a is want, (name, d)
        # the _dev form takes the host form's arguments and a stream
        assert _header_args(base + "_dev")[:-1] == _header_args(base) and _header_args(base + "_dev")[-1] == "void* stream"


def test_argument_order_follows_the_rips_entries():
    tail = ["const double* grid", "int n_grid", "int max_dim", "int* counts"]
    assert _header_args("tda_euler_dm_batch")[:6] == _header_args("tda_rips_dm_batch")[:6]
    assert _header_args("tda_euler_dm_batch")[6:] == tail + ["int* status"]
    assert _header_args("tda_euler_cloud_batch")[:8] == _header_args("tda_cloud_rips_batch")[:8]
    assert _header_args("tda_euler_cloud_batch")[8:] == tail + ["int* status"]
    assert _header_args("tda_euler_takens_batch")[:8] == _header_args("tda_takens_rips_batch")[:8]
    assert _header_args("tda_euler_takens_batch")[8:] == tail + ["int* n_points", "int* status"]
    assert [a.split()[-1].lstrip("*") for a in _header_args("tda_euler_mean")] == [
        "ctx", "counts", "n_win", "max_dim", "n_grid", "seg_off", "n_seg", "status_in", "skip_mask", "mean"]


def test_macro_is_the_headers():
    m = re.search(r"#define\s+TDA_EC_MAX_DIM\s+(\d+)\b", _header())
    assert m and int(m.group(1)) == _lib.EC_MAX_DIM == 3


def test_euler_args():
    grid, k = engine.euler_args([0.5, np.nan, 0.1], 3)
    assert grid.dtype == np.float64 and grid.flags["C_CONTIGUOUS"] and grid.shape == (3,) and k == 3 and type(k) is int
    assert engine.euler_args(np.linspace(0, 2, _lib.MAX_GRID), np.int64(1))[1] == 1
    for bad_grid in ([], np.zeros(_lib.MAX_GRID + 1), np.zeros((2, 2)), 1.0, "abc", None):
        with pytest.raises(ValueError):
            engine.euler_args(bad_grid, 3)
    for bad_dim in (0, 4, -1, 2.0, True, None, "2"):
        with pytest.raises(ValueError):
            engine.euler_args([0.0, 1.0], bad_dim)


def test_euler_names():
    names = drivers.euler_names(["alpha", "beta"], 3, np.linspace(0, 2, 7))
    assert len(names) == 2 * 5 * 7 == len(set(names))
    assert names[0] == "alpha_f0_t0" and names[-1] == "beta_chi_t6"
    assert len(drivers.euler_names(max_dim=1)) == len(drivers.BANDS) * 3 * 64
