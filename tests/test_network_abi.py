"""
The C ABI of the network curves on the built library, and the argument refusals of engine.network_args.  No GPU: nothing
here creates a context.
"""
import os
import re

import numpy as np
import pytest

from tda_eeg_audio_amd import _lib, drivers, engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASES = ("tda_network_dm_batch", "tda_network_cloud_batch", "tda_network_takens_batch", "tda_network_mean")


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
    tail = ["const double* grid", "int n_grid", "int* counts", "double* measures", "int* nodal"]
    assert _header_args("tda_network_dm_batch")[:6] == _header_args("tda_rips_dm_batch")[:6]
    assert _header_args("tda_network_dm_batch")[6:] == tail + ["int* status"]
    assert _header_args("tda_network_cloud_batch")[:8] == _header_args("tda_cloud_rips_batch")[:8]
    assert _header_args("tda_network_cloud_batch")[8:] == tail + ["int* status"]
    assert _header_args("tda_network_takens_batch")[:8] == _header_args("tda_takens_rips_batch")[:8]
    assert _header_args("tda_network_takens_batch")[8:] == tail + ["int* n_points", "int* status"]
    # ... and the Euler entries', up to max_dim
    for form, k in (("dm", 8), ("cloud", 10), ("takens", 10)):
        assert _header_args(f"tda_network_{form}_batch")[:k] == _header_args(f"tda_euler_{form}_batch")[:k]
    assert [a.split()[-1].lstrip("*") for a in _header_args("tda_network_mean")] == [
        "ctx", "counts", "measures", "nodal", "n_win", "n_grid", "n_node", "seg_off", "n_seg", "status_in", "skip_mask",
        "mean_counts", "mean_measures", "mean_nodal"]


def test_macros_are_the_headers():
    for macro, const, want in (("TDA_NET_ROWS", _lib.NET_ROWS, 10), ("TDA_NET_MEASURES", _lib.NET_MEASURES, 4),
                               ("TDA_NET_NODAL", _lib.NET_NODAL, 5)):
        m = re.search(r"#define\s+" + macro + r"\s+(\d+)\b", _header())
        assert m and int(m.group(1)) == const == want, macro
    assert len(_lib.NET_COUNT_NAMES) == _lib.NET_ROWS and len(_lib.NET_MEASURE_NAMES) == _lib.NET_MEASURES
    assert len(_lib.NET_NODAL_NAMES) == _lib.NET_NODAL
    assert _lib.NET_COUNT_NAMES[0] == "edges" and _lib.NET_COUNT_NAMES[9] == "diameter"
    # the rows are named in the header's order
    text = _header()
    sec = text[text.index("Network curves: graph measures"):text.index("#define TDA_NET_ROWS")]
    for names in (_lib.NET_COUNT_NAMES, _lib.NET_MEASURE_NAMES):
        for k, name in enumerate(names):
            assert re.search(r"\*\s+%d %s\b" % (k, name), sec), name


def test_the_key_rule_is_stated_once():
    """The network kernel has no key rule of its own: keys and status words come from rips_keys_dev.h."""
    src = open(os.path.join(ROOT, "tda_eeg_audio_amd", "csrc", "network.hip")).read()
    assert "window_keys<" in src and "win_status(" in src and '#include "rips_keys_dev.h"' in src
    assert "dm_key" not in src and "sqrt" not in src and "KeyFromPts" not in src


def test_network_args():
    grid = engine.network_args([0.5, np.nan, 0.1])
    assert grid.dtype == np.float64 and grid.flags["C_CONTIGUOUS"] and grid.shape == (3,)
    assert engine.network_args(np.linspace(0, 2, _lib.MAX_GRID)).shape == (_lib.MAX_GRID,)
    for bad_grid in ([], np.zeros(_lib.MAX_GRID + 1), np.zeros((2, 2)), 1.0, "abc", None):
        with pytest.raises(ValueError):
            engine.network_args(bad_grid)
    with pytest.raises(ValueError):
        drivers.connectivity_network_curves_from_windows([], "granger", [0.5])
    with pytest.raises(ValueError):
        drivers.connectivity_network_curves_from_windows([], "pearson", [0.5], method="angular")
    with pytest.raises(ValueError):
        drivers.connectivity_network_curves_from_windows([], "coh", [])


def test_network_names():
    names = drivers.network_names(["alpha", "beta"], np.linspace(0, 2, 7))
    assert len(names) == 2 * 14 * 7 == len(set(names))
    assert names[0] == "alpha_edges_t0" and names[-1] == "beta_path_length_t6"
    assert len(drivers.network_names()) == len(drivers.BANDS) * (_lib.NET_ROWS + _lib.NET_MEASURES) * 64
