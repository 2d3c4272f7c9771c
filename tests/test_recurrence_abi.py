"""
The C ABI of the recurrence curves on the built library, and the argument refusals of engine.recurrence_args.  No GPU:
nothing here creates a context.
"""
import os
import re

import numpy as np
import pytest

from tda_eeg_audio_amd import _lib, drivers, engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASES = ("tda_recurrence_dm_batch", "tda_recurrence_cloud_batch", "tda_recurrence_takens_batch", "tda_recurrence_mean")


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


def test_argument_order_mirrors_the_network_entries():
    """The network signatures with theiler, l_min, v_min after n_grid and hist in place of nodal."""
    def mirrored(args):
        k = args.index("int n_grid") + 1
        return [a.replace("int* nodal", "int* hist").replace("const int* nodal", "const int* hist") for a in
                args[:k] + ["int theiler", "int l_min", "int v_min"] + args[k:]]
    for form in ("dm", "cloud", "takens"):
        assert _header_args(f"tda_recurrence_{form}_batch") == mirrored(_header_args(f"tda_network_{form}_batch")), form
    assert [a.split()[-1].lstrip("*") for a in _header_args("tda_recurrence_mean")] == [
        "ctx", "counts", "measures", "hist", "n_win", "n_grid", "n_hist", "seg_off", "n_seg", "status_in", "skip_mask",
        "mean_counts", "mean_measures", "mean_hist"]
    assert [a.rsplit(" ", 1)[0] for a in _header_args("tda_recurrence_mean")] == \
        [a.rsplit(" ", 1)[0] for a in _header_args("tda_network_mean")]


def test_macros_are_the_headers():
    for macro, const, want in (("TDA_RQA_ROWS", _lib.RQA_ROWS, 7), ("TDA_RQA_MEASURES", _lib.RQA_MEASURES, 7)):
        m = re.search(r"#define\s+" + macro + r"\s+(\d+)\b", _header())
        assert m and int(m.group(1)) == const == want, macro
    assert len(_lib.RQA_COUNT_NAMES) == _lib.RQA_ROWS and len(_lib.RQA_MEASURE_NAMES) == _lib.RQA_MEASURES
    assert _lib.RQA_COUNT_NAMES[0] == "recurrences" and _lib.RQA_COUNT_NAMES[6] == "vert_longest"
    assert _lib.RQA_MEASURE_NAMES[1] == "determinism" and _lib.RQA_MEASURE_NAMES[4] == "laminarity"
    # the rows are named in the header's order
    text = _header()
    sec = text[text.index("Recurrence curves: recurrence quantification"):text.index("#define TDA_RQA_ROWS")]
    for names in (_lib.RQA_COUNT_NAMES, _lib.RQA_MEASURE_NAMES):
        for k, name in enumerate(names):
            assert re.search(r"\*\s+%d %s\b" % (k, name), sec), name


def test_the_key_rule_is_stated_once():
    """The recurrence kernel has no key rule of its own: keys and status words come from rips_keys_dev.h, which lists it."""
    csrc = os.path.join(ROOT, "tda_eeg_audio_amd", "csrc")
    src = open(os.path.join(csrc, "recurrence.hip")).read()
    assert "window_keys<" in src and "win_status(" in src and '#include "rips_keys_dev.h"' in src
    assert "dm_key" not in src and "sqrt" not in src and "KeyFromPts" not in src and "atomic" not in src.lower().replace("no atomics", "")
    assert "csrc/recurrence.hip" in open(os.path.join(csrc, "rips_keys_dev.h")).read()
    assert "recurrence.hip" in open(os.path.join(csrc, "Makefile")).read()


def test_recurrence_args():
    grid, theiler, l_min, v_min = engine.recurrence_args([0.5, np.nan, 0.1])
    assert grid.dtype == np.float64 and grid.flags["C_CONTIGUOUS"] and grid.shape == (3,)
    assert (theiler, l_min, v_min) == (1, 2, 2)
    assert engine.recurrence_args(np.linspace(0, 2, _lib.MAX_GRID), _lib.MAX_POINTS, np.int32(1), _lib.MAX_POINTS)[1:] == \
        (_lib.MAX_POINTS, 1, _lib.MAX_POINTS)
    for bad_grid in ([], np.zeros(_lib.MAX_GRID + 1), np.zeros((2, 2)), 1.0, "abc", None):
        with pytest.raises(ValueError):
            engine.recurrence_args(bad_grid)
    for bad in (0, -1, _lib.MAX_POINTS + 1, 1.0, True, None, "2"):
        for k in range(3):
            par = [1, 2, 2]
            par[k] = bad
            with pytest.raises(ValueError):
                engine.recurrence_args([0.5], *par)
    # the front ends refuse before any GPU call
    with pytest.raises(ValueError):
        engine.recurrence_dm_batch(np.zeros((1, 4, 4)), [0.5], theiler=0)
    with pytest.raises(ValueError):
        engine.recurrence_takens_batch(np.zeros((1, 50)), 3, [], 1)
    with pytest.raises(ValueError):
        drivers.recurrence_curves_from_windows([], [], [0.5], l_min=0)
    with pytest.raises(ValueError):
        drivers.recurrence_curves_from_windows([np.zeros((2, 50))], [], [0.5])
    with pytest.raises(ValueError):
        drivers.recurrence_curves_from_windows([np.zeros((2, 50))], [np.array([3, 4, 5])], [0.5])
    with pytest.raises(ValueError):
        drivers.recurrence_curves_from_windows([np.zeros((2, 50))], [2.5], [0.5])
    # groups without a window need no GPU
    out = drivers.recurrence_curves_from_windows([np.zeros((0, 50))] * 2, [3, 4], [0.5, 0.6])
    assert out.shape == (2, 14, 2) and np.isnan(out).all()
    out, his = drivers.recurrence_curves_from_windows([], [], [0.5], histograms=True)
    assert out.shape == (0, 14, 1) and his.shape == (0, 2, 1, _lib.MAX_POINTS)


def test_recurrence_names():
    names = drivers.recurrence_names(["alpha", "beta"], np.linspace(0, 2, 7))
    assert len(names) == 2 * 14 * 7 == len(set(names))
    assert names[0] == "alpha_recurrences_t0" and names[-1] == "beta_vert_entropy_t6"
    assert len(drivers.recurrence_names()) == len(drivers.BANDS) * (_lib.RQA_ROWS + _lib.RQA_MEASURES) * 64
