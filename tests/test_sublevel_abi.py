"""
The C ABI of the sublevel-set persistence on the built library, and the place of its step output.  No GPU: nothing here
creates a context.
"""
import os
import re

from tda_eeg_audio_amd import _lib, pipeline

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASE = "tda_sublevel_batch"


def _header():
    return open(os.path.join(ROOT, "include", "tdaeeg.h")).read()


def _header_args(name):
    m = re.search(r"tda_status\s+" + name + r"\s*\(([^;]*?)\)\s*;", _header(), re.S)
    assert m, name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_symbols_exported_and_bound():
    lib = _lib.load()
    for name in (BASE + "_dev", BASE):
        assert hasattr(lib, name), name
        res, args = _lib.SYMBOLS[name]
        decl = _header_args(name)
        assert res is _lib.C.c_int and len(args) == len(decl), name
        for a, d in zip(args, decl):             # double <-> c_double, int <-> c_int, every pointer <-> void*
            want = _lib.c_vp if "*" in d else _lib.C.c_double if d.startswith("double") else _lib.C.c_int
            assert a is want, (name, d)
    # the _dev form takes the host form's arguments and a stream
    assert _header_args(BASE + "_dev")[:-1] == _header_args(BASE) and _header_args(BASE + "_dev")[-1] == "void* stream"
    # the signals are addressed by the tables of tda_eeg_window_ragged_dev, in its order
    assert _header_args(BASE)[:7] == _header_args("tda_eeg_window_ragged_dev")[:6] + ["int n_t"]
    assert [a.split()[-1].lstrip("*") for a in _header_args(BASE)[7:]] == ["dgm", "cap", "cnt", "idx", "status"]


def test_macros_are_the_headers():
    text = _header()
    for macro, value in (("TDA_SL_MAX_SAMPLES", _lib.SL_MAX_SAMPLES), ("TDA_WIN_NOT_FINITE", _lib.TDA_WIN_NOT_FINITE)):
        m = re.search(r"#define\s+" + macro + r"\s+(\d+)\b", text)
        assert m and int(m.group(1)) == value, macro
    assert _lib.SL_MAX_SAMPLES == 4096 and _lib.TDA_WIN_NOT_FINITE == 64
    assert re.search(r"#define\s+TDA_SL_ROWS\(n\)\s+\(\(\(n\)\s*\+\s*1\)\s*/\s*2\)", text)
    from tda_eeg_audio_amd import engine
    assert [engine.sublevel_rows(n) for n in (1, 2, 3, 250, 4096)] == [1, 1, 2, 125, 2048]
    # the new status bit is no other one's
    bits = [int(v) for v in re.findall(r"#define\s+TDA_WIN_[A-Z0-9_]+\s+(\d+)\b", text)]
    assert len(bits) == len(set(bits)) and 64 in bits


def test_step_output_sl():
    only = pipeline.step_outputs(sublevel=True)
    assert [o.name for o in only] == ["sl"] and only[0].shape == (22,) and pipeline.SL_COLS == 22
    assert pipeline.step_outputs() == [] and pipeline.step_outputs(sublevel=False) == []
    import numpy as np
    every = pipeline.step_outputs(correlations=True, bottleneck=True, landscapes=(np.linspace(0, 1, 4), 2),
                                  images=(np.linspace(0, 1, 3), np.linspace(0, 1, 3), 0.1, 1), sliced=np.eye(2),
                                  wasserstein_q=(2, "l2"), frechet=(8, 4), kernel_distance=("pss", 0.5), fisher=0.5,
                                  sublevel=True)
    assert [o.name for o in every] == ["corr", "bott", "land", "img", "slc", "wq", "fm", "kd", "pf", "sl"]
    assert every[-1].shape == (22,)
