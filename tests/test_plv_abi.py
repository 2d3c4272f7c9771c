"""
The C ABI of the phase-locking value on the built library, and its limits.  No GPU: nothing here creates a context.
"""
import os
import re

from tda_eeg_audio_amd import _lib, engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASE = "tda_plv_dist_batch"


def _header():
    return open(os.path.join(ROOT, "include", "tdaeeg.h")).read()


def _header_args(name):
    m = re.search(r"tda_status\s+" + name + r"\s*\(([^;]*?)\)\s*;", _header(), re.S)
    assert m, name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_symbols_exported_and_bound():
    lib = _lib.load()
    for name in (BASE + "_dev", BASE):
        assert name in _lib.SYMBOLS and hasattr(lib, name), name
        res, args = _lib.SYMBOLS[name]
        decl = _header_args(name)
        assert res is _lib.C.c_int and len(args) == len(decl), name
        for a, d in zip(args, decl):             # double <-> c_double, int <-> c_int, every pointer <-> void*
            want = _lib.c_vp if "*" in d else _lib.C.c_double if d.startswith("double") else _lib.C.c_int
            assert a is want, (name, d)
    # the _dev form takes the host form's arguments and a stream
    assert _header_args(BASE + "_dev")[:-1] == _header_args(BASE) and _header_args(BASE + "_dev")[-1] == "void* stream"
    # the windows are addressed as tda_sublevel_batch addresses its signals
    assert _header_args(BASE)[:7] == _header_args("tda_sublevel_batch")[:7]
    assert [a.split()[-1].lstrip("*") for a in _header_args(BASE)[7:]] == ["g", "method", "dist", "plv", "status"]


def test_limits_are_the_headers():
    text = _header()
    for macro, value in (("TDA_PLV_MAX_CHANNELS", _lib.PLV_MAX_CHANNELS), ("TDA_PLV_MAX_SAMPLES", _lib.PLV_MAX_SAMPLES),
                         ("TDA_WIN_NOT_FINITE", _lib.TDA_WIN_NOT_FINITE)):
        m = re.search(r"#define\s+" + macro + r"\s+(\d+)\b", text)
        assert m and int(m.group(1)) == value, macro
    assert (_lib.PLV_MAX_CHANNELS, _lib.PLV_MAX_SAMPLES) == (64, 256)
    assert "Phase-locking value" in text
    # the methods are correlation_to_distance's, by number
    assert [engine.plv_method(m) for m in engine.METHOD_NAMES] == [0, 1, 2, 3] and engine.plv_method(True) == 0
    assert [engine.DIST_METHODS[m] for m in engine.METHOD_NAMES] == [0, 1, 2, 3]
