"""
The C ABI of the analytic-signal connectivity on the built library, its constants and measure numbers.  No GPU: nothing
here creates a context.
"""
import os
import re

from tda_eeg_audio_amd import _lib, engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASE = "tda_connectivity_dist_batch"


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
    # the arguments of tda_plv_dist_batch, `measure` in front of `method`, the value matrix where the plv matrix is
    plv = [a.split()[-1].lstrip("*") for a in _header_args("tda_plv_dist_batch")]
    assert plv == ["ctx", "sig", "win_start", "win_ld", "n_win", "n_ch", "n_t", "g", "method", "dist", "plv", "status"]
    want = plv[:8] + ["measure"] + plv[8:10] + ["value"] + plv[11:]
    assert [a.split()[-1].lstrip("*") for a in _header_args(BASE)] == want
    types = lambda name: [a.rsplit(" ", 1)[0] for a in _header_args(name)]      # noqa: E731
    assert types(BASE) == types("tda_plv_dist_batch")[:8] + ["int"] + types("tda_plv_dist_batch")[8:]


def test_constants_are_the_headers():
    text = _header()
    assert "Analytic-signal connectivity" in text
    m = re.search(r"#define\s+TDA_CONN_TAU\s+(\S+)", text)
    assert m and float.fromhex(m.group(1)) == _lib.CONN_TAU == 2.0 ** -40
    for name, number in (("WPLI", 0), ("IMCOH", 1), ("COH", 2), ("AEC", 3)):
        m = re.search(r"#define\s+TDA_CONN_" + name + r"\s+(\d+)\b", text)
        assert m and int(m.group(1)) == number == getattr(_lib, "TDA_CONN_" + name), name
        assert engine.CONNECTIVITY_MEASURES[name.lower()] == number
        assert re.search(r"TDA_CONN_" + name + r"\s+\(" + str(number) + r', "' + name.lower() + r'"\)', text), name
    assert len(engine.CONNECTIVITY_MEASURES) == 4
    # the limits are the phase-locking value's
    assert (_lib.PLV_MAX_CHANNELS, _lib.PLV_MAX_SAMPLES) == (64, 256)
    assert [engine.DIST_METHODS[m] for m in engine.METHOD_NAMES] == [0, 1, 2, 3]
