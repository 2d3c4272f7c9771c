"""
The C ABI of the landmark Rips route (greedy permutation, n_perm) on the built library.  No GPU: nothing here creates a
context.
"""
import os
import re

from tda_eeg_audio_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["tda_takens_landmarks", "tda_cloud_landmarks", "tda_takens_rips_landmarks"]


def _header():
    return open(os.path.join(ROOT, "include", "tdaeeg.h")).read()


def _header_args(name):
    m = re.search(r"tda_status\s+" + name + r"\s*\(([^;]*?)\)\s*;", _header(), re.S)
    assert m, name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_symbols_exported_and_bound():
    lib = _lib.load()
    for base in NAMES:
        for name in (base + "_dev", base):
            assert hasattr(lib, name), name
            res, args = _lib.SYMBOLS[name]
            decl = _header_args(name)
            assert res is _lib.C.c_int and len(args) == len(decl), name
            for a, d in zip(args, decl):         # double <-> c_double, int <-> c_int, every pointer <-> void*
                want = _lib.c_vp if "*" in d else _lib.C.c_double if d.startswith("double") else _lib.C.c_int
                assert a is want, (name, d)
        # the _dev form takes the host form's arguments and a stream
        assert _header_args(base + "_dev")[:-1] == _header_args(base) and _header_args(base + "_dev")[-1] == "void* stream"
    # the composed call: the landmark arguments of tda_takens_landmarks with thresh after n_perm, then the diagram
    # outputs of tda_takens_rips_batch
    lm, both, rips = (_header_args(n) for n in ("tda_takens_landmarks", "tda_takens_rips_landmarks", "tda_takens_rips_batch"))
    assert both[:8] == lm[:8] and both[8] == "double thresh" and both[9:15] == lm[8:]
    assert both[15:] == rips[8:]


def test_limits_are_the_headers():
    text = _header()
    for macro, value in (("TDA_LM_MAX_POINTS", _lib.LM_MAX_POINTS), ("TDA_LM_MAX_SAMPLES", _lib.LM_MAX_SAMPLES),
                         ("TDA_MAX_POINTS", _lib.MAX_POINTS)):
        m = re.search(r"#define\s+" + macro + r"\s+(\d+)\b", text)
        assert m and int(m.group(1)) == value, macro
    assert _lib.LM_MAX_POINTS == 1024
