"""
The C ABI of the persistence Fisher distance on the built library.  No GPU: nothing here creates a context.
"""
import os
import re

from tda_eeg_audio_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["tda_persistence_fisher_batch_dev", "tda_persistence_fisher_batch"]


def _header_args(name):
    text = open(os.path.join(ROOT, "include", "tdaeeg.h")).read()
    m = re.search(r"tda_status\s+" + name + r"\s*\(([^;]*?)\)\s*;", text, re.S)
    assert m, name
    return [a.strip() for a in m.group(1).split(",")]


def test_symbols_exported_and_bound():
    lib = _lib.load()
    for name in NAMES:
        assert hasattr(lib, name), name
        res, args = _lib.SYMBOLS[name]
        decl = _header_args(name)
        assert res is _lib.C.c_int and len(args) == len(decl), name
        for a, d in zip(args, decl):             # double <-> c_double, int <-> c_int, every pointer <-> void*
            want = _lib.c_vp if "*" in d else _lib.C.c_double if d.startswith("double") else _lib.C.c_int
            assert a is want, (name, d)
    # the _dev form takes the host form's arguments and a stream
    assert _header_args(NAMES[0])[:-1] == _header_args(NAMES[1]) and _header_args(NAMES[0])[-1] == "void* stream"
    # ... in the order of tda_wasserstein_q_batch up to n_pairs, which engine._pair_batch marshals
    assert _header_args(NAMES[1])[:12] == _header_args("tda_wasserstein_q_batch")[:12]


def test_max_points_is_the_headers():
    text = open(os.path.join(ROOT, "include", "tdaeeg.h")).read()
    m = re.search(r"#define\s+TDA_PF_MAX_POINTS\s+(\d+)\b", text)
    assert m and int(m.group(1)) == _lib.PF_MAX_POINTS == 512
