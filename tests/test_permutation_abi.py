"""
The C ABI of the two-sample permutation sums on the built library, and its constants.  No GPU: nothing here creates a
context.
"""
import os
import re

import numpy as np

import permutation_ref as ref
from tda_eeg_audio_amd import _lib, engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASE = "tda_perm_sums_batch"


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
        for a, d in zip(args, decl):             # every pointer <-> void*, long long <-> c_longlong, int <-> c_int
            want = _lib.c_vp if "*" in d else _lib.C.c_longlong if d.startswith("long long") else _lib.C.c_int
            assert a is want, (name, d)
    dev, host = _header_args(BASE + "_dev"), _header_args(BASE)
    # the _dev form takes the host form's arguments, the work space in front of the outputs and a stream
    assert [a for a in dev if a.split()[-1].lstrip("*") not in ("work", "work_doubles", "stream")] == host
    assert dev[-1] == "void* stream"
    assert [a.split()[-1].lstrip("*") for a in host] == ["ctx", "D", "n_mat", "n", "ld", "lab", "n_perm", "out", "n1"]


def test_constants_are_the_headers():
    text = _header()
    for macro, value in (("TDA_PT_ROW_BLOCK", _lib.PT_ROW_BLOCK), ("TDA_PT_MAX_ITEMS", _lib.PT_MAX_ITEMS),
                         ("TDA_PT_MAX_PERM", _lib.PT_MAX_PERM), ("TDA_PT_MAX_MATRICES", _lib.PT_MAX_MATRICES)):
        m = re.search(r"#define\s+" + macro + r"\s+(\d+)\b", text)
        assert m and int(m.group(1)) == value, macro
    assert _lib.PT_MAX_ITEMS == 4096 and _lib.PT_MAX_PERM >= 100000 and ref.ROW_BLOCK == _lib.PT_ROW_BLOCK
    assert "Two-sample permutation sums" in text
    # the macros of the sizes, as the header spells them
    assert re.search(r"#define\s+TDA_PT_WORDS\(n_perm\)\s+\(\(\(n_perm\)\s*\+\s*63\)\s*/\s*64\)", text)
    assert re.search(r"#define\s+TDA_PT_BLOCKS\(n\)\s+\(\(\(n\)\s*\+\s*TDA_PT_ROW_BLOCK\s*-\s*1\)\s*/\s*TDA_PT_ROW_BLOCK\)", text)
    assert [_lib.pt_words(p) for p in (1, 64, 65, 10001)] == [1, 1, 2, 157]
    assert [_lib.pt_blocks(n) for n in (2, 64, 65, 1416)] == [1, 1, 2, 23]
    assert _lib.pt_work_doubles(10, 1416, 10001) == 10 * 23 * 3 * 64 * 157


def test_pack_labels_layout():
    rng = np.random.default_rng(0)
    lab = (rng.random((131, 9)) < 0.5).astype(np.uint8)
    packed = engine.pack_labels(lab)
    assert packed.shape == (3, 9) and packed.dtype == np.uint64 and packed.flags["C_CONTIGUOUS"]
    for p in range(131):
        for j in range(9):
            assert (int(packed[p // 64, j]) >> (p % 64)) & 1 == lab[p, j]
    assert (packed[2] >> np.uint64(3) == 0).all()             # the bits past n_perm are 0
    assert engine.pack_labels(lab.astype(bool)).tobytes() == packed.tobytes()
