"""
The C ABI of the generators and representative cycles on the built library, and the argument refusals of
engine.generators_args.  No GPU: nothing here creates a context.
"""
import os
import re

import numpy as np
import pytest

from tda_eeg_audio_amd import _lib, drivers, engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASES = ("tda_generators_dm_batch", "tda_generators_cloud_batch", "tda_generators_takens_batch", "tda_generators_mean")
TAIL = ["const double* h0", "int h0_cap", "const int* h0_cnt", "const double* h1", "int h1_cap", "const int* h1_cnt",
        "const int* rips_status", "int skip_mask", "int cyc_cap", "short* h1_gen", "int* h1_flag", "short* cyc", "int* cyc_len",
        "double* part", "short* h0_edge", "int* work"]


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
    assert _header_args("tda_generators_dm_batch")[:6] == _header_args("tda_rips_dm_batch")[:6]
    assert _header_args("tda_generators_dm_batch")[6:] == TAIL + ["int* status"]
    assert _header_args("tda_generators_cloud_batch")[:8] == _header_args("tda_cloud_rips_batch")[:8]
    assert _header_args("tda_generators_cloud_batch")[8:] == TAIL + ["int* status"]
    assert _header_args("tda_generators_takens_batch")[:8] == _header_args("tda_takens_rips_batch")[:8]
    assert _header_args("tda_generators_takens_batch")[8:] == TAIL + ["int* n_points", "int* status"]
    # the rows come in the order the Rips entry points write them (there without const)
    rips = [a.replace("const ", "") for a in _header_args("tda_rips_dm_batch")[6:12]]
    assert [a.replace("const ", "") for a in TAIL[:6]] == rips
    assert [a.split()[-1].lstrip("*") for a in _header_args("tda_generators_mean")] == [
        "ctx", "part", "n_win", "n", "seg_off", "n_seg", "status_in", "skip_mask", "mean"]
    assert len(_lib._GEN) == len(TAIL)


def test_flags_are_the_headers():
    for name, value in (("BIRTH_TIED", 1), ("DEATH_TIED", 2), ("CYCLE_TRUNCATED", 4), ("NO_EDGE", 8)):
        m = re.search(r"#define\s+TDA_GEN_" + name + r"\s+(\d+)\b", _header())
        assert m and int(m.group(1)) == getattr(_lib, "TDA_GEN_" + name) == value


def test_generators_args():
    assert engine.generators_args(4) == 4 and engine.generators_args(np.int64(128)) == 128
    assert type(engine.generators_args(np.int32(9))) is int
    for bad in (3, 129, 0, -1, 8.0, True, None, "8"):
        with pytest.raises(ValueError):
            engine.generators_args(bad)
    # the host forms check the rows before any GPU call
    rows, cnt = np.zeros((2, 8, 2)), np.zeros(2, np.int32)
    for h1, c1 in ((rows[:, :0], cnt), (rows[:1], cnt), (rows, cnt[:1]), (np.zeros((2, 8, 3)), cnt)):
        with pytest.raises(ValueError):
            engine._gen_host(2, 9, None, None, h1, c1, 8, None, True, True, False)
    with pytest.raises(ValueError):
        engine._gen_host(2, 9, rows[:1], cnt, rows, cnt, 8, None, True, True, False)
    out, _, _ = engine._gen_host(2, 9, None, None, rows, cnt, 8, None, True, True, True)
    assert "h0_edge" not in out and out["part"].shape == (2, 9) and out["cyc"].shape == (2, 8, 8) and out["work"].shape == (2, 4, 2)


def test_participation_names():
    names = drivers.participation_names(["alpha", "beta"], 5)
    assert len(names) == 10 == len(set(names)) and names[0] == "alpha_part_ch0" and names[-1] == "beta_part_ch4"
    assert len(drivers.participation_names()) == len(drivers.BANDS) * 47
