"""CPU test: the two Frechet mean entry points are declared in include/tdaeeg.h with the argument lists the binding uses and
exported by the built library, and the header's limits are the ones _lib carries (no compute calls)."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["tda_frechet_mean_dev", "tda_frechet_mean_batch"]


def _header():
    return open(os.path.join(ROOT, "include", "tdaeeg.h")).read()


def test_declared_exported_and_bound():
    from tda_eeg_audio_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    protos = {m.group(1): m.group(2) for m in re.finditer(r"tda_status\s+(tda_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", src)}
    lib = _lib.load()
    for n in NAMES:
        assert n in protos, f"{n} is not declared in include/tdaeeg.h"
        assert hasattr(lib, n), f"{n} is not exported by libtdaeeg.so"
        res, args = _lib.SYMBOLS[n]
        assert len(args) == len(protos[n].split(",")), n              # one ctypes type per declared argument
    assert len(_lib.SYMBOLS["tda_frechet_mean_dev"][1]) == 17          # the issue's argument list, ctx .. stream


def test_limits_match_header():
    from tda_eeg_audio_amd import _lib
    defs = dict(re.findall(r"#define\s+(TDA_FM_[A-Z_]+)\s+(\d+)", _header()))
    assert int(defs["TDA_FM_MAX_ITER"]) == _lib.FM_MAX_ITER == 64
    assert int(defs["TDA_FM_MAX_POINTS"]) == _lib.FM_MAX_POINTS == 512


def test_engine_names():
    from tda_eeg_audio_amd import engine
    for n in ("frechet_mean_batch", "frechet_mean_dev", "frechet_args"):
        assert hasattr(engine, n), n
