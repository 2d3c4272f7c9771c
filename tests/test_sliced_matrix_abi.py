"""CPU test: the three entry points of the prepared sliced Wasserstein route are declared in include/tdaeeg.h with the
argument lists the binding uses, exported by the built library and reachable through engine (no compute calls)."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["tda_sliced_prepare_dev", "tda_sliced_prepared_pairs_dev", "tda_sliced_matrix_dev"]


def _prototypes():
    src = open(os.path.join(ROOT, "include", "tdaeeg.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return {m.group(1): m.group(2) for m in re.finditer(r"tda_status\s+(tda_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", src)}


def test_declared_exported_and_bound():
    from tda_eeg_audio_amd import _lib
    protos = _prototypes()
    lib = _lib.load()
    for n in NAMES:
        assert n in protos, f"{n} is not declared in include/tdaeeg.h"
        assert hasattr(lib, n), f"{n} is not exported by libtdaeeg.so"
        res, args = _lib.SYMBOLS[n]
        assert len(args) == len(protos[n].split(",")), n              # one ctypes type per declared argument
    # the slot tables are int64 and table_rows is passed as a 64-bit integer
    assert protos["tda_sliced_prepare_dev"].count("long long") == 2
    assert protos["tda_sliced_prepared_pairs_dev"].count("const long long*") == 2
    assert protos["tda_sliced_matrix_dev"].count("const long long*") == 2


def test_engine_names():
    from tda_eeg_audio_amd import engine
    for n in ("SlicedTable", "sliced_slots_dev", "sliced_prepare_dev", "sliced_wasserstein_prepared_dev",
              "sliced_wasserstein_gram_dev", "sliced_matrix_dev"):
        assert hasattr(engine, n), n
