"""
The C ABI and the host-side argument checks of the kernels on diagrams.  No GPU: nothing here creates a context.
"""
import os
import re

import numpy as np
import pytest

from tda_eeg_audio_amd import _lib, engine, pipeline

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["tda_diagram_kernel_pairs_dev", "tda_diagram_kernel_pairs", "tda_diagram_kernel_gram_dev", "tda_diagram_kernel_gram"]


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
    # the _dev forms take the host forms' arguments and a stream
    assert _header_args(NAMES[0])[:-1] == _header_args(NAMES[1]) and _header_args(NAMES[2])[:-1] == _header_args(NAMES[3])
    text = open(os.path.join(ROOT, "include", "tdaeeg.h")).read()
    for k, v in (("TDA_KW_ONE", _lib.TDA_KW_ONE), ("TDA_KW_PERS", _lib.TDA_KW_PERS), ("TDA_KW_ATAN", _lib.TDA_KW_ATAN)):
        assert re.search(r"#define\s+" + k + r"\s+" + str(v) + r"\b", text)


def test_diagram_kernel_args():
    ninv, mirror, scale, weight, wc = engine.diagram_kernel_args(("pss", 0.5))
    assert (ninv, mirror, weight) == (-0.25, 1, _lib.TDA_KW_ONE) and scale == 1.0 / (8.0 * np.pi * 0.5)
    assert engine.diagram_kernel_args(["pwg", 0.5, 3]) == (-2.0, 0, 1.0, _lib.TDA_KW_ATAN, 3.0)
    assert engine.diagram_kernel_args(("pss", np.float32(2.0)))[0] == -1.0 / 16.0
    bad = [None, "pss", ("pss",), ("pss", 0.0), ("pss", -1.0), ("pss", np.nan), ("pss", np.inf), ("pss", 0.1, 1.0),
           ("pwg", 0.1), ("pwg", 0.1, 0.0), ("pwg", 0.1, np.inf), ("pwg", 0.0, 1.0), ("pwg", 0.1, 1.0, 2.0), ("rbf", 0.1),
           (1, 0.1), ("pss", "0.1"), ("pss", True), ("pss", 1e-320), ("pwg", 1e-170, 1.0), 0.1, (-1.25, 1, 0.4, 0, 0.0)]
    for kernel in bad:
        with pytest.raises(_lib.TdaError):
            engine.diagram_kernel_args(kernel)


def test_step_outputs_kernel_distance():
    assert pipeline.step_outputs(kernel_distance=None) == []
    (o,) = pipeline.step_outputs(kernel_distance=("pss", 1))
    assert o.name == "kd" and o.shape == (pipeline.KD_COLS,) == (2,) and o.params == ("pss", 1.0)
    (o,) = pipeline.step_outputs(kernel_distance=["pwg", 0.5, 2])
    assert o.params == ("pwg", 0.5, 2.0)
    # the validated parameters go back in unchanged (Workspace and the passes rebuild the table from them)
    assert pipeline.step_outputs(kernel_distance=o.params)[0].params == o.params
    for bad in (True, 0.1, "pss", ("pss",), ("pss", 0.0), ("pss", np.nan), ("pwg", 0.1), ("pwg", 0.1, -2.0), ("xyz", 1.0)):
        with pytest.raises(ValueError):
            pipeline.step_outputs(kernel_distance=bad)
    everything = pipeline.step_outputs(correlations=True, bottleneck=True, landscapes=(np.linspace(0, 1, 4), 2),
                                       images=(np.linspace(0, 1, 3), np.linspace(0, 1, 4), 0.1, 1), sliced=np.eye(2),
                                       wasserstein_q=(2, "l2"), frechet=(4, 2), kernel_distance=("pss", 0.1))
    assert [o.name for o in everything] == ["corr", "bott", "land", "img", "slc", "wq", "fm", "kd"]
    assert pipeline.Workspace.PAIR_BUFFERS[-4:] == ("k0", "k1", "ks0", "ks1")
    assert pipeline.Workspace.kd is None and pipeline.Workspace.k0 is None
