"""The one-lane-per-signal filter forms, zero_phase_kernel<SosFilter> (TDA_SOS_SERIAL) and <BaFilter8> (TDA_BA_SERIAL), on
a cut of tests/front_end_cases.py, bit for bit against scipy.  The library reads the variables once per process, so
tests/test_gpu_front_end_variants.py starts this script in a fresh child with one of them set:

    TDA_SOS_SERIAL=1 python tests/front_end_serial_child.py sos
    TDA_BA_SERIAL=1  python tests/front_end_serial_child.py ba

Prints "SERIAL <kind> OK cases <n>"; exits 1 on a mismatch, 2 when the variable of <kind> is not set."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.dirname(HERE)]

import front_end_cases as fc                                    # noqa: E402


def main(kind):
    var = {"sos": "TDA_SOS_SERIAL", "ba": "TDA_BA_SERIAL"}[kind]
    if not os.environ.get(var):
        print(f"{var} is not set: this process would run the pipelined form")
        return 2
    from tda_eeg_audio_amd import _lib, preprocess
    ctx = _lib.get_ctx(0)
    designs = fc.sos_designs() if kind == "sos" else fc.ba_designs()
    n = bad = 0
    for name, L, n_sig in fc.serial_cases(kind):
        x = fc.signals(n_sig, L, 70)
        if kind == "sos":
            sos = designs[name][0]
            got, ref = preprocess.sosfiltfilt(sos, x, ctx=ctx), fc.sos_reference(sos, x)
        else:
            b, a = designs[name][:2]
            got, ref = preprocess.filtfilt(b, a, x, ctx=ctx), fc.ba_reference(b, a, x)
        n += 1
        if not np.array_equal(got, ref):
            bad += 1
            print(f"MISMATCH {kind} {name} L={L} n_sig={n_sig}: {int((got != ref).sum())} of {ref.size} samples differ")
    if bad:
        print(f"SERIAL {kind} FAILED {bad} of {n} cases")
        return 1
    print(f"SERIAL {kind} OK cases {n}")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1]))
