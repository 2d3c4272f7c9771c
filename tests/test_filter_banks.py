"""
The filter banks the recording passes design once (preprocess.SosBank, BaBank, envelope_bandpass), no GPU and no library
load: the arrays handed to the C entries are, array for array, what the per-call packing made -- _sos_plan of
design_bandpass_filter per band, stacked; zero-padded (b, a) and scipy.signal.lfilter_zi per filter.
"""
import numpy as np
import pytest
from scipy import signal

from tda_eeg_audio_amd import preprocess

BANDS = list(preprocess.FREQ_BANDS.values())


def _bas():             # as tests/test_gpu_ragged.py::_bas: the independent statement of utils.py:66-74
    return [signal.butter(4, [max(lo / 125, 0.001), min(hi / 125, 0.999)], btype="band") for lo, hi in BANDS]


def test_sos_bank_equals_per_band_plans():
    bank = preprocess.SosBank.bandpass(BANDS, 250, 4)
    plans = [preprocess._sos_plan(preprocess.design_bandpass_filter(lo, hi, 250, 4)) for lo, hi in BANDS]
    assert np.array_equal(bank.sos, np.stack([p[0] for p in plans])) and bank.sos.flags.c_contiguous
    assert np.array_equal(bank.zi, np.stack([p[1] for p in plans])) and bank.zi.flags.c_contiguous
    assert bank.sos.dtype == bank.zi.dtype == np.float64
    assert (bank.n, bank.n_sec) == (5, 4) and bank.sos.shape == (5, 4, 6) and bank.zi.shape == (5, 4, 2)
    assert all(bank.edge == p[2] for p in plans)


def test_sos_bank_refuses_filters_of_different_structure():
    with pytest.raises(AssertionError, match="share their structure"):
        preprocess.SosBank([preprocess.design_bandpass_filter(8, 13, 250, 4), preprocess.design_bandpass_filter(8, 13, 250, 3)])


@pytest.mark.parametrize("bas", [_bas(), [preprocess.envelope_lowpass(250)]], ids=["band-passes", "low-pass"])
def test_ba_bank_equals_padded_coefficients_and_lfilter_zi(bas):
    bank = preprocess.BaBank(bas)
    ntaps = max(max(len(b), len(a)) for b, a in bas)
    assert (bank.n, bank.ntaps, bank.edge) == (len(bas), ntaps, 3 * ntaps)
    assert bank.B.shape == bank.A.shape == (len(bas), ntaps) and bank.Z.shape == (len(bas), ntaps - 1)
    for f, (b, a) in enumerate(bas):
        bp, ap = np.concatenate([b, np.zeros(ntaps - len(b))]), np.concatenate([a, np.zeros(ntaps - len(a))])
        assert np.array_equal(bank.B[f], bp) and np.array_equal(bank.A[f], ap)
        assert np.array_equal(bank.Z[f], signal.lfilter_zi(bp, ap))
    assert all(m.dtype == np.float64 and m.flags.c_contiguous for m in (bank.B, bank.A, bank.Z))


def test_ba_bank_pads_a_shorter_filter():
    b1, a1 = signal.butter(2, 0.3)
    bank = preprocess.BaBank(_bas()[:1] + [(b1, a1)])
    assert bank.ntaps == 9 and np.array_equal(bank.B[1], np.concatenate([b1, np.zeros(6)]))
    assert np.array_equal(bank.Z[1], signal.lfilter_zi(bank.B[1], bank.A[1]))


def test_envelope_bandpass_equals_the_written_out_design():
    got = preprocess.envelope_bandpass(BANDS, 250)
    assert len(got) == len(BANDS)
    for (b, a), (rb, ra) in zip(got, _bas()):
        assert np.array_equal(b, rb) and np.array_equal(a, ra)
    # the clamps: a band that reaches past the Nyquist frequency, and one that starts at 0
    (b, a), = preprocess.envelope_bandpass([(0.0, 200.0)], 250)
    rb, ra = signal.butter(4, [0.001, 0.999], btype="band")
    assert np.array_equal(b, rb) and np.array_equal(a, ra)
    s = np.arange(8.0)
    assert preprocess.bandpass_filter(s, 250, 130, 140) is s          # utils.py:71-72: lo >= hi after the clamps
