"""
The ragged audio front end through every layer: tda_resample_poly_ragged_dev and tda_hilbert_envelope_ragged_dev against
scipy on every signal alone, preprocess.envelopes_ragged_dev against compute_envelope's scipy chain, and
recordings.RaggedAudioRecordingPass against RaggedRecordingPass fed the envelopes of envelopes_ragged_dev.
Rows are not compared with the scipy-envelope path: the delta-band (b, a) filter amplifies 1e-12 differences of its
input ~1e6x (see test_gpu_frontend.py::test_audio_front_end_vs_scipy).
"""
import numpy as np
import pytest
from scipy import signal

from tda_eeg_audio_amd import preprocess, recordings
from tda_eeg_audio_amd._lib import TdaError

pytestmark = pytest.mark.gpu


def _audio(rng, n, f0=220.0):
    t = np.arange(n) / 44100.0
    return np.sin(2 * np.pi * f0 * t) * (1 + 0.5 * np.sin(2 * np.pi * 3 * t)) + 0.1 * rng.standard_normal(n)


def _dev(ctx):
    import torch
    return torch.device("cuda", ctx.device)


def _split(flat, lengths):
    off = np.concatenate([[0], np.cumsum(lengths)])
    return [flat[off[i]:off[i + 1]] for i in range(len(lengths))]


def test_resample_bank_matches_resample_poly(ctx):
    dev = _dev(ctx)
    rng = np.random.default_rng(11)
    # a few seconds each; 5,000 and 1 sample: shorter than the filter (17,641 taps); outputs of both parities
    La = [44100 * 3 + 17, 5000, 44100 * 2 + 882, 1, 44100 * 4 - 5, 882 * 7]
    xs = [_audio(rng, n, 180 + 40 * i) for i, n in enumerate(La)]
    refs = [signal.resample_poly(x, 250, 44100) for x in xs]
    assert {len(r) % 2 for r in refs} == {0, 1}
    xh, lh = preprocess.pack_recordings(xs)
    P = preprocess.AudioPlan(lh).upload(dev)
    y = preprocess.resample_bank_ragged_dev(xh.to(dev), P, ctx=ctx).cpu().numpy()
    assert len(y) == sum(len(r) for r in refs)
    for n, got, ref in zip(La, _split(y, P.n_out), refs):
        assert got.shape == ref.shape, n
        assert np.abs(got - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max()), n
    # lengths given directly; an output buffer of the caller
    import torch
    out = torch.full((P.out_tb.total + 3,), float("nan"), dtype=torch.float64, device=dev)
    preprocess.resample_bank_ragged_dev(xh.to(dev), lh, y_t=out, ctx=ctx)
    assert np.array_equal(out[:P.out_tb.total].cpu().numpy(), y) and out[-3:].isnan().all()


def test_hilbert_bank_matches_scipy(ctx):
    dev = _dev(ctx)
    rng = np.random.default_rng(12)
    lengths = [1, 2, 750, 751, 3, 5741, 5740, 64, 2663, 2]
    xs = [np.abs(rng.standard_normal(n)).cumsum() * 0.01 + rng.standard_normal(n) for n in lengths]
    xh, lh = preprocess.pack_recordings(xs)
    env = preprocess.hilbert_envelope_ragged_dev(xh.to(dev), lh, ctx=ctx).cpu().numpy()
    for n, x, got in zip(lengths, xs, _split(env, lengths)):
        ref = np.abs(signal.hilbert(x))
        assert np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max(), n


def test_ragged_abi_rejects_bad_geometry(ctx):
    import ctypes as C
    import torch
    dev = _dev(ctx)
    x = torch.zeros(100, dtype=torch.float64, device=dev)
    P = preprocess.AudioPlan([100]).upload(dev)
    bad_len = np.array([0], dtype=np.int64)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = C.c_void_p(x.data_ptr())
    tb = C.c_void_p(P.in_tb.len_t.data_ptr())
    # length 0, up 0, negative n_pre_remove
    for ln, up, npr in ((bad_len, 5, 11), (P.in_tb.len_h, 0, 11), (P.in_tb.len_h, 5, -1)):
        rc = ctx.lib.tda_resample_poly_ragged_dev(ctx.h, p, 1, tb, C.c_void_p(P.in_tb.off_t.data_ptr()), preprocess.ptr(ln),
                                                  C.c_void_p(P.out_tb.off_t.data_ptr()), C.c_void_p(P.hp_t.data_ptr()), P.nq,
                                                  up, 882, npr, p, st)
        assert rc == 1                                                  # TDA_ERR_INVALID
    rc = ctx.lib.tda_hilbert_envelope_ragged_dev(ctx.h, p, 1, tb, C.c_void_p(P.in_tb.off_t.data_ptr()), preprocess.ptr(bad_len),
                                                 p, C.c_void_p(P.g_off_t.data_ptr()), p, st)
    assert rc == 1
    with pytest.raises(TdaError):
        preprocess.hilbert_envelope_ragged_dev(torch.zeros(9000, dtype=torch.float64, device=dev), np.array([9000]), ctx=ctx)


def test_envelopes_ragged_matches_compute_envelope(ctx):
    dev = _dev(ctx)
    rng = np.random.default_rng(13)
    La = [44100 * 3 + 17, 44100 * 6 + 1234, 44100 + 441, 5000, 44100 * 2 + 882]
    xs = [_audio(rng, n, 150 + 30 * i) for i, n in enumerate(La)]
    xh, lh = preprocess.pack_recordings(xs)
    env, le = preprocess.envelopes_ragged_dev(xh.to(dev), lh, ctx=ctx)
    env = env.cpu().numpy()
    b, a = signal.butter(4, min(50, 125 * 0.9) / 125, btype="low")
    assert np.array_equal(le, [len(signal.resample_poly(np.zeros(n), 250, 44100)) for n in La])
    for n, x, got in zip(La, xs, _split(env, le)):
        ref = signal.filtfilt(b, a, np.abs(signal.hilbert(signal.resample_poly(x, 250, 44100))))
        assert got.shape == ref.shape
        assert np.abs(got - ref).max() <= 1e-11 * np.abs(ref).max(), n
    # an envelope not longer than the low-pass pad length (15): 2,646 samples resample to 15
    short = [xs[0], _audio(rng, 2646)]
    xh2, lh2 = preprocess.pack_recordings(short)
    assert preprocess.AudioPlan(lh2).n_out[1] == 15
    with pytest.raises(ValueError):
        preprocess.envelopes_ragged_dev(xh2.to(dev), lh2, ctx=ctx)


# EEG lengths and envelope lengths: recording 0's audio is SHORTER than its EEG, recording 2 has no window (n_windows = 0)
PASS_L = [1500, 2663, 200, 900, 1240, 700, 1100]
PASS_LE = [1400, 2663, 300, 1000, 1240, 700, 1090]


def test_audio_pass_equals_envelope_pass(ctx):
    import torch
    dev = _dev(ctx)
    rng = np.random.default_rng(14)
    La = [le * 882 // 5 - (i % 3) * 37 for i, le in enumerate(PASS_LE)]
    auds = [_audio(rng, n, 120 + 25 * i) for i, n in enumerate(La)]
    raws = [rng.standard_normal((47, L)) + 0.5 * rng.standard_normal((1, L)) for L in PASS_L]
    xh, _ = preprocess.pack_recordings(raws)
    ah, lah = preprocess.pack_recordings(auds)
    cost = 8 * (47 * np.array(PASS_L) + lah)
    ap = recordings.RaggedAudioRecordingPass(PASS_L, lah, dev, shard_bytes=int(cost.max()), n_sets=2, ctx=ctx)
    sizes = [b - a for a, b in ap.plan.shards]
    assert len(sizes) >= 3 and max(sizes) > 1 and ap.n_sets == 2       # buffer sets are reused
    assert np.array_equal(ap.plan.Le, ap.audio_plan.n_out) and ap.plan.Le[0] < PASS_L[0]
    assert ap.empty.tolist() == [2]
    rows = ap.run(xh, ah).numpy().copy()
    # the reference: envelopes from envelopes_ragged_dev, through RaggedRecordingPass
    env, le = preprocess.envelopes_ragged_dev(ah.to(dev), lah, ctx=ctx)
    torch.cuda.synchronize()
    eh = torch.empty(env.numel(), dtype=torch.float64).pin_memory()
    eh.copy_(env.cpu())
    rp = recordings.RaggedRecordingPass(PASS_L, le, dev, shard_samples=3000, n_sets=2, ctx=ctx)
    ref = rp.run(xh, eh).numpy()
    assert rows.shape == ref.shape == (len(PASS_L), 5, 48)
    assert np.array_equal(rows, ref, equal_nan=True)
    assert np.isnan(rows[2][:, [0, 1, 2]]).all() and (rows[2][:, 3] == 0).all()
    assert (rows[[0, 1, 3, 4, 5, 6]][:, :, 3] > 0).all()
    again = ap.run(xh, ah).numpy()
    assert np.array_equal(again, rows, equal_nan=True)
