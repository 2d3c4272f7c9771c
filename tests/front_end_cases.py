"""Seeded designs, lengths and signals for the front-end kernels (csrc/filters.hip) off the reference's configuration
(4th-order Butterworth filters, 44100 -> 250 Hz): SOS cascades of 1..8 sections, (b, a) pairs of 2..17 taps, banks of
1..5 filters, the lengths at which a kernel's last 64-sample chunk is short, full or one sample over, resampling rates
with up = 1, 2, 5, 7, 8, and Hilbert lengths at the block and table-chunk boundaries.  The same builders feed
tests/test_front_end_model.py (plain restatements against scipy, no GPU), tests/test_gpu_front_end_variants.py (the
kernels against scipy) and tests/front_end_serial_child.py (the one-lane-per-signal forms).  TEST INFRASTRUCTURE."""
import functools
import math

import numpy as np
from scipy import signal

SEED = 31415
FT = 64                      # samples per chunk of every filter kernel
LOW = 0.4                    # low-pass corner, in units of the Nyquist frequency
BAND = (0.2, 0.6)            # band-pass corners; fs = 2 makes them the (lowcut, highcut) of design_bandpass_filter
FS = 2.0
# the further filters of a bank (the first is BAND / LOW): five filters is the most a launch takes
BANK_BANDS = (BAND, (0.1, 0.3), (0.3, 0.7), (0.15, 0.5), (0.25, 0.65))
BANK_LOWS = (LOW, 0.3, 0.5, 0.35, 0.45)
BANK_SIZES = (1, 2, 3, 5)
OUTPUT_BOUND = 10.0          # "of order 1" for unit-variance input: an overflowed reference would compare equal to anything


# ------------------------------------------------------------------------------------------------ designs
@functools.lru_cache(maxsize=None)
def sos_designs():
    """{name: (sos, n_sec, edge)} with n_sec and edge (scipy.signal.sosfiltfilt's pad length) written out per family,
    not taken from the package: Butterworth band-pass of order o has o sections and pads 3 * (2 o + 1); the low-pass
    has ceil(o / 2) sections, a first-order one among them for odd o, and pads 3 * (o + 1); the elliptic band-pass is
    as the Butterworth one, with numerator zeros off +-1 and a different numerator per section."""
    out = {}
    for o in range(1, 9):
        out[f"band{o}"] = (signal.butter(o, BAND, "band", output="sos"), o, 3 * (2 * o + 1))
    for o in range(1, 9):
        out[f"low{o}"] = (signal.butter(o, LOW, "low", output="sos"), (o + 1) // 2, 3 * (o + 1))
    for o in (2, 4, 6):
        out[f"ellip{o}"] = (signal.ellip(o, 1.0, 40.0, BAND, "band", output="sos"), o, 3 * (2 * o + 1))
    return out


@functools.lru_cache(maxsize=None)
def ba_designs():
    """{name: (b, a, ntaps, edge)}: Butterworth low-pass of orders 1..16 (ntaps 2..17) and band-pass of orders 1..8
    (ntaps 3, 5, ..., 17); edge = 3 * ntaps (scipy.signal.filtfilt's default)."""
    out = {}
    for o in range(1, 17):
        b, a = signal.butter(o, LOW, "low")
        out[f"low{o}"] = (b, a, o + 1, 3 * (o + 1))
    for o in range(1, 9):
        b, a = signal.butter(o, BAND, "band")
        out[f"band{o}"] = (b, a, 2 * o + 1, 3 * (2 * o + 1))
    return out


def sos_lps(n_sec):
    """Lanes per signal of sos_pipe_kernel: the section count rounded up to 2, 4 or 8."""
    return 2 if n_sec <= 2 else 4 if n_sec <= 4 else 8


def sos_spw(n_sec):
    return FT // sos_lps(n_sec)


def ba_spw(ntaps):
    """Signals per wave: ba_pipe_kernel (eight lanes per signal) up to 9 taps, zero_phase_kernel (one lane) above."""
    return 8 if ntaps <= 9 else 64


# ------------------------------------------------------------------------------------------------ lengths, counts
def first_chunk_count(edge):
    """The smallest m with 64 m - 8 >= 3 edge + 1, i.e. whose lengths are all accepted (L >= edge + 1)."""
    return -(-(3 * edge + 9) // FT)


def boundary_lengths(edge):
    """The shortest accepted length and every L whose padded length N = L + 2 edge lies in [64 m - 8, 64 m + 1] for the
    two smallest m: the last chunk of a pass with 56..63, 64 and 1 samples, and the pipelined forms' drain chunk."""
    m0 = first_chunk_count(edge)
    return [edge + 1] + [n - 2 * edge for m in (m0, m0 + 1) for n in range(FT * m - 8, FT * m + 2)]


def needs_drain_chunk(n_padded, lps):
    """A pipelined pass over N samples ends lps - 1 steps after the first section: one chunk more than ceil(N / 64)."""
    return -(-(n_padded + lps - 1) // FT) > -(-n_padded // FT)


def filter_cases(edge, spw):
    """[(L, n_sig)]: 2 spw + 1 signals at every boundary length; 1, spw - 1, spw and spw + 1 at the length whose padded
    length is a multiple of 64."""
    full = FT * first_chunk_count(edge) - 2 * edge
    return [(L, 2 * spw + 1) for L in boundary_lengths(edge)] + [(full, n) for n in (1, spw - 1, spw, spw + 1)]


def one_length(edge):
    """The length of the device-entry cases: padded length 64 m, a drain chunk at every pipeline depth."""
    return FT * first_chunk_count(edge) - 2 * edge


def signals(n_sig, L, *key):
    """(n_sig, L): every signal its own random walk plus noise (unit variance and more), so that exchanged rows show."""
    rng = np.random.default_rng([SEED, n_sig, L, *key])
    x = 0.05 * rng.standard_normal((n_sig, L)).cumsum(axis=1) + rng.standard_normal((n_sig, L))
    x.setflags(write=False)
    return x


def check_reference(ref):
    """scipy's own output must be finite and of order 1, or a comparison with it proves nothing."""
    assert np.isfinite(ref).all() and np.abs(ref).max() < OUTPUT_BOUND, float(np.abs(ref).max())
    return ref


def sos_reference(sos, x):
    """scipy.signal.sosfiltfilt row by row (axis=-1 filters every row on its own; test_front_end_model.py holds that)."""
    return check_reference(signal.sosfiltfilt(sos, x, axis=-1))


def ba_reference(b, a, x):
    return check_reference(signal.filtfilt(b, a, x, axis=-1))


# ------------------------------------------------------------------------------------------------ ragged banks
RAGGED_SOS_ORDERS = (1, 2, 3, 5, 6, 8)
DEVICE_SOS_ORDERS = (1, 2, 3, 5, 6, 8)
DEVICE_BA_TAPS = (2, 3, 4, 6, 7, 8, 10, 13, 17)


def ragged_sos_lengths(order):
    """Four recordings of a band-pass of `order`: the shortest accepted one, one whose padded length is a multiple of 64
    (a drain chunk at every depth), one at the first padded length 64 m + 66 - lps that needs the drain chunk, and an
    ordinary one -- long and short mixed."""
    edge = 3 * (2 * order + 1)
    lps = sos_lps(order)
    m0 = first_chunk_count(edge)
    lens = [FT * (m0 + 1) + 2 - lps - 2 * edge, edge + 1, FT * m0 + 21 - 2 * edge, FT * m0 - 2 * edge]
    assert needs_drain_chunk(lens[0] + 2 * edge, lps) and not needs_drain_chunk(lens[0] - 1 + 2 * edge, lps)
    assert needs_drain_chunk(lens[3] + 2 * edge, lps) and not needs_drain_chunk(lens[2] + 2 * edge, lps)
    return lens


def ragged_sos_channels(order):
    spw = sos_spw(order)
    return (1, spw, spw + 1, 47)


RAGGED_BA_TAPS = tuple(range(2, 10))
RAGGED_BA_SIGNALS = 17


def ragged_ba_lengths(ntaps):
    """17 signals = two full waves of ba_pipe_ragged_kernel and one signal more.  Padded lengths of one, two and three
    chunks inside every wave (never below the shortest accepted one, 3 edge + 1), 64 and 128 among them, the second wave
    in another order than the first."""
    edge = 3 * ntaps
    wave = [3 * edge + 1, 64, 65, 100, 128, 129, 150, 192]
    n_pad = [max(n, 3 * edge + 1) for n in wave + [wave[i] for i in (5, 2, 7, 0, 4, 1, 6, 3)] + [127]]
    assert any(n % FT == 0 for n in n_pad[:8]) and len({-(-n // FT) for n in n_pad[:8]}) >= 2
    return [n - 2 * edge for n in n_pad]


# ------------------------------------------------------------------------------------------------ serial forms
SERIAL_SOS = ("band1", "band4", "band8")          # n_sec 1, 4, 8
SERIAL_BA = ("low1", "low4", "low8")              # ntaps 2, 5, 9
SERIAL_COUNTS = (1, 64, 65)


def serial_cases(kind):
    """[(name, L, n_sig)] of the one-lane-per-signal forms (64 signals per wave)."""
    names, designs = (SERIAL_SOS, sos_designs()) if kind == "sos" else (SERIAL_BA, ba_designs())
    return [(nm, L, n) for nm in names for L in boundary_lengths(designs[nm][-1]) for n in SERIAL_COUNTS]


# ------------------------------------------------------------------------------------------------ resampler, envelope
RS_R = 4                     # outputs per wave of resample_poly_ragged_kernel: a workgroup takes up * RS_R of them
# (fs_audio, fs): up, down
RATES = {(48000, 250): (1, 192), (16000, 250): (1, 64), (1000, 250): (1, 4),
         (22050, 250): (5, 441), (400, 250): (5, 8), (300, 250): (5, 6), (350, 250): (5, 7),
         (2000, 1750): (7, 8), (1750, 2000): (8, 7),
         (200, 250): (5, 4), (150, 250): (5, 3), (125, 250): (2, 1)}
RATE_TOO_MANY_PHASES = (44100, 256)      # up = 64: resample_audio takes it, the ragged entry refuses it


def n_resampled(n_in, up, down):
    return -(-n_in * up // down)


def resample_lengths(up, down):
    """1, down - 1, down, down + 1, the three lengths around each of the first two at which the output count reaches a
    multiple of up * RS_R (a full last tile, and one output more or less), and, last, one of a few thousand samples whose
    last tile is not full: what a store without its bound would write lands behind the packed outputs."""
    out = [1, down - 1, down, down + 1]
    for k in (1, 2):
        L = next(n for n in range(1, 1 << 20) if n_resampled(n, up, down) >= up * RS_R * k)
        out += [L - 1, L, L + 1]
    out = [n for n in dict.fromkeys(out) if n >= 1]
    return out + [next(n for n in range(3000 + down, 1 << 20) if n_resampled(n, up, down) % (up * RS_R))]


def resample_overhang(n_in, up, down):
    """Outputs past the end that the lanes of a signal's last tile compute and must not store."""
    return -n_resampled(n_in, up, down) % (up * RS_R)


RESAMPLE_GUARD = 8 * RS_R    # NaN words behind the packed outputs: the longest overhang is up * RS_R - 1 <= 31


def audio(n, *key):
    rng = np.random.default_rng([SEED, n, *key])
    t = np.arange(n)
    x = np.sin(2 * np.pi * 0.013 * t) * (1 + 0.5 * np.sin(2 * np.pi * 0.0007 * t)) + 0.3 * rng.standard_normal(n)
    x.setflags(write=False)
    return x


def resample_reference(x, fs_audio, fs):
    ref = signal.resample_poly(x, fs, fs_audio)
    assert np.isfinite(ref).all()
    return ref


# block sizes 64 * ceil(ceil(N / 8) / 64): 512 / 513 change the block, 1024, 2048, ... the chunks of the g table
HILBERT_RAGGED_LENGTHS = (2049, 7, 8192, 512, 1025, 9, 2047, 513, 8191, 8, 1023, 2048, 511, 1024)
HILBERT_HOST_LENGTHS = (1, 2, 255, 256, 257, 513)
GATHER_WIN_LENGTHS = (1, 255, 256, 257, 600)


def envelope_input(n, *key):
    rng = np.random.default_rng([SEED, n, *key])
    x = np.abs(rng.standard_normal(n)).cumsum() * 0.01 + rng.standard_normal(n)
    x.setflags(write=False)
    return x


def rate_geometry(fs_audio, fs):
    g = math.gcd(int(fs), int(fs_audio))
    return int(fs) // g, int(fs_audio) // g
