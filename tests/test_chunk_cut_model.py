"""
The inputs of tests/test_gpu_chunk_cuts.py do run out of class bits inside a chunk, in every way the sweep distinguishes
(tests/chunk_cut_model.py): proved here on the CPU, from the filtration and the oracle's H1 rows.
"""
import pytest

import chunk_cut_model as M


@pytest.fixture(scope="module")
def audio32():
    return M.audio_cases(32)


def _count(per_window, name):
    return sum(name in c for c in per_window)


def test_audio_windows_hold_every_case_at_32_bits(audio32):
    every = [c for band in M.AUDIO_BANDS for c in audio32[band]]
    assert len(every) == 320
    for name in ("first", "later", "double", "lonely", "none"):
        assert _count(every, name) > 0, name
    # the model decides nearly every window (float32 lengths of continuous signals hardly tie)
    assert sum(len(c) == 0 for c in every) <= 16


def test_audio_windows_never_cut_at_64_bits():
    every = [c for band, cs in M.audio_cases(64).items() for c in cs]
    assert all(c <= {"none"} for c in every)


@pytest.mark.parametrize("name", sorted(M.LADDERS))
def test_ladders_cut_at_32_bits_without_overflow(name):
    for chunk in (512, 256):
        cs = M.ladder_cases(name, 32, chunk)
        assert all("first" in c and "overflow" not in c for c in cs), (name, chunk, cs)
        if name != "ladder60":
            assert all("double" in c for c in cs), (name, chunk, cs)


@pytest.mark.parametrize("name", ["ladder122", "ladder123", "ladder124"])
def test_four_rail_ladders_cut_at_64_bits(name):
    """in the first chunk of 512 edges (wide first pass of the cloud kernel), in the second of 256 (rips_dm_kernel)"""
    cs = M.ladder_cases(name, 64, 512)
    assert all(c == {"first"} for c in cs), (name, cs)
    cs = M.ladder_cases(name, 64, 256)
    assert all(c == {"later"} for c in cs), (name, cs)


def test_sixty_point_ladder_has_no_cut_at_64_bits():
    assert all(c == {"none"} for c in M.ladder_cases("ladder60", 64, 512))
