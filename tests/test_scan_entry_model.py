"""
The entry into the coverage scan of the Rips sweep, as a numpy model (tests/scan_entry_model.py): the scan entered from
every chunk that ends with no class alive ("direct"), not only from a quiet one ("today").  No GPU.

Model 1, the tail -- on the audio sample of the GPU tests (64 windows per band), on synth.eeg_windows(64, seed=5) and on
the explicit clouds of quiet_tail_model:
  * soundness: every rank the direct rule passes over has a common neighbour among the strictly earlier edges (from the
    rank matrix alone), and no birth and no finite death of the oracle's H1 diagram lies at a passed-over rank;
  * effect: per band and for the EEG windows the direct rule leaves at most today's chunks minus 0.8 behind the last
    busy chunk, per window on average; on the far-point clouds 2.0 chunks become 1.0;
  * every EEG window takes the new path, at 32 and at 64 class bits: the chunk in which its last class dies is not cut.

Model 2, the lull clouds (chunk ends with no class alive in the MIDDLE of a filtration): each copy that the GPU test
runs has such a chunk end in front of a birth; the direct rule starts its next chunk at the first true candidate behind
it -- the first of the merges between neighbouring circles, a few ranks in front of the birth of the large loop, or that
birth itself where no merge comes first -- with the birth inside that chunk; and every edge in between has an earlier
common neighbour.  (A chunk starts at a true candidate "whether it is a merge or a birth": with k circles the k - 1
merges come first, so the start is the first merge and not the birth.)
"""
import numpy as np
import pytest

import chunk_cut_model as C
import quiet_tail_model as Q
import scan_entry_model as S
from oracle import port
from tda_eeg_audio_amd import synth


def _sound(n, a, b, key, h1, t):
    """The ranks that the direct rule passed over: covered at their own time, and no row of the oracle hangs on them."""
    sk = np.array(t["passed"], dtype=np.int64)
    fc = Q.first_cover(n, a, b)
    assert (fc[sk] < sk).all(), "an edge without an earlier common neighbour was passed over"
    st = np.array(t["starts"], dtype=np.int64)
    assert (fc[st] > st).all(), "a chunk was started at an edge that is covered at its own time"
    passed = np.zeros(len(a), dtype=bool)
    passed[sk] = True
    _, birth = C.births(n, a, b)
    assert not (birth & passed).any(), "a birth was passed over"
    for ranks in S.oracle_ranks(key, h1):
        assert len(ranks) and not passed[ranks].all(), "a birth or death of the oracle's H1 rows was passed over"


def _mean(ts, which):
    return np.mean([t[which] for t in ts], axis=0)


def test_tail_audio_sample():
    print()
    for band, (wins, tau) in Q.audio_sample().items():
        ts = []
        for w in wins:
            dm = Q.audio_dm(w, tau)
            a, b, key = Q.filtration(dm)
            h1 = port.audio_persistence(w, tau)[0][1]
            ts.append(S.tail(len(dm), a, b, key, h1, 512))
            _sound(len(dm), a, b, key, h1, ts[-1])
        today, direct = _mean(ts, "today"), _mean(ts, "direct")
        print(f"{band}: chunks behind the last busy one, scan rounds per window: today {today[0]:.2f}, {today[1]:.2f}; "
              f"direct {direct[0]:.2f}, {direct[1]:.2f}")
        assert direct[0] <= today[0] - 0.8, (band, today, direct)


def test_tail_eeg_windows_all_take_the_new_path():
    W = synth.eeg_windows(64, seed=5)
    ts = []
    for w in range(64):
        d = port.corr_dist(W[w])[1]
        a, b, key = Q.filtration(d.astype(np.float32))
        h1 = port.rips_dm(d)[1]
        n = d.shape[0]
        ts.append(S.tail(n, a, b, key, h1, 256))
        _sound(n, a, b, key, h1, ts[-1])
        assert ts[-1]["start"] < len(a), w                  # a chunk follows the last busy one today
        for bits in (32, 64):
            chunks = S.walks(n, a, b, key, h1, 256, bits, direct=True)
            assert chunks is not None and not any(c["overflow"] for c in chunks), (w, bits)
            entered = S.busy_entries(chunks)
            assert entered and not any(c["cut"] for c in entered), (w, bits)
            assert len(chunks) < len(S.walks(n, a, b, key, h1, 256, bits, direct=False)), (w, bits)
    today, direct = _mean(ts, "today"), _mean(ts, "direct")
    print(f"\nEEG: today {today[0]:.2f}, {today[1]:.2f}; direct {direct[0]:.2f}, {direct[1]:.2f}")
    assert direct[0] <= today[0] - 0.8, (today, direct)


def test_tail_explicit_clouds():
    for name, (clouds, n_pts) in Q.explicit_clouds().items():
        ts = []
        for w in range(len(clouds)):
            pc = Q.cloud_points(clouds, n_pts, w)
            dm = port.cloud_dm(pc).astype(np.float32)
            a, b, key = Q.filtration(dm, Q.CLOUD_THRESH)
            h1 = port.rips_f32(dm, thresh=Q.CLOUD_THRESH)[1]
            ts.append(S.tail(len(pc), a, b, key, h1, 512))
            _sound(len(pc), a, b, key, h1, ts[-1])
        today, direct = _mean(ts, "today"), _mean(ts, "direct")
        print(name, "today", today, "direct", direct)
        if name.startswith("far"):
            assert today[0] == 2.0 and direct[0] == 1.0, (name, today, direct)
        else:
            assert direct[0] <= today[0], (name, today, direct)


def _lull_check(pc, chunk, bits):
    n = len(pc)
    dm = port.cloud_dm(pc).astype(np.float32)
    a, b, key = Q.filtration(dm, S.CLOUD_THRESH)
    h1 = port.rips_f32(dm, thresh=S.CLOUD_THRESH)[1]
    found = S.lull(n, a, b, key, h1, chunk, bits)
    assert found is not None, "no chunk end with every class dead in front of a birth"
    end, birth, start = found
    assert end % chunk == 0 and end < birth < len(a)
    # independent of the walk: the scan of quiet_tail_model from `end`, and the rank matrix
    scan = Q.quiet_tail(n, a, b, end, chunk, retest=True)
    fc = Q.first_cover(n, a, b)
    between = np.arange(end, start)
    assert (fc[between] < between).all(), "an edge between the lull and the next chunk has no earlier common neighbour"
    assert fc[start] > start and scan["starts"][0] == start and scan["skipped"][:start - end] == list(between)
    assert start <= birth < start + chunk, "the birth is not in the chunk that the direct rule starts"
    cand, is_birth = C.births(n, a, b)
    merges = cand[end:birth] & ~is_birth[end:birth]
    if not merges.any():
        assert start == birth
    # the lull is real: the oracle has a class born at that rank, and every class born before `end` is dead by then
    h1 = np.asarray(h1).reshape(-1, 2)
    assert (h1[:, 0] == np.float64(key[birth])).any()
    assert (h1[h1[:, 0] < np.float64(key[end]), 1] < np.float64(key[end])).all()
    return end, birth, start


@pytest.mark.parametrize("name", sorted(S.LULLS))
def test_lull_clouds(name):
    k, m, r, chunk = S.LULLS[name]
    clouds = [S.lull_cloud(k, m, r, seed) for seed in S.LULL_SEEDS] + list(S.lull_clouds(name))
    for pc in clouds:
        assert pc.shape == (k * m, 3)
        for bits in (32, 64):
            end, birth, start = _lull_check(pc, chunk, bits)
    print(name, "last copy: lull at", end, "next chunk at", start, "birth at", birth)


def test_four_by_eleven_gives_no_lull():
    for seed in S.LULL_SEEDS:
        pc = S.lull_cloud(4, 11, 0.30, seed)
        dm = port.cloud_dm(pc).astype(np.float32)
        a, b, key = Q.filtration(dm, S.CLOUD_THRESH)
        assert S.lull(len(pc), a, b, key, port.rips_f32(dm, thresh=S.CLOUD_THRESH)[1], 256) is None


def test_ladders_never_scan_behind_a_cut():
    """The class-bit ladders: their cut chunks end with classes alive or are followed at the cut; the chunk that ends calm
    is a full one.  (The kernel does not scan behind a cut chunk whatever it leaves: it ends in front of a known birth.)"""
    for name in sorted(C.LADDERS):
        cut = 0
        for pts in C.ladder_clouds(name, copies=2):
            (n, a, b, key), dg = C.cloud_filtration(pts)
            for chunk, bits in ((512, 32), (512, 64), (256, 64)):
                chunks = S.walks(n, a, b, key, dg[1], chunk, bits, direct=True)
                assert chunks is not None
                assert not any(c["cut"] and c["scanned"] for c in chunks)
                assert S.busy_entries(chunks)
                cut += sum(c["cut"] for c in chunks)
        assert cut > 0, name


def test_ring_windows_end_in_the_last_chunk():
    picked = S.ring_windows_ending_in_the_last_chunk()
    assert sum(nm == "ring60" for nm, _ in picked) >= 8 and sum(nm == "ring124" for nm, _ in picked) >= 8
