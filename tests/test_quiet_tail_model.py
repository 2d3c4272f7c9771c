"""
The quiet tail of the Rips sweep, as a numpy model (tests/quiet_tail_model.py): a stale coverage scan, the skipped edges
added, the hit re-tested exactly.  No GPU.

What is asserted, on the audio sample of the GPU test (64 windows per band), on the explicit clouds of the GPU test and
on 200 random 3-D clouds of 8 ... 124 points:
  * every edge the loop passes over without a chunk has a common neighbour among the strictly earlier edges (from the
    rank matrix alone, independent of the model's adjacency rows), so no candidate is ever skipped;
  * every rank at which the re-test rule starts a regular chunk is a true candidate (no common neighbour at its own
    time), it lies where the current rule sweeps a chunk too, and the re-test rule never starts more chunks than the
    current one.  (The plain statement "the starts are a subset of today's starts" is false: when a true candidate
    follows a false alarm by less than a chunk, today's chunk starts AT the false alarm and sweeps the candidate as an
    inner edge; the re-test rule starts at the candidate.  1 of the 64 beta windows of the sample does that.)
  * the inputs of tests/test_gpu_quiet_tail.py take the new path: at least 25 % of the windows of each audio set
    (theta, alpha, beta, gamma) show a false alarm, the far-point clouds a false alarm in front of the late merge, the
    ring clouds (two vertex words) one in front of the late birth, and the control cloud neither a stop nor a chunk.
"""
import numpy as np
import pytest

import quiet_tail_model as M
from oracle import port

CHUNK = 512          # the workgroup of the point-cloud kernels = the edges of a chunk


def _check(n, a, b, start, chunk=CHUNK):
    """Both rules from `start` on; the invariants; returns (now, retest)."""
    now = M.quiet_tail(n, a, b, start, chunk, retest=False)
    re = M.quiet_tail(n, a, b, start, chunk, retest=True)
    fc = M.first_cover(n, a, b)
    for res in (now, re):
        sk = np.array(res["skipped"], dtype=np.int64)
        assert (fc[sk] < sk).all(), "an edge without an earlier common neighbour was passed over"
    st = np.array(re["starts"], dtype=np.int64)
    assert (fc[st] > st).all(), "a chunk was started at an edge that is covered at its own time"
    al = np.array(re["alarms"], dtype=np.int64)
    assert (fc[al] < al).all()
    swept = np.zeros(len(a) + 1, dtype=bool)
    for s in now["starts"]:
        swept[s:s + chunk] = True
    assert swept[st].all(), "the re-test rule starts a chunk where the current rule sweeps none"
    assert len(re["starts"]) <= len(now["starts"])
    assert len(re["starts"]) + len(re["alarms"]) >= len(now["starts"]) or len(re["alarms"]) == 0
    return now, re


@pytest.fixture(scope="module")
def sample():
    return M.audio_sample()


def test_audio_sample_takes_the_new_path_and_skips_no_candidate(sample):
    print()
    for band in M.AUDIO_BANDS:
        wins, tau = sample[band]
        n_now, n_re, stops, alarmed = [], [], [], 0
        for w in wins:
            dm = M.audio_dm(w, tau)
            a, b, key = M.filtration(dm)
            (_, h1), npts = port.audio_persistence(w, tau)
            assert npts == len(dm)
            now, re = _check(len(dm), a, b, M.tail_start(key, h1, CHUNK))
            n_now.append(len(now["starts"])); n_re.append(len(re["starts"])); stops.append(now["stops"])
            alarmed += len(re["alarms"]) > 0
        print(f"{band}: {len(dm)} points, tail chunks per window now {np.mean(n_now):.2f}, with the re-test "
              f"{np.mean(n_re):.2f}, scan stops {np.mean(stops):.2f} (max {max(stops)}), windows with a false alarm {alarmed}/64")
        if band != "delta":
            assert alarmed >= 16, (band, alarmed)          # 25 % of the windows of every set the GPU test calls audio
            assert np.mean(n_re) < np.mean(n_now)


def test_random_clouds_skip_no_candidate():
    rng = np.random.default_rng(2024)
    alarms = 0
    for i in range(200):
        n = int(rng.integers(8, 125))
        pc = rng.random((n, 3)) if i % 2 else rng.standard_normal((n, 3))
        dm = port.cloud_dm(port.minmax_normalise(pc)).astype(np.float32)
        a, b, key = M.filtration(dm)
        h1 = port.rips_f32(dm)[1]
        for start in (M.tail_start(key, h1, CHUNK), CHUNK):       # (the second: as if no class had ever lived)
            _, re = _check(n, a, b, start)
            alarms += len(re["alarms"])
    assert alarms > 0


def test_explicit_clouds_force_each_branch():
    for name, (clouds, n_pts) in M.explicit_clouds().items():
        before = 0
        for w in range(len(clouds)):
            pc = M.cloud_points(clouds, n_pts, w)
            n = len(pc)
            dm = port.cloud_dm(pc).astype(np.float32)
            a, b, key = M.filtration(dm, M.CLOUD_THRESH)
            h1 = port.rips_f32(dm, thresh=M.CLOUD_THRESH)[1]
            if name.startswith("far"):
                # the far point is vertex 0: its first edge is the late merge, a true candidate in the tail
                late = int(np.nonzero((a == 0) | (b == 0))[0][0])
                start = M.tail_start(key, h1, CHUNK)
                assert start < late
            else:
                # the ring's class: born when the square closes, the longest-lived class by far
                ring = h1[np.argmax(h1[:, 1] - h1[:, 0])]
                assert 1.2 < ring[0] < 1.4 and 1.7 < ring[1] < 1.95, ring
                late = int(np.nonzero(key == np.float32(ring[0]))[0][0])
                start = M.tail_start(key, h1[h1[:, 0] < ring[0]], CHUNK)
                # ... and behind its death the tail goes on, up to the merge of blob and ring
                merge = int(np.nonzero((b < 4) & (a >= 4))[0][0])
                assert key[merge] > ring[1] and M.first_cover(n, a, b)[merge] > merge and merge < len(a) - 1
                _check(n, a, b, M.tail_start(key, h1, CHUNK))
            _, re = _check(n, a, b, start)
            assert late in re["starts"] or any(s <= late < s + CHUNK for s in re["starts"]), (name, w)
            before += any(x < late for x in re["alarms"])
        print(name, "copies with a false alarm in front of the late candidate:", before, "of", len(clouds))
        assert before >= len(clouds) // 4, (name, before)
    pc = M.control_cloud()
    dm = port.cloud_dm(pc).astype(np.float32)
    a, b, key = M.filtration(dm, M.CLOUD_THRESH)
    now, re = _check(len(pc), a, b, M.tail_start(key, port.rips_f32(dm, thresh=M.CLOUD_THRESH)[1], CHUNK))
    assert now["stops"] == 0 and not now["starts"] and not re["starts"] and len(a) > CHUNK
