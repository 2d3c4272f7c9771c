"""
The retry ladder of the Rips launchers as csrc/rips_ladder.h states it, without a GPU.

tests/host/rips_ladder_print.cpp is compiled against the header with the host compiler of the ROCm tree and prints, for
every flavour, class-words setting and set of rungs that fit, the launch sequence of each retry policy: F<capacity> a
first pass, R<capacity> a widening pass over the list of the flagged windows, T the last rung.  The sequences are
compared with the table below, which was written down from the rule (AUTO: F, every wider R, T; FIRST_PASS: F; ONLY: the
Rs and T; ONE_STEP: F and one R, no T; LAST_RUNG: T) and not produced by the code under test.  Capacities are u64 words
for distance matrices and bits for the fused EEG kernel and the point clouds.
"""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "tda_eeg_audio_amd", "csrc")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
POLICIES = ["AUTO", "FIRST_PASS", "ONLY", "ONE_STEP", "LAST_RUNG"]

# label printed by the program -> sequences in the order of POLICIES
EXPECTED = {
    # matrices, n <= 64, all of 1, 2, 4, 8 words fit
    "dm small 1111 0": ["F1 R2 R4 R8 T", "F1", "R2 R4 R8 T", "F1 R2", "T"],
    "dm small 1111 1": ["F1 R2 R4 R8 T", "F1", "R2 R4 R8 T", "F1 R2", "T"],
    "dm small 1111 2": ["F2 R4 R8 T", "F2", "R4 R8 T", "F2 R4", "T"],
    "dm small 1111 4": ["F4 R8 T", "F4", "R8 T", "F4 R8", "T"],
    # ... only 1, 2, 4 fit
    "dm small 1110 2": ["F2 R4 T", "F2", "R4 T", "F2 R4", "T"],
    # matrices, n > 64 (rungs 1 and 2 only), both fit
    "dm large 1100 0": ["F1 R2 T", "F1", "R2 T", "F1 R2", "T"],
    "dm large 1100 1": ["F1 R2 T", "F1", "R2 T", "F1 R2", "T"],
    "dm large 1100 2": ["F2 T", "F2", "T", "F2", "T"],
    "dm large 1100 4": ["F2 T", "F2", "T", "F2", "T"],
    # ... only 1 fits
    "dm large 1000 0": ["F1 T", "F1", "T", "F1", "T"],
    "dm large 1000 1": ["F1 T", "F1", "T", "F1", "T"],
    "dm large 1000 2": ["F1 T", "F1", "T", "F1", "T"],
    "dm large 1000 4": ["F1 T", "F1", "T", "F1", "T"],
    # fused EEG windows
    "eeg 0": ["F32 R64 R128 R512 T", "F32", "R64 R128 R512 T", "F32 R64", "T"],
    "eeg 1": ["F64 R128 R512 T", "F64", "R128 R512 T", "F64 R128", "T"],
    "eeg 2": ["F128 R512 T", "F128", "R512 T", "F128 R512", "T"],
    "eeg 4": ["F128 R512 T", "F128", "R512 T", "F128 R512", "T"],
    # point clouds: class words, whether 128 bits fit
    "cloud 1 1": ["F32 R64 R128 T", "F32", "R64 R128 T", "F32 R64", "T"],
    "cloud 1 0": ["F32 R64 T", "F32", "R64 T", "F32 R64", "T"],
    "cloud 2 1": ["F64 R128 T", "F64", "R128 T", "F64 R128", "T"],
    "cloud 2 0": ["F64 T", "F64", "T", "F64", "T"],
}


def test_every_flavour_follows_the_one_rule(tmp_path):
    exe = str(tmp_path / "rips_ladder_print")
    subprocess.check_call([os.path.join(ROCM, "llvm", "bin", "clang++"), "-std=c++17", "-Wall", "-Werror", "-I", CSRC,
                           os.path.join(HERE, "host", "rips_ladder_print.cpp"), "-o", exe])
    got = {}
    for line in subprocess.check_output([exe]).decode().splitlines():
        key, seq = line.split(":")
        label, policy = key.rsplit(" ", 1)
        got.setdefault(label, {})[policy] = seq.strip()
    for label, want in EXPECTED.items():
        assert label in got, (label, sorted(got))
        assert [got[label].get(p) for p in POLICIES] == want, label
    # the rungs that do not exist for n > 64 (4 and 8 words) change nothing there, whether their layouts would fit or not
    for w in (0, 1, 2, 4):
        assert got[f"dm large 1111 {w}"] == got[f"dm large 1110 {w}"] == got[f"dm large 1100 {w}"]
