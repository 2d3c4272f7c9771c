#!/usr/bin/env python3
"""
tools/isa_diff.py -- are the gfx950 kernels of csrc/ instruction for instruction what they were at a git revision?
    python3 tools/isa_diff.py [--rev HEAD] [--files filters rips] [--match 'sos_pipe_kernel|ba_pipe_kernel|eeg_window_kernel']
Compiles each csrc/<file>.hip device-only (the Makefile's flags) from the working tree and from `git show REV:...`,
disassembles both code objects and compares every kernel whose mangled name matches, line by line.  Addresses are
dropped, and so is the literal of the s_add_u32 / s_addc_u32 pair after an s_getpc_b64 (PC-relative offsets to constant
data, which move whenever a kernel is added anywhere in the file).  A kernel REV has and the working tree has not is
reported as MISSING, one the working tree has and REV has not as ADDED; either makes the exit status 1.  No GPU needed.
An instantiation whose template arguments grew since REV is paired with its counterpart through RENAMED (mangled
prefix at REV -> mangled prefix now):
    python3 tools/isa_diff.py --files wasserstein --match wasserstein_kernel
--resources: for a change that is expected to move instructions.  One table row per kernel -- instructions, VGPRs,
SGPRs, scratch bytes and spills (the code object's metadata note) at REV -> now -- and the exit status is 1 only if a
kernel's scratch grew, a spill count left 0, or the waves per SIMD its VGPRs allow, floor(512 / (VGPRs rounded up to
8)), changed:
    python3 tools/isa_diff.py --resources --files wasserstein wasserstein_q --match wasserstein
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tda_eeg_audio_amd", "csrc")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
FLAGS = ["-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-fvisibility=hidden"]


# wasserstein_kernel<CW> became wasserstein_kernel<CW, SRC>; the pairs from index arrays are SRC = ws_index_pairs
RENAMED = [(re.compile(r"^_Z18wasserstein_kernelILi(\d+)EEv"), r"_Z18wasserstein_kernelILi\g<1>E14ws_index_pairsEv"),
           # wq_index_pairs and wq_opts became the ws_index_pairs and ws_opts of assign_dev.h
           (re.compile(r"^(_Z20wasserstein_q_kernelILi\d+ELi\d+ELi\d+E14)wq(_index_pairsEv)"), r"\g<1>ws\g<2>"),
           # euler_kernel<NW> and generators_kernel<NW> take a WinSrc (rips_keys_dev.h) for their seven loose arguments
           (re.compile(r"^(_Z12euler_kernelILi\d+EEv)"), r"\g<1>"),
           (re.compile(r"^(_Z17generators_kernelILi\d+EEv)"), r"\g<1>"),
           # their mean kernels became the two instantiations of group_mean_kernel<T, ACC> (common.h)
           (re.compile(r"^_Z17euler_mean_kernelPKi"), r"_Z17group_mean_kernelIixEv"),
           (re.compile(r"^_Z22generators_mean_kernelPKd"), r"_Z17group_mean_kernelIddEv")]


def counterpart(old_name, new):
    """The kernel of the working tree that old_name is compared with: the same mangled name, or -- for a renamed
    instantiation -- the one whose name starts with the new prefix (the argument list that follows may be compressed
    differently)."""
    if old_name in new:
        return old_name
    for pat, rep in RENAMED:
        m = pat.match(old_name)
        if m:
            hits = [k for k in new if k.startswith(m.expand(rep))]
            if len(hits) == 1:
                return hits[0]
    return None


def disasm(src_dir, name, tmp, tag):
    co, elf = os.path.join(tmp, f"{tag}_{name}.co"), os.path.join(tmp, f"{tag}_{name}.elf")
    subprocess.check_call([f"{ROCM}/bin/hipcc", "--offload-arch=gfx950", *FLAGS, "--cuda-device-only", "-c",
                           os.path.join(src_dir, f"{name}.hip"), "-o", co], stderr=subprocess.DEVNULL)
    subprocess.check_call([f"{ROCM}/llvm/bin/clang-offload-bundler", "--unbundle", "--type=o", f"--input={co}",
                           "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={elf}"])
    text = subprocess.check_output([f"{ROCM}/llvm/bin/llvm-objdump", "-d", "--no-show-raw-insn", elf]).decode()
    funcs, cur, after_pc = {}, None, 0
    for line in text.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.*)>:", line)
        if m:
            cur = funcs.setdefault(m.group(1), []); after_pc = 0; continue
        ins = line.split("//")[0].strip()
        if cur is None or not ins or ins == "...":
            continue
        if after_pc and re.match(r"s_addc?_u32 ", ins):
            ins = re.sub(r"0x[0-9a-f]+$", "<pcrel>", ins); after_pc -= 1
        else:
            after_pc = 2 if ins.startswith("s_getpc_b64") else 0
        cur.append(ins)
    return funcs, resources(elf)


RES_KEYS = ["vgpr_count", "agpr_count", "sgpr_count", "private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count"]


def resources(elf):
    """{kernel: {key: int}} from the metadata note (the keys of a kernel come sorted, `.name` among them)."""
    text = subprocess.check_output([f"{ROCM}/llvm/bin/llvm-readelf", "--notes", elf]).decode()
    out = {}
    for block in re.split(r"^  - (?=\.agpr_count:)", text, flags=re.M)[1:]:
        name = re.search(r"^\s+\.name:\s+(\S+)", block, re.M).group(1)
        out[name] = {k: int(re.search(rf"^\s*\.{k}:\s+(\d+)", block, re.M).group(1)) for k in RES_KEYS}
    return out


def waves(r):
    return 512 // ((r["vgpr_count"] + r["agpr_count"] + 7) // 8 * 8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rev", default="HEAD")
    ap.add_argument("--files", nargs="+", default=["filters", "rips"])
    ap.add_argument("--match", default=r"sos_pipe_kernel|ba_pipe_kernel|eeg_window_kernel")
    ap.add_argument("--resources", action="store_true")
    a = ap.parse_args()
    pat, bad = re.compile(a.match), 0
    with tempfile.TemporaryDirectory() as tmp:
        old_dir = os.path.join(tmp, "old")
        os.makedirs(old_dir)
        for f in os.listdir(CSRC):                       # the revision's sources (headers included)
            if f.endswith((".hip", ".h")):
                rel = os.path.relpath(os.path.join(CSRC, f), ROOT)
                r = subprocess.run(["git", "show", f"{a.rev}:{rel}"], cwd=ROOT, capture_output=True)
                if r.returncode == 0:
                    open(os.path.join(old_dir, f), "wb").write(r.stdout)
        inc = os.path.join(tmp, "include")              # (csrc includes ../../include/tdaeeg.h)
        os.makedirs(inc)
        open(os.path.join(inc, "tdaeeg.h"), "wb").write(subprocess.check_output(["git", "show", f"{a.rev}:include/tdaeeg.h"], cwd=ROOT))
        old_csrc = os.path.join(tmp, "x", "y")
        os.makedirs(os.path.dirname(old_csrc))
        os.rename(old_dir, old_csrc)
        for name in a.files:
            (old, old_res), (new, new_res) = disasm(old_csrc, name, tmp, "old"), disasm(CSRC, name, tmp, "new")
            paired = {counterpart(k, new) for k in old}
            for k in sorted(new):                        # kernels the working tree has and REV has not
                if pat.search(k) and k not in paired:
                    bad += 1
                    print(f"ADDED  {k}")
            for k in sorted(old):
                if not pat.search(k):
                    continue
                k2 = counterpart(k, new)
                if a.resources:
                    if k2 is None:
                        bad += 1
                        print(f"MISSING  {k}")
                        continue
                    o, n = old_res[k], new_res[k2]
                    spills = lambda r: r["vgpr_spill_count"] + r["sgpr_spill_count"]
                    ok = (n["private_segment_fixed_size"] <= o["private_segment_fixed_size"] and waves(o) == waves(n)
                          and not (spills(o) == 0 and spills(n) != 0))
                    bad += not ok
                    print(f"{'ok  ' if ok else 'FAIL'}  instr {len(old[k]):5d} -> {len(new[k2]):5d} ({100.0 * (len(new[k2]) - len(old[k])) / len(old[k]):+5.1f} %)"
                          f"  vgpr {o['vgpr_count']:3d} -> {n['vgpr_count']:3d}  agpr {o['agpr_count']} -> {n['agpr_count']}"
                          f"  sgpr {o['sgpr_count']:3d} -> {n['sgpr_count']:3d}  scratch {o['private_segment_fixed_size']:3d} -> "
                          f"{n['private_segment_fixed_size']:3d} B  spills {spills(o)} -> {spills(n)}  waves/SIMD {waves(o)} -> {waves(n)}"
                          f"  {k}" + (f"  ->  {k2}" if k2 != k else ""))
                    continue
                same = k2 is not None and new[k2] == old[k]
                bad += not same
                print(f"{'same' if same else 'DIFFERENT' if k2 else 'MISSING'}  {len(old[k]):6d} instructions  {k}"
                      + (f"  ->  {k2}" if k2 and k2 != k else ""))
                if k2 and not same:
                    import difflib
                    d = [l for l in difflib.unified_diff(old[k], new[k2], lineterm="", n=0) if l[:1] in "+-" and l[:3] not in ("+++", "---")]
                    print(f"           {len(new[k2]):6d} instructions now, {len(d)} diff lines")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
