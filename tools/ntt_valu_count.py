#!/usr/bin/env python3
"""Static instruction counts of the tiled NTT kernels (no GPU needed).

Compiles csrc/ntt.hip to gfx950 assembly with the Makefile's flags and prints, for every
ntt_{fwd,inv}_{strided,contig,contig2}<16, integer mode> kernel: vector-ALU instructions per thread and per butterfly (a thread
does 64 butterflies per pass, 128 in the paired kernels ntt_*_contig2), global loads (instructions, and bytes per butterfly), v_mad_u64_u32 and how many of them multiply by a literal zero, v_mov_b32 (and how many copy
one VGPR into another), VGPRs, scratch bytes and occupancy (waves per SIMD).  The kernels are straight-line code, so the
static count is what a thread executes.

    python tools/ntt_valu_count.py [--csrc DIR] [--label TEXT] [--keep FILE.s]
"""
import argparse
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "moai-fhe-transformerinference-public_amd", "csrc")
MODES = {-3: "M_LAZY16", -2: "M_LAZY8", -1: "M_GUARD2", 0: "M_GUARD", 1: "M_NOGUARD"}
BUTTERFLIES = 64


def makefile_flags(csrc):
    """HIPCC, ARCH and CXXFLAGS as csrc/Makefile sets them (the environment overrides them like make's ?= does)"""
    var = {}
    for line in open(os.path.join(csrc, "Makefile")):
        m = re.match(r"(\w+)\s*\?=\s*(.*)", line)
        if m:
            var[m.group(1)] = os.environ.get(m.group(1), m.group(2).strip())
    flags = var["CXXFLAGS"].replace("$(ARCH)", var["ARCH"]).split()
    hipcc = var["HIPCC"] if os.path.exists(var["HIPCC"]) else (shutil.which("hipcc") or var["HIPCC"])
    return hipcc, flags


def demangle(names):
    filt = shutil.which("llvm-cxxfilt") or "/opt/rocm/llvm/bin/llvm-cxxfilt"
    if not os.path.exists(filt):
        filt = shutil.which("c++filt")
    out = subprocess.run([filt], input="\n".join(names) + "\n", capture_output=True, text=True, check=True).stdout.split("\n")
    return dict(zip(names, out))


def parse(asm):
    """{mangled name: {counts}} of every kernel (a .globl function that has an .amdhsa_kernel record)"""
    kernels = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", asm, re.M))
    res = {}
    cur = None
    for line in asm.split("\n"):
        m = re.match(r"^(\w+):", line)
        if m and m.group(1) in kernels:
            cur = res[m.group(1)] = dict(valu=0, mad=0, mad0=0, mov=0, movvv=0, gload=0, gbytes=0, vgpr=None, scratch=None, occ=None)
            continue
        if cur is None:
            continue
        s = line.strip()
        if s.startswith(".Lfunc_end"):
            continue
        m = re.match(r";\s*(NumVgprs|ScratchSize|Occupancy):\s*(\d+)", s)
        if m:
            cur[{"NumVgprs": "vgpr", "ScratchSize": "scratch", "Occupancy": "occ"}[m.group(1)]] = int(m.group(2))
            if m.group(1) == "Occupancy":
                cur = None
            continue
        m = re.match(r"global_load_(dwordx(\d)|dword|\w+)", s)
        if m:
            cur["gload"] += 1
            cur["gbytes"] += 4 * int(m.group(2)) if m.group(2) else (4 if m.group(1) == "dword" else 0)
            continue
        if not s.startswith("v_"):
            continue
        ins = s.split(";")[0]
        op, _, rest = ins.partition(" ")
        ops = [o.strip() for o in rest.split(",")]
        cur["valu"] += 1
        if op == "v_mad_u64_u32":
            cur["mad"] += 1
            # dst, carry-out, a, b, addend
            if len(ops) >= 4 and (ops[2] == "0" or ops[3] == "0"):
                cur["mad0"] += 1
        elif op == "v_mov_b32" or op == "v_mov_b32_e32":
            cur["mov"] += 1
            if len(ops) >= 2 and re.fullmatch(r"v\d+", ops[1]):
                cur["movvv"] += 1
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--csrc", default=CSRC, help="directory holding ntt.hip and the Makefile (default: this tree's)")
    ap.add_argument("--label", default="", help="printed in the heading")
    ap.add_argument("--keep", default="", help="write the assembly to this file")
    args = ap.parse_args()
    hipcc, flags = makefile_flags(args.csrc)
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "ntt.s")
        cmd = [hipcc] + flags + ["--cuda-device-only", "-S", os.path.join(args.csrc, "ntt.hip"), "-o", out]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode:
            sys.stderr.write(r.stderr)
            return 1
        asm = open(out).read()
        if args.keep:
            shutil.copy(out, args.keep)
    res = parse(asm)
    names = demangle(sorted(res))
    rows = []
    for mangled, c in res.items():
        m = re.search(r"moai::ntt_(fwd|inv)_(strided|contig2?)<16, (-?\d+)(?:, (-?\d+))?>", names[mangled])
        if not m or int(m.group(3)) not in MODES:
            continue
        mode = int(m.group(3))
        name = "ntt_%s_%s<16,%d%s>" % (m.group(1), m.group(2), mode, "," + m.group(4) if m.group(4) else "")
        rows.append((mode, m.group(1), m.group(2) != "strided" if m.group(1) == "fwd" else m.group(2) == "strided", name, c))
    rows.sort(key=lambda r: r[:4])
    print("# static counts of the LOGN = 16 integer NTT kernels%s" % (" -- " + args.label if args.label else ""))
    print("# flags: " + " ".join(flags))
    print("%-30s %-9s %6s %8s %5s %7s %5s %5s %5s %6s %5s %8s %4s" % ("kernel", "mode", "VALU", "per bfly", "gload", "B/bfly", "mad64", "zero", "v_mov",
                                                                       "vgpr2v", "VGPR", "scratch", "occ"))
    for mode, _, _, name, c in rows:
        bf = BUTTERFLIES * (2 if "contig2" in name else 1)
        print("%-30s %-9s %6d %8.2f %5d %7.2f %5d %5d %5d %6d %5d %8d %4d" % (name, MODES[mode], c["valu"], c["valu"] / bf, c["gload"], c["gbytes"] / bf,
                                                                               c["mad"], c["mad0"], c["mov"], c["movvv"], c["vgpr"], c["scratch"], c["occ"]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
