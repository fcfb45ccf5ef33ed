"""The scratch planner of the hybrid key switch (csrc/hybrid_scratch.h) on the CPU: tests/cpp/test_hybrid_scratch_host.cpp, a program
of its own that includes the header the library compiles and touches no device.  It checks the row totals of every call family against
the formulas of include/moai_hip.h, the plans against the chunk functions they replaced, and every layout's offsets.  Built and run with
the address and undefined-behaviour sanitizers on the host side."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "moai-fhe-transformerinference-public_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "cpp", "test_hybrid_scratch_host.cpp")
SAN = "-fsanitize=address,undefined"


def test_plans_match_the_formulas_and_the_functions_they_replace(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    exe = tmp_path / "test_hybrid_scratch_host"
    # the same build as tests/test_rowlaunch_host.py: the HIP compiler, the sanitizers on the host side only
    cmd = [hipcc, "-x", "hip", "--offload-arch=gfx950", "-std=c++17", "-O1", "-Wall", "-I" + CSRC, "-Xarch_host", SAN, "-Xarch_host",
           "-fno-sanitize-recover=undefined", SRC, "-x", "none", SAN, "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ALL PASS" in r.stdout and "runtime error" not in r.stderr, (r.stdout[-3000:], r.stderr[-2000:])
