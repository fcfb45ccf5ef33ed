"""The host helpers of csrc/rowlaunch.h (align256, at_bytes, hy_row_prime, hy_rowmap) on the CPU: tests/cpp/test_rowlaunch_host.cpp, a
program of its own that includes the header the library compiles and touches no device.  Built and run with the address and
undefined-behaviour sanitizers on the host side."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "moai-fhe-transformerinference-public_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "cpp", "test_rowlaunch_host.cpp")
SAN = "-fsanitize=address,undefined"


def test_row_helpers_match_the_loops_they_replace(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    exe = tmp_path / "test_rowlaunch_host"
    # the header includes the HIP runtime's declarations, so the HIP compiler builds it; the sanitizers go to the host side only
    cmd = [hipcc, "-x", "hip", "--offload-arch=gfx950", "-std=c++17", "-O1", "-Wall", "-I" + CSRC, "-Xarch_host", SAN, "-Xarch_host",
           "-fno-sanitize-recover=undefined", SRC, "-x", "none", SAN, "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ALL PASS" in r.stdout and "runtime error" not in r.stderr, (r.stdout[-3000:], r.stderr[-2000:])
