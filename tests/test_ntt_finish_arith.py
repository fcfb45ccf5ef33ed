"""N^-1 by shift and the one-step final reduction of the 60-bit NTT (csrc/ntt_finish.h) against 128-bit arithmetic on the CPU:
tests/cpp/test_ntt_finish_arith.cpp, a program of its own that includes the header the kernels compile.  Built and run twice,
plainly and with the undefined-behaviour sanitizer."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "moai-fhe-transformerinference-public_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "cpp", "test_ntt_finish_arith.cpp")


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-fsanitize=undefined", "-fno-sanitize-recover=undefined"]], ids=["plain", "ubsan"])
def test_finish_arithmetic_matches_128_bit_arithmetic(tmp_path, flags):
    exe = tmp_path / "test_ntt_finish_arith"
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-I" + CSRC] + flags + [SRC, "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ALL PASS" in r.stdout and "runtime error" not in r.stderr, (r.stdout[-3000:], r.stderr[-2000:])
