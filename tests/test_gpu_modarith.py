"""The device arithmetic helpers (csrc/modarith.hip.h, csrc/ntt_finish.h, the load functors and lazy_final of csrc/ntt_kernels.hip.h)
one by one on the device against 128-bit host arithmetic, at the limit primes of mode_limits.chain(12) and chain(16):
tests/cpp/test_modarith_device.hip, run once as a child process.  Residues, the output bounds of the helpers' comments, and for
the FP64 helpers the exact bits; no tolerance."""
import subprocess

import pytest

from test_modarith_device import EXE, chain_args

pytestmark = pytest.mark.gpu


def test_device_helpers_meet_their_contracts_at_the_limit_primes():
    r = subprocess.run([EXE] + chain_args(), capture_output=True, text=True, timeout=120)
    tail = "\n".join(line for line in r.stdout.split("\n") if "MISMATCH" in line or "FAIL" in line or "HIP error" in line)[-4000:]
    assert r.returncode == 0, (tail, r.stdout[-1500:], r.stderr[-2000:])
    assert "ALL PASS" in r.stdout, r.stdout[-1500:]
    assert r.stderr == "", r.stderr[-2000:]
