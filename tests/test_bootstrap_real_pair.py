"""The "real" bootstrap variants (bootstrap_real_3) and two real ciphertexts per bootstrap (bootstrap_real_pair_3,
bootstrap_real_many_3, the opt-in Bootstrapper::pair_real) on the device: tests/cpp_real/test_bootstrap_real_pair.cpp
(build() builds the binary)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp_real")


def _run(name, *args, timeout):
    exe = os.path.join(BIN, name)
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", BIN, "-s", name])
    env = dict(os.environ)
    env.pop("MOAI_BOOT_PAIR_REAL", None)  # the binary checks that pairing is off by default
    r = subprocess.run([exe, *args], capture_output=True, text=True, timeout=timeout, env=env)
    print(r.stdout)
    assert r.returncode == 0 and "ALL OK" in r.stdout, r.stdout[-6000:] + r.stderr[-4000:]
    return r.stdout


@pytest.mark.gpu
def test_bootstrap_real_pair_n2048():
    out = _run("test_bootstrap_real_pair", timeout=900)
    assert "logn 7 real:" in out and "logn 9 real:" in out and "logn 10 real:" in out
    assert "real and complex together: 2 runs for 2 ciphertexts" in out
    assert out.count("PAIR_TABLE") == 4


@pytest.mark.gpu
def test_bootstrap_real_pair_moai_chain():
    out = _run("test_bootstrap_real_pair", "--full", timeout=1800)
    assert "logn 12 real:" in out and "logn 15 real:" in out
    assert out.count("PAIR_TABLE") == 4
