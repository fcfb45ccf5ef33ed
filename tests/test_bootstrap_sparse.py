"""Sparse-slot bootstrapping (logn < logNh): the diagonal sets against their definition (CPU) and the drop-in Bootstrapper
with real constants on the device (tests/cpp_sparse/test_bootstrap_sparse.cpp; build() builds the binaries)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp_sparse")


def _run(name, *args, timeout):
    exe = os.path.join(BIN, name)
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", BIN, "-s", name])
    r = subprocess.run([exe, *args], capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0 and "ALL OK" in r.stdout, r.stdout[-4000:] + r.stderr[-4000:]
    return r.stdout


def test_sparse_diagonals_against_definition():
    out = _run("test_sparse_setup", timeout=300)
    for logn in range(3, 10):
        assert "logn %d " % logn in out


@pytest.mark.gpu
def test_bootstrap_sparse_n2048():
    out = _run("test_bootstrap_sparse", timeout=900)
    assert "logn 7:" in out and "logn 9:" in out and "logn 10:" in out
    assert "logn 10 and 7 together: 2 runs for 2 ciphertexts" in out


@pytest.mark.gpu
def test_bootstrap_sparse_moai_chain():
    out = _run("test_bootstrap_sparse", "--full", timeout=1800)
    assert "logn 12:" in out
