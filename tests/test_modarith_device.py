"""tests/cpp/test_modarith_device.hip without a GPU: the program is built, its case table covers every device helper of
csrc/modarith.hip.h, every input it generates lies in its case's domain (--host-only), the lines it cites are the helpers', and it is
compiled with the library's own optimisation level, language standard, target and -ffp-contract.  The device run is
tests/test_gpu_modarith.py."""
import os
import re
import subprocess

import pytest

import mode_limits as ml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "moai-fhe-transformerinference-public_amd", "csrc")
EXE = os.path.join(ROOT, "tests", "cpp", "test_modarith_device")

# helpers of modarith.hip.h that no case of the table names, each with its reason
EXEMPT = {
    "mulhi64": "a one-line wrapper of __umul64hi; every Shoup and Barrett case runs through it",
    "u2d": "a bit cast; every FP64 case passes its operands and results through it",
    "d2u": "a bit cast; every FP64 case passes its operands and results through it",
    "lazy16_inv_kind": "an index function of the register schedule, no arithmetic; the kernels' whole-transform tests cover it",
}


def chain_args():
    """the command line of the program: chain(12) and chain(16) under the names of mode_limits"""
    args = []
    for logn in (12, 16):
        args.append(str(logn))
        args += ["%s=%d" % (name, q) for name, q in ml.chain(logn).items()]
    return args


@pytest.fixture(scope="module")
def table():
    assert os.path.isfile(EXE) and os.access(EXE, os.X_OK), "tests/cpp/test_modarith_device is not built (make -C tests/cpp)"
    r = subprocess.run([EXE, "--host-only"] + chain_args(), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stderr == "", (r.stdout[-3000:], r.stderr[-2000:])
    return r.stdout


def test_host_only_every_input_in_its_domain(table):
    assert "HOST ONLY: ALL INPUTS IN THEIR DOMAINS" in table and "FAIL" not in table
    # no case without a prime, none sampled away: every (case, prime) line reports its inputs
    cases = re.findall(r"^case \d+: ", table, flags=re.M)
    assert len(cases) > 100
    assert len(re.findall(r"^    ok: ", table, flags=re.M)) == len(cases)
    for count in re.findall(r": (\d+) inputs, all in the domain", table):
        assert 0 < int(count) <= 1 << 16


def test_table_covers_every_device_helper(table):
    src = open(os.path.join(CSRC, "modarith.hip.h")).read()
    helpers = set(re.findall(r"__device__ __forceinline__ [\w:<> ]*?[ &*](\w+)\(", src))
    assert {"mul_shoup_approx", "fp_mulmod_q", "csub_carry", "gs_bfly_last_lazy16", "mac2", "u2d"} <= helpers  # the pattern still finds them
    names = " ".join(re.findall(r"^case \d+: (.*)$", table, flags=re.M))
    missing = sorted(h for h in helpers if h not in EXEMPT and not re.search(r"\b%s\b" % h, names))
    assert not missing, "device helpers without a case in tests/cpp/test_modarith_device.hip and without an exemption: %s" % missing
    stale = sorted(h for h in EXEMPT if h not in helpers)
    assert not stale, "exemptions of helpers that no longer exist: %s" % stale


def test_cited_lines_define_the_helpers(table):
    """every case cites file:line of the helper's definition, below the comment that is its contract"""
    cited = re.findall(r"^case \d+: (\w+).*\[([\w.]+):(\d+)\]$", table, flags=re.M)
    assert len(cited) > 100
    for name, fname, line in cited:
        name = {"seed2": "mac2"}.get(name, name)
        text = open(os.path.join(CSRC, fname)).read().split("\n")[int(line) - 1]
        assert re.search(r"\b%s\b" % name, text), "%s:%s does not define %s: %r" % (fname, line, name, text)


def _flags(path, var):
    text = open(path).read()
    arch = re.search(r"^ARCH \?= (\S+)", text, flags=re.M).group(1)
    flags = re.search(r"^%s \?= (.*)$" % var, text, flags=re.M).group(1).replace("$(ARCH)", arch).split()
    pick = lambda prefix: sorted(f for f in flags if f.startswith(prefix))
    return {"opt": pick("-O"), "std": pick("-std"), "contract": pick("-ffp-contract"), "arch": pick("--offload-arch")}


def test_compiled_with_the_librarys_flags():
    lib = _flags(os.path.join(CSRC, "Makefile"), "CXXFLAGS")
    mine = _flags(os.path.join(ROOT, "tests", "cpp", "Makefile"), "HIPFLAGS")
    assert all(len(v) == 1 for v in lib.values()), lib
    assert mine == lib
    # and the rule uses them
    rule = open(os.path.join(ROOT, "tests", "cpp", "Makefile")).read()
    assert re.search(r"^test_modarith_device:.*\n\t\$\(HIPCC\) \$\(HIPFLAGS\) ", rule, flags=re.M)
