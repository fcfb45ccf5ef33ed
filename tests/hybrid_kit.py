"""What the tests of the hybrid key switch share (tests/test_gpu_hybrid_*.py, tests/test_hybrid_*_cpu.py,
tests/test_cabi_hybrid_ptrs_cpu.py): the environment of one chain of primes (Env), the four shapes most of them run at (ENVS and
the fixtures env_small1 .. env_tiled3), constants, the tuning-knob and op-trace context managers, and the checks of the C ABI that
need no device.  Not collected: the tests themselves, their cases and their restatements stay in their own files."""
import contextlib
import ctypes as C
import os

import numpy as np
import pytest

import client_sampling as CS
import hybrid_ref as HR
import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, EINVAL = 0, -1
IDENT = "identity"  # a step that is no rotation: the Galois element 1
MOAI_DATA_BITS = [51] + [46] * 20 + [51] * 14  # MOAI's 35 data primes
PATTERN = 0xABCD  # what an output buffer holds before a call that must write all of it
FILL = 7  # what an output buffer holds before a call that must leave it alone
KEY = bytes(range(32))  # the CPU tests' sampling key

# (logn, data bits, special bits): the small transform (logn 10) and the tiled one (logn 12), at alpha = 1 and above
ENVS = {"small1": (10, [60, 60], [60]), "tiled1": (12, [51, 46, 46], [58]), "small2": (10, [40, 41, 42, 43, 44], [60, 60]),
        "tiled3": (12, [51, 46, 46, 46, 51, 46, 51], [58, 60, 60])}


class Env:
    """one chain of primes, the last alpha of them special: the oracle's context and the device's"""

    def __init__(self, moai, logn, data_bits=None, special_bits=None, primes=None, alpha=None, oracle=True):
        self.moai = moai
        self.logn, self.n = logn, 1 << logn
        self.alpha = len(special_bits) if primes is None else alpha
        self.primes = O.coeff_modulus_create(self.n, list(data_bits) + list(special_bits)) if primes is None else list(primes)
        self.k = len(self.primes)
        self.lmax = self.k - self.alpha
        self.octx = O.Context(logn, self.primes) if oracle else None
        self.ctx = moai.Context(logn, self.primes)
        self.digits = HR.beta(self.lmax, self.alpha)
        self.cache = {}  # what a test file computes once per environment

    def up(self, a):
        return self.moai.DeviceBuffer.from_numpy(a)

    def filled(self, shape, value):
        return self.up(np.full(shape, value, dtype=np.uint64))

    def random_key(self, rng):
        return O.uniform_rns(rng, self.primes, (self.digits, 2), self.n)

    def elts(self, steps):
        """Galois elements of rotation steps: IDENT -> 1, step 0 -> the conjugation"""
        return [1 if s == IDENT else (self.ctx.galois_elt_from_step(s) if s else 2 * self.n - 1) for s in steps]

    def rows(self, L):
        """the primes of a plaintext's L + alpha rows"""
        return [self.primes[i] for i in list(range(L)) + list(range(self.k - self.alpha, self.k))]

    def random_input(self, rng, L, B):
        """[B][2][L][N] with no zero coefficient in any INTT(c1)"""
        ct = O.uniform_rns(rng, self.primes[:L], (B, 2), self.n)
        for b in range(B):
            assert self.octx.ntt(ct[b, 1], L, inverse=True).all(), b
        return ct

    def edge_targets(self, L):
        """[L][N] twice: every row m - 1, and zero"""
        top = np.stack([np.full(self.n, q - 1, dtype=np.uint64) for q in self.primes[:L]])
        return top, np.zeros_like(top)

    def edges(self, L, polys):
        """edge_targets as ciphertexts of `polys` polynomials"""
        return tuple(np.stack([a] * polys) for a in self.edge_targets(L))

    def close(self):
        self.ctx.close()


def _env_fixture(name):
    @pytest.fixture(scope="module", name="env_" + name)
    def fixture(moai):
        return Env(moai, *ENVS[name])
    return fixture


# module-scoped: a test file that imports them gets contexts of its own, which live as long as its tests
env_small1, env_tiled1, env_small2, env_tiled3 = (_env_fixture(name) for name in ENVS)


def cached(cache, key, make):
    if key not in cache:
        cache[key] = make()
    return cache[key]


def unit_plain(e, L):
    return lambda: np.ones((L + e.alpha, e.n), dtype=np.uint64)


@contextlib.contextmanager
def tuned(moai, **knobs):
    """set the named tuning knobs; on exit drop every override, those set inside the block too"""
    try:
        for knob, value in knobs.items():
            moai.hip.set_tuning(knob, value)
        yield
    finally:
        moai.hip.reset_tuning()


@contextlib.contextmanager
def traced(moai):
    """count the operations asked for inside the block; yields op_trace_counts, to be called once the count is wanted"""
    moai.hip.op_trace(True)
    try:
        yield moai.hip.op_trace_counts
    finally:
        moai.hip.op_trace(False)


# ---- the CPU files ------------------------------------------------------------------------------------------------------------------
# (data bits, special bits, levels) of the identities of hybrid_dot_ref and hybrid_bsgs_ref
UNIT_CASES = [([30, 31, 32], [40], (3, 1)), ([30, 31, 32, 33, 34], [40, 41], (5, 3, 1)), ([30, 31, 32, 33], [40, 41, 42], (4, 2))]
# (data bits, special bits, L, steps (0 = conjugation), bits of the plaintext coefficients) of their noise bounds
NOISE_CASES = [
    ([40, 41, 42, 43, 44], [60, 60], 5, [1, 3, -2, 5, 0], 20),
    ([40, 41, 42, 43, 44], [60, 60], 3, [1, 3, -2, 5, 0], 20),
    ([40, 41, 42, 43, 44], [60, 60], 1, [1, 0], 10),
    ([36] * 7, [58, 60, 60], 7, [1, 2, 3, 4, 5, -1, -2, 0], 16),
]


def elt_of(logn, step):
    return O.galois_elt_from_step(logn, step) if step else 2 * (1 << logn) - 1


def secret(octx, key, seq):
    """a ternary secret: (coefficients, NTT form over all k primes)"""
    s = CS.ternary(key, CS.nonce(CS.TERNARY, seq), octx.n)
    return s, octx.ntt(CS.to_rns(s, octx.primes), octx.k)


def exported(moai, names, methods):
    """the library exports `names`, the package declares them, and Context binds `methods`"""
    L = C.CDLL(moai.lib_path())
    for name in names:
        assert hasattr(L, name), name
        assert name in moai.hip.SYMBOLS, name
    for method in methods:
        assert callable(getattr(moai.Context, method)), method


def header():
    return open(os.path.join(ROOT, "include", "moai_hip.h")).read()


def header_comment(name):
    """the comment that sits directly on the declaration of `name` in include/moai_hip.h"""
    hdr = header()
    at = hdr.index(" " + name + "(")
    at = hdr.rindex("\n", 0, at) + 1  # the start of the declaration's line
    comment = hdr[hdr.rindex("/*", 0, at):at]
    assert comment.rstrip().endswith("*/"), name
    return comment
