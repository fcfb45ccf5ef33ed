"""CPU-only checks of the hoisted rotations over the hybrid key switch (include/moai_hip.h, "hoisted rotations over the hybrid key
switch").
(a) the identity: tests/hybrid_hoist_ref.py (digits of the unpermuted c1 built once, permuted per rotation, plus the correction)
    equals tests/hybrid_ref.py's apply_galois per rotation bit for bit, with digits of two and three primes, a partial last digit,
    alpha = 1, rotations to the left and right and the conjugation;
(b) the two symbols are exported and bound, their comments cite reference lines, and the refusals that need no context are answered
    before the device is touched."""
import ctypes as C
import re

import numpy as np
import pytest

import hybrid_hoist_ref as HH
import hybrid_ref as HR
import oracle as O
from hybrid_kit import EINVAL, exported, header, header_comment

NAMES = ("moai_hybrid_hoist_correction", "moai_apply_galois_hybrid_hoisted")

# (logn, data bits, special bits, L, steps); step 0 is the conjugation
SHAPES = [
    (5, [30, 31, 32, 33, 34], [40, 41], 5, [1, -2, 0]),
    (5, [30, 31, 32, 33, 34], [40, 41], 3, [3]),
    (6, [30, 31, 32, 33], [40, 41, 42], 4, [1, 0]),
    (5, [30, 31, 32], [40], 3, [1]),
]


# ---- (a) the identity -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("logn,data,special,L,steps", SHAPES)
def test_hoisted_restatement_equals_separate_rotations(logn, data, special, L, steps):
    alpha = len(special)
    primes = O.coeff_modulus_create(1 << logn, data + special)
    octx = O.Context(logn, primes)
    rng = np.random.default_rng(1000 * logn + 10 * alpha + L)
    ct = O.uniform_rns(rng, primes[:L], (2,), octx.n)
    assert octx.ntt(ct[1], L, inverse=True).all()  # the identity's precondition: no zero coefficient in INTT(c1)
    elts = [O.galois_elt_from_step(logn, s) for s in steps]
    keys = [O.uniform_rns(rng, primes, (HR.beta(len(data), alpha), 2), octx.n) for _ in steps]
    got = HH.apply_galois_hoisted(octx, ct, L, elts, keys, alpha)
    for r, (elt, key) in enumerate(zip(elts, keys)):
        assert (got[r] == HR.apply_galois(octx, ct, L, elt, key, alpha)).all(), (steps[r], "rotation")


def test_sign_mask_marks_the_negated_coefficients():
    """x -> x^elt on a polynomial of ones: the coefficients that come out as q - 1 are the mask"""
    logn, q = 5, 97 * 64 + 1
    n = 1 << logn
    for elt in (3, 5, 2 * n - 1):
        out = np.zeros(n, dtype=np.int64)
        for i in range(n):
            raw = (i * elt) % (2 * n)
            out[raw % n] = q - 1 if raw >= n else 1
        assert ((out == q - 1) == (HH.sign_mask(logn, elt) == 1)).all(), elt


# ---- (b) the C ABI --------------------------------------------------------------------------------------------------------------
def test_symbols_exported_and_declared(moai):
    exported(moai, NAMES, ("hybrid_hoist_correction", "apply_galois_hybrid_hoisted"))


def test_header_comments_cite_reference_lines():
    for name in NAMES:
        assert re.search(r"SEAL/evaluator\.cpp:2724-3020", header_comment(name)), name
    assert "MOAI_HYBRID_HOIST_NR" in header()


def test_arguments_refused_without_a_device(moai):
    lib = moai.hip.lib()
    p = 0x1000  # never dereferenced: every call below returns before it reaches the context
    corr, hoisted = lib.moai_hybrid_hoist_correction, lib.moai_apply_galois_hybrid_hoisted
    fb = C.c_int(7)
    arr = (C.c_void_p * 1)(p)
    elts = (C.c_uint32 * 1)(3)

    def call(L, alpha):
        return hoisted(None, p, arr, L, alpha, elts, arr, arr, 1, 1, C.byref(fb), None)

    # alpha = 0
    assert corr(None, p, 3, 3, 0, p, None) == EINVAL and b"alpha = 0" in lib.moai_last_error()
    assert call(3, 0) == EINVAL and b"alpha = 0" in lib.moai_last_error()
    # L = 0
    assert corr(None, p, 3, 0, 2, p, None) == EINVAL and b"L = 0" in lib.moai_last_error()
    assert call(0, 2) == EINVAL and b"L = 0" in lib.moai_last_error()
    # an even Galois element
    assert corr(None, p, 6, 3, 2, p, None) == EINVAL and b"Galois element is not valid" in lib.moai_last_error()
    # with arguments that need the context to be judged, the missing context is what is reported
    assert corr(None, p, 3, 3, 2, p, None) == EINVAL and b"null context" in lib.moai_last_error()
    assert call(3, 2) == EINVAL and b"null context" in lib.moai_last_error()
    assert fb.value == 0  # the flag is cleared before anything is judged
