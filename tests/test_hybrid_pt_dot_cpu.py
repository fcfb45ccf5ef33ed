"""CPU-only checks of the plaintext-weighted sums of hoisted rotations (include/moai_hip.h, moai_hybrid_rotate_pt_dot).
(a) with one output, one rotation and p = 1 the integer restatement tests/hybrid_dot_ref.py is hybrid_ref.apply_galois bit for bit,
    at alpha = 1, 2, 3; an identity term is the plain product;
(b) with real keys for sigma_r(s) -> s and plaintexts of uniform integer coefficients, decrypting the restatement's outputs with
    exact CRT gives an error within the header's bound (sum_r |p_r|_1) beta N alpha 21 D_max / P + (alpha - 1/2)(1 + |s|_1);
(c) the symbol is exported and bound, its comment cites reference lines, and the refusals that need no context are answered before
    the device is touched."""
import ctypes as C
import re

import numpy as np
import pytest

import hybrid_dot_ref as HD
import hybrid_ref as HR
import oracle as O
from hybrid_kit import EINVAL, KEY, NOISE_CASES, UNIT_CASES, elt_of, exported, header_comment, secret

NAME = "moai_hybrid_rotate_pt_dot"


# ---- (a) one rotation with p = 1 is the separate rotation ----------------------------------------------------------------------
@pytest.mark.parametrize("data,special,levels", UNIT_CASES)
def test_one_rotation_with_the_unit_plaintext_is_apply_galois(data, special, levels):
    logn, alpha = 5, len(special)
    primes = O.coeff_modulus_create(1 << logn, data + special)
    octx = O.Context(logn, primes)
    rng = np.random.default_rng(alpha)
    key = O.uniform_rns(rng, primes, (HR.beta(len(data), alpha), 2), octx.n)
    for L in levels:
        ct = O.uniform_rns(rng, primes[:L], (2,), octx.n)
        one = HD.ones_plain(octx, L, alpha)
        for step in (1, -2, 0):
            elt = elt_of(logn, step)
            got = HD.rotate_pt_dot(octx, ct, L, alpha, [elt], [key], [[one]])
            assert (got[0] == HR.apply_galois(octx, ct, L, elt, key, alpha)).all(), (L, step)
        # the element 1 is a plain product and reads no key; an output of such terms only skips step 5
        got = HD.rotate_pt_dot(octx, ct, L, alpha, [1], [None], [[one]])
        assert (got[0] == ct).all(), L


# ---- (b) the noise bound ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("data,special,L,steps,bits", NOISE_CASES)
def test_decryption_error_is_within_the_bound(data, special, L, steps, bits):
    logn, alpha = 6, len(special)
    primes = O.coeff_modulus_create(1 << logn, data + special)
    octx = O.Context(logn, primes)
    s, sk = secret(octx, KEY, 1)
    rng = np.random.default_rng(1000 * alpha + 10 * L + len(steps))
    elts = [elt_of(logn, st) for st in steps]
    keys = [HR.keygen(octx, KEY, 100 * (r + 1), sk, sk[:, O.galois_table_ntt(logn, elt)], alpha) for r, elt in enumerate(elts)]
    coeffs = [[rng.integers(-(1 << bits) + 1, 1 << bits, octx.n) for _ in elts] for _ in range(2)]
    plains = [[HD.encode_plain(octx, c, L, alpha) for c in row] for row in coeffs]
    plains[1][1] = None  # the second output lacks one rotation
    ct = O.uniform_rns(rng, primes[:L], (2,), octx.n)
    outs = HD.rotate_pt_dot(octx, ct, L, alpha, elts, keys, plains)
    for g in range(2):
        l1 = sum(int(np.abs(coeffs[g][r]).sum()) for r in range(len(steps)) if plains[g][r] is not None)
        err = HD.dot_error(octx, outs[g], ct, sk, L, elts, plains[g])
        worst = max(abs(int(e)) for e in err)
        bound = HD.noise_bound(octx, L, alpha, int(np.count_nonzero(s)), l1)
        print("alpha %d L %d R %d output %d: max |E| = %d, bound = %.1f" % (alpha, L, len(steps), g, worst, bound))
        assert worst <= bound, (alpha, L, g, worst, bound)


# ---- (c) the C ABI --------------------------------------------------------------------------------------------------------------
def test_symbol_exported_and_declared(moai):
    exported(moai, [NAME], ["hybrid_rotate_pt_dot"])


def test_header_comment_cites_reference_lines():
    comment = header_comment(NAME)
    assert re.search(r"Bootstrapper\.cpp:2017-2042, 2082-2108", comment)
    assert re.search(r"SEAL/evaluator\.cpp:2724-3020", comment)


def test_arguments_refused_without_a_device(moai):
    lib = moai.hip.lib()
    p = 0x1000  # never dereferenced: every call below returns before it reaches the context
    fb = C.c_int(7)
    arr = (C.c_void_p * 1)(p)

    def call(L, alpha, elt=3):
        elts = (C.c_uint32 * 1)(elt)
        return lib.moai_hybrid_rotate_pt_dot(None, p, arr, 1, L, alpha, elts, arr, arr, 1, arr, 1, C.byref(fb), None)

    assert call(3, 0) == EINVAL and b"alpha = 0" in lib.moai_last_error()
    assert call(0, 2) == EINVAL and b"L = 0" in lib.moai_last_error()
    assert call(3, 2, elt=6) == EINVAL and b"Galois element is not valid" in lib.moai_last_error()
    # with arguments that need the context to be judged, the missing context is what is reported
    assert call(3, 2) == EINVAL and b"null context" in lib.moai_last_error()
    assert fb.value == 0  # the flag is cleared before anything is judged
