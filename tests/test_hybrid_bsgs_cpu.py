"""CPU-only checks of the giant steps summed in the extended basis (include/moai_hip.h, moai_hybrid_bsgs_dot).
(a) the two identities on the integer restatement tests/hybrid_bsgs_ref.py, at alpha = 1, 2, 3: one giant step of element 1 is
    hybrid_dot_ref.rotate_pt_dot with one output, and one identity baby term with the all-ones plaintext under one giant step E is
    hybrid_ref.apply_galois, both bit for bit;
(b) with real keys for sigma(s) -> s and plaintexts of uniform integer coefficients, decrypting the restatement's output with exact
    CRT gives an error within the header's bound
    (alpha - 1/2)(1 + |s|_1) + sum_g [ l_g u + [E_g != 1](u + (alpha - 1/2)|s|_1) ],  u = beta N alpha 21 D_max / P;
(c) the symbol is exported, declared and bound, its comment cites reference lines, and the refusals that need no context are
    answered before the device is touched."""
import ctypes as C
import re

import numpy as np
import pytest

import hybrid_bsgs_ref as HB
import hybrid_dot_ref as HD
import hybrid_ref as HR
import oracle as O
from hybrid_kit import EINVAL, KEY, NOISE_CASES, UNIT_CASES, elt_of, exported, header_comment, secret

NAME = "moai_hybrid_bsgs_dot"


# ---- (a) the two identities -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("data,special,levels", UNIT_CASES)
def test_one_giant_step_of_element_1_is_rotate_pt_dot(data, special, levels):
    logn, alpha = 5, len(special)
    primes = O.coeff_modulus_create(1 << logn, data + special)
    octx = O.Context(logn, primes)
    rng = np.random.default_rng(10 + alpha)
    elts = [1, elt_of(logn, 1), elt_of(logn, -2), elt_of(logn, 0)]
    keys = [None] + [O.uniform_rns(rng, primes, (HR.beta(len(data), alpha), 2), octx.n) for _ in elts[1:]]
    for L in levels:
        ct = O.uniform_rns(rng, primes[:L], (2,), octx.n)
        rows = [primes[i] for i in HD.HH.rows_of(octx, L, alpha)]
        plains = [[O.uniform_rns(rng, rows, (), octx.n) for _ in elts]]
        plains[0][2] = None
        got = HB.bsgs_dot(octx, ct, L, alpha, elts, keys, [1], [None], plains)
        assert (got == HD.rotate_pt_dot(octx, ct, L, alpha, elts, keys, plains)[0]).all(), L


@pytest.mark.parametrize("data,special,levels", UNIT_CASES)
def test_a_unit_plaintext_giant_step_is_apply_galois(data, special, levels):
    logn, alpha = 5, len(special)
    primes = O.coeff_modulus_create(1 << logn, data + special)
    octx = O.Context(logn, primes)
    rng = np.random.default_rng(20 + alpha)
    key = O.uniform_rns(rng, primes, (HR.beta(len(data), alpha), 2), octx.n)
    for L in levels:
        ct = O.uniform_rns(rng, primes[:L], (2,), octx.n)
        one = HD.ones_plain(octx, L, alpha)
        for step in (1, -2, 0):
            E = elt_of(logn, step)
            got = HB.bsgs_dot(octx, ct, L, alpha, [1], [None], [E], [key], [[one]])
            assert (got == HR.apply_galois(octx, ct, L, E, key, alpha)).all(), (L, step)


# ---- (b) the noise bound ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("data,special,L,steps,bits", NOISE_CASES)
def test_decryption_error_is_within_the_bound(data, special, L, steps, bits):
    """4 baby terms (one the identity), 4 giant steps (one the identity, one the conjugation), one absent term"""
    logn, alpha = 6, len(special)
    bits = max(bits, 16)  # 16 to 20 bits on every chain
    primes = O.coeff_modulus_create(1 << logn, data + special)
    octx = O.Context(logn, primes)
    s, sk = secret(octx, KEY, 1)
    rng = np.random.default_rng(2000 * alpha + 10 * L)
    baby = [1, elt_of(logn, 1), elt_of(logn, 2), elt_of(logn, 3)]
    giant = [1, elt_of(logn, 4), elt_of(logn, -8), elt_of(logn, 0)]

    def key_for(elt, seq):
        return None if elt == 1 else HR.keygen(octx, KEY, seq, sk, sk[:, O.galois_table_ntt(logn, elt)], alpha)

    bkeys = [key_for(e, 100 * (r + 1)) for r, e in enumerate(baby)]
    gkeys = [key_for(e, 100 * (g + 11)) for g, e in enumerate(giant)]
    coeffs = [[rng.integers(-(1 << bits) + 1, 1 << bits, octx.n) for _ in baby] for _ in giant]
    plains = [[HD.encode_plain(octx, c, L, alpha) for c in row] for row in coeffs]
    plains[1][2] = None
    ct = O.uniform_rns(rng, primes[:L], (2,), octx.n)
    out = HB.bsgs_dot(octx, ct, L, alpha, baby, bkeys, giant, gkeys, plains)
    l1 = [sum(int(np.abs(coeffs[g][r]).sum()) for r, e in enumerate(baby) if e != 1 and plains[g][r] is not None) for g in range(len(giant))]
    err = HB.bsgs_error(octx, out, ct, sk, L, baby, giant, plains)
    worst = max(abs(int(e)) for e in err)
    bound = HB.noise_bound(octx, L, alpha, int(np.count_nonzero(s)), giant, l1)
    print("alpha %d L %d: max |E| = %d, bound = %.1f" % (alpha, L, worst, bound))
    assert worst <= bound, (alpha, L, worst, bound)


# ---- (c) the C ABI --------------------------------------------------------------------------------------------------------------
def test_symbol_exported_declared_and_bound(moai):
    exported(moai, [NAME], ["hybrid_bsgs_dot"])


def test_header_comment_cites_reference_lines():
    comment = header_comment(NAME)
    assert re.search(r"Bootstrapper\.cpp:1997-2062", comment)
    assert re.search(r"SEAL/evaluator\.cpp:2724-3020", comment)


def test_arguments_refused_without_a_device(moai):
    lib = moai.hip.lib()
    p = 0x1000  # never dereferenced: every call below returns before it reaches the context
    fb = C.c_int(7)
    arr = (C.c_void_p * 1)(p)

    def call(L, alpha, baby=3, giant=5):
        be, ge = (C.c_uint32 * 1)(baby), (C.c_uint32 * 1)(giant)
        return lib.moai_hybrid_bsgs_dot(None, p, p + 0x100000, L, alpha, be, arr, arr, 1, ge, arr, 1, arr, 1, C.byref(fb), None)

    assert call(3, 0) == EINVAL and b"alpha = 0" in lib.moai_last_error()
    assert call(0, 2) == EINVAL and b"L = 0" in lib.moai_last_error()
    assert call(3, 2, baby=6) == EINVAL and b"Galois element is not valid" in lib.moai_last_error()
    assert call(3, 2, giant=8) == EINVAL and b"Galois element is not valid" in lib.moai_last_error()
    # with arguments that need the context to be judged, the missing context is what is reported
    assert call(3, 2) == EINVAL and b"null context" in lib.moai_last_error()
    assert fb.value == 0  # the flag is cleared before anything is judged
