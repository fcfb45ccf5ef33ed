"""CPU-only checks of the hybrid key switch (include/moai_hip.h, "hybrid key switching").
(a) the integer restatement tests/hybrid_ref.py at alpha = 1 IS the reference's switch and key: bit for bit the oracle's
    switch_key / relinearize / apply_galois and client_sampling's switching key;
(b) for alpha in {2, 3}, with full and partial last digits, decrypting the restatement's output with exact CRT gives an error
    within the header's bound B;
(c) the five symbols are exported and bound, their comments cite reference lines, and the refusals that need no context are
    answered before the device is touched."""
import re

import numpy as np
import pytest

import client_sampling as CS
import hybrid_ref as HR
import oracle as O
from hybrid_kit import EINVAL, KEY, exported, header_comment, secret

NAMES = ("moai_hybrid_digits", "moai_hybrid_keygen", "moai_switch_key_hybrid", "moai_relinearize_hybrid", "moai_apply_galois_hybrid")


# ---- (a) alpha = 1 is the reference -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=[6, 10])
def env1(request):
    logn = request.param
    primes = O.coeff_modulus_create(1 << logn, [40, 36, 36, 45])
    octx = O.Context(logn, primes)
    rng = np.random.default_rng(logn)
    return octx, rng, O.uniform_rns(rng, primes, (octx.k - 1, 2), octx.n)


@pytest.mark.parametrize("level", ["top", "one"])
def test_alpha_1_switch_is_the_oracles(env1, level):
    octx, rng, key = env1
    L = octx.k - 1 if level == "top" else 1
    ct = O.uniform_rns(rng, octx.primes[:L], (2,), octx.n)
    target = O.uniform_rns(rng, octx.primes[:L], (), octx.n)
    assert (HR.switch_key(octx, ct, target, key, L, 1) == octx.switch_key(ct, target, key, L).reshape(2, L, octx.n)).all()
    # limits of the residues: every row m - 1, and all zero
    top = np.stack([np.full(octx.n, q - 1, dtype=np.uint64) for q in octx.primes[:L]])
    for tgt in (top, np.zeros_like(top)):
        assert (HR.switch_key(octx, ct, tgt, key, L, 1) == octx.switch_key(ct, tgt, key, L).reshape(2, L, octx.n)).all()


@pytest.mark.parametrize("level", ["top", "one"])
def test_alpha_1_relinearize_and_galois_are_the_oracles(env1, level):
    octx, rng, key = env1
    L = octx.k - 1 if level == "top" else 1
    ct3 = O.uniform_rns(rng, octx.primes[:L], (3,), octx.n)
    assert (HR.relinearize(octx, ct3, key, L, 1) == octx.relinearize(ct3, key, L)).all()
    elt = O.galois_elt_from_step(octx.logn, 1)
    assert (HR.apply_galois(octx, ct3[:2], L, elt, key, 1) == octx.apply_galois(ct3[:2], L, elt, key).reshape(2, L, octx.n)).all()


def test_alpha_1_key_is_client_samplings(env1):
    octx, _, _ = env1
    _, sk = secret(octx, KEY, 1)
    _, new = secret(octx, KEY, 2)
    want = np.stack([CS.kswitch_digit(octx, KEY, 77, sk, new, J) for J in range(octx.k - 1)])
    assert (HR.keygen(octx, KEY, 77, sk, new, 1) == want).all()


# ---- (b) alpha > 1 is a key switch within the bound ---------------------------------------------------------------------------
# (alpha, data bits, special bits, levels): the top level with a full last digit, one with a partial last digit, one digit of one prime
NOISE_CASES = [(2, [30, 31, 32, 33], [40, 41], (4, 3, 1)), (3, [30, 31, 32, 30, 31, 32], [40, 41, 42], (6, 4, 2)),
               (1, [30, 31, 32], [40], (3, 1))]


@pytest.mark.parametrize("alpha,data,special,levels", NOISE_CASES)
def test_decryption_error_is_within_the_bound(alpha, data, special, levels):
    logn = 6
    primes = O.coeff_modulus_create(1 << logn, data + special)
    octx = O.Context(logn, primes)
    s, sk = secret(octx, KEY, 1)
    _, new = secret(octx, KEY, 2)
    key = HR.keygen(octx, KEY, 5, sk, new, alpha)
    assert key.shape == (HR.beta(len(data), alpha), 2, octx.k, octx.n)
    rng = np.random.default_rng(alpha)
    for L in levels:
        c = O.uniform_rns(rng, primes[:L], (), octx.n)
        d = HR.switch_key(octx, np.zeros((2, L, octx.n), dtype=np.uint64), c, key, L, alpha)
        err = HR.switch_error(octx, d, c, sk, new, L)
        worst = max(abs(int(e)) for e in err)
        bound = HR.noise_bound(octx, L, alpha, int(np.count_nonzero(s)))
        print("alpha %d L %d: max |E| = %d, B = %.1f" % (alpha, L, worst, bound))
        assert worst <= bound, (alpha, L, worst, bound)


# ---- (c) the C ABI --------------------------------------------------------------------------------------------------------------
def test_symbols_exported_and_declared(moai):
    exported(moai, NAMES, ("hybrid_digits", "hybrid_keygen", "switch_key_hybrid", "relinearize_hybrid", "apply_galois_hybrid"))


def test_header_comments_cite_reference_lines():
    for name in NAMES:
        assert re.search(r"SEAL/(evaluator\.cpp:2724-3020|keygenerator\.cpp:303-336)", header_comment(name)), name


def test_arguments_refused_without_a_device(moai):
    lib = moai.hip.lib()
    p = 0x1000  # never dereferenced: every call below returns before it reaches the context
    sw, rel, gal, gen, dig = (lib.moai_switch_key_hybrid, lib.moai_relinearize_hybrid, lib.moai_apply_galois_hybrid,
                              lib.moai_hybrid_keygen, lib.moai_hybrid_digits)
    # alpha = 0
    assert sw(None, p, p, p, 3, 0, 1, None) == EINVAL and b"alpha = 0" in lib.moai_last_error()
    assert rel(None, p, p, p, 3, 0, 1, None) == EINVAL and b"alpha = 0" in lib.moai_last_error()
    assert gal(None, p, 3, 0, 3, p, 1, None) == EINVAL and b"alpha = 0" in lib.moai_last_error()
    assert gen(None, KEY, 0, p, p, 0, p, None) == EINVAL and b"alpha = 0" in lib.moai_last_error()
    assert dig(None, 0, 3) == 0 and b"alpha = 0" in lib.moai_last_error()
    # L = 0
    assert sw(None, p, p, p, 0, 2, 1, None) == EINVAL and b"L = 0" in lib.moai_last_error()
    assert rel(None, p, p, p, 0, 2, 1, None) == EINVAL and b"L = 0" in lib.moai_last_error()
    assert gal(None, p, 0, 2, 3, p, 1, None) == EINVAL and b"L = 0" in lib.moai_last_error()
    assert dig(None, 2, 0) == 0 and b"L = 0" in lib.moai_last_error()
    # an even Galois element
    assert gal(None, p, 3, 2, 6, p, 1, None) == EINVAL and b"Galois element is not valid" in lib.moai_last_error()
    # with arguments that need the context to be judged, the missing context is what is reported
    assert sw(None, p, p, p, 3, 2, 1, None) == EINVAL and b"null context" in lib.moai_last_error()
    assert rel(None, p, p, p, 3, 2, 1, None) == EINVAL and b"null context" in lib.moai_last_error()
    assert gal(None, p, 3, 2, 3, p, 1, None) == EINVAL and b"null context" in lib.moai_last_error()
    assert gen(None, KEY, 0, p, p, 2, p, None) == EINVAL and b"null context" in lib.moai_last_error()
    assert dig(None, 2, 3) == 0 and b"null context" in lib.moai_last_error()
