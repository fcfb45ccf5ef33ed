"""CPU-only checks of the hybrid relinearize + rescale (include/moai_hip.h, "hybrid relinearize + rescale").  They pin the integer
restatement tests/hybrid_rescale_ref.py, at N = 2^6 with real keys for s^2 from hybrid_ref.keygen:
(a) with Z_p formed by exact CRT over Q_L P, floor((Z_p + H) / W) - out_p mod Q_{L-1}, centred, lies in [0, alpha] for every
    coefficient: the result is the rounded quotient less the fast conversion's overflow u' in [0, alpha];
(b) the distance to the composition oracle.rescale(hybrid_ref.relinearize(...)) lies in [-(alpha + 1), 1];
(c) the header's noise inequality holds;
(d) both symbols are exported, declared and bound, their comments cite the reference lines, and the refusals that need no context
    are answered before the device is touched.
Cases of (a)-(c): alpha in {1, 2, 3} with full and partial last digits, L down to 2, and alpha = 15 with seventeen 30-bit data primes."""
import re

import numpy as np
import pytest

import hybrid_ref as HR
import hybrid_rescale_ref as RR
import oracle as O
from hybrid_kit import EINVAL, KEY, exported, header, header_comment, secret

NAMES = ("moai_relinearize_rescale_hybrid", "moai_multiply_relin_rescale_hybrid")
LOGN = 6

# (alpha, data bits, special bits, levels): a full last digit, a partial one, q_{L-1} alone in the last digit, and L = 2
CASES = [(1, [30, 31, 32], [40], (3, 2)),
         (2, [30, 31, 32, 33, 34], [40, 41], (5, 4, 3, 2)),
         (3, [30, 31, 32, 30, 31, 32, 33], [40, 41, 42], (7, 6, 4, 2)),
         (15, [30] * 17, [32] * 15, (17, 16, 2))]
PAIRS = [(ci, L) for ci, case in enumerate(CASES) for L in case[3]]
_env, _run = {}, {}


def env(ci):
    """(octx, secret coefficients, secret NTT, relinearization key) of a case, made once"""
    if ci not in _env:
        alpha, data, special, _ = CASES[ci]
        octx = O.Context(LOGN, O.coeff_modulus_create(1 << LOGN, data + special))
        s, sk = secret(octx, KEY, 1)
        s2 = np.stack([HR._u64(HR._obj(sk[r]) * HR._obj(sk[r]) % q) for r, q in enumerate(octx.primes)])
        _env[ci] = octx, s, sk, HR.keygen(octx, KEY, 5, sk, s2, alpha)
    return _env[ci]


def run(ci, L):
    """(ct3, the restatement's output) of a case at L, computed once and shared by (a)-(c)"""
    if (ci, L) not in _run:
        octx, _, _, key = env(ci)
        rng = np.random.default_rng(100 * ci + L)
        ct3 = O.uniform_rns(rng, octx.primes[:L], (3,), octx.n)
        _run[ci, L] = ct3, RR.relinearize_rescale(octx, ct3, key, L, CASES[ci][0])
    return _run[ci, L]


def coefficients(octx, poly, L):
    """a polynomial [L][N] in NTT form as centred-free integers in [0, Q_L)"""
    return RR.crt(octx, list(poly), range(L))


# ---- (a) the rounded quotient less an overflow in [0, alpha] ----------------------------------------------------------------------
@pytest.mark.parametrize("ci,L", PAIRS)
def test_result_is_the_rounded_quotient_less_the_overflow(ci, L):
    octx, _, _, key = env(ci)
    alpha = CASES[ci][0]
    ct3, out = run(ci, L)
    sp = HR.special_rows(octx.k, alpha)
    W = HR._prod(octx.primes[r] for r in [L - 1] + sp)
    Q_lo = HR._prod(octx.primes[:L - 1])
    Z = RR.lifted(octx, ct3, key, L, alpha)
    seen = set()
    for p in range(2):
        z = RR.crt(octx, list(Z[p]), list(range(L)) + sp)  # exact, in [0, Q_L P)
        u = RR.centred(((z + W // 2) // W - coefficients(octx, out[p], L - 1)) % Q_lo, Q_lo)
        seen |= set(int(v) for v in u)
    print("alpha %d L %d: overflow values %s" % (alpha, L, sorted(seen)))
    assert min(seen) >= 0 and max(seen) <= alpha, (alpha, L, sorted(seen))


# ---- (b) the distance to the composition ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("ci,L", PAIRS)
def test_distance_to_the_composition(ci, L):
    octx, _, _, key = env(ci)
    alpha = CASES[ci][0]
    ct3, out = run(ci, L)
    comp = octx.rescale(HR.relinearize(octx, ct3, key, L, alpha), 2, L)
    Q_lo = HR._prod(octx.primes[:L - 1])
    seen = set()
    for p in range(2):
        d = RR.centred((coefficients(octx, out[p], L - 1) - coefficients(octx, comp[p], L - 1)) % Q_lo, Q_lo)
        seen |= set(int(v) for v in d)
    print("alpha %d L %d: out - composition in %s" % (alpha, L, sorted(seen)))
    assert min(seen) >= -(alpha + 1) and max(seen) <= 1, (alpha, L, sorted(seen))


# ---- (c) the noise inequality -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ci,L", PAIRS)
def test_noise_is_within_the_bound(ci, L):
    octx, s, sk, _ = env(ci)
    alpha = CASES[ci][0]
    ct3, out = run(ci, L)
    err = RR.rescale_error(octx, out, ct3, sk, L)
    worst = max(abs(int(e)) for e in err)
    bound = RR.noise_bound(octx, L, alpha, int(np.count_nonzero(s)))
    print("alpha %d L %d: max |E| = %d, bound = %.4g, ratio %.3f" % (alpha, L, worst, bound, worst / bound))
    assert worst <= bound, (alpha, L, worst, bound)


def test_product_is_the_oracles_multiply_and_square():
    octx = env(1)[0]
    L = 4
    rng = np.random.default_rng(7)
    x, y = O.uniform_rns(rng, octx.primes[:L], (2,), octx.n), O.uniform_rns(rng, octx.primes[:L], (2,), octx.n)
    assert (RR.ct_product(octx, x, y, L) == octx.multiply(x, y, L)).all()
    assert (RR.ct_product(octx, x, x, L) == octx.square(x, L)).all()


# ---- (d) the C ABI ------------------------------------------------------------------------------------------------------------------
def test_symbols_exported_and_declared(moai):
    exported(moai, NAMES, ("relinearize_rescale_hybrid", "multiply_relin_rescale_hybrid"))
    hdr = header()
    for name in NAMES:
        assert re.search(r"^int " + name + r"\(", hdr, re.M), name


def test_header_comments_cite_reference_lines():
    for name in NAMES:
        comment = header_comment(name)
        assert "SEAL/evaluator.cpp:2724-3020" in comment, name  # switch_key_inplace
        for cite in ("SEAL/evaluator.cpp:1682-1720", ":1402-1481", "SEAL/util/rns.cpp:830-901"):  # what moai_rescale's comment cites
            assert cite in comment, (name, cite)


def test_arguments_refused_without_a_device(moai):
    lib = moai.hip.lib()
    p = 0x1000  # never dereferenced: every call below returns before it reaches the context
    calls = (lambda L, alpha: lib.moai_relinearize_rescale_hybrid(None, p, p, p, L, alpha, 1, None),
             lambda L, alpha: lib.moai_multiply_relin_rescale_hybrid(None, p, p, p, p, L, alpha, 1, None))
    for call in calls:
        # hy_check's own, in its order, then the two this section adds
        for L, alpha, msg in ((3, 0, b"alpha = 0"), (1, 0, b"alpha = 0"), (0, 2, b"L = 0"), (0, 16, b"L = 0"), (1, 2, b"L = 1"),
                              (1, 16, b"L = 1"), (3, 16, b"alpha = 16")):
            assert call(L, alpha) == EINVAL and msg in lib.moai_last_error(), (L, alpha, lib.moai_last_error())
        # with arguments that need the context to be judged, the missing context is what is reported
        assert call(3, 2) == EINVAL and b"null context" in lib.moai_last_error()
        assert call(2, 15) == EINVAL and b"null context" in lib.moai_last_error()
