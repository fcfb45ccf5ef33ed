"""CPU-only checks behind tests/test_gpu_hybrid_limits.py: the chains of tests/mode_limits.py for the hybrid key switch, and the two
integer restatements at those primes.
(a) every prime of every chain is prime, = 1 (mod 2N), distinct and on the intended side of its limit; worst_coeff gives the
    largest scaled residue q_r - 1 in every row of every digit and holds no zero;
(b) tests/hybrid_ref.py at alpha = 1 is the oracle's switch_key on both nine-prime orders of mode_limits.ORDERS, with key and digits
    all q - 1: the restatement is pinned at these primes, not only at the 30..45-bit ones of tests/test_hybrid_ref_cpu.py;
(c) tests/hybrid_hoist_ref.py equals tests/hybrid_ref.py's apply_galois per rotation on special_large and special_small, with
    worst_coeff digits, an all m - 1 key and a random key."""
import numpy as np
import pytest

import hybrid_hoist_ref as HH
import hybrid_ref as HR
import mode_limits as ML
import oracle as O

# the half-open range [lo, hi) every chain name promises; 'x-' lies in the range of x, below x
SIDE = {
    "small": ((1 << 40) + 1, ML.FPN_LIMIT + 1),
    "fpn_hi": ((1 << 40) + 1, ML.FPN_LIMIT + 1),
    "fpr_lo": (ML.FPN_LIMIT + 1, ML.FPR_LIMIT),
    "fpr_hi": (ML.FPN_LIMIT + 1, ML.FPR_LIMIT),
    "int_lo": (ML.FPR_LIMIT, ML.NOGUARD_LIMIT),
    "ng_hi": (ML.FPR_LIMIT, ML.NOGUARD_LIMIT),
    "g_lo": (ML.NOGUARD_LIMIT, ML.LAZY_LIMIT),
    "g60": (ML.NOGUARD_LIMIT, ML.LAZY_LIMIT),
    "g61": (ML.LAZY_LIMIT, 1 << 61),
}
ALL_CHAINS = [("special_large", None), ("special_small", None), ("long63", None)] + [("wide", a) for a in ML.WIDE_ALPHAS]


# ---- (a) the chains -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("logn", [10, 12, 16])
@pytest.mark.parametrize("which,alpha", ALL_CHAINS)
def test_chain_primes(logn, which, alpha):
    primes, names, a = ML.hybrid_chain(logn, which, alpha)
    c = ML.chain(logn)
    assert len(primes) == len(names) == len(set(primes))
    for q, name in zip(primes, names):
        base = name.rstrip("-")
        lo, hi = SIDE[base]
        assert ML.is_prime(q) and q % (2 << logn) == 1, (name, q)
        assert lo <= q < hi, (name, q)
        assert (q < c[base]) if name.endswith("-") else (q == c[base]), (name, q)
    L = len(primes) - a
    if which == "wide":
        assert a == alpha and L == alpha + 1 and all(q >> 60 for q in primes[:alpha] + primes[L:]) and names[alpha] == "small"
        assert primes[:alpha] + primes[L:] == sorted(primes[:alpha] + primes[L:], reverse=True)  # a run of neighbours, descending
    elif which == "long63":
        assert a == 1 and len(primes) == 64 and all(q >> 60 for q in primes) and primes == sorted(primes, reverse=True)
    else:
        assert a == 3 and L == 7
        D_max = max(HR._prod(primes[r] for r in HR.digit_rows(j, L, a)) for j in range(HR.beta(L, a)))
        P = HR._prod(primes[L:])
        assert (P > D_max) == (which == "special_large")
        if which == "special_small":
            assert max(primes[L:]) < ML.FPR_LIMIT and min(primes[L:]) < min(primes[:L])  # FP64 rows, one below every data prime


@pytest.mark.parametrize("which,alpha,L", [("special_large", None, 7), ("special_small", None, 4), ("special_small", None, 1),
                                           ("wide", 16, 17), ("wide", 4, 4), ("long63", None, 63)])
def test_worst_coeff_is_the_largest_scaled_residue(which, alpha, L):
    logn, n = 10, 8
    primes, _, a = ML.hybrid_chain(logn, which, alpha)
    c = ML.worst_coeff(primes, L, a, n)
    assert c.shape == (L, n) and c.all()
    for j in range(HR.beta(L, a)):
        R = HR.digit_rows(j, L, a)
        D = HR._prod(primes[r] for r in R)
        for r in R:
            q = primes[r]
            assert (c[r] < q).all()
            assert ((HR._obj(c[r]) * pow((D // q) % q, -1, q)) % q == q - 1).all(), (j, r)  # y_r of hybrid_ref.mod_up


# ---- (b) the restatement at alpha = 1 is the oracle's switch at the limit primes ---------------------------------------------------
@pytest.mark.parametrize("order", list(ML.ORDERS))
def test_alpha_1_restatement_is_the_oracles_switch_at_the_limits(order):
    logn, L = 12, 8
    n = 1 << logn
    primes = ML.ordered(logn, order)
    octx = O.Context(logn, primes)
    rng = np.random.default_rng(6100)
    key = np.empty((L, 2, len(primes), n), dtype=np.uint64)
    for i, q in enumerate(primes):
        key[:, :, i, :] = q - 1
    target = octx.ntt(np.stack([np.full(n, q - 1, dtype=np.uint64) for q in primes[:L]]), L)  # the digits are all q - 1
    ct = O.uniform_rns(rng, primes[:L], (2,), n)
    assert (HR.switch_key(octx, ct, target, key, L, 1) == octx.switch_key(ct, target, key, L).reshape(2, L, n)).all()


# ---- (c) the hoisted restatement equals separate rotations ---------------------------------------------------------------------------
@pytest.mark.parametrize("which", list(ML.HYBRID_CHAINS))
@pytest.mark.parametrize("L", [7, 4])
def test_hoisted_restatement_equals_separate_rotations_at_the_limits(which, L):
    logn = 12
    n = 1 << logn
    primes, _, alpha = ML.hybrid_chain(logn, which)
    octx = O.Context(logn, primes)
    rng = np.random.default_rng(6200 + L)
    digits = HR.beta(len(primes) - alpha, alpha)
    key_max = np.empty((digits, 2, len(primes), n), dtype=np.uint64)
    for i, q in enumerate(primes):
        key_max[:, :, i, :] = q - 1
    keys = [key_max, O.uniform_rns(rng, primes, (digits, 2), n)]
    elts = [O.galois_elt_from_step(logn, 1), 2 * n - 1]
    ct = O.uniform_rns(rng, primes[:L], (2,), n)
    ct[1] = octx.ntt(ML.worst_coeff(primes, L, alpha, n), L)
    got = HH.apply_galois_hoisted(octx, ct, L, elts, keys, alpha)
    for r, (elt, key) in enumerate(zip(elts, keys)):
        assert (got[r] == HR.apply_galois(octx, ct, L, elt, key, alpha)).all(), r
