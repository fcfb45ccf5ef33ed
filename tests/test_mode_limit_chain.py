"""The primes of tests/mode_limits.py sit where they claim to: on the stated side of each arithmetic mode's limit, with no
admissible prime between them and the limit, in exact integers; and the oracle round-trips every input pattern under them."""
import numpy as np
import pytest

import mode_limits as ML
import oracle as O

LOGNS = [12, 13, 14, 15, 16]

# the primes the oracle's own primality test finds on a CPU (cross-check of the search, not its source)
KNOWN = {
    12: [136472715927553, 136472716189697, 2251799813554177, 2251799813824513, 512409557603033089, 512409557603074049,
         1152921504606830593, 2305843009213554689, 1099511799809],
    16: [136472711790593, 136472717688833, 2251799813554177, 2251799815520257, 512409557602271233, 512409557604106241,
         1152921504606584833, 2305843009211596801, 1099512938497],
}


@pytest.mark.parametrize("logn", LOGNS)
def test_chain_is_distinct_prime_and_ntt_friendly(logn):
    c = ML.chain(logn)
    assert tuple(c) == ML.NAMES
    qs = list(c.values())
    assert len(set(qs)) == 9
    for q in qs:
        assert ML.is_prime(q) and O.lib().mo_is_prime(q), q
        assert q % (2 << logn) == 1, q
    if logn in KNOWN:
        assert qs == KNOWN[logn]
    for order in ML.ORDERS:
        assert sorted(ML.ordered(logn, order)) == sorted(qs)
    assert ML.ordered(logn, "g61_last")[-1] == c["g61"] and ML.ordered(logn, "fpr_hi_last")[-1] == c["fpr_hi"]
    # the oracle accepts the chain in both orders
    for order in ML.ORDERS:
        O.Context(logn, ML.ordered(logn, order))


@pytest.mark.parametrize("logn", LOGNS)
def test_each_prime_is_on_its_side_of_its_limit(logn):
    c = ML.chain(logn)
    assert 33 * c["fpn_hi"] < 1 << 52
    assert 33 * c["fpr_lo"] >= 1 << 52 and c["fpr_lo"] < 1 << 51
    assert c["fpr_hi"] < 1 << 51 and 33 * c["fpr_hi"] >= 1 << 52
    assert (1 << 51) <= c["int_lo"] < ML.NOGUARD_LIMIT
    assert (1 << 51) <= c["ng_hi"] < ML.NOGUARD_LIMIT and 36 * c["ng_hi"] < 1 << 64
    assert ML.NOGUARD_LIMIT <= c["g_lo"] < 1 << 60
    assert ML.NOGUARD_LIMIT <= c["g60"] < 1 << 60
    assert (1 << 60) <= c["g61"] < 1 << 61
    assert (1 << 40) < c["small"] and 33 * c["small"] < 1 << 52
    # the limits are the ones the code tests: 33 q < 2^52 <=> q <= FPN_LIMIT, q < floor((2^64 - 1) / 36)
    assert 33 * ML.FPN_LIMIT < 1 << 52 <= 33 * (ML.FPN_LIMIT + 1)
    assert ML.NOGUARD_LIMIT == 0xFFFFFFFFFFFFFFFF // 36


@pytest.mark.parametrize("logn", LOGNS)
def test_no_admissible_prime_between_a_prime_and_its_limit(logn):
    """walking one step of 2N at a time from each prime towards its limit meets no prime before it crosses the limit"""
    c = ML.chain(logn)
    m = 2 << logn

    def none_between(q, step, stays_inside):
        v = q + step * m
        while stays_inside(v):
            assert not ML.is_prime(v), (q, v)
            v += step * m

    none_between(c["fpn_hi"], +1, lambda v: 33 * v < 1 << 52)
    none_between(c["fpr_lo"], -1, lambda v: 33 * v >= 1 << 52)
    none_between(c["fpr_hi"], +1, lambda v: v < 1 << 51)
    none_between(c["int_lo"], -1, lambda v: v >= 1 << 51)
    none_between(c["ng_hi"], +1, lambda v: v < ML.NOGUARD_LIMIT)
    none_between(c["g_lo"], -1, lambda v: v >= ML.NOGUARD_LIMIT)
    none_between(c["g60"], +1, lambda v: v < 1 << 60)
    none_between(c["g61"], +1, lambda v: v < 1 << 61)
    none_between(c["small"], -1, lambda v: v > 1 << 40)
    # so the neighbour across each limit is on the other side: the pairs of the chain are adjacent admissible primes
    assert c["fpn_hi"] < c["fpr_lo"] and c["fpr_hi"] < c["int_lo"] and c["ng_hi"] < c["g_lo"]


def test_noguard_mac_switch_over_is_36():
    """36 q^2 L < 2^128 holds up to L = 36 for the prime just below 2^64 / 36 (not 35: q is below the limit), and fails at 37"""
    for logn in LOGNS:
        q = ML.chain(logn)["ng_hi"]
        Ls = ML.largest_noguard_L(q)
        assert 36 * q * q * Ls < 1 << 128 <= 36 * q * q * (Ls + 1)
        assert Ls == 36


def test_reference_key_cap():
    """the reference's own 128-bit lazy sum admits every key at the nine-prime chain's L = 8; on the long chains it caps the
    61-bit prime's key rows only"""
    for logn in LOGNS:
        for q in ML.chain(logn).values():
            assert ML.reference_key_cap(q, 8) == q - 1 and ML.reference_key_cap(q, 16) == q - 1
    for logn, k, Ls in ((12, 38, (17, 36, 37)), (16, 18, (17,))):
        primes, names = ML.long_chain(logn, k)
        for L in Ls:
            capped = [nm for q, nm in zip(primes, names) if ML.reference_key_cap(q, L) < q - 1]
            assert capped == ["g61"], (logn, L, capped)
            v = ML.reference_key_cap(primes[-1], L)
            assert 4 * primes[-1] * v * L < 1 << 128 <= 4 * primes[-1] * (v + 1) * L


@pytest.mark.parametrize("logn,k", [(12, 38), (16, 18)])
def test_long_chain(logn, k):
    primes, names = ML.long_chain(logn, k)
    assert len(primes) == k == len(set(primes)) == len(names)
    assert primes[:8] == ML.ordered(logn, "g61_last")[:8] and primes[-1] == ML.chain(logn)["g61"]
    for q, name in zip(primes, names):
        assert ML.is_prime(q) and q % (2 << logn) == 1
        if name.startswith("fpn_hi"):
            assert 33 * q < 1 << 52
        if name.startswith("fpr_hi"):
            assert 33 * q >= 1 << 52 and q < 1 << 51
        if name.startswith("ng_hi"):
            assert (1 << 51) <= q < ML.NOGUARD_LIMIT and ML.largest_noguard_L(q) == 36
    O.Context(logn, primes)


@pytest.mark.parametrize("logn", LOGNS)
def test_oracle_round_trips_every_pattern(logn):
    n = 1 << logn
    primes = ML.ordered(logn, "g61_last")
    x = ML.pattern_rows(primes, n, np.random.default_rng(logn))
    octx = O.Context(logn, primes)
    y = octx.ntt(x, len(primes))
    assert all((y[:, i] < q).all() for i, q in enumerate(primes))
    assert (octx.ntt(y, len(primes), inverse=True) == x).all()
    assert (octx.ntt(octx.ntt(x, len(primes), inverse=True), len(primes)) == x).all()
    for i, q in enumerate(primes):
        r = ML.rounding_row(q, n)
        assert (octx.ntt(octx.ntt(r, 1, prime_index=[i]), 1, prime_index=[i], inverse=True).reshape(n) == r).all()
