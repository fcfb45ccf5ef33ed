"""Primes at the size limit of every arithmetic mode of the library (csrc/modarith.hip.h M_*), for the tests that run the
transforms, the key switch and mod-down where those limits bind.  No GPU, exact Python integers only.

Limits (each is what the code tests, in the same integer arithmetic):
    M_FPN      33 q < 2^52                           csrc/context.hip build_prime
    M_FPR      q < 2^51                              csrc/context.hip build_prime
    M_NOGUARD  q < floor((2^64 - 1) / 36)            csrc/ntt.hip noguard_ok; key switch: also 36 q^2 L < 2^128 (ks_mode)
    M_LAZY*    q < 2^60                              csrc/ntt.hip lazy8_ok (plain transforms only)
    M_GUARD*   q < 2^61
"""
import numpy as np

FPN_LIMIT = ((1 << 52) - 1) // 33  # largest q with 33 q < 2^52 (33 does not divide 2^52)
FPR_LIMIT = 1 << 51                # q < 2^51
NOGUARD_LIMIT = ((1 << 64) - 1) // 36  # q < this
LAZY_LIMIT = 1 << 60               # q < 2^60

# the names of chain(), in the order of their definition
NAMES = ("fpn_hi", "fpr_lo", "fpr_hi", "int_lo", "ng_hi", "g_lo", "g60", "g61", "small")
# two orders of the nine primes (the last one is the special prime of a key switch and the first one dropped by rescale):
#   g61_last     the special prime is the largest, SEAL's normal case
#   fpr_hi_last  the special prime is smaller than several data primes (the oracle's qk > qi branch), and the row that
#                mod-down inverts is an FP64 one
ORDERS = {
    "g61_last": ("fpn_hi", "fpr_lo", "fpr_hi", "int_lo", "ng_hi", "g_lo", "g60", "small", "g61"),
    "fpr_hi_last": ("g61", "g60", "g_lo", "ng_hi", "int_lo", "small", "fpr_lo", "fpn_hi", "fpr_hi"),
}
PATTERNS = ("all q-1", "all 0", "alternating 0 / q-1", "q/2 and q/2+1", "random")


def is_prime(n):
    """Miller-Rabin with the bases that decide every n < 2^64"""
    if n < 2:
        return False
    small = (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37)
    for p in small:
        if n % p == 0:
            return n == p
    d, s = n - 1, 0
    while d % 2 == 0:
        d //= 2
        s += 1
    for a in small:
        x = pow(a, d, n)
        if x in (1, n - 1):
            continue
        for _ in range(s - 1):
            x = x * x % n
            if x == n - 1:
                break
        else:
            return False
    return True


def prime_at_most(logn, bound):
    """the largest prime q = 1 (mod 2N) with q <= bound"""
    m = 2 << logn
    q = bound - (bound - 1) % m
    while not is_prime(q):
        q -= m
    return q


def prime_at_least(logn, bound):
    """the smallest prime q = 1 (mod 2N) with q >= bound"""
    m = 2 << logn
    q = bound + (1 - bound) % m
    while not is_prime(q):
        q += m
    return q


_chains = {}


def chain(logn):
    """{name: prime} for the nine names of NAMES"""
    if logn not in _chains:
        _chains[logn] = {
            "fpn_hi": prime_at_most(logn, FPN_LIMIT),         # largest with 33 q < 2^52
            "fpr_lo": prime_at_least(logn, FPN_LIMIT + 1),    # smallest with 33 q >= 2^52
            "fpr_hi": prime_at_most(logn, FPR_LIMIT - 1),     # largest below 2^51
            "int_lo": prime_at_least(logn, FPR_LIMIT),        # smallest at or above 2^51
            "ng_hi": prime_at_most(logn, NOGUARD_LIMIT - 1),  # largest below (2^64 - 1) / 36
            "g_lo": prime_at_least(logn, NOGUARD_LIMIT),      # smallest at or above it
            "g60": prime_at_most(logn, (1 << 60) - 1),        # largest below 2^60
            "g61": prime_at_most(logn, (1 << 61) - 1),        # largest below 2^61
            "small": prime_at_least(logn, (1 << 40) + 1),     # smallest above 2^40
        }
    return dict(_chains[logn])


def ordered(logn, order):
    """the nine primes in one of ORDERS"""
    c = chain(logn)
    return [c[name] for name in ORDERS[order]]


def long_chain(logn, k):
    """k distinct primes: the nine of chain() in the order g61_last, with the next primes below fpn_hi, below fpr_hi and below
    ng_hi, in turn, inserted before the special prime g61.  Returns (primes, names): names[i] is the chain name of prime i or
    the name of the limit prime it was found below, with a '-' suffix."""
    c = chain(logn)
    names = list(ORDERS["g61_last"])
    primes = [c[x] for x in names]
    m = 2 << logn
    cursor = {x: c[x] for x in ("fpn_hi", "fpr_hi", "ng_hi")}
    extra, extra_names = [], []
    turn = 0
    while len(primes) + len(extra) < k:
        x = ("fpn_hi", "fpr_hi", "ng_hi")[turn % 3]
        turn += 1
        q = prime_at_most(logn, cursor[x] - m)
        cursor[x] = q
        if q not in primes and q not in extra:
            extra.append(q)
            extra_names.append(x + "-")
    primes = primes[:-1] + extra + primes[-1:]
    names = names[:-1] + extra_names + names[-1:]
    assert len(set(primes)) == k
    return primes[:k], names[:k]


def largest_noguard_L(q):
    """the largest L with 36 q^2 L < 2^128 (the key switch's 128-bit lazy MAC, csrc/keyswitch.hip ks_mode)"""
    return ((1 << 128) - 1) // (36 * q * q)


def reference_key_cap(q, L):
    """The largest key residue under modulus q at which the REFERENCE's key switch at L digits is exact.  It adds the L products
    of a lazily transformed digit (below 4q, ntt_negacyclic_harvey_lazy) and a key residue in 128 bits and reduces once at the
    end (SEAL/evaluator.cpp:2856-2910; its counter allows 256 summands), so it needs 4 q v L < 2^128.  That is q - 1 for every
    prime below 2^60 at any L <= 64 and for 61-bit primes up to L = 16; beyond, a key of all q - 1 wraps the reference's sum
    (the library normalises the digit first and needs only q^2 L < 2^128)."""
    return min(q - 1, ((1 << 128) - 1) // (4 * q * L))


def pattern_rows(primes, n, rng):
    """uint64 [len(PATTERNS)][len(primes)][n]: every pattern under every prime"""
    out = np.zeros((len(PATTERNS), len(primes), n), dtype=np.uint64)
    for i, q in enumerate(primes):
        out[0, i, :] = q - 1
        out[2, i, 1::2] = q - 1
        out[3, i, 0::2] = q // 2
        out[3, i, 1::2] = q // 2 + 1
        out[4, i, :] = rng.integers(0, q, size=n, dtype=np.uint64)
    return out


def rounding_row(q, n):
    """the coefficients of a dropped row around the rounding boundary of divide-and-round: 0, q-1, q/2, q/2 +- 1, 1"""
    return np.resize(np.array([0, q - 1, q // 2, q // 2 + 1, q // 2 - 1, 1], dtype=np.uint64), n)
