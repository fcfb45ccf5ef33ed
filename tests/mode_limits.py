"""Primes at the size limit of every arithmetic mode of the library (csrc/modarith.hip.h M_*), for the tests that run the
transforms, the key switch and mod-down where those limits bind.  No GPU, exact Python integers only.

Limits (each is what the code tests, in the same integer arithmetic):
    M_FPN      33 q < 2^52                           csrc/context.hip build_prime
    M_FPR      q < 2^51                              csrc/context.hip build_prime
    M_NOGUARD  q < floor((2^64 - 1) / 36)            csrc/ntt.hip noguard_ok; key switch: also 36 q^2 L < 2^128 (ks_mode)
    M_LAZY*    q < 2^60                              csrc/ntt.hip lazy8_ok (plain transforms only)
    M_GUARD*   q < 2^61
and, outside the modes, the fold period of the FP64 matrix product (csrc/elementwise.hip ct_pt_matmul_fp_kernel):
    every 16 rows   q < floor(2^52 / 25), every row otherwise (the kernel itself is taken when every prime is below 2^51)

Every search below works at any degree: chain(), ordered() and long_chain() hold for logn 1 .. 16 and give primes of the same bit
lengths (47, 47, 51, 52, 59, 59, 60, 61, 41) at each of them; the degrees below 2^12 have no arithmetic modes, the limits are the
same numbers there.
"""
import numpy as np

FPN_LIMIT = ((1 << 52) - 1) // 33  # largest q with 33 q < 2^52 (33 does not divide 2^52)
FPR_LIMIT = 1 << 51                # q < 2^51
NOGUARD_LIMIT = ((1 << 64) - 1) // 36  # q < this
LAZY_LIMIT = 1 << 60               # q < 2^60
MATMUL_FOLD_LIMIT = (1 << 52) // 25  # q < this: ct_pt_matmul_fp_kernel folds its sums every 16 rows, else every row

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


_matmul_chains = {}


def matmul_chain(logn):
    """chain(logn) and the two primes on either side of the FP64 matrix product's fold limit (NAMES and ORDERS do not know them):
    mm_hi the largest below MATMUL_FOLD_LIMIT, mm_lo the smallest at or above it"""
    if logn not in _matmul_chains:
        _matmul_chains[logn] = dict(chain(logn), mm_hi=prime_at_most(logn, MATMUL_FOLD_LIMIT - 1),
                                    mm_lo=prime_at_least(logn, MATMUL_FOLD_LIMIT))
    return dict(_matmul_chains[logn])


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


# ---- the written contract of the plain transforms: the arithmetic class of every chain prime ----------------------------------
# plain forward transform: (MOAI_NTT_FP=1, MOAI_NTT_FP=0)
FWD_CLASS = {
    "fpn_hi": ("FPN", "NOGUARD"), "fpr_lo": ("FPR", "NOGUARD"), "fpr_hi": ("FPR", "NOGUARD"), "int_lo": ("NOGUARD", "NOGUARD"),
    "ng_hi": ("NOGUARD", "NOGUARD"), "g_lo": ("LAZY16", "LAZY16"), "g60": ("LAZY16", "LAZY16"), "g61": ("GUARD2", "GUARD2"),
    "small": ("FPN", "NOGUARD"),
}
# plain inverse transform: GUARD = the exact integer butterflies
INV_CLASS = {
    "fpn_hi": ("FPN", "LAZY16"), "fpr_lo": ("FPR", "LAZY16"), "fpr_hi": ("FPR", "LAZY16"), "int_lo": ("LAZY16", "LAZY16"),
    "ng_hi": ("LAZY16", "LAZY16"), "g_lo": ("LAZY16", "LAZY16"), "g60": ("LAZY16", "LAZY16"), "g61": ("GUARD", "GUARD"),
    "small": ("FPN", "LAZY16"),
}


# ---- chains for the hybrid key switch (alpha special primes, digits of alpha data primes) ------------------------------------
# name: (data primes, special primes); 'x-' is the next prime = 1 (mod 2N) below the limit prime x, as in long_chain
HYBRID_CHAINS = {
    # P above every digit's product; the classes of the data rows interleave
    "special_large": (("fpn_hi", "g_lo", "fpr_hi", "ng_hi", "small", "fpr_lo", "int_lo"), ("g60", "g61", "ng_hi-")),
    # P far below D_max (the header's P >= D_max is a precondition of use, not of bit-exactness): the mod-down's inverse
    # transform runs on FP64 rows, its conversion goes from small sources to 61-bit targets, the mod-up from 61-bit sources to
    # the prime just above 2^40
    "special_small": (("g61", "fpn_hi", "g60", "fpr_lo", "g_lo", "int_lo", "ng_hi"), ("fpr_hi", "small", "fpn_hi-")),
}
WIDE_ALPHAS = (2, 4, 8, 16)


def primes_below(logn, q, count):
    """the next `count` primes = 1 (mod 2N) below q, descending"""
    m = 2 << logn
    out = []
    for _ in range(count):
        q = prime_at_most(logn, q - m)
        out.append(q)
    return out


def hybrid_chain(logn, which, alpha=None):
    """(primes, names, alpha): the data primes, then the alpha special primes; all distinct.  names[i] is the chain() name of prime i,
    or the name of the limit prime it was found below with a '-' suffix.
        special_large, special_small   HYBRID_CHAINS, alpha = 3
        wide (alpha in WIDE_ALPHAS)    data: g61 and the next alpha - 1 primes below it (digit 0, all 61-bit), then small as a last
                                       digit of one prime; special: the next alpha primes below those
        long63                         alpha = 1; data: g61 and the 62 next primes below it; special: the next one (k = 64, the
                                       library's MOAI_MAX_RNS, and 63 digits at L = 63)"""
    c = chain(logn)
    if which in HYBRID_CHAINS:
        assert alpha in (None, 3)
        names = list(HYBRID_CHAINS[which][0] + HYBRID_CHAINS[which][1])
        primes = [primes_below(logn, c[x[:-1]], 1)[0] if x.endswith("-") else c[x] for x in names]
        alpha = 3
    elif which == "wide":
        assert alpha in WIDE_ALPHAS
        run = primes_below(logn, c["g61"], 2 * alpha - 1)
        primes = [c["g61"]] + run[:alpha - 1] + [c["small"]] + run[alpha - 1:]
        names = ["g61"] + ["g61-"] * (alpha - 1) + ["small"] + ["g61-"] * alpha
    elif which == "long63":
        assert alpha in (None, 1)
        alpha = 1
        primes = [c["g61"]] + primes_below(logn, c["g61"], 63)
        names = ["g61"] + ["g61-"] * 63
    else:
        raise ValueError(which)
    assert len(set(primes)) == len(primes) == len(names)
    return primes, names, alpha


def worst_coeff(primes, L, alpha, n):
    """uint64 [L][n], coefficient form: row r of digit j (rows R_j = [j alpha, min((j + 1) alpha, L)), D_j their product) holds
    c_r = (q_r - 1) (D_j / q_r) mod q_r in every coefficient.  The scaled residue y_r = c_r (D_j / q_r)^-1 mod q_r that the fast base
    conversion multiplies its weights with is then q_r - 1, the largest there is, in every row of every digit; and no coefficient is
    zero (both factors are units), so the hoisted rotations do not fall back."""
    out = np.empty((L, n), dtype=np.uint64)
    for lo in range(0, L, alpha):
        rows = range(lo, min(lo + alpha, L))
        for r in rows:
            q, rest = primes[r], 1
            for s in rows:
                if s != r:
                    rest = rest * primes[s] % q
            out[r, :] = (q - 1) * rest % q
    return out


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


# ---- element-wise kernels ------------------------------------------------------------------------------------------------------
def pair_values(q):
    """the residues whose sums, differences and products sit on the boundaries of the conditional subtractions and of Barrett's
    quotient estimate"""
    return (0, 1, q - 1, q // 2, q // 2 + 1)


def pair_patterns(q, n, rng):
    """(a, b), uint64 [n] each: the 25 ordered pairs of pair_values(q) in coefficients 0 .. 24 (a walks the five values with period 5,
    b with period 25), uniform residues below q from coefficient 25 on.  For n < 25 only the first n pairs fit: a row of a smaller
    degree does not hold all of them (pair_rows starts every row elsewhere in the cycle, so that the pairs of short rows differ)."""
    v = np.array(pair_values(q), dtype=np.uint64)
    a = rng.integers(0, q, size=n, dtype=np.uint64)
    b = rng.integers(0, q, size=n, dtype=np.uint64)
    m = min(n, 25)
    i = np.arange(m)
    a[:m] = v[i % 5]
    b[:m] = v[i // 5]
    return a, b


def pair_rows(primes, n_poly, n, rng):
    """(a, b) uint64 [n_poly][len(primes)][n]: pair_patterns per row.  Polynomial p and row r start 5 (p + r) + p pairs into the cycle
    of 25 (both operands alike, so the pairs stay pairs): a short row (n < 25) then holds other pairs in every row and
    polynomial, and the nine rows of a polynomial hold all 25 between them from n = 8 on"""
    a = np.empty((n_poly, len(primes), n), dtype=np.uint64)
    b = np.empty_like(a)
    for p in range(n_poly):
        for r, q in enumerate(primes):
            x, y = pair_patterns(q, max(n, 32), rng)
            s = -(5 * (p + r) + p) % 25
            x[:25], y[:25] = np.roll(x[:25], s), np.roll(y[:25], s)
            a[p, r], b[p, r] = x[:n], y[:n]
    return a, b


def matmul_worst(q, rows, cols, n, rng):
    """(x, w, w_neg) for one prime of ct_pt_matmul: x uint64 [rows][n], w and w_neg uint64 [rows][cols].
    x: h = (q - 1) / 2 in the even coefficients and h + 1 in the odd ones, in every row: +h and -h in the balanced representation
    the FP64 kernel works in.  w[j][c] = 2 m + 1 with a fresh m < 2^16 per (j, c), so x w = m q + (h - m): the residue of every
    product is within 2^16 of q / 2, with one sign for all rows of a coefficient (+ in the even, - in the odd ones), and the real
    quotient (m + 1/2 - (m + 1/2) / q) is within 2^-30 of a half-integer, where the kernel's estimate rint(h qinv) may go either
    way.  w_neg = q - w: the same with the signs exchanged."""
    h = (q - 1) // 2
    x = np.empty((rows, n), dtype=np.uint64)
    x[:, 0::2] = h
    x[:, 1::2] = h + 1
    w = rng.integers(0, 1 << 16, size=(rows, cols), dtype=np.uint64) * np.uint64(2) + np.uint64(1)
    return x, w, np.uint64(q) - w


def _shift_mod(v, bits, q):
    """v 2^bits mod q for uint64 v below q < 2^52, twelve bits at a time (v 2^12 < 2^64)"""
    q = np.uint64(q)
    while bits:
        s = min(bits, 12)
        v = (v << np.uint64(s)) % q
        bits -= s
    return v


def matmul_mod(x, w, q):
    """sum_j x[j] w[j][c] mod q as uint64 [cols][...] for x uint64 [rows][...] and w uint64 [rows][cols], both below q < 2^52, at
    most 2^12 rows; exact integer arithmetic: operands split at bit 26, the four sums of partial products stay below 2^64
    (tests/test_elementwise_limits_cpu.py pins it against Python integers)"""
    assert q < 1 << 52 and x.shape[0] == w.shape[0] <= 1 << 12
    lo = np.uint64((1 << 26) - 1)
    xs = x.reshape(x.shape[0], -1)
    x0, x1, w0, w1 = xs & lo, xs >> np.uint64(26), w & lo, w >> np.uint64(26)
    qq = np.uint64(q)
    s00, s01, s10, s11 = (np.tensordot(b, a, axes=(0, 0)) % qq for a, b in ((x0, w0), (x0, w1), (x1, w0), (x1, w1)))
    out = (s00 + _shift_mod((s01 + s10) % qq, 26, q) + _shift_mod(s11, 52, q)) % qq
    return out.reshape((w.shape[1],) + x.shape[1:])
