"""The constructors of tests/mode_limits.py that the element-wise and small-degree GPU tests stand on, pinned in exact Python
integers: the primes on either side of the FP64 matrix product's fold limit, the pair patterns, the worst-case matrix product
and the exact reference product.  No GPU."""
import numpy as np
import pytest

import mode_limits as ML
import oracle as O

MM_KNOWN = {12: (180143985008641, 180143985131521), 8: (180143985086977, 180143985096193)}


@pytest.mark.parametrize("logn", [8, 12])
def test_matmul_fold_primes_are_adjacent_to_the_limit(logn):
    """mm_hi < 2^52 / 25 <= mm_lo < 2^51, both NTT primes, no admissible prime between either and the limit, and the limit is the
    number the kernel tests (q < (1ull << 52) / 25, an integer division)"""
    assert ML.MATMUL_FOLD_LIMIT == (1 << 52) // 25
    c = ML.matmul_chain(logn)
    hi, lo = c["mm_hi"], c["mm_lo"]
    assert (hi, lo) == MM_KNOWN[logn]
    assert hi < ML.MATMUL_FOLD_LIMIT <= lo < 1 << 51
    m = 2 << logn
    for q in (hi, lo):
        assert ML.is_prime(q) and O.lib().mo_is_prime(q) and q % m == 1
    assert not any(ML.is_prime(v) for v in range(hi + m, lo, m))
    # the nine names are untouched, the two new primes are none of them and sit between fpr_lo and fpr_hi
    assert {k: v for k, v in c.items() if k in ML.NAMES} == ML.chain(logn) and set(c) == set(ML.NAMES) | {"mm_hi", "mm_lo"}
    assert c["fpr_lo"] < hi and lo < c["fpr_hi"]


@pytest.mark.parametrize("logn", range(1, 12))
def test_chain_holds_at_the_small_degrees(logn):
    """chain() below 2^12: nine distinct NTT primes of the same bit lengths as at the tiled degrees, each on its side of its limit,
    and the oracle builds its tables for both orders"""
    c = ML.chain(logn)
    qs = list(c.values())
    assert len(set(qs)) == 9 and all(ML.is_prime(q) and q % (2 << logn) == 1 for q in qs)
    assert [q.bit_length() for q in qs] == [q.bit_length() for q in ML.chain(12).values()] == [47, 47, 51, 52, 59, 59, 60, 61, 41]
    assert 33 * c["fpn_hi"] < 1 << 52 <= 33 * c["fpr_lo"]
    assert c["fpr_hi"] < 1 << 51 <= c["int_lo"]
    assert c["ng_hi"] < ML.NOGUARD_LIMIT <= c["g_lo"]
    assert c["g60"] < 1 << 60 <= c["g61"] < 1 << 61
    for order in ML.ORDERS:
        O.Context(logn, ML.ordered(logn, order))


def test_long_chain_at_2_11_and_its_reference_key_cap():
    """64 primes at N = 2^11: MOAI_MAX_RNS rows; at L = 17 and L = 63 the reference's own sum caps the 61-bit prime's key rows only,
    and the library's unfolded 128-bit sum of L products of canonical residues fits (L q^2 < 2^128)"""
    primes, names = ML.long_chain(11, 64)
    assert len(set(primes)) == 64 and all(ML.is_prime(q) and q % 4096 == 1 for q in primes) and names[-1] == "g61"
    for L in (17, 63):
        assert [nm for q, nm in zip(primes, names) if ML.reference_key_cap(q, L) < q - 1] == ["g61"]
        assert all(L * (q - 1) * (q - 1) < 1 << 128 for q in primes)


@pytest.mark.parametrize("n", [2, 8, 25, 256, 4096])
def test_pair_patterns_hold_every_ordered_pair(n):
    q = ML.chain(12)["g61"]
    a, b = ML.pair_patterns(q, n, np.random.default_rng(n))
    assert a.shape == b.shape == (n,) and a.dtype == b.dtype == np.uint64
    assert (a < q).all() and (b < q).all()
    vals = ML.pair_values(q)
    assert vals == (0, 1, q - 1, q // 2, q // 2 + 1)
    pairs = [(u, v) for v in vals for u in vals]  # a has period 5, b period 25
    got = list(zip(a.tolist(), b.tolist()))
    assert got[:25] == pairs[:n]
    if n >= 25:
        assert set(pairs) <= set(got) and len(set(pairs)) == 25
    if n >= 256:
        assert len(set(a[25:].tolist())) > (n - 25) // 2  # the rest is random


def balanced(v, q):
    v %= q
    return v - q if v > q // 2 else v


@pytest.mark.parametrize("name", ["mm_hi", "fpr_hi"])
def test_matmul_worst_is_the_worst(name):
    """every product of matmul_worst has its balanced residue within 2^16 of +-q/2, all rows of a coefficient agree in sign (+ in
    the even and - in the odd coefficients for w, exchanged for q - w), the real quotient is within 2^-30 of a half-integer, and
    sixteen consecutive rows sum to at least 7.9 q in magnitude; the reference product is the plain sum(x w) % q"""
    q = ML.matmul_chain(12)[name]
    rows, cols, n = 49, 17, 8
    x, w, wn = ML.matmul_worst(q, rows, cols, n, np.random.default_rng(17))
    h = (q - 1) // 2
    assert x.shape == (rows, n) and w.shape == wn.shape == (rows, cols)
    assert (x[:, 0::2] == h).all() and (x[:, 1::2] == h + 1).all()
    assert ((w & np.uint64(1)) == 1).all() and (w < 1 << 17).all() and (wn == np.uint64(q) - w).all()
    assert len(set(w.reshape(-1).tolist())) > rows * cols // 2  # a fresh draw per (j, c)
    for wt, sign_even in ((w, 1), (wn, -1)):
        for coef, sign in ((0, sign_even), (1, -sign_even)):
            xb = balanced(int(x[0, coef]), q)
            assert abs(xb) == h
            for c in range(cols):
                r = [balanced(xb * int(wt[j, c]), q) for j in range(rows)]
                assert all(abs(v) * 2 >= q - (2 << 16) for v in r)
                assert all((v > 0) == (sign > 0) for v in r)
                # the quotient of the product the kernel forms, balanced x times the canonical weight
                for j in range(rows):
                    p = xb * int(wt[j, c])
                    frac2 = (2 * p) % (2 * q)  # 2 frac(p / q) q
                    assert abs(frac2 - q) << 30 <= q  # | frac(p / q) - 1/2 | <= 2^-31
                for j0 in range(rows - 15):
                    assert abs(sum(r[j0:j0 + 16])) * 10 >= 79 * q
    for wt in (w, wn):
        want = np.array([[sum(int(x[j, i]) * int(wt[j, c]) for j in range(rows)) % q for i in range(n)] for c in range(cols)],
                        dtype=np.uint64)
        assert (ML.matmul_mod(x, wt, q) == want).all()


@pytest.mark.parametrize("name", ["small", "mm_hi", "mm_lo", "fpr_hi", "int_lo"])
def test_matmul_mod_is_the_sum_of_products(name):
    """the uint64 reference product against Python integers, on operands that include q - 1 against q - 1"""
    q = ML.matmul_chain(8)[name]
    rng = np.random.default_rng(q % 1000)
    rows, cols = 49, 5
    x = rng.integers(0, q, size=(rows, 2, 16), dtype=np.uint64)
    w = rng.integers(0, q, size=(rows, cols), dtype=np.uint64)
    x[:, 0, :4] = q - 1
    w[:, 0] = q - 1
    want = np.tensordot(w.astype(object), x.astype(object), axes=(0, 0)) % q
    got = ML.matmul_mod(x, w, q)
    assert got.shape == (cols, 2, 16) and (got.astype(object) == want).all()
    assert int(got[0, 0, 0]) == rows * (q - 1) * (q - 1) % q


def test_pair_rows_cover_every_pair():
    """what the per-coefficient GPU tests stand on: every ordered pair of the five values meets in polynomial 0 of every row at N >= 32, and
    over the nine rows at N = 8"""
    for logn in (3, 8):
        n = 1 << logn
        primes = ML.ordered(logn, "g61_last")
        a, b = ML.pair_rows(primes, 3, n, np.random.default_rng(1))
        seen = set()
        for r, q in enumerate(primes):
            idx = {v: i for i, v in enumerate(ML.pair_values(q))}
            row = {(idx[u], idx[v]) for u, v in zip(a[0, r].tolist(), b[0, r].tolist()) if u in idx and v in idx}
            assert n < 32 or len(row) == 25, (logn, r)
            seen |= row
        assert len(seen) == 25, logn
