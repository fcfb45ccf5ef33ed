"""CPU-only checks behind tests/test_gpu_hybrid_sums_limits.py and tests/test_gpu_hybrid_forms_limits.py: the integer restatements of
the plaintext-weighted sums (tests/hybrid_dot_ref.py), of the BSGS sum (tests/hybrid_bsgs_ref.py) and of the exact rounding mode
(tests/hybrid_exact_ref.py) at the chains special_large and special_small of tests/mode_limits.py, as tests/test_hybrid_limits_cpu.py
pins hybrid_ref and hybrid_hoist_ref there.  N = 2^10 (the chains hold primes of the same bit lengths at every degree), L = 7 (digits
of 3, 3, 1) and 4 (a partial last digit), c1 the NTT form of worst_coeff, one key all m - 1 and one uniform key.
(a) rotate_pt_dot with one output, one rotation and the all-ones plaintext is hybrid_ref.apply_galois, for a rotation and the
    conjugation;
(b) bsgs_dot with one giant step of element 1 is rotate_pt_dot with one output; with one identity baby term of ones under one rotated
    giant step it is hybrid_ref.apply_galois;
(c) on special_large (P > D_max, the precondition of the header's bounds) with real keys and a ternary secret the decryption errors
    of both sums are within the header's bounds;
(d) the exact switch and the exact merged rescale are within 1/2 + 2^-40 of the exact quotient in every coefficient: the property of
    tests/test_hybrid_exact_cpu.py with sources of 41, 47 and 51 bits together, the data prime ng_hi or fpr_lo among them in the rescale's
    set, and targets far above and far below the sources."""
import numpy as np
import pytest

import hybrid_bsgs_ref as HB
import hybrid_dot_ref as HD
import hybrid_exact_ref as HX
import hybrid_ref as HR
import hybrid_rescale_ref as RR
import mode_limits as ML
import oracle as O
from hybrid_kit import KEY, elt_of, secret

LOGN = 10
CHAINS = list(ML.HYBRID_CHAINS)
LEVELS = [7, 4]
KEYS = ["max", "rnd"]
_envs = {}


class Env:
    def __init__(self, which):
        self.primes, _, self.alpha = ML.hybrid_chain(LOGN, which)
        self.octx = O.Context(LOGN, self.primes)
        self.n, self.k = self.octx.n, len(self.primes)
        self.digits = HR.beta(self.k - self.alpha, self.alpha)
        top = np.empty((self.digits, 2, self.k, self.n), dtype=np.uint64)
        for i, m in enumerate(self.primes):
            top[:, :, i, :] = m - 1
        self.keys = {"max": top, "rnd": O.uniform_rns(np.random.default_rng(8100), self.primes, (self.digits, 2), self.n)}

    def rows(self, L):
        return [self.primes[i] for i in list(range(L)) + list(range(self.k - self.alpha, self.k))]

    def ct(self, L, seed):
        """(c0 uniform, c1 = NTT(worst_coeff))"""
        ct = O.uniform_rns(np.random.default_rng(seed), self.primes[:L], (2,), self.n)
        ct[1] = self.octx.ntt(ML.worst_coeff(self.primes, L, self.alpha, self.n), L)
        return ct


def env(which):
    if which not in _envs:
        _envs[which] = Env(which)
    return _envs[which]


# ---- (a), (b) the identities ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KEYS)
@pytest.mark.parametrize("L", LEVELS)
@pytest.mark.parametrize("which", CHAINS)
def test_one_rotation_with_the_unit_plaintext_is_apply_galois(which, L, kind):
    e = env(which)
    ct, key, one = e.ct(L, 8200 + L), e.keys[kind], HD.ones_plain(e.octx, L, e.alpha)
    for step in (1, 0):
        elt = elt_of(LOGN, step)
        got = HD.rotate_pt_dot(e.octx, ct, L, e.alpha, [elt], [key], [[one]])
        assert (got[0] == HR.apply_galois(e.octx, ct, L, elt, key, e.alpha)).all(), step


@pytest.mark.parametrize("kind", KEYS)
@pytest.mark.parametrize("L", LEVELS)
@pytest.mark.parametrize("which", CHAINS)
def test_one_giant_step_of_element_1_is_rotate_pt_dot(which, L, kind):
    e = env(which)
    rng = np.random.default_rng(8300 + L)
    ct, key = e.ct(L, 8300 + L), e.keys[kind]
    elts = [1, elt_of(LOGN, 1), elt_of(LOGN, 0)]
    top = np.stack([np.full(e.n, m - 1, dtype=np.uint64) for m in e.rows(L)])
    plains = [[O.uniform_rns(rng, e.rows(L), (), e.n), top, O.uniform_rns(rng, e.rows(L), (), e.n)]]
    keys = [None, key, key]
    got = HB.bsgs_dot(e.octx, ct, L, e.alpha, elts, keys, [1], [None], plains)
    assert (got == HD.rotate_pt_dot(e.octx, ct, L, e.alpha, elts, keys, plains)[0]).all()


@pytest.mark.parametrize("kind", KEYS)
@pytest.mark.parametrize("L", LEVELS)
@pytest.mark.parametrize("which", CHAINS)
def test_a_unit_plaintext_giant_step_is_apply_galois(which, L, kind):
    e = env(which)
    ct, key, one = e.ct(L, 8400 + L), e.keys[kind], HD.ones_plain(e.octx, L, e.alpha)
    for step in (1, 0):
        E = elt_of(LOGN, step)
        got = HB.bsgs_dot(e.octx, ct, L, e.alpha, [1], [None], [E], [key], [[one]])
        assert (got == HR.apply_galois(e.octx, ct, L, E, key, e.alpha)).all(), step


# ---- (c) the noise bounds on special_large ------------------------------------------------------------------------------------------
def test_decryption_errors_are_within_the_bounds_on_special_large():
    """L = 4, plaintexts of 16-bit coefficients: two switched baby terms and the identity; giant steps 1 and a rotation"""
    e, L, bits = env("special_large"), 4, 16
    octx, alpha = e.octx, e.alpha
    D_max = max(HR._prod(e.primes[r] for r in HR.digit_rows(j, L, alpha)) for j in range(HR.beta(L, alpha)))
    assert HR._prod(e.primes[e.k - alpha:]) > D_max
    s, sk = secret(octx, KEY, 1)
    s_l1 = int(np.count_nonzero(s))
    rng = np.random.default_rng(8500)
    baby = [1, elt_of(LOGN, 1), elt_of(LOGN, 0)]
    giant = [1, elt_of(LOGN, 4)]

    def key_for(elt, seq):
        return None if elt == 1 else HR.keygen(octx, KEY, seq, sk, sk[:, O.galois_table_ntt(LOGN, elt)], alpha)

    bkeys = [key_for(elt, 100 * (r + 1)) for r, elt in enumerate(baby)]
    gkeys = [key_for(elt, 100 * (g + 11)) for g, elt in enumerate(giant)]
    coeffs = [[rng.integers(-(1 << bits) + 1, 1 << bits, e.n) for _ in baby] for _ in giant]
    plains = [[HD.encode_plain(octx, c, L, alpha) for c in row] for row in coeffs]
    l1 = [sum(int(np.abs(coeffs[g][r]).sum()) for r, elt in enumerate(baby) if elt != 1) for g in range(len(giant))]
    ct = O.uniform_rns(rng, e.primes[:L], (2,), e.n)
    out = HD.rotate_pt_dot(octx, ct, L, alpha, baby, bkeys, plains[:1])[0]
    worst = max(abs(int(v)) for v in HD.dot_error(octx, out, ct, sk, L, baby, plains[0]))
    bound = HD.noise_bound(octx, L, alpha, s_l1, l1[0])
    print("pt-dot: max |E| = %d, bound = %.1f" % (worst, bound))
    assert worst <= bound
    out = HB.bsgs_dot(octx, ct, L, alpha, baby, bkeys, giant, gkeys, plains)
    worst = max(abs(int(v)) for v in HB.bsgs_error(octx, out, ct, sk, L, baby, giant, plains))
    bound = HB.noise_bound(octx, L, alpha, s_l1, giant, l1)
    print("bsgs: max |E| = %d, bound = %.1f" % (worst, bound))
    assert worst <= bound


# ---- (d) the exact mode's property ----------------------------------------------------------------------------------------------------
def limit_ct3(e, L, kind, seed):
    """c2 = NTT(worst_coeff); c0 and c1 every row all q - 1 with the key `max`, uniform with the other"""
    if kind == "max":
        ct3 = np.stack([np.stack([np.full(e.n, q - 1, dtype=np.uint64) for q in e.primes[:L]])] * 3)
    else:
        ct3 = O.uniform_rns(np.random.default_rng(seed), e.primes[:L], (3,), e.n)
    ct3[2] = e.octx.ntt(ML.worst_coeff(e.primes, L, e.alpha, e.n), L)
    return ct3


@pytest.mark.parametrize("kind", KEYS)
@pytest.mark.parametrize("L", LEVELS)
@pytest.mark.parametrize("which", CHAINS)
def test_the_exact_switch_is_within_half_of_the_quotient(which, L, kind):
    e = env(which)
    ct3, key = limit_ct3(e, L, kind, 8600 + L), e.keys[kind]
    zero = np.zeros((2, L, e.n), dtype=np.uint64)
    out = HX.switch_key(e.octx, zero, ct3[2], key, L, e.alpha, exact=True)
    acc = HD.accumulators(e.octx, ct3[2], key, L, e.alpha)
    for p in range(2):
        err, W = HX.quotient_error(e.octx, HX.acc_rows(e.octx, acc, p, L, e.alpha), out[p], L, e.alpha)
        print("%s L %d %s p %d: max |out - Z/W| = %.6f" % (which, L, kind, p, max(abs(int(v)) for v in err) / W))
        assert HX.within_half(err, W).all(), p


@pytest.mark.parametrize("kind", KEYS)
@pytest.mark.parametrize("L", LEVELS)
@pytest.mark.parametrize("which", CHAINS)
def test_the_exact_merged_rescale_is_within_half_of_the_quotient(which, L, kind):
    e = env(which)
    ct3, key = limit_ct3(e, L, kind, 8700 + L), e.keys[kind]
    Z = RR.lifted(e.octx, ct3, key, L, e.alpha)
    out = HX.relinearize_rescale(e.octx, ct3, key, L, e.alpha, exact=True)
    assert (out == HX.relinearize_rescale(e.octx, ct3, key, L, e.alpha, exact=True, Z=Z)).all()
    for p in range(2):
        err, W = HX.quotient_error(e.octx, Z[p], out[p], L, e.alpha, rescale=True)
        print("%s L %d %s p %d: max |out - Z/W| = %.6f" % (which, L, kind, p, max(abs(int(v)) for v in err) / W))
        assert HX.within_half(err, W).all(), p
