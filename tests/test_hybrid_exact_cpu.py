"""CPU-only checks of the exact rounding mode of the hybrid mod-downs (include/moai_hip.h, "hybrid rounding mode").  They pin the
restatement tests/hybrid_exact_ref.py:
1. alpha = 1: the exact switch is hybrid_ref.switch_key bit for bit (one source, v* = 0 = v; the clamp is what makes it so).  The
   merged rescale has TWO sources at alpha = 1 (q_{L-1} and p_0), so its fast form carries an overflow u' in {0, 1} there and the
   exact form cannot be its bits: it is hybrid_rescale_ref.relinearize_rescale PLUS that overflow, coefficient for coefficient, and
   its bits wherever the overflow is zero;
2. the property |out - Z / W| <= 1/2 + 2^-40 in exact rational arithmetic for every coefficient: switch and merged rescale, alpha 2
   and 3, and 16 and 17 sources of 61-bit primes;
3. the same check finds a coefficient off by a whole unit in the DEFAULT restatement at every alpha >= 2;
4. on seeded random inputs the guard band is empty and the output is floor((Z + H) / W) computed with big integers alone;
5. directed boundaries: X' in {0, 1, 2, W-2, W-1, H-1, H, H+1}, and y at the clamp (one source, y = m - 1);
6. with real keys the decryption errors are within the header's exact-mode bounds; the maxima of both modes are printed
   (profiles/hybrid_exact_noise.txt is this output).
And the C ABI: both symbols exported, declared and bound; the refusals that need no context."""
import ctypes as C
import re

import numpy as np
import pytest

import hybrid_bsgs_ref as HB
import hybrid_dot_ref as HD
import hybrid_exact_ref as HX
import hybrid_hoist_ref as HH
import hybrid_ref as HR
import hybrid_rescale_ref as RR
import mode_limits as ML
import oracle as O
from hybrid_kit import EINVAL, KEY, NOISE_CASES, OK, UNIT_CASES, elt_of, exported, header, secret

NAMES = ("moai_hybrid_set_rounding", "moai_hybrid_rounding")
LOGN = 5
_wide = {}


def small_env(data, special, seed):
    primes = O.coeff_modulus_create(1 << LOGN, data + special)
    octx = O.Context(LOGN, primes)
    rng = np.random.default_rng(seed)
    return octx, rng, O.uniform_rns(rng, primes, (HR.beta(len(data), len(special)), 2), octx.n)


def wide_env():
    """eighteen 61-bit primes: alpha = 16 has sixteen sources in step 5 and seventeen in the merged mod-down, alpha = 15 sixteen there"""
    if not _wide:
        g61 = ML.chain(LOGN)["g61"]
        primes = [g61] + ML.primes_below(LOGN, g61, 17)
        assert all(p >> 60 == 1 for p in primes)
        _wide["octx"] = O.Context(LOGN, primes)
    return _wide["octx"]


def random_rows(octx, rng, L, alpha):
    """a uniform accumulator [L + alpha][N]: any integer below Q_L P"""
    rows = HH.rows_of(octx, L, alpha)
    return O.uniform_rns(rng, [octx.primes[r] for r in rows], (), octx.n)


def worst(e, W):
    return max(abs(int(v)) for v in e) / W


# ---- 1. alpha = 1 -----------------------------------------------------------------------------------------------------------------
def test_alpha_1_switch_is_the_fast_switch_bit_for_bit():
    data, special, levels = UNIT_CASES[0]
    octx, rng, key = small_env(data, special, 1)
    for L in levels:
        ct = O.uniform_rns(rng, octx.primes[:L], (2,), octx.n)
        target = O.uniform_rns(rng, octx.primes[:L], (), octx.n)
        assert (HX.switch_key(octx, ct, target, key, L, 1) == HR.switch_key(octx, ct, target, key, L, 1)).all(), L


def test_alpha_1_rescale_is_the_fast_rescale_plus_its_overflow():
    data, special, _ = UNIT_CASES[0]
    octx, rng, key = small_env(data, special, 2)
    for L in (3, 2):
        ct3 = O.uniform_rns(rng, octx.primes[:L], (3,), octx.n)
        fast, exact = RR.relinearize_rescale(octx, ct3, key, L, 1), HX.relinearize_rescale(octx, ct3, key, L, 1)
        assert (HX.relinearize_rescale(octx, ct3, key, L, 1, exact=False) == fast).all()  # the conversion's fast form is that module's
        Z = RR.lifted(octx, ct3, key, L, 1)
        Qlo = HR._prod(octx.primes[:L - 1])
        for p in range(2):
            diag = {}
            HX.mod_down_rows(octx, Z[p], L, 1, rescale=True, diag=diag)
            d = RR.centred((RR.crt(octx, list(exact[p]), range(L - 1)) - RR.crt(octx, list(fast[p]), range(L - 1))) % Qlo, Qlo)
            assert (d == diag["vstar"]).all() and set(d) <= {0, 1}, (L, p)
            assert (diag["v"] == diag["vstar"]).all()
            same = np.flatnonzero(diag["vstar"] == 0)
            assert len(same) and len(same) < octx.n  # both kinds of coefficient occur
            coef = lambda a: octx.ntt(a, L - 1, inverse=True)  # noqa: E731
            assert (coef(exact[p])[:, same] == coef(fast[p])[:, same]).all()


# ---- 2., 3., 4. the property, its discrimination, and the integer comparator ---------------------------------------------------------
def check_polynomial(octx, Z, L, alpha, rescale, label, fast_out=None):
    """2. and 4. for one lifted polynomial Z [L + alpha][N]; with fast_out, 3. for the default restatement's result"""
    out = HX.mod_down_rows(octx, Z, L, alpha, rescale=rescale)
    e, W = HX.quotient_error(octx, Z, out, L, alpha, rescale)
    print("%s: exact max |out - Z/W| = %.6f" % (label, worst(e, W)))
    assert HX.within_half(e, W).all(), label
    assert HX.guard_band(octx, Z, L, alpha, rescale) == [], label  # a condition on the seeded inputs: 2^-39 per coefficient
    assert (out == HX.rounded_quotient(octx, Z, L, alpha, rescale)).all(), label
    if fast_out is not None:
        ef, _ = HX.quotient_error(octx, Z, fast_out, L, alpha, rescale)
        off = int((~HX.within_half(ef, W)).sum())
        print("%s: fast  max |out - Z/W| = %.6f, %d coefficients beyond 1/2 + 2^-40" % (label, worst(ef, W), off))
        assert off >= 1 and worst(ef, W) > 1.0, label


@pytest.mark.parametrize("data,special,levels", UNIT_CASES[1:])
def test_property_switch(data, special, levels):
    alpha = len(special)
    octx, rng, key = small_env(data, special, 10 + alpha)
    zero = np.zeros((2, max(levels), octx.n), dtype=np.uint64)
    for L in levels:
        target = O.uniform_rns(rng, octx.primes[:L], (), octx.n)
        acc = HD.accumulators(octx, target, key, L, alpha)
        fast = HR.switch_key(octx, zero[:, :L], target, key, L, alpha)  # the DEFAULT restatement, no addend
        assert (HX.switch_key(octx, zero[:, :L], target, key, L, alpha, exact=False) == fast).all()
        for p in range(2):
            check_polynomial(octx, HX.acc_rows(octx, acc, p, L, alpha), L, alpha, False, "switch alpha %d L %d p %d" % (alpha, L, p), fast[p])


@pytest.mark.parametrize("data,special,levels", UNIT_CASES[1:])
def test_property_rescale(data, special, levels):
    alpha = len(special)
    octx, rng, key = small_env(data, special, 20 + alpha)
    for L in [L for L in levels if L >= 2]:
        ct3 = O.uniform_rns(rng, octx.primes[:L], (3,), octx.n)
        Z = RR.lifted(octx, ct3, key, L, alpha)
        fast = RR.relinearize_rescale(octx, ct3, key, L, alpha)
        assert (HX.relinearize_rescale(octx, ct3, key, L, alpha, Z=Z) == np.stack(
            [HX.mod_down_rows(octx, Z[p], L, alpha, rescale=True) for p in range(2)])).all()
        for p in range(2):
            check_polynomial(octx, Z[p], L, alpha, True, "rescale alpha %d L %d p %d" % (alpha, L, p), fast[p])


@pytest.mark.parametrize("alpha,L,rescale,nsrc", [(16, 2, False, 16), (16, 2, True, 17), (15, 3, True, 16), (15, 3, False, 15)])
def test_property_wide_sources(alpha, L, rescale, nsrc):
    octx = wide_env()
    assert len(HX.bases(octx, L, alpha, rescale)[0]) == nsrc
    rng = np.random.default_rng(30 + nsrc + rescale)
    for rep in range(2):
        Z = random_rows(octx, rng, L, alpha)
        fast = HX.mod_down_rows(octx, Z, L, alpha, rescale=rescale, exact=False)
        check_polynomial(octx, Z, L, alpha, rescale, "%d sources (61 bits) rep %d" % (nsrc, rep), fast)


# ---- 5. directed boundaries -------------------------------------------------------------------------------------------------------
def boundary_rows(octx, rng, L, alpha, rescale):
    """Z [L + alpha][N] whose coefficient c has X' = targets[c % 8], the quotient above it random; returns (Z, the targets per
    coefficient)"""
    src, ntgt = HX.bases(octx, L, alpha, rescale)
    W = HR._prod(octx.primes[r] for r in src)
    H, Qlo = W // 2, HR._prod(octx.primes[:ntgt])
    targets = [0, 1, 2, W - 2, W - 1, H - 1, H, H + 1]
    want = [targets[c % 8] for c in range(octx.n)]
    z = [int(rng.integers(0, 1 << 62)) % Qlo * W + (x - H) % W for x in want]
    rows = HH.rows_of(octx, L, alpha)
    coef = np.stack([HR._u64(np.array([v % octx.primes[r] for v in z], dtype=object)) for r in rows])
    return octx.ntt(coef, len(rows), prime_index=rows), want


def check_boundaries(octx, rng, L, alpha, rescale, label):
    Z, want = boundary_rows(octx, rng, L, alpha, rescale)
    diag = {}
    out = HX.mod_down_rows(octx, Z, L, alpha, rescale=rescale, diag=diag)
    assert list(diag["X"]) == want, label  # the restatement says what Z really was
    e, W = HX.quotient_error(octx, Z, out, L, alpha, rescale)
    for c in range(8):
        print("%s: X' = %s: v = %d, v* = %d, out - Z/W = %+.6f" % (label, ["0", "1", "2", "W-2", "W-1", "H-1", "H", "H+1"][c],
                                                                  diag["v"][c], diag["vstar"][c], int(e[c]) / W))
    assert HX.within_half(e, W).all(), label
    assert max(abs(int(a) - int(b)) for a, b in zip(diag["v"], diag["vstar"])) <= 1
    assert len(HX.guard_band(octx, Z, L, alpha, rescale)) == 5 * octx.n // 8, label  # 0, 1, 2, W-2, W-1
    inner = [c for c in range(octx.n) if c % 8 >= 5]  # H-1, H, H+1: far from the band, the exact rounded quotient
    assert (octx.ntt(out, len(out), inverse=True)[:, inner]
            == octx.ntt(HX.rounded_quotient(octx, Z, L, alpha, rescale), len(out), inverse=True)[:, inner]).all(), label
    return diag


@pytest.mark.parametrize("case", [1, 2])
@pytest.mark.parametrize("rescale", [False, True])
def test_boundaries(case, rescale):
    data, special, levels = UNIT_CASES[case]
    octx, rng, _ = small_env(data, special, 40 + case)
    check_boundaries(octx, rng, levels[0], len(special), rescale, "alpha %d %s" % (len(special), "rescale" if rescale else "switch"))


@pytest.mark.parametrize("alpha,L,rescale", [(16, 2, False), (16, 2, True)])
def test_boundaries_wide_sources(alpha, L, rescale):
    check_boundaries(wide_env(), np.random.default_rng(50 + rescale), L, alpha, rescale, "%d sources" % (alpha + rescale))


def test_the_clamp_one_source_at_y_equal_m_minus_1():
    """n = 1: y = X' and v* = 0 always.  At y = m - 1 on a 61-bit prime (double)y is (double)m, and the product with RN(1 / m) may round
    to 1.0, where floor(f) = 1 = n: the clamp brings v back to 0 whatever the product rounds to.  Both 61-bit primes of the chain's top"""
    g61 = ML.chain(LOGN)["g61"]
    below = ML.primes_below(LOGN, g61, 1)[0]
    for primes in ([below, g61], [g61, below]):
        octx = O.Context(LOGN, primes)
        m = primes[-1]
        diag = check_boundaries(octx, np.random.default_rng(60), 1, 1, False, "one source m = %d" % m)
        at = [c for c in range(octx.n) if c % 8 == 4]
        assert all(int(diag["y"][0][c]) == m - 1 for c in at)
        f = np.float64(m - 1) * (np.float64(1.0) / np.float64(float(m)))
        print("m = %d: (double)(m - 1) * (1.0 / m) = %r, floor %d" % (m, f, int(np.floor(f))))
        assert all(int(diag["v"][c]) == 0 and int(diag["vstar"][c]) == 0 for c in range(octx.n))


# ---- 6. noise with real keys --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("data,special,L,steps,bits", NOISE_CASES)
def test_noise_is_within_the_exact_bounds(data, special, L, steps, bits):
    logn, alpha = 6, len(special)
    primes = O.coeff_modulus_create(1 << logn, data + special)
    octx = O.Context(logn, primes)
    s, sk = secret(octx, KEY, 1)
    s_l1 = int(np.count_nonzero(s))
    unit = 1 + s_l1
    rng = np.random.default_rng(3000 * alpha + 10 * L)
    s2 = np.stack([HR._u64(HR._obj(sk[r]) * HR._obj(sk[r]) % q) for r, q in enumerate(primes)])
    rkey = HR.keygen(octx, KEY, 5, sk, s2, alpha)
    label = "alpha %d L %d" % (alpha, L)

    def report(what, fast, exact, bound, scale=1):
        print("noise %s %-8s fast max |E| = %.3f, exact max |E| = %.3f (units of 1 + |s|_1 = %d); exact bound %.3f"
              % (label, what, fast / scale / unit, exact / scale / unit, unit, bound / scale / unit))
        assert exact <= bound, (what, exact, bound)

    # the switch: c s^2 under s
    zero, target = np.zeros((2, L, octx.n), dtype=np.uint64), O.uniform_rns(rng, primes[:L], (), octx.n)
    err = [max(abs(int(v)) for v in HR.switch_error(octx, f(octx, zero, target, rkey, L, alpha), target, sk, s2, L))
           for f in (HR.switch_key, HX.switch_key)]
    report("switch", err[0], err[1], HX.switch_noise_bound(octx, L, alpha, s_l1))
    # the merged rescale
    if L >= 2:
        ct3 = O.uniform_rns(rng, primes[:L], (3,), octx.n)
        err = [max(abs(int(v)) for v in RR.rescale_error(octx, f(octx, ct3, rkey, L, alpha), ct3, sk, L))
               for f in (RR.relinearize_rescale, HX.relinearize_rescale)]
        report("rescale", err[0], err[1], HX.rescale_noise_bound(octx, L, alpha, s_l1), scale=primes[L - 1])
    # pt-dot and bsgs: two switched baby steps and the identity, two giant steps
    baby = [1] + [elt_of(logn, st) for st in steps[:2]]
    giant = [1, elt_of(logn, steps[-1])]
    key_for = lambda elt, seq: None if elt == 1 else HR.keygen(octx, KEY, seq, sk, sk[:, O.galois_table_ntt(logn, elt)], alpha)  # noqa: E731
    bkeys, gkeys = [key_for(e, 100 * (r + 1)) for r, e in enumerate(baby)], [key_for(e, 100 * (g + 11)) for g, e in enumerate(giant)]
    coeffs = [[rng.integers(-(1 << bits) + 1, 1 << bits, octx.n) for _ in baby] for _ in giant]
    plains = [[HD.encode_plain(octx, c, L, alpha) for c in row] for row in coeffs]
    l1 = [sum(int(np.abs(coeffs[g][r]).sum()) for r, e in enumerate(baby) if e != 1) for g in range(len(giant))]
    ct = O.uniform_rns(rng, primes[:L], (2,), octx.n)

    def both(run):
        fast = run()
        with HX.patched():
            exact = run()
        assert HH.mod_down is not HX.mod_down
        return fast, exact

    dots = both(lambda: HD.rotate_pt_dot(octx, ct, L, alpha, baby, bkeys, plains[:1]))
    err = [max(abs(int(v)) for v in HD.dot_error(octx, o[0], ct, sk, L, baby, plains[0])) for o in dots]
    report("pt-dot", err[0], err[1], HX.dot_noise_bound(octx, L, alpha, s_l1, l1[0]))
    sums = both(lambda: HB.bsgs_dot(octx, ct, L, alpha, baby, bkeys, giant, gkeys, plains))
    err = [max(abs(int(v)) for v in HB.bsgs_error(octx, o, ct, sk, L, baby, giant, plains)) for o in sums]
    report("bsgs", err[0], err[1], HX.bsgs_noise_bound(octx, L, alpha, s_l1, giant, l1))


def test_patched_restatements_reduce_to_the_exact_switch():
    """inside patched() the hoisted rotations are exact apply_galois bit for bit, as they are the fast one outside it"""
    data, special, levels = UNIT_CASES[1]
    alpha, L = len(special), levels[0]
    octx, rng, key = small_env(data, special, 70)
    ct = O.uniform_rns(rng, octx.primes[:L], (2,), octx.n)
    elts = [elt_of(LOGN, 1), elt_of(LOGN, 0)]
    with HX.patched():
        got = HH.apply_galois_hoisted(octx, ct, L, elts, [key, key], alpha)
    for r, elt in enumerate(elts):
        assert (got[r] == HX.apply_galois(octx, ct, L, elt, key, alpha)).all()
        assert (got[r] != HR.apply_galois(octx, ct, L, elt, key, alpha)).any()


# ---- the C ABI --------------------------------------------------------------------------------------------------------------------
def test_symbols_exported_declared_and_bound(moai):
    exported(moai, NAMES, ("hybrid_set_rounding", "hybrid_rounding"))
    hdr = header()
    for name in NAMES:
        assert re.search(r"^int " + name + r"\(", hdr, re.M), name
    assert re.search(r"^#define MOAI_HYBRID_ROUND_FAST 0\b", hdr, re.M) and re.search(r"^#define MOAI_HYBRID_ROUND_EXACT 1\b", hdr, re.M)
    assert (moai.hip.HYBRID_ROUND_FAST, moai.hip.HYBRID_ROUND_EXACT) == (0, 1)


def test_header_states_the_contract():
    hdr = header()
    for text in ("r_m    = 1.0 / (double)m", "v      = min(max(floor(f), 0), n - 1)", "| out_p - Z_p / W |  <=  1/2 + 2^-40",
                 "AT alpha = 1 BOTH MODES GIVE THE SAME BITS", "(1/2 + 2^-40)(1 + |s|_1)", "[-1, +1]"):
        assert text in hdr, text


def test_arguments_refused_without_a_device(moai):
    lib = moai.hip.lib()
    mode = C.c_int(7)
    assert lib.moai_hybrid_set_rounding(None, 0) == EINVAL and b"null context" in lib.moai_last_error()
    assert lib.moai_hybrid_rounding(None, C.byref(mode)) == EINVAL and b"null context" in lib.moai_last_error()
    assert mode.value == 7 and OK == 0
