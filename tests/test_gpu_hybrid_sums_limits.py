"""The plaintext-weighted sums of hoisted rotations and the BSGS sum (moai_hybrid_rotate_pt_dot, moai_hybrid_bsgs_dot; csrc/hybrid.hip,
csrc/hybrid_kernels.hip.h) on the chains special_large and special_small of tests/mode_limits.py, whose rows interleave every
arithmetic class of the transforms and whose mod-down sources lie far above or far below its targets; bit for bit against the integer
restatements tests/hybrid_dot_ref.py and tests/hybrid_bsgs_ref.py, pinned at these primes by tests/test_hybrid_sums_limits_cpu.py.

What each test reaches:
    test_pt_dot_at_the_limits            hy_hoisted_dot_kernel<4> (a pass of 4 and a pass of 1), hy_dot_term_kernel (the identity
                                         term), hy_step5 on (output, ciphertext) pairs: its sliced inverse transform of the special
                                         rows (FP64 ones on special_small) and hy_convert_kernel into rows of every class
    test_pt_dot_rotations_per_pass       hy_hoisted_dot_kernel<2> and <1>: S and the addend carried between passes as canonical residues
    test_pt_dot_small_transform          the same at N = 2^10, where the mod-down copies its source slice
    test_pt_dot_fallback                 the zero probe and the unhoisted route (hy_decompose of the permuted input, hy_mac_kernel)
    test_bsgs_at_the_limits              hy_c1_moddown_permute_kernel (source slice of stride 2 (L + alpha) at offset (L + alpha) + L),
                                         hy_decompose of the permuted c1', hy_bsgs_mac_kernel and its lift by P mod q_row, for the three
                                         kinds of giant step: rotated with a mod-down, rotated without a switched term, element 1
    test_bsgs_one_giant_step_per_group   the same with Z read back and written once per giant step (zseeded = 1 on later groups)
    test_bsgs_rotations_per_pass, test_bsgs_small_transform, test_bsgs_fallback
    test_65_rotations_..., test_65_giant_steps_...    the running sums carried past 63 terms on rows of every class

Shapes: N = 2^12 (the arithmetic classes exist from there on; every such test asserts the class of every row first), L = 7 (digits of 3,
3, 1) and L = 4 (a partial last digit); N = 2^10 once per chain.  Keys: rotation r takes the key all m - 1 and the uniform key in turn,
and both orders run.  A batch of three ciphertexts, one per c1: the NTT form of worst_coeff (c0 every row q - 1), of coefficients all
q - 1 and of a uniform draw (c0 uniform), each free of zero coefficients, so the flag must be False; a fourth with one zero coefficient
in one row must set it.  Plaintexts come round: every row m - 1, q/2 and q/2 + 1 alternating, uniform.  Cases and their restatements
are made once per (chain, degree, level, key order) and shared."""
import numpy as np
import pytest

import hybrid_ref as HR
import mode_limits as ML
import oracle as O
from hybrid_cases import BABY, GIANT, STEPS, BsgsCase, DotCase, LimitEnv, assert_modes
from hybrid_kit import IDENT, tuned

pytestmark = pytest.mark.gpu

CHAINS = list(ML.HYBRID_CHAINS)
KEYS = ["max", "rnd"]  # every row all m - 1; uniform
LEVELS = [7, 4]
_envs, _cases = {}, {}


@pytest.fixture(scope="module", autouse=True)
def release_device_contexts():
    """the cached contexts, keys and cases live as long as this module's tests, whichever ran"""
    yield
    _cases.clear()
    for e in _envs.values():
        e.close()
    _envs.clear()


def env(moai, logn, which):
    if (logn, which) not in _envs:
        _envs[(logn, which)] = LimitEnv(moai, logn, which, None)
    return _envs[(logn, which)]


def kinds_from(lead, count):
    """rotation r takes the key `lead` where r is even and the other one where it is odd"""
    other = KEYS[1 - KEYS.index(lead)]
    return [lead if r % 2 == 0 else other for r in range(count)]


# ---- the inputs, named --------------------------------------------------------------------------------------------------------------
def top_rows(primes, n):
    return np.stack([np.full(n, q - 1, dtype=np.uint64) for q in primes])


def limit_ciphertexts(e, L):
    """[3][2][L][N]: (c0 every row q - 1, c1 = NTT(worst_coeff)), (uniform, NTT(coefficients all q - 1)), (uniform, NTT(uniform)); every
    INTT(c1) is checked to be free of zeros"""
    def make():
        rng = np.random.default_rng(9100 + 100 * e.logn + L)
        coeff = [ML.worst_coeff(e.primes, L, e.alpha, e.n), top_rows(e.primes[:L], e.n), O.uniform_rns(rng, e.primes[:L], (), e.n)]
        ct = O.uniform_rns(rng, e.primes[:L], (3, 2), e.n)
        ct[0, 0] = top_rows(e.primes[:L], e.n)
        for b, cf in enumerate(coeff):
            ct[b, 1] = e.octx.ntt(cf, L)
            assert e.octx.ntt(ct[b, 1], L, inverse=True).all(), b
        ct.setflags(write=False)
        return ct
    if ("sums in", L) not in e.cache:
        e.cache[("sums in", L)] = make()
    return e.cache[("sums in", L)]


def zero_ciphertext(e, L):
    """[1][2][L][N]: c0 every row q - 1; INTT(c1) is uniform but for ONE zero, coefficient 5 of the last row"""
    rng = np.random.default_rng(9200 + 100 * e.logn + L)
    coeff = O.uniform_rns(rng, e.primes[:L], (), e.n)
    assert coeff.all()
    coeff[L - 1, 5] = 0
    ct = np.stack([top_rows(e.primes[:L], e.n), e.octx.ntt(coeff, L)])[None]
    assert np.count_nonzero(e.octx.ntt(ct[0, 1], L, inverse=True) == 0) == 1
    return ct


def limit_plains(e, L, rng):
    """a source of plaintexts over e.rows(L) that come round: every row m - 1, q/2 and q/2 + 1 alternating, uniform"""
    rows = e.rows(L)
    top = top_rows(rows, e.n)
    halves = np.empty_like(top)
    for i, m in enumerate(rows):
        halves[i, 0::2], halves[i, 1::2] = m // 2, m // 2 + 1
    count = [0]

    def new_plain():
        count[0] += 1
        turn = (count[0] - 1) % 3
        return top if turn == 0 else halves if turn == 1 else O.uniform_rns(rng, rows, (), e.n)
    return new_plain


def dot_case(e, L, lead, fallback=False):
    def make():
        ct = zero_ciphertext(e, L) if fallback else limit_ciphertexts(e, L)
        plain = limit_plains(e, L, np.random.default_rng(9300 + L))
        return DotCase(e, L, B=len(ct), ct=lambda rng: ct, plain=plain, kinds=kinds_from(lead, len(STEPS)))
    key = ("dot", e.which, e.logn, L, lead, fallback)
    if key not in _cases:
        _cases[key] = make()
    return _cases[key]


def bsgs_case(e, L, lead, fallback=False):
    def make():
        ct = zero_ciphertext(e, L) if fallback else limit_ciphertexts(e, L)
        plain = limit_plains(e, L, np.random.default_rng(9400 + L))
        return BsgsCase(e, L, B=len(ct), ct=lambda rng: ct, plain=plain, kinds=kinds_from(lead, len(BABY)),
                        giant_kinds=kinds_from(lead, len(GIANT)))
    key = ("bsgs", e.which, e.logn, L, lead, fallback)
    if key not in _cases:
        _cases[key] = make()
    return _cases[key]


def same(c, got):
    for i in range(len(c.want)):
        assert (got[i] == c.want[i]).all(), i  # per output (pt_dot) or per ciphertext (BSGS)


# ---- moai_hybrid_rotate_pt_dot --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lead", KEYS)
@pytest.mark.parametrize("L", LEVELS)
@pytest.mark.parametrize("which", CHAINS)
def test_pt_dot_at_the_limits(moai, which, L, lead):
    """steps [1, 3, -2, 64, conjugation, identity], three outputs: output 1 lacks two terms, output 2 holds only the identity term"""
    e = env(moai, 12, which)
    with tuned(moai):
        assert_modes(moai, e)
        c = dot_case(e, L, lead)
        assert (c.B, c.n_out, c.R) == (3, 3, 6) and c.plains[2][:5] == [None] * 5 and c.plains[2][5] is not None and c.plains[1][1] is None
        fb, got = c.run()
    assert not fb, "fallback taken"
    same(c, got)


@pytest.mark.parametrize("lead", KEYS)
@pytest.mark.parametrize("L", LEVELS)
@pytest.mark.parametrize("which", CHAINS)
def test_pt_dot_rotations_per_pass(moai, which, L, lead):
    e = env(moai, 12, which)
    with tuned(moai):
        assert_modes(moai, e)
        c = dot_case(e, L, lead)
        for per_pass in (2, 1):
            moai.hip.set_tuning("MOAI_HYBRID_HOIST_NR", per_pass)
            fb, got = c.run()
            assert not fb, per_pass
            same(c, got)


@pytest.mark.parametrize("which", CHAINS)
def test_pt_dot_small_transform(moai, which):
    e = env(moai, 10, which)
    c = dot_case(e, 7, "max")
    fb, got = c.run()
    assert not fb, "fallback taken"
    same(c, got)


@pytest.mark.parametrize("L", LEVELS)
@pytest.mark.parametrize("which", CHAINS)
def test_pt_dot_fallback(moai, which, L):
    """one zero coefficient in one row of INTT(c1): the flag is set, and the unhoisted route gives the restatement's bits"""
    e = env(moai, 12, which)
    with tuned(moai):
        assert_modes(moai, e)
        c = dot_case(e, L, "rnd", fallback=True)
        fb, got = c.run()
    assert fb, "the hoisted route was taken"
    same(c, got)


# ---- moai_hybrid_bsgs_dot -------------------------------------------------------------------------------------------------------------
def check_giant_kinds(c):
    """giant step 0 is the element 1; giant step 1 is rotated and has switched baby terms (its c1' takes a mod-down); giant step 2 is
    rotated and holds only the identity baby term"""
    assert c.giant[0] == 1 and c.giant[1] != 1 and c.giant[2] != 1 and c.baby[0] == 1
    assert any(p is not None for p in c.plains[1][1:]) and c.plains[2][0] is not None and c.plains[2][1:] == [None] * 5


@pytest.mark.parametrize("lead", KEYS)
@pytest.mark.parametrize("L", LEVELS)
@pytest.mark.parametrize("which", CHAINS)
def test_bsgs_at_the_limits(moai, which, L, lead):
    """baby steps [identity, 1, 3, -2, 64, conjugation], giant steps [identity, 4, -8]"""
    e = env(moai, 12, which)
    with tuned(moai):
        assert_modes(moai, e)
        c = bsgs_case(e, L, lead)
        check_giant_kinds(c)
        fb, got = c.run()
    assert not fb, "fallback taken"
    same(c, got)


def bsgs_rows(L, alpha):
    """the header's scratch formula in rows of N words: (per ciphertext, per ciphertext and giant step in flight)"""
    beta = HR.beta(L, alpha)
    shared = beta * (L + alpha) + 2 * L + 2 * (L + alpha) + 2 * (L + alpha) + 2 * alpha + 2 * L
    giant = 2 * (L + alpha) + 2 * L + alpha + L + L + beta * (L + alpha)
    return shared, giant


@pytest.mark.parametrize("lead", KEYS)
@pytest.mark.parametrize("L", LEVELS)
@pytest.mark.parametrize("which", CHAINS)
def test_bsgs_one_giant_step_per_group(moai, which, L, lead):
    """a budget that holds one ciphertext with one giant step in flight and not two: three groups, Z read back by the second and third"""
    e = env(moai, 12, which)
    shared, giant = bsgs_rows(L, e.alpha)
    assert (shared, giant) == {7: (104, 81), 4: (64, 47)}[L]
    row_kib = e.n * 8 // 1024
    kb = (shared + giant) * row_kib
    assert (kb << 10) // (e.n * 8) < shared + 2 * giant
    with tuned(moai, MOAI_HYBRID_TMP_KB=kb):
        assert_modes(moai, e)
        c = bsgs_case(e, L, lead)
        fb, got = c.run()
    assert not fb, "fallback taken"
    same(c, got)


@pytest.mark.parametrize("L", LEVELS)
@pytest.mark.parametrize("which", CHAINS)
def test_bsgs_rotations_per_pass(moai, which, L):
    e = env(moai, 12, which)
    with tuned(moai):
        assert_modes(moai, e)
        c = bsgs_case(e, L, "max")
        for per_pass in (2, 1):
            moai.hip.set_tuning("MOAI_HYBRID_HOIST_NR", per_pass)
            fb, got = c.run()
            assert not fb, per_pass
            same(c, got)


@pytest.mark.parametrize("which", CHAINS)
def test_bsgs_small_transform(moai, which):
    e = env(moai, 10, which)
    c = bsgs_case(e, 7, "rnd")
    check_giant_kinds(c)
    fb, got = c.run()
    assert not fb, "fallback taken"
    same(c, got)


@pytest.mark.parametrize("L", LEVELS)
@pytest.mark.parametrize("which", CHAINS)
def test_bsgs_fallback(moai, which, L):
    e = env(moai, 12, which)
    with tuned(moai):
        assert_modes(moai, e)
        c = bsgs_case(e, L, "max", fallback=True)
        fb, got = c.run()
    assert fb, "the hoisted route was taken"
    same(c, got)


# ---- more than 63 terms ---------------------------------------------------------------------------------------------------------------
CYCLE = [1, 3, -2, 5, 0]


def test_65_rotations_of_full_size_plaintexts_sum_exactly_on_every_class(moai):
    """special_large, L = 7, N = 2^10, one ciphertext (c1 = NTT(worst_coeff)): 65 rotations that cycle five elements under the key all
    m - 1, every plaintext row all m - 1, into one sum.  The sum travels between the passes as canonical residues on rows of 41 to
    61 bits; the restatement shares the five distinct accumulators."""
    e, L = env(moai, 10, "special_large"), 7
    top = top_rows(e.rows(L), e.n)
    ct = limit_ciphertexts(e, L)[:1]
    c = DotCase(e, L, steps=[CYCLE[r % 5] for r in range(65)], B=1, n_out=1, ct=lambda rng: ct, plain=lambda: top, kinds=["max"] * 65)
    assert c.R == 65 and all(p is top for p in c.plains[0])
    c.check()


def test_65_giant_steps_of_full_size_plaintexts_sum_exactly_on_every_class(moai):
    """the same chain and ciphertext: one identity baby term whose plaintext rows are all m - 1 under 65 giant steps that cycle five
    elements with the key all m - 1.  At most 16 giant steps are in flight, so Z travels between five groups as canonical residues."""
    e, L = env(moai, 10, "special_large"), 7
    top = top_rows(e.rows(L), e.n)
    ct = limit_ciphertexts(e, L)[:1]
    c = BsgsCase(e, L, baby=[IDENT], giant=[CYCLE[g % 5] for g in range(65)], B=1, ct=lambda rng: ct, plain=lambda: top,
                 kinds=[None], giant_kinds=["max"] * 65)
    assert c.ng == 65 and all(len(row) == 1 and row[0] is top for row in c.plains)
    c.check()
