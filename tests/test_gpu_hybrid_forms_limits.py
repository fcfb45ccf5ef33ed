"""The list forms of the hybrid key switch, the merged relinearize + rescale and the exact rounding mode (csrc/hybrid.hip,
csrc/hybrid_kernels.hip.h) on the chains special_large and special_small of tests/mode_limits.py, bit for bit against the integer
restatements themselves: tests/hybrid_ref.py, tests/hybrid_rescale_ref.py, tests/hybrid_exact_ref.py (pinned at these primes by
tests/test_hybrid_limits_cpu.py and tests/test_hybrid_sums_limits_cpu.py).  N = 2^12, where the rows of both chains interleave every
arithmetic class of the transforms; every test asserts the class of every row first.  L = 7 (digits of 3, 3, 1), 4 (a partial last
digit) and, for the merged rescale, 2 (one output row; on special_small q_{L-1} is then fpn_hi among specials of 40, 47 and 51 bits,
and ng_hi at L = 7).

What each test reaches:
    test_apply_galois_list                 moai_apply_galois_hybrid_ptrs without and with sums: the gather into scratch through the
                                           KsList records (five members, two keys, two elements), hy_mac_kernel<LIST>,
                                           moddown_finalize<LIST> with and without the addend
    test_to_and_acc                        moai_apply_galois_hybrid_to / _acc at batch 3
    test_relinearize_list                  moai_relinearize_hybrid_ptrs: source slice of stride 3L at offset 2L per member
    test_relinearize_rescale_list          moai_relinearize_rescale_hybrid_ptrs: hy_lift_last_row_kernel<LIST>, hy_rescale_finalize_kernel<LIST>
    test_merged_rescale_at_the_limits      moai_relinearize_rescale_hybrid: q - 1 operands, partial digits, L = 2; the conversion from
                                           {q_{L-1}, p_0, p_1, p_2}
    test_multiply_relin_rescale            hy_ct_product_kernel on the 25 boundary pairs of every row ((q - 1)(q - 1) among them), y != x
                                           and the square, against hybrid_rescale_ref.multiply_relin_rescale
    test_exact_switch_and_rescale          hy_convert_kernel<.., true> with sources of mixed size, targets far above and far below
    test_exact_sums                        the exact step 5 of moai_hybrid_rotate_pt_dot and moai_hybrid_bsgs_dot (patched restatements)
    test_exact_boundaries                  X' on 0, 1, 2, W-2, W-1, H-1, H, H+1: src_rinv and tgt_negw of a mixed-size source set
    test_fast_after_exact                  the cached tables do not depend on the mode

List members, each in a block of its own: c1 placed so that its rotation is the NTT form of worst_coeff; every row q - 1; zero;
uniform; a repeat of member 0's key and element.  Members take the key all m - 1 and the uniform key in turn, and a rotation and the
conjugation in turn.  Outputs are pre-filled with a pattern; inputs and keys are read back after every call.  Restatements are
computed once per (chain, level, key, input) and shared."""
import numpy as np
import pytest

import hybrid_bsgs_ref as HB
import hybrid_dot_ref as HD
import hybrid_exact_ref as HX
import hybrid_ref as HR
import hybrid_rescale_ref as RR
import mode_limits as ML
import oracle as O
from hybrid_cases import BsgsCase, DotCase, LimitEnv, assert_modes, check_boundaries, exact, run_rescale, run_switch
from hybrid_kit import PATTERN, tuned

pytestmark = pytest.mark.gpu

CHAINS = list(ML.HYBRID_CHAINS)
KEYS = ["max", "rnd"]  # every row all m - 1; uniform
LEVELS = [7, 4]
MEMBER_KINDS = ["max", "rnd", "max", "rnd", "max"]
MEMBER_STEPS = [1, 0, 1, 0, 1]  # 0 = conjugation
MEMBER_NAMES = ["worst_coeff", "all q-1", "zero", "uniform", "repeat of member 0's key and element"]
_envs = {}


@pytest.fixture(scope="module", autouse=True)
def release_device_contexts():
    yield
    for e in _envs.values():
        e.close()
    _envs.clear()


def env(moai, which):
    if which not in _envs:
        _envs[which] = LimitEnv(moai, 12, which, None)
    return _envs[which]


def top_rows(e, L, polys):
    return np.stack([np.stack([np.full(e.n, q - 1, dtype=np.uint64) for q in e.primes[:L]])] * polys)


def modulus(e, L):
    return np.array(e.primes[:L], dtype=np.uint64).reshape(1, L, 1)


def unchanged(bufs, hosts):
    for i, (d, h) in enumerate(zip(bufs, hosts)):
        assert (d.to_numpy(words=h.size) == h.reshape(-1)).all(), "input %d was written" % i


def keys_unchanged(e):
    for kind in KEYS:
        assert (e.dkey(kind).to_numpy(e.key(kind).shape) == e.key(kind)).all(), "key %s was written" % kind


# ---- list forms: rotations ------------------------------------------------------------------------------------------------------------
def members(e, L):
    """(ciphertexts [5][2][L][N], elements, HR.apply_galois per member)"""
    def make():
        rng = np.random.default_rng(9500 + L)
        elts = e.elts(MEMBER_STEPS)
        cts = O.uniform_rns(rng, e.primes[:L], (5, 2), e.n)
        cts[0, 1][..., O.galois_table_ntt(e.logn, elts[0])] = e.octx.ntt(ML.worst_coeff(e.primes, L, e.alpha, e.n), L)
        cts[1], cts[2] = e.edges(L, 2)
        cts.setflags(write=False)
        refs = [HR.apply_galois(e.octx, cts[i], L, elts[i], e.key(MEMBER_KINDS[i]), e.alpha) for i in range(5)]
        return cts, elts, refs
    if ("members", L) not in e.cache:
        e.cache[("members", L)] = make()
    return e.cache[("members", L)]


@pytest.mark.parametrize("L", LEVELS)
@pytest.mark.parametrize("which", CHAINS)
def test_apply_galois_list(moai, which, L):
    """without sums, then with sums on members 0 (an addend of all q - 1), 2 and 4 (uniform)"""
    e = env(moai, which)
    with tuned(moai):
        assert_modes(moai, e)
        cts, elts, refs = members(e, L)
        assert (elts[4], MEMBER_KINDS[4]) == (elts[0], MEMBER_KINDS[0]) and len(set(elts)) == 2
        addends = O.uniform_rns(np.random.default_rng(9600 + L), e.primes[:L], (5, 2), e.n)
        addends[0] = top_rows(e, L, 2)
        dkeys = [e.dkey(kind) for kind in MEMBER_KINDS]
        for with_sums in (False, True):
            d_in = [e.up(ct) for ct in cts]
            d_out = [e.filled((2, L, e.n), PATTERN) for _ in cts]
            sums = [e.up(addends[i]) if i % 2 == 0 else None for i in range(5)] if with_sums else None
            e.ctx.apply_galois_hybrid_ptrs(d_in, d_out, L, e.alpha, elts, dkeys, sums)
            for i in range(5):
                want = (refs[i] + addends[i]) % modulus(e, L) if with_sums and i % 2 == 0 else refs[i]
                assert (d_out[i].to_numpy((2, L, e.n)) == want).all(), (with_sums, MEMBER_NAMES[i])
            unchanged(d_in, cts)
            if with_sums:
                unchanged(sums[0::2], addends[0::2])
            for b in d_in + d_out + ([s for s in sums if s is not None] if with_sums else []):
                b.free()
    keys_unchanged(e)


@pytest.mark.parametrize("L", LEVELS)
@pytest.mark.parametrize("which", CHAINS)
def test_to_and_acc(moai, which, L):
    """members 0 and 4 (one key, one element) and the member of all q - 1 under them, in one batch of 3"""
    e = env(moai, which)
    with tuned(moai):
        assert_modes(moai, e)
        cts, elts, refs = members(e, L)
        kind, elt = MEMBER_KINDS[0], elts[0]
        if ("to ref", L) not in e.cache:
            e.cache[("to ref", L)] = HR.apply_galois(e.octx, cts[1], L, elt, e.key(kind), e.alpha)
        batch, want = cts[[0, 1, 4]], np.stack([refs[0], e.cache[("to ref", L)], refs[4]])
        src, dst = e.up(batch), e.filled(batch.shape, PATTERN)
        e.ctx.apply_galois_hybrid_to(src, dst, L, e.alpha, elt, e.dkey(kind), 3)
        assert (dst.to_numpy(batch.shape) == want).all()
        unchanged([src], [batch])
        base = O.uniform_rns(np.random.default_rng(9700 + L), e.primes[:L], (3, 2), e.n)
        base[1] = top_rows(e, L, 2)
        acc = e.up(base)
        e.ctx.apply_galois_hybrid_acc(src, acc, L, e.alpha, elt, e.dkey(kind), 3)
        assert (acc.to_numpy(batch.shape) == (want + base) % modulus(e, L)).all()
        unchanged([src], [batch])
        for b in (src, dst, acc):
            b.free()
    keys_unchanged(e)


# ---- list forms: relinearize ------------------------------------------------------------------------------------------------------------
CT3_NAMES = ["c2 worst_coeff", "all q-1", "zero", "uniform", "c0, c1 all q-1 and c2 q/2, q/2+1"]


def ct3_members(e, L):
    """[5][3][L][N]"""
    def make():
        rng = np.random.default_rng(9800 + L)
        c = O.uniform_rns(rng, e.primes[:L], (5, 3), e.n)
        c[0, 2] = e.octx.ntt(ML.worst_coeff(e.primes, L, e.alpha, e.n), L)
        c[1], c[2] = e.edges(L, 3)
        c[4, :2] = top_rows(e, L, 2)
        c[4, 2] = e.octx.ntt(ML.pattern_rows(e.primes[:L], e.n, rng)[3], L)
        c.setflags(write=False)
        return c
    if ("ct3", L) not in e.cache:
        e.cache[("ct3", L)] = make()
    return e.cache[("ct3", L)]


def ct3_refs(e, L, kind, rescale):
    at = ("ct3 ref", L, kind, rescale)
    if at not in e.cache:
        f = RR.relinearize_rescale if rescale else HR.relinearize
        e.cache[at] = [f(e.octx, c, e.key(kind), L, e.alpha) for c in ct3_members(e, L)]
    return e.cache[at]


def check_relin_list(moai, e, L, kind, rescale):
    with tuned(moai):
        assert_modes(moai, e)
        ct3, refs = ct3_members(e, L), ct3_refs(e, L, kind, rescale)
        Lout = L - 1 if rescale else L
        d_in = [e.up(c) for c in ct3]
        d_out = [e.filled((2, Lout, e.n), PATTERN) for _ in ct3]
        call = e.ctx.relinearize_rescale_hybrid_ptrs if rescale else e.ctx.relinearize_hybrid_ptrs
        call(d_in, d_out, e.dkey(kind), L, e.alpha)
        for i in range(5):
            assert (d_out[i].to_numpy((2, Lout, e.n)) == refs[i]).all(), CT3_NAMES[i]
        unchanged(d_in, ct3)
        for b in d_in + d_out:
            b.free()
    keys_unchanged(e)


@pytest.mark.parametrize("kind", KEYS)
@pytest.mark.parametrize("L", LEVELS)
@pytest.mark.parametrize("which", CHAINS)
def test_relinearize_list(moai, which, L, kind):
    check_relin_list(moai, env(moai, which), L, kind, False)


@pytest.mark.parametrize("kind", KEYS)
@pytest.mark.parametrize("L", LEVELS)
@pytest.mark.parametrize("which", CHAINS)
def test_relinearize_rescale_list(moai, which, L, kind):
    check_relin_list(moai, env(moai, which), L, kind, True)


# ---- the merged rescale -------------------------------------------------------------------------------------------------------------------
def rescale_inputs(e, L):
    """[3][3][L][N]: every row q - 1; (alternating 0 / q - 1, q/2 and q/2 + 1, all q - 1) of ML.pattern_rows; uniform"""
    if ("rescale in", L) not in e.cache:
        rng = np.random.default_rng(9900 + L)
        pat = ML.pattern_rows(e.primes[:L], e.n, rng)
        ct3 = np.stack([top_rows(e, L, 3), pat[[2, 3, 0]], O.uniform_rns(rng, e.primes[:L], (3,), e.n)])
        ct3.setflags(write=False)
        e.cache[("rescale in", L)] = ct3
    return e.cache[("rescale in", L)]


@pytest.mark.parametrize("kind", KEYS)
@pytest.mark.parametrize("L", [7, 4, 2])
@pytest.mark.parametrize("which", CHAINS)
def test_merged_rescale_at_the_limits(moai, which, L, kind):
    e = env(moai, which)
    with tuned(moai):
        assert_modes(moai, e)
        if which == "special_small":
            assert e.names[L - 1] == {7: "ng_hi", 4: "fpr_lo", 2: "fpn_hi"}[L]
        ct3 = rescale_inputs(e, L)
        at = ("rescale ref", L, kind)
        if at not in e.cache:
            e.cache[at] = np.stack([RR.relinearize_rescale(e.octx, c, e.key(kind), L, e.alpha) for c in ct3])
        d3, out = e.up(ct3), e.filled((3, 2, L - 1, e.n), PATTERN)
        e.ctx.relinearize_rescale_hybrid(d3, e.dkey(kind), out, L, e.alpha, 3)
        got = out.to_numpy((3, 2, L - 1, e.n))
        unchanged([d3], [ct3])
        d3.free()
        out.free()
    for b, name in enumerate(("all q-1", "patterns", "uniform")):
        assert (got[b] == e.cache[at][b]).all(), name
    keys_unchanged(e)


@pytest.mark.parametrize("square", [False, True])
@pytest.mark.parametrize("kind", KEYS)
@pytest.mark.parametrize("L", [7, 4, 2])
@pytest.mark.parametrize("which", CHAINS)
def test_multiply_relin_rescale(moai, which, L, kind, square):
    """x, y [2][2][L][N] from ML.pair_rows: coefficients 0 .. 24 of every row hold the 25 ordered pairs of (0, 1, q - 1, q/2, q/2 + 1)
    in (x0, y0) and in (x1, y1), (q - 1, q - 1) among them; coefficient 25 is q - 1 in all four polynomials, so the middle sum is
    (q - 1)(q - 1) twice there; the second ciphertext is the pair exchanged"""
    e = env(moai, which)
    with tuned(moai):
        assert_modes(moai, e)
        a, b = ML.pair_rows(e.primes[:L], 2, e.n, np.random.default_rng(10000 + L))
        for r, q in enumerate(e.primes[:L]):
            at = int(-(5 * r) % 25)  # where polynomial 0 of row r starts in the cycle: pair 12 of it is (q - 1, q - 1)
            assert (a[0, r, (12 + at) % 25], b[0, r, (12 + at) % 25]) == (q - 1, q - 1), r
        for r, q in enumerate(e.primes[:L]):
            a[:, r, 25] = b[:, r, 25] = q - 1
        x, y = np.stack([a, b]), np.stack([b, a])
        if square:
            y = x
        want = np.stack([RR.multiply_relin_rescale(e.octx, x[i], y[i], e.key(kind), L, e.alpha) for i in range(2)])
        dx = e.up(x)
        dy = dx if square else e.up(y)
        out = e.filled((2, 2, L - 1, e.n), PATTERN)
        e.ctx.multiply_relin_rescale_hybrid(dx, dy, e.dkey(kind), out, L, e.alpha, 2)
        got = out.to_numpy(want.shape)
        unchanged([dx, dy], [x, y])
    assert (got == want).all()
    keys_unchanged(e)


# ---- the exact rounding mode --------------------------------------------------------------------------------------------------------------
def exact_inputs(e, L):
    """[3][3][L][N]: (c0, c1 all q - 1, c2 = NTT(worst_coeff)); every row q - 1; uniform"""
    if ("exact in", L) not in e.cache:
        ct3 = np.stack([top_rows(e, L, 3), top_rows(e, L, 3), O.uniform_rns(np.random.default_rng(10100 + L), e.primes[:L], (3,), e.n)])
        ct3[0, 2] = e.octx.ntt(ML.worst_coeff(e.primes, L, e.alpha, e.n), L)
        ct3.setflags(write=False)
        e.cache[("exact in", L)] = ct3
    return e.cache[("exact in", L)]


@pytest.mark.parametrize("kind", KEYS)
@pytest.mark.parametrize("L", LEVELS)
@pytest.mark.parametrize("which", CHAINS)
def test_exact_switch_and_rescale(moai, which, L, kind):
    e = env(moai, which)
    with tuned(moai):
        assert_modes(moai, e)
        ct3, key = exact_inputs(e, L), e.key(kind)
        with exact(e):
            sw = run_switch(e, ct3[:, :2], ct3[:, 2], e.dkey(kind), L)
            rs = run_rescale(e, ct3, e.dkey(kind), L)
    differs = False
    for b, name in enumerate(("worst_coeff", "all q-1", "uniform")):
        want = HX.switch_key(e.octx, ct3[b, :2], ct3[b, 2], key, L, e.alpha)
        assert (sw[b] == want).all(), ("switch", name)
        assert (rs[b] == HX.relinearize_rescale(e.octx, ct3[b], key, L, e.alpha)).all(), ("rescale", name)
        differs = differs or (want != HX.switch_key(e.octx, ct3[b, :2], ct3[b, 2], key, L, e.alpha, exact=False)).any()
    assert differs  # an implementation that leaves the overflow in gives the fast bits
    keys_unchanged(e)


@pytest.mark.parametrize("which", CHAINS)
def test_exact_sums(moai, which):
    """the default cases of the two sums at L = 7 on one ciphertext (c1 = NTT(worst_coeff), c0 all q - 1), against the restatements
    with the exact step 5 in place"""
    e, L = env(moai, which), 7
    with tuned(moai):
        assert_modes(moai, e)
        ct = exact_inputs(e, L)[:1, [0, 2]]
        assert e.octx.ntt(ct[0, 1], L, inverse=True).all()
        dot = DotCase(e, L, B=1, ct=lambda rng: ct, kinds=MEMBER_KINDS + [None], want=False)
        bsgs = BsgsCase(e, L, B=1, ct=lambda rng: ct, kinds=[None] + MEMBER_KINDS, giant_kinds=[None, "rnd", "max"], want=False)
        with exact(e):
            fb_dot, got_dot = dot.run()
            fb_bsgs, got_bsgs = bsgs.run()
    assert not fb_dot and not fb_bsgs, "fallback taken"
    with HX.patched():
        assert (got_dot[:, 0] == HD.rotate_pt_dot(e.octx, ct[0], L, e.alpha, dot.elts, dot.keys, dot.plains)).all()
        want = HB.bsgs_dot(e.octx, ct[0], L, e.alpha, bsgs.baby, bsgs.bkeys, bsgs.giant, bsgs.gkeys, bsgs.plains)
    assert (got_bsgs[0] == want).all()
    assert (want != HB.bsgs_dot(e.octx, ct[0], L, e.alpha, bsgs.baby, bsgs.bkeys, bsgs.giant, bsgs.gkeys, bsgs.plains)).any()  # not the fast bits


@pytest.mark.parametrize("rescale", [False, True])
@pytest.mark.parametrize("which", CHAINS)
def test_exact_boundaries(moai, which, rescale):
    """a single-digit switch (L = 1) and merged rescale (L = 2) whose accumulators put X' on 0, 1, 2, W-2, W-1, H-1, H, H+1.  On
    special_small the sources are the specials fpr_hi, small and the prime below fpn_hi (and the data prime fpn_hi in the rescale's set)
    under the 61-bit target; on special_large g60, g61 and the prime below ng_hi (and g_lo) over the 47-bit target fpn_hi"""
    e = env(moai, which)
    with tuned(moai):
        assert_modes(moai, e)
        check_boundaries(e, rescale)


@pytest.mark.parametrize("which", CHAINS)
def test_fast_after_exact(moai, which):
    """exact, then fast on the same context and cached tables: the exact restatement, then hybrid_ref and hybrid_rescale_ref again"""
    e, L, kind = env(moai, which), 4, "rnd"
    with tuned(moai):
        assert_modes(moai, e)
        ct3, key = exact_inputs(e, L)[2:], e.key(kind)
        with exact(e):
            first = run_switch(e, ct3[:, :2], ct3[:, 2], e.dkey(kind), L), run_rescale(e, ct3, e.dkey(kind), L)
        second = run_switch(e, ct3[:, :2], ct3[:, 2], e.dkey(kind), L), run_rescale(e, ct3, e.dkey(kind), L)
    assert (first[0][0] == HX.switch_key(e.octx, ct3[0, :2], ct3[0, 2], key, L, e.alpha)).all()
    assert (first[1][0] == HX.relinearize_rescale(e.octx, ct3[0], key, L, e.alpha)).all()
    assert (second[0][0] == HR.switch_key(e.octx, ct3[0, :2], ct3[0, 2], key, L, e.alpha)).all()
    assert (second[1][0] == RR.relinearize_rescale(e.octx, ct3[0], key, L, e.alpha)).all()
    assert (first[0] != second[0]).any() and (first[1] != second[1]).any()
