"""GPU tests of the giant steps summed in the extended basis (include/moai_hip.h: moai_hybrid_bsgs_dot), bit for bit against the
integer restatement tests/hybrid_bsgs_ref.py (pinned by tests/test_hybrid_bsgs_cpu.py) unless said otherwise.

1. alpha = 1, tiled and small transforms.
2. alpha > 1: full digits, a partial last digit, one digit of one prime; small and tiled transforms.
3. Digits of 6 and 12 primes.
4. The two identities against the device's own calls: one giant step of element 1 is moai_hybrid_rotate_pt_dot with one output; one
   identity baby term with the all-ones plaintext under one giant step is moai_apply_galois_hybrid on a copy, also at MOAI's
   parameters; N = 2^16 against the restatement.
5. A zero coefficient in INTT(c1) of one ciphertext sets the flag and gives the same bits.
6. MOAI_HYBRID_HOIST_NR = 4, 2, 1 give the same bits.
7. Chunks of ciphertexts and groups of giant steps under a scratch budget do not change the result.
8. 65 giant steps at 61-bit primes with plaintexts of m - 1: the sum Z is carried as residues past 63 terms.
9. Every refusal is MOAI_EINVAL and leaves the output and the input alone; batch = 0 is MOAI_OK.
10. Op-trace counts.

The default case: baby steps [identity, 1, 3, -2, 64, conjugation] (five switched rotations: passes of 4 and of 1), giant steps
[identity, 4, -8], every rotation with its own random key.  Giant step 1 lacks two terms; giant step 2 holds only the identity baby
term, so its c1' takes no step 5.  A batch of 3 at N = 2^10 and of 2 at N = 2^12.  Every input is checked on the CPU to have no zero
coefficient in INTT(c1) (fixed seeds), and is unchanged after every call."""
import ctypes as C

import numpy as np
import pytest

import hybrid_bsgs_ref as HB
import hybrid_ref as HR
import mode_limits as ML
import oracle as O
from hybrid_kit import EINVAL, FILL, IDENT, MOAI_DATA_BITS, OK, PATTERN, Env, cached, traced, tuned, unit_plain
from hybrid_kit import env_small1, env_small2, env_tiled1, env_tiled3  # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu

BABY = [IDENT, 1, 3, -2, 64, 0]  # 0 = conjugation (Galois element 2N - 1)
GIANT = [IDENT, 4, -8]


def default_absent(baby, giant):
    """giant step 1 lacks baby terms 1 and 3; the last giant step holds only the identity baby term"""
    if len(giant) < 3 or IDENT not in baby:
        return set()
    return {(1, 1), (1, 3)} | {(len(giant) - 1, r) for r, s in enumerate(baby) if s != IDENT}


class Case:
    """one call: the operands on the device, and the restatement's output computed once (want=False: not at all)"""

    def __init__(self, e, L, baby=BABY, giant=GIANT, B=None, seed=0, ct=None, plain=None, shared_key=False, want=True):
        B = (3 if e.logn == 10 else 2) if B is None else B
        self.e, self.L, self.B, self.R, self.ng = e, L, B, len(baby), len(giant)
        rng = np.random.default_rng(e.logn * 1000 + e.alpha * 100 + L * 10 + seed + 5)
        self.baby, self.giant = e.elts(baby), e.elts(giant)
        one_key = e.random_key(rng) if shared_key else None
        self.bkeys = [None if elt == 1 else (one_key if shared_key else e.random_key(rng)) for elt in self.baby]
        self.gkeys = [None if elt == 1 else (one_key if shared_key else e.random_key(rng)) for elt in self.giant]
        dk = {}
        self.dbkeys = [None if k is None else cached(dk, id(k), lambda: e.up(k)) for k in self.bkeys]
        self.dgkeys = [None if k is None else cached(dk, id(k), lambda: e.up(k)) for k in self.gkeys]
        self.ct = e.random_input(rng, L, B) if ct is None else ct(rng)
        self.dct = e.up(self.ct)
        dc = {}
        self.corrs = [None if k is None else cached(dc, (id(k), elt), lambda: e.ctx.hybrid_hoist_correction(k, elt, L, e.alpha))
                      for k, elt in zip(self.dbkeys, self.baby)]
        absent = default_absent(baby, giant)
        new_plain = plain or (lambda: O.uniform_rns(rng, e.rows(L), (), e.n))
        self.plains = [[None if (g, r) in absent else new_plain() for r in range(self.R)] for g in range(self.ng)]
        dp = {}
        self.dplains = [[None if p is None else cached(dp, id(p), lambda: e.up(p)) for p in row] for row in self.plains]
        self.shape = (B, 2, L, e.n)
        if want:
            self.want = np.stack([HB.bsgs_dot(e.octx, self.ct[b], L, e.alpha, self.baby, self.bkeys, self.giant, self.gkeys, self.plains)
                                  for b in range(B)])

    def run(self):
        """(fallback flag, output [B][2][L][N]) from an output buffer filled with a pattern"""
        out = self.e.filled(self.shape, PATTERN)
        fb = self.e.ctx.hybrid_bsgs_dot(self.dct, out, self.L, self.e.alpha, self.baby, self.dbkeys, self.corrs, self.giant, self.dgkeys,
                                        self.dplains, self.B)
        got = out.to_numpy(self.shape)
        assert (self.dct.to_numpy(self.ct.shape) == self.ct).all()  # the input is left alone
        return fb, got

    def check(self):
        fb, got = self.run()
        assert not fb
        assert (got == self.want).all()


@pytest.fixture(scope="module")
def case_tiled3(env_tiled3):
    """the default case at alpha = 3, L = 7, shared by the tests of the knobs"""
    return Case(env_tiled3, 7)


# ---- 1. alpha = 1 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [3, 1])
def test_alpha_1_tiled_transform(env_tiled1, L):
    Case(env_tiled1, L).check()


def test_alpha_1_small_transform(env_small1):
    Case(env_small1, 2).check()


# ---- 2. alpha > 1 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [5, 3, 1])
def test_alpha_2_small_transform(env_small2, L):
    Case(env_small2, L).check()


def test_alpha_3_tiled_transform_full_digits(case_tiled3):
    case_tiled3.check()


def test_alpha_3_tiled_transform_partial_digit(env_tiled3):
    Case(env_tiled3, 4).check()


# ---- 3. wide digits -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alpha", [6, 12])
def test_wide_digits(moai, alpha):
    e = Env(moai, 10, [40] * (alpha + 1), [50] * alpha)
    Case(e, alpha + 1, baby=[1, 0], giant=[IDENT, 4], B=1).check()
    e.close()


# ---- 4. the two identities against the device's own calls -----------------------------------------------------------------------
@pytest.mark.parametrize("L", [5, 3])
def test_one_giant_step_of_element_1_is_hybrid_rotate_pt_dot(env_small2, L):
    e = env_small2
    c = Case(e, L, giant=[IDENT], want=False)
    out = e.filled(c.shape, 0)
    fb = e.ctx.hybrid_rotate_pt_dot(c.dct, [out], L, e.alpha, c.baby, c.dbkeys, c.corrs, c.dplains, c.B)
    assert not fb
    fb, got = c.run()
    assert not fb
    assert (got == out.to_numpy(c.shape)).all()


def check_unit_giant_step(e, L, B):
    c = Case(e, L, baby=[IDENT], giant=[3], B=B, plain=unit_plain(e, L), want=False)
    d = e.up(c.ct)
    e.ctx.apply_galois_hybrid(d, L, e.alpha, c.giant[0], c.dgkeys[0], B)
    fb, got = c.run()
    assert not fb
    assert (got == d.to_numpy(c.shape)).all()


def test_a_unit_plaintext_giant_step_is_apply_galois_hybrid(env_small2):
    for L in (5, 3):
        check_unit_giant_step(env_small2, L, 3)


def test_a_unit_plaintext_giant_step_at_moais_parameters(moai):
    """N = 2^16, MOAI's 35 data primes plus twelve 60-bit special primes, L = 35: three digits, two of 12 primes and one of 11"""
    e = Env(moai, 16, MOAI_DATA_BITS, [60] * 12)
    check_unit_giant_step(e, 35, 1)
    e.close()


def test_degree_65536_equals_the_restatement(moai):
    e = Env(moai, 16, [51, 46, 46], [60, 60])
    Case(e, 3, baby=[IDENT, 1], giant=[IDENT, 4], B=1).check()
    e.close()


# ---- 5. fallback ----------------------------------------------------------------------------------------------------------------
def test_a_zero_coefficient_sets_the_flag_and_gives_the_same_bits(env_small2):
    e, L = env_small2, 5

    def with_sparse_c1(rng):
        ct = e.random_input(rng, L, 3)
        sparse = np.zeros((1, L, e.n), dtype=np.uint64)
        sparse[0, :, 1] = 5
        ct[0, 1] = e.octx.ntt(sparse, L)[0]
        return ct

    c = Case(e, L, ct=with_sparse_c1)
    fb, got = c.run()
    assert fb
    assert (got == c.want).all()


# ---- 6. every instantiation -----------------------------------------------------------------------------------------------------
def test_rotations_per_pass_do_not_change_the_bits(moai, case_tiled3):
    c = case_tiled3
    with tuned(moai):
        for per_pass in (4, 2, 1):
            moai.hip.set_tuning("MOAI_HYBRID_HOIST_NR", per_pass)
            fb, got = c.run()
            assert not fb and (got == c.want).all(), per_pass


# ---- 7. chunking ----------------------------------------------------------------------------------------------------------------
def test_chunks_and_giant_groups_give_the_unchunked_result(moai, case_tiled3):
    """L = 7, alpha = 3, beta = 3, rows of 32 KiB, a batch of 2 and 3 giant steps.  The header's formula:
    cb (beta (L + alpha) + 2 L + 2 (L + alpha) + 2 (L + alpha) + 2 alpha + 2 L) + cb G (2 (L + alpha) + 2 L + alpha + L + L + beta (L + alpha))
    = 104 cb + 81 cb G rows, the giant steps first.  347 rows hold one ciphertext with all three giant steps in flight and not two: the
    batch is split.  266 rows do not hold the three, so one ciphertext goes with the two that fit: groups of two and one.  185 rows:
    groups of one.  1 KiB is the floor of one and one."""
    c = case_tiled3
    e, L = c.e, c.L
    assert (c.B, c.ng) == (2, 3)
    beta = HR.beta(L, e.alpha)
    shared = beta * (L + e.alpha) + 2 * L + 2 * (L + e.alpha) + 2 * (L + e.alpha) + 2 * e.alpha + 2 * L
    giant, row_kib = 2 * (L + e.alpha) + 2 * L + e.alpha + L + L + beta * (L + e.alpha), e.n * 8 // 1024
    budgets = [(shared + 3 * giant) * row_kib, (shared + 2 * giant) * row_kib, (shared + giant) * row_kib, 1]
    assert budgets == [347 * 32, 266 * 32, 185 * 32, 1]
    with tuned(moai):
        for kb in budgets:
            moai.hip.set_tuning("MOAI_HYBRID_TMP_KB", kb)
            fb, got = c.run()
            assert not fb and (got == c.want).all(), kb


# ---- 8. more than 63 terms ------------------------------------------------------------------------------------------------------
def test_65_giant_steps_of_full_size_plaintexts_sum_exactly(moai):
    """L = 1, alpha = 1 at two 61-bit primes, one key shared by 65 giant steps that cycle five elements, one identity baby term
    whose plaintext rows are all m - 1.  At most 16 giant steps are in flight, so Z travels between five groups as residues, past
    63 terms; the worst case of a single 128-bit sum rests on the kernel comment's arithmetic."""
    primes = ML.hybrid_chain(10, "long63")[0][:2]
    assert all(p >> 60 == 1 for p in primes)
    e = Env(moai, 10, primes=primes, alpha=1)
    top = np.stack([np.full(e.n, q - 1, dtype=np.uint64) for q in e.rows(1)])
    giant = [[1, 3, -2, 5, 0][g % 5] for g in range(65)]
    Case(e, 1, baby=[IDENT], giant=giant, B=1, plain=lambda: top, shared_key=True).check()
    e.close()


# ---- 9. refusals ----------------------------------------------------------------------------------------------------------------
def test_every_refusal_is_einval_and_leaves_the_output_alone(moai, env_small2):
    e, n, k, alpha = env_small2, env_small2.n, env_small2.k, env_small2.alpha
    L, B, R, G = e.lmax, 2, 2, 2
    lib = moai.hip.lib()
    words = B * 2 * L * n
    fill = np.full(words, FILL, dtype=np.uint64)
    out, src = e.up(fill), e.filled(words, 5)
    dkey, dcorr = moai.DeviceBuffer(e.digits * 2 * k * n), moai.DeviceBuffer(2 * (L + alpha) * n)
    dplain = moai.DeviceBuffer((L + alpha) * n)
    h, s, o, ky, co, pl = e.ctx.h, src.ptr, out.ptr, dkey.ptr, dcorr.ptr, dplain.ptr
    vp = C.c_void_p

    def arr(*ptrs):
        return (vp * len(ptrs))(*ptrs)

    def u32(*v):
        return (C.c_uint32 * len(v))(*v)

    bkeys, corrs, gkeys, plains = arr(ky, ky), arr(co, co), arr(ky, ky), arr(pl, pl, pl, None)
    belts, gelts = u32(3, 5), u32(9, 25)
    fb = C.c_int(0)

    def dot(ctx=h, src=s, out=o, L=L, alpha=alpha, belts=belts, bkeys=bkeys, corrs=corrs, R=R, gelts=gelts, gkeys=gkeys, n_giant=G,
            plains=plains, batch=B):
        return lib.moai_hybrid_bsgs_dot(ctx, src, out, L, alpha, belts, bkeys, corrs, R, gelts, gkeys, n_giant, plains, batch, C.byref(fb), None)

    calls = [
        # what every hybrid entry point refuses
        lambda: dot(ctx=None),
        lambda: dot(alpha=0),
        lambda: dot(alpha=k, L=1),
        lambda: dot(alpha=17, L=1),
        lambda: dot(L=0),
        lambda: dot(L=L + 1),
        # a null array, the giant ones among them
        lambda: dot(src=None),
        lambda: dot(out=None),
        lambda: dot(belts=None),
        lambda: dot(bkeys=None),
        lambda: dot(corrs=None),
        lambda: dot(plains=None),
        lambda: dot(gelts=None),
        lambda: dot(gkeys=None),
        # a null key or correction of a baby step, a null key of a giant step
        lambda: dot(bkeys=arr(ky, None)),
        lambda: dot(corrs=arr(None, co)),
        lambda: dot(gkeys=arr(ky, None)),
        # an even or out-of-range Galois element on either side
        lambda: dot(belts=u32(3, 4)),
        lambda: dot(belts=u32(2 * n + 1, 3)),
        lambda: dot(gelts=u32(9, 4)),
        lambda: dot(gelts=u32(2 * n + 1, 9)),
        # the output is the input or overlaps it
        lambda: dot(out=s),
        lambda: dot(src=o + 8 * n),
        # a giant step with no present term; no baby steps, no giant steps
        lambda: dot(plains=arr(pl, pl, None, None)),
        lambda: dot(R=0),
        lambda: dot(n_giant=0),
    ]
    for i, call in enumerate(calls):
        assert call() == EINVAL, i
        assert lib.moai_last_error(), i
    # the element 1 reads no key on either side: null entries are accepted there, and refused for the step beside it
    assert dot(belts=u32(1, 3), bkeys=arr(None, None), corrs=arr(None, co)) == EINVAL
    assert dot(gelts=u32(1, 9), gkeys=arr(None, None)) == EINVAL
    # batch = 0 is MOAI_OK and enqueues nothing
    assert dot(batch=0) == OK
    assert (out.to_numpy() == fill).all()
    assert (src.to_numpy() == 5).all()


# ---- 10. op trace ---------------------------------------------------------------------------------------------------------------
def test_op_trace_counts(moai, env_small2):
    e, L = env_small2, 3
    c = Case(e, L, baby=[IDENT, 1], giant=[IDENT, 4], B=3, seed=9, want=False)
    with traced(moai) as trace:
        c.run()
    counts = trace()
    assert counts.get(("hybrid_bsgs_dot", L)) == 3
    assert ("hybrid_rotate_pt_dot", L) not in counts
    assert ("apply_galois_hybrid", L) not in counts
