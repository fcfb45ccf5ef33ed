"""GPU tests of the plaintext-weighted sums of hoisted rotations (include/moai_hip.h: moai_hybrid_rotate_pt_dot), bit for bit against
the integer restatement tests/hybrid_dot_ref.py (pinned by tests/test_hybrid_pt_dot_cpu.py) unless said otherwise.

1. alpha = 1, tiled and small transforms.
2. alpha > 1: full digits, a partial last digit, one digit of one prime; small and tiled transforms.
3. Digits of 6 and 12 primes.
4. One output, one rotation, p = 1 is moai_apply_galois_hybrid on a copy, also at MOAI's parameters; N = 2^16 against the restatement.
5. A zero coefficient in INTT(c1) takes the unhoisted route, sets the flag and gives the same bits.
6. MOAI_HYBRID_HOIST_NR = 4, 2, 1 give the same bits.
7. Chunks of ciphertexts and groups of outputs under a scratch budget do not change the result.
8. 65 rotations into one sum at 61-bit primes with plaintexts of m - 1: the sum is carried past 63 terms.
9. Every refusal is MOAI_EINVAL and leaves the outputs and the input alone; zero sizes are MOAI_OK.
10. Op-trace counts.

The default case: a batch of 3, 3 outputs, 6 terms with steps [1, 3, -2, 64, conjugation, identity] (five switched rotations: passes
of 4 and of 2 leave a remainder), each rotation with its own random key.  Output 1 lacks two terms; output 2 holds only the identity
term, so its step 5 is skipped.  Every input is checked on the CPU to have no zero coefficient in INTT(c1) (fixed seeds), and is
unchanged after every call."""
import ctypes as C

import numpy as np
import pytest

import hybrid_dot_ref as HD
import hybrid_ref as HR
import mode_limits as ML
import oracle as O
from hybrid_kit import EINVAL, FILL, IDENT, MOAI_DATA_BITS, OK, PATTERN, Env, cached, traced, tuned, unit_plain
from hybrid_kit import env_small1, env_small2, env_tiled1, env_tiled3  # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu

STEPS = [1, 3, -2, 64, 0, IDENT]  # 0 = conjugation (Galois element 2N - 1)


def default_absent(steps, n_out):
    """output 1 lacks terms 1 and 3; the last output holds only the identity term"""
    if n_out < 3 or IDENT not in steps:
        return set()
    return {(1, 1), (1, 3)} | {(n_out - 1, r) for r, s in enumerate(steps) if s != IDENT}


class Case:
    """one call: the operands on the device, and the restatement's outputs computed once (want=False: not at all)"""

    def __init__(self, e, L, steps=STEPS, B=3, n_out=3, seed=0, ct=None, plain=None, shared_key=False, want=True):
        self.e, self.L, self.B, self.R, self.n_out = e, L, B, len(steps), n_out
        rng = np.random.default_rng(e.logn * 1000 + e.alpha * 100 + L * 10 + seed)
        self.elts = e.elts(steps)
        one_key = e.random_key(rng) if shared_key else None
        self.keys = [None if elt == 1 else (one_key if shared_key else e.random_key(rng)) for elt in self.elts]
        dk = {}
        self.dkeys = [None if k is None else cached(dk, id(k), lambda: e.up(k)) for k in self.keys]
        self.ct = e.random_input(rng, L, B) if ct is None else ct(rng)
        self.dct = e.up(self.ct)
        dc = {}
        self.corrs = [None if k is None else cached(dc, (id(k), elt), lambda: e.ctx.hybrid_hoist_correction(k, elt, L, e.alpha))
                      for k, elt in zip(self.dkeys, self.elts)]
        absent = default_absent(steps, n_out)
        new_plain = plain or (lambda: O.uniform_rns(rng, e.rows(L), (), e.n))
        self.plains = [[None if (g, r) in absent else new_plain() for r in range(self.R)] for g in range(n_out)]
        dp = {}
        self.dplains = [[None if p is None else cached(dp, id(p), lambda: e.up(p)) for p in row] for row in self.plains]
        self.shape = (n_out, B, 2, L, e.n)
        if want:
            self.want = np.empty(self.shape, dtype=np.uint64)
            for b in range(B):
                self.want[:, b] = HD.rotate_pt_dot(e.octx, self.ct[b], L, e.alpha, self.elts, self.keys, self.plains)

    def run(self):
        """(fallback flag, outputs [n_out][B][2][L][N]) from output buffers filled with a pattern"""
        out = self.e.filled(self.shape, PATTERN)
        fb = self.e.ctx.hybrid_rotate_pt_dot(self.dct, out, self.L, self.e.alpha, self.elts, self.dkeys, self.corrs, self.dplains, self.B)
        got = out.to_numpy(self.shape)
        assert (self.dct.to_numpy(self.ct.shape) == self.ct).all()  # the input is left alone
        return fb, got

    def check(self):
        fb, got = self.run()
        assert not fb
        for g in range(self.n_out):
            assert (got[g] == self.want[g]).all(), g


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
    Case(e, alpha + 1, steps=[1, 0], B=1, n_out=1).check()
    e.close()


# ---- 4. the unit plaintext is the separate rotation -----------------------------------------------------------------------------
def check_unit_rotation(e, L, B):
    c = Case(e, L, steps=[3], B=B, n_out=1, plain=unit_plain(e, L), want=False)
    d = e.up(c.ct)
    e.ctx.apply_galois_hybrid(d, L, e.alpha, c.elts[0], c.dkeys[0], B)
    fb, got = c.run()
    assert not fb
    assert (got[0] == d.to_numpy(c.shape[1:])).all()


def test_one_rotation_with_the_unit_plaintext_is_apply_galois_hybrid(env_small2):
    for L in (5, 3):
        check_unit_rotation(env_small2, L, 3)


def test_one_rotation_with_the_unit_plaintext_at_moais_parameters(moai):
    """N = 2^16, MOAI's 35 data primes plus twelve 60-bit special primes, L = 35: three digits, two of 12 primes and one of 11"""
    e = Env(moai, 16, MOAI_DATA_BITS, [60] * 12)
    check_unit_rotation(e, 35, 1)
    e.close()


def test_degree_65536_equals_the_restatement(moai):
    e = Env(moai, 16, [51, 46, 46], [60, 60])
    Case(e, 3, steps=[1, 0, IDENT], B=1, n_out=2).check()
    e.close()


# ---- 5. fallback ----------------------------------------------------------------------------------------------------------------
def test_a_zero_coefficient_takes_the_unhoisted_route_and_the_same_bits(env_small2):
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
def test_chunks_and_output_groups_give_the_unchunked_result(moai, case_tiled3):
    """L = 7, alpha = 3, beta = 3, rows of 32 KiB.  The header's formula: cb (beta (L + alpha) + 4 L + 2 alpha) + cb G (6 L + 4 alpha) =
    64 cb + 54 cb G rows.  236 rows hold two ciphertexts with one output in flight (chunks of 2 and 1; the two switched outputs one
    after the other), 172 rows one ciphertext with two outputs, and 1 KiB is the floor of one and one."""
    c = case_tiled3
    e, L = c.e, c.L
    shared = HR.beta(L, e.alpha) * (L + e.alpha) + 4 * L + 2 * e.alpha
    per_output, row_kib = 6 * L + 4 * e.alpha, e.n * 8 // 1024
    budgets = [2 * (shared + per_output) * row_kib, (shared + 2 * per_output) * row_kib, 1]
    assert budgets == [236 * 32, 172 * 32, 1]
    with tuned(moai):
        for kb in budgets:
            moai.hip.set_tuning("MOAI_HYBRID_TMP_KB", kb)
            fb, got = c.run()
            assert not fb and (got == c.want).all(), kb


# ---- 8. more than 63 terms ------------------------------------------------------------------------------------------------------
def test_65_rotations_of_full_size_plaintexts_sum_exactly(moai):
    """L = 1, alpha = 1 at two 61-bit primes, one key and five corrections reused by 65 rotations, every plaintext row all m - 1.  The
    accumulators cannot be forced to m - 1, so the worst case rests on the kernel comment's arithmetic (a residue plus at most four
    products per 128-bit sum); this pins that the sum is carried as residues past 63 terms."""
    primes = ML.hybrid_chain(10, "long63")[0][:2]
    assert all(p >> 60 == 1 for p in primes)
    e = Env(moai, 10, primes=primes, alpha=1)
    top = np.stack([np.full(e.n, q - 1, dtype=np.uint64) for q in e.rows(1)])
    steps = [[1, 3, -2, 5, 0][r % 5] for r in range(65)]
    Case(e, 1, steps=steps, B=1, n_out=1, plain=lambda: top, shared_key=True).check()
    e.close()


# ---- 9. refusals ----------------------------------------------------------------------------------------------------------------
def test_every_refusal_is_einval_and_leaves_the_outputs_alone(moai, env_small2):
    e, n, k, alpha = env_small2, env_small2.n, env_small2.k, env_small2.alpha
    L, B, R, G = e.lmax, 2, 2, 2
    lib = moai.hip.lib()
    words = B * 2 * L * n
    fill = np.full(G * words, FILL, dtype=np.uint64)
    out, src = e.up(fill), e.filled(words, 5)
    dkey, dcorr = moai.DeviceBuffer(e.digits * 2 * k * n), moai.DeviceBuffer(2 * (L + alpha) * n)
    dplain = moai.DeviceBuffer((L + alpha) * n)
    h, s, ky, co, pl = e.ctx.h, src.ptr, dkey.ptr, dcorr.ptr, dplain.ptr
    vp = C.c_void_p

    def arr(*ptrs):
        return (vp * len(ptrs))(*ptrs)

    outs, keys, corrs, plains = arr(out.ptr, out.ptr + words * 8), arr(ky, ky), arr(co, co), arr(pl, pl, pl, None)
    elts = (C.c_uint32 * R)(3, 5)
    fb = C.c_int(0)

    def dot(ctx=h, src=s, outs=outs, n_out=G, L=L, alpha=alpha, elts=elts, keys=keys, corrs=corrs, R=R, plains=plains, batch=B):
        return lib.moai_hybrid_rotate_pt_dot(ctx, src, outs, n_out, L, alpha, elts, keys, corrs, R, plains, batch, C.byref(fb), None)

    calls = [
        # what every hybrid entry point refuses
        lambda: dot(ctx=None),
        lambda: dot(alpha=0),
        lambda: dot(alpha=k, L=1),
        lambda: dot(alpha=17, L=1),
        lambda: dot(L=0),
        lambda: dot(L=L + 1),
        # a null array
        lambda: dot(src=None),
        lambda: dot(outs=None),
        lambda: dot(elts=None),
        lambda: dot(keys=None),
        lambda: dot(corrs=None),
        lambda: dot(plains=None),
        # a null key or correction of a rotation, a null output
        lambda: dot(keys=arr(ky, None)),
        lambda: dot(corrs=arr(None, co)),
        lambda: dot(outs=arr(out.ptr, None)),
        # an even or out-of-range Galois element
        lambda: dot(elts=(C.c_uint32 * R)(3, 4)),
        lambda: dot(elts=(C.c_uint32 * R)(2 * n + 1, 3)),
        # an output that is the input, or overlaps it or another output
        lambda: dot(outs=arr(out.ptr, s)),
        lambda: dot(src=out.ptr + 8 * n),
        lambda: dot(outs=arr(out.ptr, out.ptr + 8 * n)),
        # an output with no present term; no terms at all
        lambda: dot(plains=arr(pl, pl, None, None)),
        lambda: dot(R=0),
    ]
    for i, call in enumerate(calls):
        assert call() == EINVAL, i
        assert lib.moai_last_error(), i
    # the element 1 reads neither key nor correction: null entries are accepted there, and refused for the rotation beside it
    assert dot(elts=(C.c_uint32 * R)(1, 3), keys=arr(None, None), corrs=arr(None, co)) == EINVAL
    # zero sizes are MOAI_OK and enqueue nothing
    assert dot(batch=0) == OK
    assert dot(n_out=0) == OK
    assert dot(n_out=0, R=0) == OK
    assert (out.to_numpy() == fill).all()
    assert (src.to_numpy() == 5).all()


# ---- 10. op trace ---------------------------------------------------------------------------------------------------------------
def test_op_trace_counts(moai, env_small2):
    e, L = env_small2, 3
    c = Case(e, L, steps=[1, IDENT], B=3, n_out=2, seed=9, want=False)
    with traced(moai) as trace:
        c.run()
    counts = trace()
    assert counts.get(("hybrid_rotate_pt_dot", L)) == 3 * 2
    assert ("apply_galois_hybrid", L) not in counts
    assert ("apply_galois_hybrid_hoisted", L) not in counts
