"""GPU tests of the hoisted rotations over the hybrid key switch (include/moai_hip.h: moai_hybrid_hoist_correction,
moai_apply_galois_hybrid_hoisted).  The oracle is bit-identity with R separate moai_apply_galois_hybrid calls (themselves pinned to
tests/hybrid_ref.py by tests/test_gpu_hybrid_keyswitch.py); the correction is compared with tests/hybrid_hoist_ref.py.

1. alpha = 1 is the existing hoisted path (moai_hoist_correction, moai_apply_galois_hoisted) word for word.
2. alpha > 1: full digits, a partial last digit, a last digit of one prime, one digit of one prime; small and tiled transforms.
3. Digits of 6 and 12 primes.
4. A zero coefficient in INTT(c1) takes the fallback and still gives the same bits.
5. MOAI_HYBRID_HOIST_NR = 4, 2, 1 give the same bits.
6. Chunks of ciphertexts and groups of rotations under a scratch budget do not change the result.
7. MOAI's parameters once: N = 2^16, 35 data primes, 12 special primes.
8. Every refusal is MOAI_EINVAL and leaves the outputs alone.
9. Op-trace counts.

Unless said otherwise R = 5 rotations (passes of 4 and of 2 leave a remainder), each with its own random key, on a batch of 3; every
input is checked on the CPU to have no zero coefficient in INTT(c1) (fixed seeds)."""
import ctypes as C

import numpy as np
import pytest

import hybrid_hoist_ref as HH
import hybrid_ref as HR
from hybrid_kit import EINVAL, FILL, MOAI_DATA_BITS, OK, PATTERN, Env, traced, tuned
from hybrid_kit import env_small1, env_small2, env_tiled1, env_tiled3  # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu

STEPS = [1, 3, -2, 64, 0]  # 0 = conjugation (Galois element 2N - 1)


class Case:
    """R rotations of one batch: the operands on the device, and the R separate moai_apply_galois_hybrid calls computed once"""

    def __init__(self, e, L, steps=STEPS, B=3, seed=0, ct=None):
        self.e, self.L, self.B, self.R = e, L, B, len(steps)
        rng = np.random.default_rng(e.logn * 1000 + e.alpha * 100 + L * 10 + seed)
        self.elts = e.elts(steps)
        self.keys = [e.random_key(rng) for _ in steps]
        self.dkeys = [e.up(k) for k in self.keys]
        self.ct = e.random_input(rng, L, B) if ct is None else ct(rng)
        self.dct = e.up(self.ct)
        self.corrs = [e.ctx.hybrid_hoist_correction(dk, elt, L, e.alpha) for dk, elt in zip(self.dkeys, self.elts)]
        self.shape = (self.R, B, 2, L, e.n)
        self.want = np.empty(self.shape, dtype=np.uint64)
        for r in range(self.R):
            d = e.up(self.ct)
            e.ctx.apply_galois_hybrid(d, L, e.alpha, self.elts[r], self.dkeys[r], B)
            self.want[r] = d.to_numpy(self.shape[1:])

    def hoisted(self):
        """(fallback flag, outputs [R][B][2][L][N]) from output buffers filled with a pattern"""
        out = self.e.filled(self.shape, PATTERN)
        fb = self.e.ctx.apply_galois_hybrid_hoisted(self.dct, out, self.L, self.e.alpha, self.elts, self.dkeys, self.corrs, self.B)
        return fb, out.to_numpy(self.shape)

    def check(self):
        fb, got = self.hoisted()
        assert not fb
        for r in range(self.R):
            assert (got[r] == self.want[r]).all(), r
        assert (self.dct.to_numpy(self.ct.shape) == self.ct).all()  # the input is left alone

    def check_corrections(self):
        e = self.e
        for r in range(self.R):
            want = HH.hoist_correction(e.octx, self.keys[r], self.elts[r], self.L, e.alpha)
            assert (self.corrs[r].to_numpy(want.shape) == want).all(), r


# ---- 1. alpha = 1 is the existing hoisted path ---------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [3, 1])
def test_alpha_1_equals_the_existing_hoisted_entry_points(moai, env_tiled1, L):
    e = env_tiled1
    c = Case(e, L)
    c.check()
    old_corrs = [e.ctx.hoist_correction(dk, elt, L) for dk, elt in zip(c.dkeys, c.elts)]
    for r in range(c.R):
        assert (c.corrs[r].to_numpy() == old_corrs[r].to_numpy()).all(), r
    out = moai.DeviceBuffer(int(np.prod(c.shape)))
    assert not e.ctx.apply_galois_hoisted(c.dct, out, L, c.elts, c.dkeys, old_corrs, c.B)
    assert (out.to_numpy(c.shape) == c.hoisted()[1]).all()


def test_alpha_1_small_transform_equals_separate_calls(env_small1):
    c = Case(env_small1, env_small1.lmax)
    c.check()
    c.check_corrections()


# ---- 2. alpha > 1 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [5, 3, 1])
def test_alpha_2_small_transform_equals_separate_calls(env_small2, L):
    c = Case(env_small2, L)
    c.check()
    c.check_corrections()


@pytest.mark.parametrize("L", [7, 4])
def test_alpha_3_tiled_transform_equals_separate_calls(env_tiled3, L):
    c = Case(env_tiled3, L)
    c.check()
    c.check_corrections()


# ---- 3. wide digits -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alpha", [6, 12])
def test_wide_digits_equal_separate_calls(moai, alpha):
    e = Env(moai, 10, [40] * (alpha + 1), [50] * alpha)
    Case(e, alpha + 1, steps=[1, 0], B=1).check()
    e.close()


# ---- 4. fallback ----------------------------------------------------------------------------------------------------------------
def test_a_zero_coefficient_takes_the_fallback_and_the_same_bits(env_small2):
    e, L = env_small2, 5

    def with_sparse_c1(rng):
        ct = e.random_input(rng, L, 3)
        sparse = np.zeros((1, L, e.n), dtype=np.uint64)
        sparse[0, :, 1] = 5
        ct[0, 1] = e.octx.ntt(sparse, L)[0]
        return ct

    c = Case(e, L, ct=with_sparse_c1)
    fb, got = c.hoisted()
    assert fb
    assert (got == c.want).all()
    assert (c.dct.to_numpy(c.ct.shape) == c.ct).all()


# ---- 5. every instantiation -----------------------------------------------------------------------------------------------------
def test_rotations_per_pass_do_not_change_the_bits(moai, env_tiled3):
    c = Case(env_tiled3, 7, seed=5)
    with tuned(moai):
        for per_pass in (4, 2, 1):
            moai.hip.set_tuning("MOAI_HYBRID_HOIST_NR", per_pass)
            fb, got = c.hoisted()
            assert not fb and (got == c.want).all(), per_pass


# ---- 6. chunking ----------------------------------------------------------------------------------------------------------------
def test_chunks_and_groups_give_the_unchunked_result(moai, env_tiled3):
    """L = 7, alpha = 3, beta = 3, rows of 32 KiB.  The header's formula: cb beta (L + alpha) + cb G (5 L + 4 alpha) = 30 cb + 47 cb G
    rows.  154 rows hold two ciphertexts with one rotation in flight (chunks of 2, 2, 1; five groups each), 124 rows one ciphertext
    with two rotations (five chunks; groups of 2, 2, 1), and 1 KiB is the floor of one and one."""
    e, L, B = env_tiled3, 7, 5
    c = Case(e, L, B=B, seed=6)
    shared, per_rotation, row_kib = HR.beta(L, e.alpha) * (L + e.alpha), 5 * L + 4 * e.alpha, e.n * 8 // 1024
    budgets = [2 * (shared + per_rotation) * row_kib, (shared + 2 * per_rotation) * row_kib, 1]
    assert budgets == [154 * 32, 124 * 32, 1]
    c.check()  # unchunked
    with tuned(moai):
        for kb in budgets:
            moai.hip.set_tuning("MOAI_HYBRID_TMP_KB", kb)
            fb, got = c.hoisted()
            assert not fb and (got == c.want).all(), kb


# ---- 7. MOAI's parameters -------------------------------------------------------------------------------------------------------
def test_moais_parameters_equal_separate_calls(moai):
    """N = 2^16, MOAI's 35 data primes plus twelve 60-bit special primes, L = 35: three digits, two of 12 primes and one of 11"""
    e = Env(moai, 16, MOAI_DATA_BITS, [60] * 12)
    Case(e, 35, steps=[1, 0], B=1).check()
    e.close()


# ---- 8. refusals ----------------------------------------------------------------------------------------------------------------
def test_every_refusal_is_einval_and_leaves_the_outputs_alone(moai, env_small2):
    e, n, k, alpha = env_small2, env_small2.n, env_small2.k, env_small2.alpha
    L, B, R = e.lmax, 2, 2
    lib = moai.hip.lib()
    words = B * 2 * L * n
    fill = np.full(R * words, FILL, dtype=np.uint64)
    out, src = e.up(fill), e.filled(words, 5)
    corr_fill = np.full(2 * (L + alpha) * n, 9, dtype=np.uint64)
    dkey, dcorr = moai.DeviceBuffer(e.digits * 2 * k * n), e.up(corr_fill)
    h, s, ky, co = e.ctx.h, src.ptr, dkey.ptr, dcorr.ptr
    vp = C.c_void_p

    def arr(*ptrs):
        return (vp * len(ptrs))(*ptrs)

    outs, keys, corrs = arr(out.ptr, out.ptr + words * 8), arr(ky, ky), arr(co, co)
    elts = (C.c_uint32 * R)(3, 5)
    fb = C.c_int(0)

    def hoisted(ctx=h, src=s, outs=outs, L=L, alpha=alpha, elts=elts, keys=keys, corrs=corrs, R=R, batch=B):
        return lib.moai_apply_galois_hybrid_hoisted(ctx, src, outs, L, alpha, elts, keys, corrs, R, batch, C.byref(fb), None)

    def correction(ctx=h, key=ky, elt=3, L=L, alpha=alpha, corr=co):
        return lib.moai_hybrid_hoist_correction(ctx, key, elt, L, alpha, corr, None)

    calls = [
        # what every hybrid entry point refuses
        lambda: hoisted(ctx=None),
        lambda: hoisted(alpha=0),
        lambda: hoisted(alpha=k, L=1),
        lambda: hoisted(alpha=17, L=1),
        lambda: hoisted(L=0),
        lambda: hoisted(L=L + 1),
        lambda: correction(ctx=None),
        lambda: correction(alpha=0),
        lambda: correction(alpha=k, L=1),
        lambda: correction(L=0),
        lambda: correction(L=L + 1),
        # a null array, a null entry in one
        lambda: hoisted(src=None),
        lambda: hoisted(outs=None),
        lambda: hoisted(elts=None),
        lambda: hoisted(keys=None),
        lambda: hoisted(corrs=None),
        lambda: hoisted(outs=arr(out.ptr, None)),
        lambda: hoisted(keys=arr(ky, None)),
        lambda: hoisted(corrs=arr(None, co)),
        lambda: correction(key=None),
        lambda: correction(corr=None),
        # an even or out-of-range Galois element
        lambda: hoisted(elts=(C.c_uint32 * R)(3, 4)),
        lambda: hoisted(elts=(C.c_uint32 * R)(2 * n + 1, 3)),
        lambda: correction(elt=4),
        lambda: correction(elt=2 * n + 1),
        # an output that is the input, or overlaps it or another output
        lambda: hoisted(outs=arr(out.ptr, s)),
        lambda: hoisted(src=out.ptr + 8 * n),
        lambda: hoisted(outs=arr(out.ptr, out.ptr + 8 * n)),
    ]
    for i, call in enumerate(calls):
        assert call() == EINVAL, i
        assert lib.moai_last_error(), i
    # batch = 0 and R = 0 are MOAI_OK and enqueue nothing
    assert hoisted(batch=0) == OK
    assert hoisted(R=0) == OK
    assert (out.to_numpy() == fill).all()
    assert (dcorr.to_numpy() == corr_fill).all()
    assert (src.to_numpy() == 5).all()


# ---- 9. op trace ----------------------------------------------------------------------------------------------------------------
def test_op_trace_counts(moai, env_small2):
    e, L = env_small2, 3
    c = Case(e, L, steps=[1, 0], B=3, seed=9)
    with traced(moai) as trace:
        e.ctx.hybrid_hoist_correction(c.dkeys[0], c.elts[0], L, e.alpha)
        c.hoisted()
    counts = trace()
    assert counts.get(("hybrid_hoist_correction", L)) == 1
    assert counts.get(("apply_galois_hybrid_hoisted", L)) == 3 * 2
    assert ("apply_galois_hybrid", L) not in counts
