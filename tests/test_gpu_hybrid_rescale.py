"""GPU tests of the hybrid relinearize + rescale (include/moai_hip.h: moai_relinearize_rescale_hybrid and
moai_multiply_relin_rescale_hybrid), bit for bit against the integer restatement tests/hybrid_rescale_ref.py (pinned by
tests/test_hybrid_rescale_cpu.py) unless said otherwise.

1. alpha = 1, tiled and small transforms, L = 3 and 2.
2. alpha = 2, small transforms: q_{L-1} alone in the last digit, full digits, a partial digit, one output row; batch 3.
3. alpha = 3, tiled transforms, L = 7, 6, 4; batch 2.
4. Wide digits: 6 and 12 primes; alpha = 8 (nine sources: the 16-source conversion); alpha = 15 (sixteen sources) on 61-bit primes with
   the key all m - 1 and ct3 all q - 1, and a random case; the chains whose sources lie far above and far below the targets.
5. Against the device's own composition relinearize_hybrid + rescale: the difference is one small integer d per coefficient, in
   [-(alpha + 1), 1], the same in every row; also at MOAI's parameters (no restatement at that size).
6. multiply_relin_rescale_hybrid is ct_multiply (ct_square where y is x) followed by call 1, bit for bit.
7. A batch of 3 under a scratch budget that holds one ciphertext gives the same bits.
8. Every refusal is MOAI_EINVAL with its message and leaves the output and the inputs alone; batch = 0 is MOAI_OK.
9. Op-trace counts.

Every call is followed by a check that its inputs are unchanged."""
import numpy as np
import pytest

import hybrid_ref as HR
import hybrid_rescale_ref as RR
import mode_limits as ML
import oracle as O
from hybrid_kit import EINVAL, FILL, MOAI_DATA_BITS, OK, PATTERN, Env, cached, traced, tuned
from hybrid_kit import env_small1, env_small2, env_tiled1, env_tiled3  # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu

def key_of(e):
    """one uniform key per environment, (host, device), made once"""
    def make():
        k = O.uniform_rns(np.random.default_rng(e.logn * 100 + e.alpha), e.primes, (e.digits, 2), e.n)
        return k, e.up(k)
    return cached(e.cache, "key", make)


def default_batch(e):
    return {1: 1, 2: 3, 3: 2}.get(e.alpha, 1)


class Case:
    """one call: ct3 [B][3][L][N] and the key on the device, and the restatement's output computed once (want=False: not at all)"""

    def __init__(self, e, L, B=None, seed=0, ct3=None, key=None, want=True):
        self.e, self.L = e, L
        self.B = B = default_batch(e) if B is None else B
        rng = np.random.default_rng(e.logn * 1000 + e.alpha * 100 + L * 10 + seed + 3)
        self.ct3 = O.uniform_rns(rng, e.primes[:L], (B, 3), e.n) if ct3 is None else ct3
        self.dct3 = e.up(self.ct3)
        self.key, self.dkey = key_of(e) if key is None else (key, e.up(key))
        self.shape = (B, 2, L - 1, e.n)
        if want:
            self.want = np.stack([RR.relinearize_rescale(e.octx, self.ct3[b], self.key, L, e.alpha) for b in range(B)])

    def run(self):
        """the output [B][2][L-1][N], from a buffer filled with a pattern"""
        out = self.e.filled(self.shape, PATTERN)
        self.e.ctx.relinearize_rescale_hybrid(self.dct3, self.dkey, out, self.L, self.e.alpha, self.B)
        got = out.to_numpy(self.shape)
        assert (self.dct3.to_numpy(self.ct3.shape) == self.ct3).all()  # the inputs are left alone
        assert (self.dkey.to_numpy(self.key.shape) == self.key).all()
        return got

    def check(self):
        assert (self.run() == self.want).all()


def case(e, L):
    """the default case of an environment at L, shared by the tests that run at the shapes of 2 and 3"""
    return cached(e.cache, ("case", L), lambda: Case(e, L))


# ---- 1. alpha = 1 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [3, 2])
def test_alpha_1_tiled_transform(env_tiled1, L):
    Case(env_tiled1, L).check()


def test_alpha_1_small_transform(env_small1):
    Case(env_small1, 2).check()


# ---- 2., 3. alpha > 1 -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [5, 4, 3, 2])
def test_alpha_2_small_transform(env_small2, L):
    case(env_small2, L).check()


@pytest.mark.parametrize("L", [7, 6, 4])
def test_alpha_3_tiled_transform(env_tiled3, L):
    case(env_tiled3, L).check()


# ---- 4. wide digits ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alpha", [6, 8, 12])
def test_wide_digits(moai, alpha):
    """alpha = 8: nine sources, which only the 16-source instantiation of the conversion holds"""
    e = Env(moai, 10, [40] * (alpha + 1), [50] * alpha)
    Case(e, alpha + 1, B=1).check()
    e.close()


@pytest.fixture(scope="module")
def env_sixteen_sources(moai):
    """alpha = 15 on 61-bit primes: sixteen data primes (a digit of 15 and q_{L-1} alone) and fifteen special ones"""
    logn = 10
    g61 = ML.chain(logn)["g61"]
    primes = [g61] + ML.primes_below(logn, g61, 30)
    assert all(p >> 60 == 1 for p in primes)
    return Env(moai, logn, primes=primes, alpha=15)


def test_sixteen_sources_at_the_residues_limits(env_sixteen_sources):
    e, L = env_sixteen_sources, 16
    key = np.empty((e.digits, 2, e.k, e.n), dtype=np.uint64)
    for r, m in enumerate(e.primes):
        key[:, :, r, :] = m - 1
    ct3 = np.empty((1, 3, L, e.n), dtype=np.uint64)
    for i in range(L):
        ct3[:, :, i, :] = e.primes[i] - 1
    Case(e, L, B=1, ct3=ct3, key=key).check()


def test_sixteen_sources_random(env_sixteen_sources):
    Case(env_sixteen_sources, 16, B=1).check()


@pytest.mark.parametrize("logn", [10, 12])
@pytest.mark.parametrize("which", ["special_small", "special_large"])
def test_sources_far_from_the_targets(moai, which, logn):
    primes, _, alpha = ML.hybrid_chain(logn, which)
    e = Env(moai, logn, primes=primes, alpha=alpha)
    Case(e, e.lmax, B=1).check()
    e.close()


# ---- 5. against the device's own composition --------------------------------------------------------------------------------------
def check_distance_to_the_composition(e, c, got):
    """got - rescale(relinearize_hybrid(ct3)), per output row in coefficient form: the residue of one integer d in [-(alpha + 1), 1],
    the same in every row"""
    ctx, L, B, n = e.ctx, c.L, c.B, e.n
    relin, comp = e.moai.DeviceBuffer(B * 2 * L * n), e.moai.DeviceBuffer(B * 2 * (L - 1) * n)
    ctx.relinearize_hybrid(c.dct3, c.dkey, relin, L, e.alpha, B)
    ctx.rescale(relin, comp, 2, L, B)
    diff, dgot = e.moai.DeviceBuffer(B * 2 * (L - 1) * n), e.up(got)
    ctx.sub(dgot, comp, diff, B * 2, L - 1)
    ctx.ntt_inverse(diff, B * 2, L - 1)
    r = diff.to_numpy(c.shape)
    q = np.array(e.primes[:L - 1], dtype=np.uint64).reshape(1, 1, L - 1, 1)
    d = np.where(r > q // 2, r.astype(np.int64) - q.astype(np.int64), r.astype(np.int64))
    print("alpha %d L %d: out - composition in [%d, %d]" % (e.alpha, L, d.min(), d.max()))
    assert d.min() >= -(e.alpha + 1) and d.max() <= 1
    assert (d == d[:, :, :1, :]).all()


@pytest.mark.parametrize("L", [5, 4, 3, 2])
def test_distance_to_the_composition_alpha_2(env_small2, L):
    c = case(env_small2, L)
    check_distance_to_the_composition(env_small2, c, c.run())


@pytest.mark.parametrize("L", [7, 6, 4])
def test_distance_to_the_composition_alpha_3(env_tiled3, L):
    c = case(env_tiled3, L)
    check_distance_to_the_composition(env_tiled3, c, c.run())


def test_distance_to_the_composition_at_moais_parameters(moai):
    """N = 2^16, MOAI's 35 data primes plus twelve 60-bit special primes, L = 35 and 15, batch 2, a uniform key"""
    e = Env(moai, 16, MOAI_DATA_BITS, [60] * 12)
    for L in (35, 15):
        c = Case(e, L, B=2, want=False)
        check_distance_to_the_composition(e, c, c.run())
    e.close()


# ---- 6. the product in scratch ------------------------------------------------------------------------------------------------------
def check_multiply(e, L, B):
    ctx, n = e.ctx, e.n
    rng = np.random.default_rng(e.logn * 1000 + e.alpha * 100 + L * 10 + 77)
    x, y = O.uniform_rns(rng, e.primes[:L], (B, 2), n), O.uniform_rns(rng, e.primes[:L], (B, 2), n)
    dx, dy = e.up(x), e.up(y)
    _, dkey = key_of(e)
    shape = (B, 2, L - 1, n)
    for other, dother, product in ((y, dy, lambda t: ctx.ct_multiply(dx, dy, t, L, B)), (x, dx, lambda t: ctx.ct_square(dx, t, L, B))):
        ct3, want = e.moai.DeviceBuffer(B * 3 * L * n), e.moai.DeviceBuffer(int(np.prod(shape)))
        product(ct3)
        ctx.relinearize_rescale_hybrid(ct3, dkey, want, L, e.alpha, B)
        out = e.filled(shape, PATTERN)
        ctx.multiply_relin_rescale_hybrid(dx, dother, dkey, out, L, e.alpha, B)
        assert (out.to_numpy(shape) == want.to_numpy(shape)).all()
        assert (dx.to_numpy(x.shape) == x).all() and (dother.to_numpy(other.shape) == other).all()  # the inputs are left alone


@pytest.mark.parametrize("L", [5, 4, 3, 2])
def test_multiply_is_the_product_then_call_1_alpha_2(env_small2, L):
    check_multiply(env_small2, L, 3)


@pytest.mark.parametrize("L", [7, 6, 4])
def test_multiply_is_the_product_then_call_1_alpha_3(env_tiled3, L):
    check_multiply(env_tiled3, L, 2)


def test_multiply_equals_the_restatement(env_small2):
    e, L = env_small2, 4
    rng = np.random.default_rng(11)
    x, y = O.uniform_rns(rng, e.primes[:L], (1, 2), e.n), O.uniform_rns(rng, e.primes[:L], (1, 2), e.n)
    key, dkey = key_of(e)
    out = e.moai.DeviceBuffer(2 * (L - 1) * e.n)
    e.ctx.multiply_relin_rescale_hybrid(e.up(x), e.up(y), dkey, out, L, e.alpha, 1)
    assert (out.to_numpy((2, L - 1, e.n)) == RR.multiply_relin_rescale(e.octx, x[0], y[0], key, L, e.alpha)).all()


# ---- 7. chunking ------------------------------------------------------------------------------------------------------------------
def test_a_budget_of_one_ciphertext_gives_the_same_bits(moai, env_small2):
    """L = 5, alpha = 2, beta = 3, rows of 8 KiB: the header's beta (L + alpha) + 2 (L + alpha) + 2 (alpha + 1) + 2 (L - 1) = 49 rows
    hold one ciphertext of the batch of 3 (64 with the product's 3 L), and 1 KiB is the floor of one"""
    e, L = env_small2, 5
    c = case(e, L)
    assert c.B == 3
    rows = HR.beta(L, e.alpha) * (L + e.alpha) + 2 * (L + e.alpha) + 2 * (e.alpha + 1) + 2 * (L - 1)
    assert rows == 49
    x = e.up(c.ct3[:, :2].copy())
    _, dkey = key_of(e)
    unchunked = moai.DeviceBuffer(int(np.prod(c.shape)))
    e.ctx.multiply_relin_rescale_hybrid(x, x, dkey, unchunked, L, e.alpha, c.B)
    with tuned(moai):
        for kb in (rows * e.n * 8 // 1024, (rows + 3 * L) * e.n * 8 // 1024, 1):
            moai.hip.set_tuning("MOAI_HYBRID_TMP_KB", kb)
            assert (c.run() == c.want).all(), kb
            out = moai.DeviceBuffer(int(np.prod(c.shape)))
            e.ctx.multiply_relin_rescale_hybrid(x, x, dkey, out, L, e.alpha, c.B)
            assert (out.to_numpy() == unchunked.to_numpy()).all(), kb


# ---- 8. refusals ------------------------------------------------------------------------------------------------------------------
def test_every_refusal_is_einval_and_leaves_everything_alone(moai, env_small2):
    e, n, k, alpha = env_small2, env_small2.n, env_small2.k, env_small2.alpha
    L, B = e.lmax, 2
    lib = moai.hip.lib()
    fill = np.full(B * 2 * (L - 1) * n, FILL, dtype=np.uint64)
    out = e.up(fill)
    src = e.filled(B * 3 * L * n, 5)  # ct3; x and y are its first B * 2 * L * N words
    dkey = e.filled(e.digits * 2 * k * n, 3)
    h, s, o, ky = e.ctx.h, src.ptr, out.ptr, dkey.ptr

    def rr(ctx=h, ct3=s, key=ky, out=o, L=L, alpha=alpha, batch=B):
        return lib.moai_relinearize_rescale_hybrid(ctx, ct3, key, out, L, alpha, batch, None)

    def mm(ctx=h, x=s, y=s, key=ky, out=o, L=L, alpha=alpha, batch=B):
        return lib.moai_multiply_relin_rescale_hybrid(ctx, x, y, key, out, L, alpha, batch, None)

    for call in (rr, mm):
        refused = [
            # what every hybrid entry point refuses, in hy_check's order, with the two this section adds behind L = 0
            (dict(alpha=0), b"alpha = 0"),
            (dict(L=0), b"L = 0"),
            (dict(L=1), b"L = 1"),
            (dict(alpha=16), b"alpha = 16"),
            (dict(ctx=None), b"null context"),
            (dict(alpha=k, L=2), b"leaves no data prime"),
            (dict(alpha=17, L=2), b"alpha = 17"),
            (dict(L=L + 1), b"out of range"),
            # a null pointer
            (dict(key=None), b"null argument"),
            (dict(out=None), b"null argument"),
            # the output overlaps an input or the key
            (dict(out=s), b"overlap"),
            (dict(out=s + 8 * n), b"overlap"),
            (dict(out=ky + 8 * n), b"overlap"),
        ]
        # the order: L = 1 and alpha = 16 come before the context is looked at, alpha = 0 and L = 0 before them
        refused += [(dict(ctx=None, L=1), b"L = 1"), (dict(ctx=None, alpha=16), b"alpha = 16"), (dict(alpha=0, L=1), b"alpha = 0"),
                    (dict(alpha=16, L=0), b"L = 0"), (dict(alpha=16, L=1), b"L = 1")]
        for kw, msg in refused:
            assert call(**kw) == EINVAL, kw
            assert msg in lib.moai_last_error(), (kw, lib.moai_last_error())
        assert call(batch=0) == OK
    assert rr(ct3=None) == EINVAL and b"null argument" in lib.moai_last_error()
    assert mm(x=None) == EINVAL and b"null argument" in lib.moai_last_error()
    assert mm(y=None) == EINVAL and b"null argument" in lib.moai_last_error()
    assert mm(y=o) == EINVAL and b"overlap" in lib.moai_last_error()
    assert (out.to_numpy() == fill).all()
    assert (src.to_numpy() == 5).all() and (dkey.to_numpy() == 3).all()


# ---- 9. op trace ------------------------------------------------------------------------------------------------------------------
def test_op_trace_counts(moai, env_small2):
    e, L = env_small2, 3
    c = case(e, L)
    x = e.up(c.ct3[:, :2].copy())
    out = moai.DeviceBuffer(int(np.prod(c.shape)))
    with traced(moai) as trace:
        c.run()
        counts1 = trace()
    with traced(moai) as trace:
        e.ctx.multiply_relin_rescale_hybrid(x, x, c.dkey, out, L, e.alpha, c.B)
    counts2 = trace()
    assert counts1.get(("relinearize_rescale_hybrid", L)) == c.B
    assert counts2.get(("multiply_relin_rescale_hybrid", L)) == c.B
    for counts in (counts1, counts2):
        for name in ("relinearize_hybrid", "rescale", "ct_multiply", "ct_square", "switch_key_hybrid"):
            assert not any(op == name for op, _ in counts), (name, counts)
    assert ("relinearize_rescale_hybrid", L) not in counts2
