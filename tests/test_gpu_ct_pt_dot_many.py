"""moai_ct_pt_dot_many (csrc/ctpt_many.hip.h): every output word against sum_t x[xi[g][t]] p[pi[g][t]] mod q in Python integers, at
the seams of the kernel -- 12 outputs per group and 8 per group of the four-polynomial form, 4 / 3 / 1 polynomials per thread, a
fold of the 128-bit sums every 32 columns, 64 columns per group, 256 coefficients per workgroup -- on the largest sums it accepts,
and against the moai_ct_pt_dot calls it replaces.  Index lists are drawn with repeats from a pool a little larger than the longest
list, so they are unsorted, differ in length and do not nest; term 1 of every list repeats the operand of term 0."""
import numpy as np
import pytest

import hybrid_kit as HK
import mode_limits as ML
from test_gpu_matmul_mfma import NEG128, all127

MIXED = ("fpr_hi", "int_lo", "g61")  # below 2^51, between 2^51 and 2^54, 61 bits
_ctxs = {}


@pytest.fixture(scope="module", autouse=True)
def release_device_contexts():
    yield
    for ctx in _ctxs.values():
        ctx.close()
    _ctxs.clear()


def setup(moai, logn, names, n_out, terms, n_poly, pool=None, fill=None, seed=1):
    """(ctx, primes, x [pool][n_poly][L][N], p [pool][L][N], x lists, p lists); terms is cycled over the outputs"""
    chain = ML.chain(logn)
    primes = [chain[name] for name in names]
    ctx = HK.cached(_ctxs, (logn, tuple(primes)), lambda: moai.Context(logn, primes))
    rng = np.random.default_rng(seed)
    pool = pool or max(terms) + 3
    draw = lambda shape: np.stack([np.full(shape, fill(q), dtype=np.uint64) if fill else rng.integers(0, q, shape, dtype=np.uint64)
                                   for q in primes], axis=-2)
    x, p = draw((pool, n_poly, 1 << logn)), draw((pool, 1 << logn))
    xi = [rng.integers(0, pool, terms[g % len(terms)]).tolist() for g in range(n_out)]
    for lst in xi:
        lst[1:2] = lst[:1] * len(lst[1:2])
    pi = [rng.integers(0, pool, len(lst)).tolist() for lst in xi]
    return ctx, primes, x, p, xi, pi


def exact(x, p, xi, pi, primes):
    xo, po = x.astype(object), p.astype(object)
    want = np.empty((len(xi),) + x.shape[1:], dtype=np.uint64)
    for g, (lx, lp) in enumerate(zip(xi, pi)):
        total = sum(xo[a] * po[b][None] for a, b in zip(lx, lp))
        for r, q in enumerate(primes):
            want[g, :, r] = (total[:, r] % q).astype(np.uint64)
    return want


def run(moai, ctx, x, p, xi, pi, gap=5):
    """the outputs, `gap` sentinel words between the blocks untouched"""
    block = int(np.prod(x.shape[1:]))
    host = np.full((len(xi), block + gap), 0xDEADBEEF, dtype=np.uint64)
    dout = moai.DeviceBuffer.from_numpy(host)
    ctx.ct_pt_dot_many(moai.DeviceBuffer.from_numpy(x), moai.DeviceBuffer.from_numpy(p), dout, block + gap, xi, pi, x.shape[1], x.shape[2])
    got = dout.to_numpy(host.shape)
    assert (got[:, block:] == 0xDEADBEEF).all()
    return got[:, :block].reshape((len(xi),) + x.shape[1:])


CASES = (
    # n_out: 8 | 9 between the two kernels, 12 | 13 one group and two, 24 | 25 two groups and three; n_poly 5 = 4 + 1 and 3 + 2
    [(4, MIXED, n_out, (7, 3, 9), 5) for n_out in (1, 2, 3, 8, 9, 11, 12, 13, 24, 25)]
    # terms: the fold after column 32 and the longest list; three outputs of 64 random terms need more than 64 columns
    + [(4, MIXED, n_out, (terms,), 3) for n_out in (3, 9) for terms in (1, 7, 8, 9, 32, 33, 64)]
    # n_poly around the 4, 3 and 1 polynomials of a thread
    + [(4, MIXED, n_out, (5, 2), n_poly) for n_out in (2, 9) for n_poly in (1, 2, 3, 4, 5, 7)]
    # N: a workgroup with idle threads, one full and two workgroups per row; L = 1; the limit prime of every arithmetic mode
    + [(logn, MIXED, 9, (7, 4), 5) for logn in (3, 6, 8, 9)]
    + [(4, ("g61",), 9, (7, 4), 2), (4, ML.NAMES, 13, (9, 33), 4)]
)


@pytest.mark.gpu
@pytest.mark.parametrize("logn,names,n_out,terms,n_poly", CASES)
def test_matches_exact_integers(moai, logn, names, n_out, terms, n_poly):
    ctx, primes, x, p, xi, pi = setup(moai, logn, names, n_out, terms, n_poly, seed=1000 * n_out + 10 * max(terms) + n_poly)
    bad = np.argwhere(run(moai, ctx, x, p, xi, pi) != exact(x, p, xi, pi, primes))
    assert not len(bad), ("first of %d at [output, polynomial, prime, coeff]" % len(bad), bad[0].tolist())


@pytest.mark.gpu
@pytest.mark.parametrize("what,fill", [("q - 1", lambda q: q - 1), ("zero", lambda q: 0), ("digits -128", lambda q: NEG128 if NEG128 < q else NEG128 & 0xFFFFFFFFFFFF), ("digits +127", all127)])
def test_directed_values_at_64_terms(moai, what, fill):
    """every operand and weight the same value, 64 terms in each of 13 outputs: q - 1 gives the largest sums"""
    ctx, primes, x, p, xi, pi = setup(moai, 4, MIXED, 13, (64,), 4, fill=fill)
    assert (run(moai, ctx, x, p, xi, pi) == exact(x, p, xi, pi, primes)).all()


@pytest.mark.gpu
@pytest.mark.parametrize("logn,n_out,n_poly", [(4, 13, 5), (3, 3, 2)])
def test_equals_the_ct_pt_dot_calls(moai, logn, n_out, n_poly):
    ctx, primes, x, p, xi, pi = setup(moai, logn, MIXED, n_out, (9, 40, 4), n_poly)
    got = run(moai, ctx, x, p, xi, pi)
    dx, dp, one = moai.DeviceBuffer.from_numpy(x), moai.DeviceBuffer.from_numpy(p), moai.DeviceBuffer(got[0].size)
    for g in range(n_out):
        ctx.ct_pt_dot(dx, dp, one, xi[g], pi[g], n_poly, len(primes))
        assert (one.to_numpy(got[g].shape) == got[g]).all(), g


@pytest.mark.gpu
def test_refusals_leave_the_output_untouched(moai):
    ctx, primes, x, p, xi, pi = setup(moai, 4, MIXED, 3, (5,), 2)
    block, L = x[0].size, len(primes)
    dx, dp = moai.DeviceBuffer.from_numpy(x), moai.DeviceBuffer.from_numpy(p)
    dout = moai.DeviceBuffer.from_numpy(np.full(3 * block, 0xDEADBEEF, dtype=np.uint64))
    inside = dx.ptr + 8 * block * (max(max(l) for l in xi) - 1)  # the three outputs would end in the last operand that is read
    for args in ((None, dp, dout, block, xi, pi), (dx, None, dout, block, xi, pi), (dx, dp, None, block, xi, pi),
                 (dx, dp, dout, block, [[0] * 65] + xi[1:], [[0] * 65] + pi[1:]), (dx, dp, dout, block, [[]] + xi[1:], [[]] + pi[1:]),
                 (dx, dp, dout, block - 1, xi, pi), (dx, dp, dout, block, [xi[0], [1 << 16]], [pi[0], [0]]),
                 (dx, dp, inside, block, xi, pi), (dx, dp, dp, block, xi, pi)):
        with pytest.raises(moai.hip.MoaiError) as err:
            ctx.ct_pt_dot_many(*args, 2, L)
        assert err.value.code == moai.hip.MOAI_EINVAL, args[3:]
    assert (dout.to_numpy((3 * block,)) == 0xDEADBEEF).all()
    assert (dx.to_numpy(x.shape) == x).all() and (dp.to_numpy(p.shape) == p).all()


def test_declared_exported_and_bound(moai):
    assert "int moai_ct_pt_dot_many(moai_ctx *ctx, const uint64_t *x, const uint64_t *p, uint64_t *out, size_t out_stride," in HK.header()
    assert "Bootstrapper.cpp:2024-2062" in HK.header_comment("moai_ct_pt_dot_many")
    HK.exported(moai, ["moai_ct_pt_dot_many"], ["ct_pt_dot_many"])
