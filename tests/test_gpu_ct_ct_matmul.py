"""moai_ct_ct_matmul (csrc/ctct_mfma.hip.h): every output word against c0 = sum a0 b0, c1 = sum (a0 b1 + a1 b0), c2 = sum a1 b1 mod q
in Python integers, at the seams of its tiles (8 ciphertexts of a per M tile, 8 of b per N tile and two N tiles per wave, 8 terms per
K-step, 16 coefficients per workgroup), on operands at the edges of the byte-limb split in both halves of the middle term, at the
largest sum the call accepts, and against the moai_ct_dot calls it replaces.

int32 headroom: the largest diagonal of a residue below 2^61 is 7 * 2^14 (digits (1, -128 x 7)), so 2 * k * worst reaches 2^31 at
k = 9363; the test pins 2 * 4096 * worst = 939 524 096 <= 2^31 - 1 < 2 * (4096 + 8192) * worst = 2 818 572 288.  (With 4096 more
terms the sum is 1 879 048 192 and still fits: no canonical residue makes that side of the statement true, the kernel's limit of
4096 comes from the bound 8 * 2^14 per term.)"""
import numpy as np
import pytest

import hybrid_kit as HK
from test_gpu_matmul_mfma import NEG128, all127, classes, digits

_ctxs = {}


def values(q):
    """the value list of test_gpu_matmul_mfma.directed"""
    return [0, 1, q - 1, q // 2, q // 2 + 1, all127(q), 0x7F, 0x80, 0x807F, 0x7F80, 0x8080808080, 0x7F7F7F7F80] + [NEG128] * (NEG128 < q)


@pytest.fixture(scope="module", autouse=True)
def release_device_contexts():
    yield
    for ctx in _ctxs.values():
        ctx.close()
    _ctxs.clear()


def context(moai, logn, primes):
    return HK.cached(_ctxs, (logn, tuple(primes)), lambda: moai.Context(logn, list(primes)))


def exact(a, b, primes):
    """[nb][m][3][L][N] in Python integers from a [m][k][2][L][N] and b [nb][k][2][L][N]"""
    ao, bo = a.astype(object)[None], b.astype(object)[:, None]
    want = np.empty((b.shape[0], a.shape[0], 3) + a.shape[3:], dtype=np.uint64)
    for r, q in enumerate(primes):
        a0, a1, b0, b1 = ao[:, :, :, 0, r], ao[:, :, :, 1, r], bo[:, :, :, 0, r], bo[:, :, :, 1, r]
        for comp, terms in enumerate((a0 * b0, a0 * b1 + a1 * b0, a1 * b1)):
            want[:, :, comp, r] = (terms.sum(axis=2) % q).astype(np.uint64)
    return want


def run(moai, ctx, a, b):
    (m, k, _, L, n), nb = a.shape, b.shape[0]
    dout = moai.DeviceBuffer(nb * m * 3 * L * n)
    ctx.ct_ct_matmul(moai.DeviceBuffer.from_numpy(a), moai.DeviceBuffer.from_numpy(b), dout, m, nb, k, L)
    return dout.to_numpy((nb, m, 3, L, n))


def random_operands(primes, m, nb, k, n, seed):
    rng = np.random.default_rng(seed)
    return tuple(np.stack([rng.integers(0, q, (cts, k, 2, n), dtype=np.uint64) for q in primes], axis=3) for cts in (m, nb))


def directed(q, m, nb, k, n):
    """word n of polynomial p of term t holds value n + t + p - i in a[i] and value n + t + p + j in b[j]: over n every value
    sits in every a word position, and i + j + p' - p takes every residue mod len(vals) (i + j runs to 16 >= 13) for (p, p') =
    (0, 1) and (1, 0) alike, so every ordered pair of values meets in an a0 b1 product and in an a1 b0 product"""
    pick = np.array(values(q), dtype=np.uint64)
    assert len(pick) <= min(n, m + nb - 1)
    t, p, w = np.arange(k)[None, :, None, None], np.arange(2)[None, None, :, None], np.arange(n)[None, None, None, :]
    a = pick[(w + t + p - np.arange(m)[:, None, None, None]) % len(pick)]
    b = pick[(w + t + p + np.arange(nb)[:, None, None, None]) % len(pick)]
    return np.ascontiguousarray(a[:, :, :, None]), np.ascontiguousarray(b[:, :, :, None])


# nb = 17 is one ciphertext past the two N tiles of a wave; k = 17 at the full tile is three stages in LDS
SEAMS = [("seam", logn, ("p46", "fpr_hi", "g61"), m, nb, k)
         for logn in (4, 5, 7) for m in (1, 8, 9) for nb in (1, 8, 9, 17) for k in (1, 7, 8, 9, 17)
         if m * nb * k * 4 * 3 << logn <= 2_000_000]
DIRECTED = [("directed", 4, (name,), 9, 9, 9) for name in classes(4)]


@pytest.mark.gpu
@pytest.mark.parametrize("kind,logn,names,m,nb,k", SEAMS + DIRECTED)
def test_matches_exact_integers(moai, kind, logn, names, m, nb, k):
    primes = [classes(logn)[name] for name in names]
    if kind == "directed":
        a, b = directed(primes[0], m, nb, k, 1 << logn)
    else:
        a, b = random_operands(primes, m, nb, k, 1 << logn, 55000 + 1000 * m + 50 * nb + k)
    bad = np.argwhere(run(moai, context(moai, logn, primes), a, b) != exact(a, b, primes))
    assert not len(bad), ("first of %d at [j, i, component, prime, coeff]" % len(bad), bad[0].tolist())


@pytest.mark.gpu
@pytest.mark.parametrize("pattern", ["-128", "+127"])
def test_int32_headroom_of_the_summed_middle_term(moai, pattern):
    """k = 4096, every operand word the pattern: the two halves of c1 are added as int32 diagonal sums; one term more is refused"""
    q = classes(4)["g61"]
    v = NEG128 if pattern == "-128" else all127(q)
    d = digits(v)
    assert sum(x << 8 * i for i, x in enumerate(d)) == v and (min(d) == -128 if pattern == "-128" else max(d) == 127)
    worst = max(abs(sum(d[x] * d[s - x] for x in range(8) if 0 <= s - x < 8)) for s in range(15))
    k = 4096
    assert 2 * k * worst <= (1 << 31) - 1 < 2 * (k + 8192) * worst
    ctx = context(moai, 4, [q])
    a = np.full((1, k, 2, 1, 16), v, dtype=np.uint64)
    assert (run(moai, ctx, a, a.copy()) == exact(a, a, [q])).all()
    a = np.zeros((1, k + 1, 2, 1, 16), dtype=np.uint64)
    with pytest.raises(moai.hip.MoaiError) as err:
        run(moai, ctx, a, a.copy())
    assert err.value.code == moai.hip.MOAI_EINVAL


@pytest.mark.gpu
@pytest.mark.parametrize("logn", [4, 3])
def test_equals_the_ct_dot_calls_and_ignores_zero_padding(moai, logn):
    """word for word the m * nb moai_ct_dot calls (logn = 3: the small-ring path); three zero ciphertexts appended change nothing"""
    primes = [classes(logn)[name] for name in ("p46", "fpr_hi", "g61")]
    ctx, (m, nb, k, L, n) = context(moai, logn, primes), (3, 2, 5, 3, 1 << logn)
    a, b = random_operands(primes, m, nb, k, n, 55001)
    got = run(moai, ctx, a, b)
    dout = moai.DeviceBuffer(3 * L * n)
    for j in range(nb):
        for i in range(m):
            ctx.ct_dot(moai.DeviceBuffer.from_numpy(a[i]), moai.DeviceBuffer.from_numpy(b[j]), dout, k, L)
            assert (got[j, i] == dout.to_numpy((3, L, n))).all(), (j, i)
    assert (got == exact(a, b, primes)).all()
    pad = lambda x: np.concatenate([x, np.zeros((x.shape[0], 3) + x.shape[2:], dtype=np.uint64)], axis=1)
    assert (run(moai, ctx, pad(a), pad(b)) == got).all()


def test_declared_exported_and_bound(moai):
    assert "int moai_ct_ct_matmul(moai_ctx *ctx, const uint64_t *a, const uint64_t *b, uint64_t *out, size_t m, size_t nb" in HK.header()
    HK.exported(moai, ["moai_ct_ct_matmul"], ["ct_ct_matmul"])
