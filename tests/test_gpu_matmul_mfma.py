"""moai_ct_pt_matmul on the int8 matrix cores (MOAI_MATMUL_MFMA=1, csrc/matmul_mfma.hip.h): every output word against
sum(int(x) * int(w)) % q in Python integers, at the seams of its tiles (8 rows per K-step, 16 columns per tile, 32 per wave, 16
coefficients per wave, 64 per workgroup), on operands at the edges of the byte-limb split, across the K-chunk seam, and on both
sides of the prime size where seven digits stop being enough.

The last K-chunk case ran at 8201 rows x 17 columns x 16 coefficients, 2.2 million products."""
import numpy as np
import pytest

import hybrid_kit as HK
import mode_limits as ML

KNOB = "MOAI_MATMUL_MFMA"
CHUNK = 8192  # MM_KC of csrc/matmul_mfma.hip.h: rows per K-chunk
NEG128 = 0x007F7F7F7F7F7F80  # digits (1, -128 x 7)
_ctxs = {}


@pytest.fixture(scope="module", autouse=True)
def release_device_contexts():
    yield
    for ctx in _ctxs.values():
        ctx.close()
    _ctxs.clear()


def context(moai, logn, primes):
    return HK.cached(_ctxs, (logn, tuple(primes)), lambda: moai.Context(logn, list(primes)))


def classes(logn):
    """the limit primes of every arithmetic mode, a 46-bit prime, and the pair on either side of 2^54 (seven / eight digits)"""
    c = ML.chain(logn)
    c.update(p46=ML.prime_at_most(logn, (1 << 46) - 1), d7=ML.prime_at_most(logn, 1 << 54), d8=ML.prime_at_least(logn, (1 << 54) + 1))
    return c


def all127(q):
    v = 0x7F7F7F7F7F7F7F7F
    while v >= q:
        v >>= 8
    return v


def directed(q, rows, cols, n):
    """every pair of the directed values meets in a product: row j holds value (j + n) of x at coefficient n and value (j + c) of w
    in column c, and there are no more values than coefficients"""
    vals = [0, 1, q - 1, q // 2, q // 2 + 1, all127(q), 0x7F, 0x80, 0x807F, 0x7F80, 0x8080808080, 0x7F7F7F7F80] + [NEG128] * (NEG128 < q)
    assert len(vals) <= min(n, cols) and all(v < q for v in vals)
    j = np.arange(rows)[:, None]
    pick = np.array(vals, dtype=np.uint64)
    return pick[(j + np.arange(n)) % len(vals)][:, None, None, :], pick[(j + np.arange(cols)) % len(vals)][None]


def exact(x, w, primes):
    """[cols][size][L][N] in Python integers"""
    xo, wo = x.astype(object), w.astype(object)
    rows, size, L, n = x.shape
    want = np.empty((w.shape[2], size, L, n), dtype=np.uint64)
    for r, q in enumerate(primes):
        for s in range(size):
            want[:, s, r] = (np.dot(wo[r].T, xo[:, s, r]) % q).astype(np.uint64)
    return want


def run(moai, ctx, x, w, knob):
    rows, size, L, n = x.shape
    cols = w.shape[2]
    dout = moai.DeviceBuffer(cols * size * L * n)
    with HK.tuned(moai, **{KNOB: knob}):
        path = ctx.ct_pt_matmul_path(rows, cols, size, L)
        ctx.ct_pt_matmul(moai.DeviceBuffer.from_numpy(x), moai.DeviceBuffer.from_numpy(w), dout, rows, cols, size, L)
        return path, dout.to_numpy((cols, size, L, n))


def random_operands(primes, rows, cols, size, n, seed):
    rng = np.random.default_rng(seed)
    x = np.stack([rng.integers(0, q, (rows, size, n), dtype=np.uint64) for q in primes], axis=2)
    w = np.stack([rng.integers(0, q, (rows, cols), dtype=np.uint64) for q in primes])
    return x, w


# 33 = one column past the 16 * MM_CT = 32 of a wave; N = 4096 is 64 workgroups per row, kept to two million products
SEAMS = [("seam", logn, ("p46", "fpr_hi", "g61"), rows, cols, size)
         for logn in (4, 5, 12) for rows in (1, 7, 8, 9, 70) for cols in (1, 16, 17, 33) for size in (1, 2)
         if rows * cols * size * 3 << logn <= 2_000_000]
DIRECTED = [("directed", 4, (name,), 9, 17, 1) for name in classes(4)]


@pytest.mark.gpu
@pytest.mark.parametrize("kind,logn,names,rows,cols,size", SEAMS + DIRECTED)
def test_matches_exact_integers(moai, kind, logn, names, rows, cols, size):
    primes = [classes(logn)[name] for name in names]
    n = 1 << logn
    if kind == "directed":
        x, w = directed(primes[0], rows, cols, n)
        x, w = np.ascontiguousarray(x), np.ascontiguousarray(w)
    else:
        x, w = random_operands(primes, rows, cols, size, n, 54000 + rows * 100 + cols)
    path, got = run(moai, context(moai, logn, primes), x, w, 1)
    assert path == moai.hip.MATMUL_PATH_MFMA
    bad = np.argwhere(got != exact(x, w, primes))
    assert not len(bad), ("first of %d at [col, poly, prime, coeff]" % len(bad), bad[0].tolist())


@pytest.mark.gpu
@pytest.mark.parametrize("names,old", [(("p46", "fpr_hi"), "MATMUL_PATH_FP64"), (("p46", "g61"), "MATMUL_PATH_INT")])
def test_path_and_isolation(moai, names, old):
    """knob 0: the path of before and the same words as knob 1; knob 1: the matrix cores from N = 16, the old paths below"""
    for logn, new in ((4, "MATMUL_PATH_MFMA"), (3, old)):
        primes = [classes(logn)[name] for name in names]
        ctx = context(moai, logn, primes)
        x, w = random_operands(primes, 9, 17, 2, 1 << logn, 54001)
        path0, got0 = run(moai, ctx, x, w, 0)
        path1, got1 = run(moai, ctx, x, w, 1)
        assert (path0, path1) == (getattr(moai.hip, old), getattr(moai.hip, new))
        assert (got0 == got1).all() and (got0 == exact(x, w, primes)).all()
        with HK.tuned(moai, **{KNOB: 1, "MOAI_MATMUL_FP": 0}):
            assert ctx.ct_pt_matmul_path(9, 17, 2, len(primes)) == getattr(moai.hip, new if logn == 4 else "MATMUL_PATH_INT")


def digits(v):
    c = 0x8080808080808080
    return [b - 256 * (b > 127) for b in ((v + c) ^ c).to_bytes(8, "little")]


@pytest.mark.gpu
@pytest.mark.parametrize("cols", [1, 17])
@pytest.mark.parametrize("pattern", ["-128", "+127"])
def test_k_chunk_seam_and_int32_headroom(moai, pattern, cols):
    """one full K-chunk and nine rows, every operand the pattern; the chunk's largest diagonal sum fits int32 and would not with
    16384 rows more"""
    q = classes(4)["g61"]
    v = NEG128 if pattern == "-128" else all127(q)
    d = digits(v)
    assert sum(a << 8 * i for i, a in enumerate(d)) == v and (min(d) == -128 if pattern == "-128" else max(d) == 127)
    worst = max(abs(sum(d[a] * d[k - a] for a in range(8) if 0 <= k - a < 8)) for k in range(15))
    assert CHUNK * worst <= (1 << 31) - 1 < (CHUNK + 16384) * worst
    rows = CHUNK + 9
    x = np.full((rows, 1, 1, 16), v, dtype=np.uint64)
    w = np.full((1, rows, cols), v, dtype=np.uint64)
    path, got = run(moai, context(moai, 4, [q]), x, w, 1)
    assert path == moai.hip.MATMUL_PATH_MFMA and (got == exact(x, w, [q])).all()


def test_path_query_is_declared_exported_and_bound(moai):
    assert "int moai_ct_pt_matmul_path(moai_ctx *ctx" in HK.header()
    HK.exported(moai, ["moai_ct_pt_matmul_path"], ["ct_pt_matmul_path"])
    assert (moai.hip.MATMUL_PATH_INT, moai.hip.MATMUL_PATH_FP64, moai.hip.MATMUL_PATH_MFMA) == (0, 1, 2)
