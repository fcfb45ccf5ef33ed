"""The contiguous NTT passes that transform the same tile of two polynomials per workgroup and fetch its twiddles once
(ntt_fwd_contig2 / ntt_inv_contig2, MOAI_NTT_PAIR), against the CPU oracle, bit for bit, and against the single kernels
(MOAI_NTT_PAIR=0).  Rows: the primes of test_gpu_ntt_lazy16 -- the largest below 2^60, the smallest above 2^59, a 52-bit, a
58-bit and a 61-bit prime --, so one call has several arithmetic classes and launches with different row counts.  Polynomial
counts 1 (no pair at all), 2, 3 and 5 (a pair or two and the unpaired last one); inputs all q-1, all 0, alternating 0 / q-1
with the two polynomials of a pair different, and random with a seed per polynomial.  One polynomial of sentinel words behind
the last one must stay what it was."""
import numpy as np
import pytest

import oracle as O
from test_gpu_ntt_lazy16 import primes_for

pytestmark = pytest.mark.gpu

PATTERNS = ("all q-1", "all 0", "alternating", "random")
SENTINEL = np.uint64(0xA5A55A5AC3C33C3C)
_cases = {}


def freeze(c):
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


def case(logn, npoly):
    """inputs [pattern][npoly][L][N] and the oracle's transforms of them, computed once per (size, count), never written to;
    the tests of fewer polynomials take the leading ones"""
    if (logn, npoly) in _cases:
        return _cases[(logn, npoly)]
    n = 1 << logn
    primes = primes_for(logn)
    L = len(primes)
    qm1 = np.array(primes, dtype=np.uint64)[:, None] - np.uint64(1)
    x = np.zeros((len(PATTERNS), npoly, L, n), dtype=np.uint64)
    x[0] = qm1
    for p in range(npoly):
        x[2, p, :, (p + 1) % 2::2] = qm1  # polynomial 2i: odd coefficients, 2i + 1: even ones
        x[3, p] = O.uniform_rns(np.random.default_rng(7000 + 100 * logn + p), primes, (), n)
    octx = O.Context(logn, primes)
    flat = x.reshape(-1, L, n)
    c = freeze(dict(primes=primes, x=x, fwd=octx.ntt(flat, L).reshape(x.shape), inv=octx.ntt(flat, L, inverse=True).reshape(x.shape)))
    _cases[(logn, npoly)] = c
    return c


def with_guard(a):
    """the words of `a` and one polynomial of sentinel words behind them"""
    poly = a[0].size
    return np.concatenate([a.reshape(-1), np.full(poly, SENTINEL, dtype=np.uint64)])


def read(d, shape, what):
    out = d.to_numpy()
    words = int(np.prod(shape))
    assert (out[words:] == SENTINEL).all(), "words behind the last polynomial changed: " + what
    return out[:words].reshape(shape)


def transforms(moai, ctx, x, L):
    """forward, inverse of that, inverse of the input: the three outputs of one buffer with its sentinel checked after every call"""
    npoly = x.shape[0]
    d = moai.DeviceBuffer.from_numpy(with_guard(x))
    ctx.ntt_forward(d, npoly, L)
    f = read(d, x.shape, "forward")
    ctx.ntt_inverse(d, npoly, L)
    r = read(d, x.shape, "inverse")
    ctx.ntt_inverse(d, npoly, L)  # canonical data that is no transform of anything in particular
    i = read(d, x.shape, "inverse of the input")
    d.free()
    return f, r, i


SIZES = [(12, 1), (12, 2), (12, 3), (12, 5), (16, 1), (16, 2), (16, 3), (16, 5), (13, 3), (14, 3), (15, 3)]


@pytest.mark.parametrize("logn,npoly", SIZES)
def test_pair_matches_oracle_and_single(moai, logn, npoly):
    c = case(logn, 5 if logn in (12, 16) else 3)
    primes, L = c["primes"], len(c["primes"])
    ctx = moai.Context(logn, primes)
    try:
        for k, name in enumerate(PATTERNS):
            x = c["x"][k, :npoly]
            got = {}
            for pair in (1, 0):
                moai.hip.set_tuning("MOAI_NTT_PAIR", pair)
                got[pair] = transforms(moai, ctx, x, L)
                what = "%s, MOAI_NTT_PAIR=%d" % (name, pair)
                assert (got[pair][0] == c["fwd"][k, :npoly]).all(), "forward, " + what
                assert (got[pair][1] == x).all(), "round trip, " + what
                assert (got[pair][2] == c["inv"][k, :npoly]).all(), "inverse, " + what
            for a, b in zip(got[1], got[0]):
                assert (a == b).all(), "paired and single kernels differ, " + name
    finally:
        moai.hip.reset_tuning()


def test_pair_under_chunk_schedule_with_odd_chunks(moai):
    """seven polynomials in chunks of three on two side streams: two chunks of a pair and a single, one chunk of a single"""
    logn, npoly = 12, 7
    c = case(logn, npoly)
    primes, L = c["primes"], len(c["primes"])
    ctx = moai.Context(logn, primes)
    x = c["x"][3]
    try:
        got = {}
        for pair in (1, 0):
            moai.hip.set_tuning("MOAI_NTT_PAIR", pair)
            moai.hip.set_tuning("MOAI_NTT_CHUNK_MB", 0)
            moai.hip.set_tuning("MOAI_NTT_CHUNK_KB", 3 * L * (8 << logn) >> 10)
            moai.hip.set_tuning("MOAI_NTT_PIPE", 2)
            moai.hip.set_tuning("MOAI_NTT_PIPE_MIN", 1)
            assert moai.hip.ntt_pipe_plan(npoly, L, 1 << logn, 3 * L * (8 << logn), 2, 1) == 2  # three chunks, two streams
            got[pair] = transforms(moai, ctx, x, L)
            assert (got[pair][0] == c["fwd"][3]).all(), "forward, MOAI_NTT_PAIR=%d" % pair
            assert (got[pair][1] == x).all(), "round trip, MOAI_NTT_PAIR=%d" % pair
            assert (got[pair][2] == c["inv"][3]).all(), "inverse, MOAI_NTT_PAIR=%d" % pair
        for a, b in zip(got[1], got[0]):
            assert (a == b).all(), "paired and single kernels differ"
    finally:
        moai.hip.reset_tuning()


def test_pair_reads_a_source_slice(moai):
    """The key switch starts with the inverse transform of c1 of every ciphertext, read in place from the batch (NttArgs::src: a
    slice of a larger layout).  Three ciphertexts: a pair and the unpaired last one."""
    logn, B = 12, 3
    primes = primes_for(logn)
    n, k, L = 1 << logn, len(primes), len(primes) - 1
    octx = O.Context(logn, primes)
    ctx = moai.Context(logn, primes)
    rng = np.random.default_rng(7300)
    key = O.uniform_rns(rng, primes, (k - 1, 2), n)
    ct = O.uniform_rns(rng, primes[:L], (B, 2), n)
    elt = ctx.galois_elt_from_step(1)
    exp = np.stack([octx.apply_galois(ct[b], L, elt, key).reshape(2, L, n) for b in range(B)])
    dkey = moai.DeviceBuffer.from_numpy(key)
    try:
        got = {}
        for pair in (1, 0):
            moai.hip.set_tuning("MOAI_NTT_PAIR", pair)
            dct = moai.DeviceBuffer.from_numpy(with_guard(ct))
            ctx.apply_galois(dct, L, elt, dkey, B)
            got[pair] = read(dct, ct.shape, "apply_galois")
            dct.free()
            assert (got[pair] == exp).all(), "apply_galois, MOAI_NTT_PAIR=%d" % pair
        assert (got[1] == got[0]).all()
    finally:
        moai.hip.reset_tuning()
