"""The 60-bit NTT rows that keep values below 16q and guard only where the bound needs it (M_LAZY16, modarith.hip.h),
against the CPU oracle, bit for bit, for every tiled size and with the knob MOAI_NTT_LAZY16 on and off (off: the kernels
with a guard in every stage).  Rows: the primes at both ends of the range the mode serves -- the largest below 2^60, where
16q comes closest to 2^64, and the smallest above 2^59 --, a 52-bit and a 58-bit prime (other integer kernels) and a 61-bit
prime (the exact butterflies) as controls that the knob must leave alone.  Inputs: all q-1, all 0, alternating 0 / q-1,
random."""
import numpy as np
import pytest

import oracle as O

pytestmark = pytest.mark.gpu

NPOLY = 2


def is_prime(n):
    """Miller-Rabin with the bases that decide every n < 2^64"""
    if n < 2:
        return False
    small = (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37)
    for p in small:
        if n % p == 0:
            return n == p
    d, s = n - 1, 0
    while d % 2 == 0:
        d //= 2
        s += 1
    for a in small:
        x = pow(a, d, n)
        if x in (1, n - 1):
            continue
        for _ in range(s - 1):
            x = x * x % n
            if x == n - 1:
                break
        else:
            return False
    return True


def ntt_prime(logn, start, step_sign):
    """the first prime = 1 (mod 2N) at or beyond `start`, walking down (-1) or up (+1)"""
    m = 2 << logn
    q = start - (start - 1) % m if step_sign < 0 else start + (1 - start) % m
    while not is_prime(q):
        q += step_sign * m
    return q


def primes_for(logn):
    return [
        ntt_prime(logn, (1 << 60) - 1, -1),  # largest below 2^60
        ntt_prime(logn, (1 << 59) + 1, +1),  # smallest above 2^59
        ntt_prime(logn, (1 << 52) - 1, -1),  # 52 bits
        ntt_prime(logn, (1 << 58) - 1, -1),  # 58 bits
        ntt_prime(logn, (1 << 61) - 1, -1),  # 61 bits: never on the lazy kernels
    ]


PATTERNS = ("all q-1", "all 0", "alternating", "random")
_cases = {}


def case(logn):
    """inputs [pattern][NPOLY][L][N] and the oracle's transforms of them, computed once per size and never written to"""
    if logn in _cases:
        return _cases[logn]
    n = 1 << logn
    primes = primes_for(logn)
    L = len(primes)
    assert primes[0] < (1 << 60) and primes[0] > (1 << 60) - (1 << 30) and (1 << 59) < primes[1] < (1 << 59) + (1 << 30)
    assert all((q - 1) % (2 * n) == 0 for q in primes) and primes[4] > (1 << 60)
    rng = np.random.default_rng(1600 + logn)
    qcol = np.array(primes, dtype=np.uint64)[None, :, None]
    x = np.zeros((len(PATTERNS), NPOLY, L, n), dtype=np.uint64)
    x[0] = qcol - np.uint64(1)
    x[2, 0, :, 1::2] = (qcol - np.uint64(1))[0]
    x[2, 1, :, 0::2] = (qcol - np.uint64(1))[0]
    x[3] = O.uniform_rns(rng, primes, (NPOLY,), n)
    octx = O.Context(logn, primes)
    flat = x.reshape(-1, L, n)
    pidx = [L - 1 - i for i in range(L)]
    y = np.stack([rng.integers(0, primes[p], size=n, dtype=np.uint64) for p in pidx])[None].repeat(NPOLY, axis=0)
    y[1] = np.stack([np.full(n, primes[p] - 1, dtype=np.uint64) for p in pidx])
    c = dict(primes=primes, x=x, fwd=octx.ntt(flat, L).reshape(x.shape), inv=octx.ntt(flat, L, inverse=True).reshape(x.shape),
             pidx=pidx, y=y, yfwd=octx.ntt(y, L, prime_index=pidx), yinv=octx.ntt(y, L, prime_index=pidx, inverse=True))
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    _cases[logn] = c
    return c


@pytest.mark.parametrize("lazy16", [1, 0])
@pytest.mark.parametrize("logn", [12, 13, 14, 15, 16])
def test_lazy16_matches_oracle(moai, logn, lazy16):
    c = case(logn)
    primes, L = c["primes"], len(c["primes"])
    ctx = moai.Context(logn, primes)
    moai.hip.set_tuning("MOAI_NTT_LAZY16", lazy16)
    try:
        for k, name in enumerate(PATTERNS):
            x = c["x"][k]
            d = moai.DeviceBuffer.from_numpy(x)
            ctx.ntt_forward(d, NPOLY, L)
            assert (d.to_numpy(x.shape) == c["fwd"][k]).all(), "forward, " + name
            ctx.ntt_inverse(d, NPOLY, L)
            assert (d.to_numpy(x.shape) == x).all(), "round trip, " + name
            ctx.ntt_inverse(d, NPOLY, L)  # canonical data that is no transform of anything in particular
            assert (d.to_numpy(x.shape) == c["inv"][k]).all(), "inverse, " + name
        y, pidx = c["y"], c["pidx"]
        d = moai.DeviceBuffer.from_numpy(y)
        ctx.ntt_forward(d, NPOLY, L, prime_index=pidx)
        assert (d.to_numpy(y.shape) == c["yfwd"]).all(), "forward, permuted prime_index"
        ctx.ntt_inverse(d, NPOLY, L, prime_index=pidx)
        assert (d.to_numpy(y.shape) == y).all(), "round trip, permuted prime_index"
        ctx.ntt_inverse(d, NPOLY, L, prime_index=pidx)
        assert (d.to_numpy(y.shape) == c["yinv"]).all(), "inverse, permuted prime_index"
    finally:
        moai.hip.reset_tuning()
