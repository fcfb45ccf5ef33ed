"""csrc/client.hip at the limit primes of tests/mode_limits.py, bit for bit against tests/client_sampling.py: both orders of the nine
primes (a 61-bit prime and the prime just above 2^40 side by side; the prime that public-key encryption drops is the 61-bit one in
one order and the largest FP64-class one in the other) at N = 16 and N = 4096.

1. the three samplers over all nine rows and over a permuted prime_index (mod128 under every limit prime);
2. symmetric encryption (cl_sym_finish) with secret and plaintext rows all q - 1, all 0, alternating and random;
3. public-key encryption (cl_pk_finish, the rescale by the dropped prime, cl_add_c0) at the key level, one below and at one prime;
4. switching-key digits at N = 16."""
import numpy as np
import pytest

import client_limit_cases as CL
import client_sampling as CS
import mode_limits as ML
import oracle as O

pytestmark = pytest.mark.gpu

K = 9
KEY = bytes((11 * i + 5) & 0xFF for i in range(32))
ROWS5 = [7, 2, 8, 0, 4]
PATTERNS4 = (0, 1, 2, 4)  # of ML.PATTERNS: all q-1, all 0, alternating 0 / q-1, random
_ctxs = {}


@pytest.fixture(scope="module", autouse=True)
def release_device_contexts():
    yield
    for entry in _ctxs.values():
        entry[-1].close()
    _ctxs.clear()


@pytest.fixture(params=[(logn, order) for logn in (4, 12) for order in CL.ORDER_NAMES], ids=lambda p: "%d-%s" % p)
def env(request, moai):
    logn, order = request.param
    if (logn, order) not in _ctxs:
        primes = ML.ordered(logn, order)
        _ctxs[(logn, order)] = (primes, O.Context(logn, primes), moai.Context(logn, primes))
    return (logn,) + _ctxs[(logn, order)]


def up(moai, a):
    return moai.DeviceBuffer.from_numpy(np.ascontiguousarray(a))


def _secret(octx, rng, primes):
    s = rng.integers(-1, 2, size=octx.n)
    return octx.ntt(CS.to_rns(s, primes), len(primes))


def test_samplers_at_the_limit_primes(moai, env):
    logn, primes, octx, ctx = env
    n = 1 << logn
    nonce = (3 << 56) | 4321
    got = ctx.sample_uniform(KEY, nonce, 2, K).to_numpy((2, K, n))
    for p in range(2):
        assert (got[p] == CS.uniform(KEY, nonce + p, primes, n)).all()
        assert (got[p] < np.array(primes, dtype=np.uint64)[:, None]).all()
    sub = [primes[i] for i in ROWS5]
    got = ctx.sample_uniform(KEY, 91, 2, len(ROWS5), prime_index=ROWS5).to_numpy((2, len(ROWS5), n))
    for p in range(2):
        assert (got[p] == CS.uniform(KEY, 91 + p, sub, n)).all()
    for fn, ref in ((ctx.sample_ternary, CS.ternary), (ctx.sample_cbd, CS.cbd)):
        got = fn(KEY, nonce, 2, K).to_numpy((2, K, n))
        for p in range(2):
            assert (got[p] == CS.to_rns(ref(KEY, nonce + p, n), primes)).all()
        got = fn(KEY, 92, 2, len(ROWS5), prime_index=ROWS5).to_numpy((2, len(ROWS5), n))
        for p in range(2):
            assert (got[p] == CS.to_rns(ref(KEY, 92 + p, n), sub)).all()


def test_encrypt_symmetric_at_the_limit_primes(moai, env):
    """the secret's rows and the plaintexts' rows are the patterns themselves (any NTT-form row is a valid operand of the dyadic
    product): a (.) s with s = q - 1 throughout, plaintext q - 1 added to it"""
    logn, primes, octx, ctx = env
    n = 1 << logn
    rng = np.random.default_rng(6600 + logn)
    pat = ML.pattern_rows(primes, n, rng)[list(PATTERNS4)]  # [4][9][n]
    B = len(PATTERNS4)
    for L in (K, K - 1, 2):
        plain = np.ascontiguousarray(pat[:, :L])
        d_plain = up(moai, plain)
        for i, name in enumerate(PATTERNS4):
            seq = 1000 * L + 10 * i
            s_ntt = pat[i]
            got = ctx.encrypt_symmetric(KEY, seq, up(moai, s_ntt), L, B, plain=d_plain).to_numpy((B, 2, L, n))
            assert (got == CS.encrypt_symmetric(octx, KEY, seq, s_ntt, L, B, plain)).all(), (L, ML.PATTERNS[name])
    # without a plaintext, under a real secret
    s_ntt = _secret(octx, rng, primes)
    got = ctx.encrypt_symmetric(KEY, 77, up(moai, s_ntt), K, 2).to_numpy((2, 2, K, n))
    assert (got == CS.encrypt_symmetric(octx, KEY, 77, s_ntt, K, 2)).all()


def test_encrypt_asymmetric_at_the_limit_primes(moai, env):
    logn, primes, octx, ctx = env
    n = 1 << logn
    rng = np.random.default_rng(6700 + logn)
    pat = ML.pattern_rows(primes, n, rng)[list(PATTERNS4)]
    B = len(PATTERNS4)
    # two public keys: an encryption of zero under a ternary secret, and rows of all q - 1 (pk (.) u + e with every key residue q - 1)
    d_sk = up(moai, _secret(octx, rng, primes))
    d_pk = ctx.encrypt_symmetric(KEY, 0, d_sk, K)
    pk_max = np.stack([pat[0], pat[0]])
    for name, d_key, pk in (("real", d_pk, d_pk.to_numpy((2, K, n))), ("all q-1", up(moai, pk_max), pk_max)):
        for L in (K, K - 1, 1):
            plain = np.ascontiguousarray(pat[:, :L])
            got = ctx.encrypt_asymmetric(KEY, 20 + L, d_key, L, B, plain=up(moai, plain)).to_numpy((B, 2, L, n))
            assert (got == CS.encrypt_asymmetric(octx, KEY, 20 + L, pk, L, B, plain)).all(), (name, L)
            got = ctx.encrypt_asymmetric(KEY, 40 + L, d_key, L, 1).to_numpy((1, 2, L, n))
            assert (got == CS.encrypt_asymmetric(octx, KEY, 40 + L, pk, L, 1)).all(), (name, L)


@pytest.mark.parametrize("order", CL.ORDER_NAMES)
def test_kswitch_keygen_at_the_limit_primes(moai, order):
    logn = 4
    n = 1 << logn
    primes = ML.ordered(logn, order)
    if (logn, order) not in _ctxs:
        _ctxs[(logn, order)] = (primes, O.Context(logn, primes), moai.Context(logn, primes))
    _, octx, ctx = _ctxs[(logn, order)]
    rng = np.random.default_rng(6800)
    s_ntt, s2_ntt = _secret(octx, rng, primes), _secret(octx, rng, primes)
    got = ctx.kswitch_keygen(KEY, 500, up(moai, s_ntt), up(moai, s2_ntt)).to_numpy((K - 1, 2, K, n))
    for J in range(K - 1):
        assert (got[J] == CS.kswitch_digit(octx, KEY, 500, s_ntt, s2_ntt, J)).all(), J
        # c0 + c1 s = (p mod q_J) s' in row J plus CBD noise, in Python integers
        for r in range(K):
            q = primes[r]
            m = (got[J, 0, r].astype(object) + got[J, 1, r].astype(object) * s_ntt[r].astype(object)) % q
            if r == J:
                m = (m - s2_ntt[r].astype(object) * (primes[K - 1] % q)) % q
            coeff = octx.ntt(m.astype(np.uint64)[None], 1, prime_index=[r], inverse=True)[0]
            e = [int(v) - q if int(v) > q // 2 else int(v) for v in coeff]
            assert max(abs(v) for v in e) <= 21
