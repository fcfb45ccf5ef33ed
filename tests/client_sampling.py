"""The client's randomness and encryption as include/moai_hip.h ("client randomness and encryption") specifies them, in numpy:
a ChaCha20 block function (RFC 8439, 64-bit counter in state words 12-13, 64-bit nonce in 14-15), the samplers' mappings
from stream words to coefficients, and the compositions (symmetric encryption, public-key encryption with the division by
the dropped prime, switching-key digits) built from the KAT-pinned oracle NTT and rescale (tests/oracle.py).
tests/test_oracle_client.py pins this module; tests/test_gpu_client.py compares the device with it.  CPU only."""
import numpy as np

SIGMA = (0x61707865, 0x3320646E, 0x79622D32, 0x6B206574)  # "expand 32-byte k"
UNIFORM, TERNARY, NOISE0, NOISE1 = 1, 2, 3, 4  # nonce purposes
M32 = np.uint64(0xFFFFFFFF)


def nonce(purpose, seq):
    assert 0 <= seq < 1 << 56
    return (purpose << 56) | seq


def _rotl(v, c):
    return ((v << np.uint32(c)) | (v >> np.uint32(32 - c))).astype(np.uint32)


def chacha_blocks(key, nonce_, counters):
    """uint32 [len(counters)][16]: the ChaCha20 blocks of (key, nonce) at the given 64-bit counters."""
    key = bytes(key)
    assert len(key) == 32
    kw = np.frombuffer(key, dtype="<u4").astype(np.uint32)
    ctr = np.asarray(counters, dtype=np.uint64)
    nb = ctr.size
    s = np.empty((16, nb), dtype=np.uint32)
    for i in range(4):
        s[i] = SIGMA[i]
    for i in range(8):
        s[4 + i] = kw[i]
    s[12] = (ctr & M32).astype(np.uint32)
    s[13] = (ctr >> np.uint64(32)).astype(np.uint32)
    s[14] = nonce_ & 0xFFFFFFFF
    s[15] = (nonce_ >> 32) & 0xFFFFFFFF
    x = s.copy()

    def qr(a, b, c, d):
        x[a] += x[b]
        x[d] = _rotl(x[d] ^ x[a], 16)
        x[c] += x[d]
        x[b] = _rotl(x[b] ^ x[c], 12)
        x[a] += x[b]
        x[d] = _rotl(x[d] ^ x[a], 8)
        x[c] += x[d]
        x[b] = _rotl(x[b] ^ x[c], 7)

    with np.errstate(over="ignore"):
        for _ in range(10):
            qr(0, 4, 8, 12)
            qr(1, 5, 9, 13)
            qr(2, 6, 10, 14)
            qr(3, 7, 11, 15)
            qr(0, 5, 10, 15)
            qr(1, 6, 11, 12)
            qr(2, 7, 8, 13)
            qr(3, 4, 9, 14)
        x += s
    return x.T.copy()


def words(key, nonce_, first_block, n_blocks):
    """the 64-bit words W[8 first_block .. 8 (first_block + n_blocks)) of the stream (key, nonce)"""
    b = chacha_blocks(key, nonce_, np.arange(first_block, first_block + n_blocks, dtype=np.uint64)).astype(np.uint64)
    w = b[:, 0::2] | (b[:, 1::2] << np.uint64(32))
    return w.reshape(-1)


# ---- the mappings -------------------------------------------------------------------------------------------------------
def map_uniform(lo, hi, q):
    """(hi * 2^64 + lo) mod q, exactly"""
    lo = np.asarray(lo, dtype=np.uint64).astype(object)
    hi = np.asarray(hi, dtype=np.uint64).astype(object)
    return (((hi << 64) | lo) % int(q)).astype(np.uint64)


def map_ternary(w):
    """((3 w) >> 64) - 1"""
    w = np.asarray(w, dtype=np.uint64)
    # 3 w = 2 w + w; the high word of a 66-bit sum from the 32-bit halves
    hi, lo = w >> np.uint64(32), w & M32
    t_lo = 3 * lo
    t_hi = 3 * hi + (t_lo >> np.uint64(32))
    return (t_hi >> np.uint64(32)).astype(np.int64) - 1


def _popcount(v):
    v = np.asarray(v, dtype=np.uint64)
    c = np.zeros(v.shape, dtype=np.int64)
    for b in range(64):
        c += ((v >> np.uint64(b)) & np.uint64(1)).astype(np.int64)
    return c


def map_cbd(w):
    """popcount(x0) + popcount(x1) + popcount(x2 & 0x1f) - popcount(x3) - popcount(x4) - popcount(x5 & 0x1f)"""
    w = np.asarray(w, dtype=np.uint64)
    return _popcount(w & np.uint64(0x1FFFFF)) - _popcount((w >> np.uint64(24)) & np.uint64(0x1FFFFF))


# ---- samplers -----------------------------------------------------------------------------------------------------------
def uniform(key, nonce_, primes, n, rows=None):
    """[len(primes)][n]: row r under primes[r] (rows: compute only these row indices, the others are zero)"""
    out = np.zeros((len(primes), n), dtype=np.uint64)
    for r in range(len(primes)) if rows is None else rows:
        w = words(key, nonce_, r * n // 4, n // 4)  # row r takes words 2 (r N + i), 2 (r N + i) + 1
        out[r] = map_uniform(w[0::2], w[1::2], primes[r])
    return out


def ternary(key, nonce_, n):
    return map_ternary(words(key, nonce_, 0, n // 8))


def cbd(key, nonce_, n):
    return map_cbd(words(key, nonce_, 0, n // 8))


def to_rns(v, primes):
    v = np.asarray(v, dtype=np.int64)
    out = np.empty((len(primes), v.size), dtype=np.uint64)
    for r, q in enumerate(primes):
        out[r] = np.where(v < 0, v + int(q), v).astype(np.uint64)  # q < 2^62: no overflow in int64
    return out


# ---- compositions -------------------------------------------------------------------------------------------------------
def _mulmod(a, b, q):
    return ((a.astype(object) * b.astype(object)) % int(q)).astype(np.uint64)


def _sym_one(octx, key, seq, sk_ntt, L, rows=None):
    """(c0, c1) of encrypt_zero_symmetric at the first L primes, NTT form; rows restricts the rows computed"""
    n, primes = octx.n, octx.primes[:L]
    e = octx.ntt(to_rns(cbd(key, nonce(NOISE0, seq), n), primes), L)
    a = uniform(key, nonce(UNIFORM, seq), primes, n, rows)
    if rows is None:
        # e - a (.) s: the oracle's dyadic product and difference
        return octx.sub(e, octx.multiply_plain(a, 1, L, np.ascontiguousarray(sk_ntt[:L])), 1, L), a
    c0 = np.zeros((L, n), dtype=np.uint64)
    for r in rows:
        q = primes[r]
        as_ = _mulmod(a[r], sk_ntt[r], q)
        c0[r] = ((e[r].astype(object) - as_.astype(object)) % q).astype(np.uint64)
    return c0, a


def encrypt_symmetric(octx, key, seq, sk_ntt, L, n_batch=1, plain=None):
    """[n_batch][2][L][N] (moai_encrypt_symmetric with prime_index = NULL)"""
    out = np.empty((n_batch, 2, L, octx.n), dtype=np.uint64)
    for b in range(n_batch):
        c0, c1 = _sym_one(octx, key, seq + b, sk_ntt, L)
        if plain is not None:
            for r in range(L):
                c0[r] = (c0[r].astype(object) + plain[b][r].astype(object)) % octx.primes[r]
        out[b, 0], out[b, 1] = c0, c1
    return out


def kswitch_digit(octx, key, seq, sk_ntt, new_key_ntt, J, rows=None):
    """digit J [2][k][N] of moai_kswitch_keygen(seq): Enc_s(0) with sequence seq + J, plus (p mod q_J) s'[J] in row J of c0"""
    k = octx.k
    c0, c1 = _sym_one(octx, key, seq + J, sk_ntt, k, rows)
    qJ = octx.primes[J]
    f = octx.primes[k - 1] % qJ
    c0[J] = (c0[J].astype(object) + new_key_ntt[J].astype(object) * f) % qJ
    return np.stack([c0, c1])


def encrypt_asymmetric(octx, key, seq, pk, L, n_batch=1, plain=None):
    """[n_batch][2][L][N] (moai_encrypt_asymmetric): encrypt_zero_asymmetric over M = L + 1 primes (M = L = k at the key
    level), the oracle's rescale (divide_and_round_q_last_ntt), then the plaintext added to c0"""
    n, k = octx.n, octx.k
    M = L + 1 if L < k else L
    primes = octx.primes[:M]
    out = np.empty((n_batch, 2, L, n), dtype=np.uint64)
    for b in range(n_batch):
        u = octx.ntt(to_rns(ternary(key, nonce(TERNARY, seq + b), n), primes), M)
        e = np.stack([octx.ntt(to_rns(cbd(key, nonce(purpose, seq + b), n), primes), M) for purpose in (NOISE0, NOISE1)])
        # pk_i (.) u + e_i over rows [0, M): the oracle's dyadic product and sum (multiply_plain, add)
        ct = octx.add(octx.multiply_plain(np.ascontiguousarray(pk[:, :M]), 2, M, u), e, 2, M)
        if M > L:
            ct = octx.rescale(ct, 2, M)
        if plain is not None:
            for r in range(L):
                ct[0, r] = (ct[0, r].astype(object) + plain[b][r].astype(object)) % primes[r]
        out[b] = ct
    return out
