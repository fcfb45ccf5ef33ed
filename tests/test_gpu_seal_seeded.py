"""GPU parity of the SEAL-seeded generating side over the C ABI (include/moai_hip.h, "SEAL's own format"):
moai_encrypt_symmetric_seal_seeded and moai_kswitch_keygen_seal_seeded word for word against restatements this file does not own
-- a from tests/seal_format.py's sample_poly_uniform (pinned against fixtures SEAL itself wrote), e from tests/client_sampling.py's
CBD stream, NTT and products from the oracle -- plus the rejection count, the noise's independence of the source of a, and the
argument errors."""
import json
import os

import numpy as np
import pytest

import client_sampling as CS
import oracle as O
import seal_format as SF

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "seal_format")
SEEDS = [bytes((t * 64 + i) % 256 for i in range(64)) for t in range(4)]
NOISE_KEY = bytes((11 * i + 5) & 0xFF for i in range(32))


def _json(name):
    with open(os.path.join(GOLDEN, name)) as f:
        return json.load(f)


def _marks(seed, primes, n):
    """words of the first L n of the stream that sample_poly_uniform rejects, per row (replacements not counted)"""
    L = len(primes)
    w = np.frombuffer(SF.prng_buffers(seed, 0, -(-L * n // 512)), dtype="<u8")[:L * n].reshape(L, n)
    return [int((w[j] >= np.uint64(SF.max_multiple(int(q)))).sum()) for j, q in enumerate(primes)]


def _secret(octx, rng):
    return octx.ntt(CS.to_rns(rng.integers(-1, 2, size=octx.n), octx.primes), octx.k)


def _noise_ntt(octx, seq):
    """NTT(e) of the ciphertext or digit with sequence seq, under all of octx's primes"""
    return octx.ntt(CS.to_rns(CS.cbd(NOISE_KEY, CS.nonce(CS.NOISE0, seq), octx.n), octx.primes), octx.k)


def _mul(octx, a, s):
    return octx.multiply_plain(a, 1, octx.k, np.ascontiguousarray(s))


def _expected_c0(octx, seed, seq, s_ntt, plain=None):
    """(c0, a, rejections) of one ciphertext under all of octx's primes: NTT(e) - a (.) s (+ plain)"""
    a, rejected = SF.sample_poly_uniform(seed, octx.primes, octx.n)
    c0 = octx.sub(_noise_ntt(octx, seq), _mul(octx, a, s_ntt), 1, octx.k)
    if plain is not None:
        c0 = octx.add(c0, plain, 1, octx.k)
    return c0, a, sum(rejected)


def _check_encrypt(moai, logn, primes, L, seeds, seq, prime_index=None, rng_seed=0):
    n = 1 << logn
    sel = [primes[i] for i in prime_index] if prime_index is not None else primes[:L]
    octx = O.Context(logn, sel)  # the selected rows as a chain of their own: the oracle's NTT depends on the prime alone
    ctx = moai.Context(logn, primes)
    rng = np.random.default_rng(rng_seed)
    s_ntt = _secret(octx, rng)
    plain = O.uniform_rns(rng, sel, (len(seeds),), n)
    d_sk, d_plain = moai.DeviceBuffer.from_numpy(s_ntt), moai.DeviceBuffer.from_numpy(plain)
    want = [_expected_c0(octx, seeds[b], seq + b, s_ntt, plain[b]) for b in range(len(seeds))]
    out, rejected, overflow = ctx.encrypt_symmetric_seal_seeded(NOISE_KEY, seeds, seq, d_sk, L, plain=d_plain, prime_index=prime_index)
    got = out.to_numpy((len(seeds), L, n))
    for b in range(len(seeds)):
        assert (got[b] == want[b][0]).all(), b
    total = sum(w[2] for w in want)
    print("logn %d L %d batch %d: rejected %d (restatement %d)" % (logn, L, len(seeds), rejected, total))
    assert rejected == total and overflow is False
    # without a plaintext and without the counters: the same call minus plain
    out0, none, _ = ctx.encrypt_symmetric_seal_seeded(NOISE_KEY, seeds[:1], seq, d_sk, L, prime_index=prime_index, count_rejected=False)
    assert none is None
    assert (out0.to_numpy((L, n)) == _expected_c0(octx, seeds[0], seq, s_ntt)[0]).all()
    return total


def test_set_a_preconditions():
    """what the cases below rest on: every seed has a rejected word and seed 0 a replacement that is itself rejected"""
    primes = _json("a.json")["primes"]
    counts = [SF.sample_poly_uniform(s, primes, 64)[1] for s in SEEDS]
    assert counts == [[0, 2, 2, 5], [2, 1, 3, 1], [3, 1, 2, 4], [2, 2, 1, 2]]
    assert all(sum(c) > 0 for c in counts)
    assert _marks(SEEDS[0], primes, 64)[3] == 4  # 5 draws for 4 marks


def test_encrypt_set_a(moai):
    """N = 64 (the narrow fill path), batch 4 at L = 4, then L = 2 under prime_index [1, 3]"""
    info = _json("a.json")
    primes = info["primes"]
    assert info["n"] == 64 and len(primes) == 4
    total = _check_encrypt(moai, 6, primes, 4, SEEDS, 700)
    assert total == 9 + 7 + 10 + 7  # test_set_a_preconditions' rows
    _check_encrypt(moai, 6, primes, 2, SEEDS, 900, prime_index=[1, 3], rng_seed=1)


def test_encrypt_set_b(moai):
    """N = 1024, three primes, batch 2: the wide fill path, and replacements that are themselves rejected"""
    info = _json("b.json")
    primes, n = info["primes"], info["n"]
    assert n == 1024 and len(primes) == 3
    for s in SEEDS:
        counts, marks = SF.sample_poly_uniform(s, primes, n)[1], _marks(s, primes, n)
        assert 58 <= marks[0] <= 72 and sum(counts) > sum(marks)
    _check_encrypt(moai, 10, primes, 3, SEEDS[:2], 40, rng_seed=2)


def test_encrypt_tiled_ntt_in_chunks(moai):
    """N = 4096 under 60, 40 and 60 bits, batch 3: the tiled transform, and a batch larger than one chunk -- a ciphertext needs
    2 * 3 * 4096 * 8 + 12 = 196620 bytes of scratch, so MOAI_CLIENT_TMP_KB = 400 holds two: chunks of 2 and 1"""
    primes = O.coeff_modulus_create(4096, [60, 40, 60])
    moai.hip.set_tuning("MOAI_CLIENT_TMP_KB", 400)
    try:
        _check_encrypt(moai, 12, primes, 3, SEEDS[:3], 5000, rng_seed=3)
    finally:
        moai.hip.reset_tuning()
    _check_encrypt(moai, 12, primes, 3, SEEDS[:3], 5000, rng_seed=3)  # and in one chunk


def _check_keygen(moai, logn, primes, seq, rng_seed, chunk_kb=None):
    n, k = 1 << logn, len(primes)
    octx = O.Context(logn, primes)
    ctx = moai.Context(logn, primes)
    rng = np.random.default_rng(rng_seed)
    s_ntt, new_ntt = _secret(octx, rng), _secret(octx, rng)
    seeds = SEEDS[:k - 1]
    if chunk_kb:
        moai.hip.set_tuning("MOAI_CLIENT_TMP_KB", chunk_kb)
    try:
        out, rejected, overflow = ctx.kswitch_keygen_seal_seeded(NOISE_KEY, seeds, seq, moai.DeviceBuffer.from_numpy(s_ntt),
                                                                 moai.DeviceBuffer.from_numpy(new_ntt))
    finally:
        moai.hip.reset_tuning()
    got = out.to_numpy((k - 1, k, n))
    total = 0
    for J in range(k - 1):
        a, rej = SF.sample_poly_uniform(seeds[J], primes, n)
        total += sum(rej)
        # c0 + a (.) s - (q_{k-1} mod q_J) new_key[J] [row = J] == NTT(e_J)
        m = octx.add(got[J], _mul(octx, a, s_ntt), 1, k)
        fac = np.zeros((k, n), dtype=np.uint64)
        fac[J] = primes[k - 1] % primes[J]
        m = octx.sub(m, _mul(octx, fac, new_ntt), 1, k)
        assert (m == _noise_ntt(octx, seq + J)).all(), J
    assert rejected == total and overflow is False
    return got, s_ntt, new_ntt, octx, ctx


def test_keygen_set_a(moai):
    """k = 4: three digits, three seeds"""
    _check_keygen(moai, 6, _json("a.json")["primes"], 1 << 30, 4)


def test_keygen_tiled(moai):
    """N = 4096, k = 3: two digits, in one chunk and one digit per chunk (a digit needs 196620 bytes of scratch)"""
    primes = O.coeff_modulus_create(4096, [60, 40, 60])
    whole = _check_keygen(moai, 12, primes, 77, 5)[0]
    assert (_check_keygen(moai, 12, primes, 77, 5, chunk_kb=200)[0] == whole).all()


def test_noise_is_that_of_the_chacha_seeded_calls(moai):
    """c0_seal + a_seal (.) s == c0_chacha + a_chacha (.) s for the same noise key and sequence: only a differs"""
    info = _json("a.json")
    primes, n, k = info["primes"], 64, 4
    octx = O.Context(6, primes)
    ctx = moai.Context(6, primes)
    rng = np.random.default_rng(6)
    s_ntt, new_ntt = _secret(octx, rng), _secret(octx, rng)
    d_sk, d_new = moai.DeviceBuffer.from_numpy(s_ntt), moai.DeviceBuffer.from_numpy(new_ntt)
    public = bytes((3 * i + 1) & 0xFF for i in range(32))
    seq, B = 123, 3
    seal = ctx.encrypt_symmetric_seal_seeded(NOISE_KEY, SEEDS[:B], seq, d_sk, k)[0].to_numpy((B, k, n))
    cha = ctx.encrypt_symmetric_seeded(NOISE_KEY, public, seq, d_sk, k, n_batch=B).to_numpy((B, k, n))
    kseal = ctx.kswitch_keygen_seal_seeded(NOISE_KEY, SEEDS[:k - 1], seq, d_sk, d_new)[0].to_numpy((k - 1, k, n))
    kcha = ctx.kswitch_keygen_seeded(NOISE_KEY, public, seq, d_sk, d_new).to_numpy((k - 1, k, n))
    assert (seal != cha).any()
    for b in range(B):
        a_seal = SF.sample_poly_uniform(SEEDS[b], primes, n)[0]
        a_cha = CS.uniform(public, CS.nonce(CS.UNIFORM, seq + b), primes, n)
        for c_seal, c_cha in ((seal[b], cha[b]), (kseal[b], kcha[b])):
            assert (octx.add(c_seal, _mul(octx, a_seal, s_ntt), 1, k) == octx.add(c_cha, _mul(octx, a_cha, s_ntt), 1, k)).all(), b


def test_argument_errors(moai):
    primes = _json("a.json")["primes"]
    n, k = 64, 4
    ctx = moai.Context(6, primes)
    lib = moai.hip.lib()
    d = moai.DeviceBuffer.from_numpy(np.zeros((4, k, n), dtype=np.uint64))
    seeds = b"".join(SEEDS)
    EINVAL = moai.hip.MOAI_EINVAL
    assert lib.moai_encrypt_symmetric_seal_seeded(ctx.h, NOISE_KEY, None, 0, d.ptr, None, d.ptr, 1, k, None, None, None) == EINVAL
    assert b"null seed" in lib.moai_last_error()
    assert lib.moai_kswitch_keygen_seal_seeded(ctx.h, NOISE_KEY, None, 0, d.ptr, d.ptr, d.ptr, None, None) == EINVAL
    assert b"null seed" in lib.moai_last_error()
    assert lib.moai_encrypt_symmetric_seal_seeded(ctx.h, NOISE_KEY, seeds, 2**56 - 1, d.ptr, None, d.ptr, 2, k, None, None, None) == EINVAL
    assert b"2^56" in lib.moai_last_error()
    assert lib.moai_kswitch_keygen_seal_seeded(ctx.h, NOISE_KEY, seeds, 2**56 - 2, d.ptr, d.ptr, d.ptr, None, None) == EINVAL
    assert b"2^56" in lib.moai_last_error()
    with pytest.raises(moai.MoaiError, match="null key"):
        ctx.encrypt_symmetric_seal_seeded(None, SEEDS[:1], 0, d, k)
    with pytest.raises(moai.MoaiError, match="invalid level"):
        ctx.encrypt_symmetric_seal_seeded(NOISE_KEY, SEEDS[:1], 0, d, k + 1)
    with pytest.raises(moai.MoaiError, match="null argument"):
        ctx.encrypt_symmetric_seal_seeded(NOISE_KEY, SEEDS[:1], 0, None, k)
    with pytest.raises(moai.MoaiError, match="null argument"):
        ctx.kswitch_keygen_seal_seeded(NOISE_KEY, SEEDS[:3], 0, d, None)
    with pytest.raises(ValueError):
        ctx.kswitch_keygen_seal_seeded(NOISE_KEY, SEEDS[:2], 0, d, d)
    one = moai.Context(6, primes[:1])
    with pytest.raises(moai.MoaiError, match="keyswitching"):
        one.kswitch_keygen_seal_seeded(NOISE_KEY, [], 0, d, d)
    # nothing was enqueued: the buffer still holds zeros
    assert not d.to_numpy().any()
