"""GPU parity of SEAL's generator and uniform sampler (include/moai_hip.h, "SEAL's own format: the generator of seeded
objects") over the C ABI: moai_seal_prng_bytes and moai_seal_sample_uniform bit for bit against tests/seal_format.py (pinned by
tests/test_seal_format.py against fixtures SEAL itself wrote), the rejection count, the residue check and the argument errors."""
import hashlib
import json
import os

import numpy as np
import pytest

import oracle as O
import seal_format as SF

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "seal_format")
SET_A = [1085102592571152769, 461168601842740097, 558992244657868289, 922337203685478017]
DIVISORS = (17, 40, 33, 20)  # Set A's primes are the first ones = 1 mod 2N above 2^64 / d: 2^64 = (d - 1) q + (almost q)


def _seed(tag):
    return hashlib.sha512(b"seal format test seed %d" % tag).digest()


def _is_prime(q):
    for p in (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37):
        if q % p == 0:
            return q == p
    d, s = q - 1, 0
    while d % 2 == 0:
        d, s = d // 2, s + 1
    for a in (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37):
        x = pow(a, d, q)
        if x in (1, q - 1):
            continue
        for _ in range(s - 1):
            x = x * x % q
            if x == q - 1:
                break
        else:
            return False
    return True


def _primes_above(n, d, count):
    """the first `count` primes above 2^64 / d that are 1 mod 2n: each rejects about 1 / d of all words"""
    out = []
    q = ((1 << 64) // d // (2 * n) + 1) * (2 * n) + 1
    while len(out) < count:
        if _is_prime(q):
            out.append(q)
        q += 2 * n
    return out


def _rejecting_primes(n):
    return [_primes_above(n, d, 1)[0] for d in DIVISORS]


def _json(name):
    with open(os.path.join(GOLDEN, name)) as f:
        return json.load(f)


def _bytes(name):
    with open(os.path.join(GOLDEN, name), "rb") as f:
        return f.read()


def test_prng_bytes(moai):
    ctx = moai.Context(10, O.coeff_modulus_create(1 << 10, [51, 46, 58]))
    seed = _seed(0)
    assert ctx.seal_prng_bytes(seed, 0, 3) == SF.prng_buffers(seed, 0, 3)
    # the counter's high word matters, and so does every lane group of a wavefront's 16 buffers and a second workgroup
    first = (1 << 32) + 5
    got = ctx.seal_prng_bytes(seed, first, 70)
    assert got == SF.prng_buffers(seed, first, 70)
    assert got[:4096] != SF.prng_buffers(seed, 5, 1)
    ct = SF.read_ciphertext(_bytes("b_ct_seeded.bin"))
    assert ctx.seal_prng_bytes(ct["seed"], 0, 1) == SF.prng_buffers(ct["seed"], 0, 1)


def _check_sample(moai, logn, primes, L, seeds, prime_index=None):
    n = 1 << logn
    ctx = moai.Context(logn, primes)
    sel = [primes[i] for i in prime_index] if prime_index is not None else primes[:L]
    want = [SF.sample_poly_uniform(s, sel, n) for s in seeds]
    out, rejected, overflow = ctx.seal_sample_uniform(seeds, L, prime_index=prime_index)
    got = out.to_numpy((len(seeds), L, n))
    for b in range(len(seeds)):
        assert (got[b] == want[b][0]).all(), b
    total = sum(sum(w[1]) for w in want)
    print("logn %d L %d count %d: rejected %d (restatement %d)" % (logn, L, len(seeds), rejected, total))
    assert rejected == total and overflow is False
    assert ctx.check_residues(out, len(seeds), L, prime_index) is False
    return ctx, want, total


def test_sample_bulk_smaller_than_a_buffer(moai):
    """logn 6, L = 3: 192 words, the tail starts inside buffer 0"""
    _, _, total = _check_sample(moai, 6, SET_A, 3, [_seed(i) for i in range(1, 9)])
    assert total >= 8


def test_sample_two_rows_share_a_buffer(moai):
    """logn 8, L = 4, primes found the way Set A's were"""
    assert _rejecting_primes(64) == SET_A
    primes = _rejecting_primes(256)
    assert all(q < 1 << 60 and q % 512 == 1 for q in primes)
    assert all(((1 << 64) - 1 - SF.max_multiple(q)) * 41 > 1 << 64 for q in primes)  # each rejects more than 1 / 41
    _, _, total = _check_sample(moai, 8, primes, 4, [_seed(20), _seed(21), _seed(22)])
    assert total >= 20


def test_sample_against_seals_own_residues(moai):
    """Set B: N = 1024, L = 2, a replacement word that is itself rejected; the expansion is what SEAL's load produced"""
    info = _json("b.json")
    ct = SF.read_ciphertext(_bytes("b_ct_seeded.bin"))
    ctx = moai.Context(10, info["primes"])
    out, rejected, overflow = ctx.seal_sample_uniform([ct["seed"]], 2)
    a = out.to_numpy((2, 1024))
    assert hashlib.sha256(np.stack([ct["data"][0], a]).astype("<u8").tobytes()).hexdigest() == info["ct_sha256"]
    want = SF.sample_poly_uniform(ct["seed"], info["primes"][:2], 1024)
    assert rejected == sum(want[1]) >= 2 and overflow is False
    # the key level: both digits of the relinearisation key in one call, into polynomial 1 of each [2][k][N] digit
    rk = SF.read_kswitch_keys(_bytes("b_rk_seeded.bin"))
    digits = [d for ds in rk["keys"] for d in ds]
    key = np.zeros((len(digits), 2, 3, 1024), dtype=np.uint64)
    for i, d in enumerate(digits):
        key[i, 0] = d["data"][0]
    dkey = moai.DeviceBuffer.from_numpy(key)
    ctx.seal_sample_uniform([d["seed"] for d in digits], 3, out=dkey.ptr + 8 * 3 * 1024, stride_words=2 * 3 * 1024)
    assert hashlib.sha256(dkey.to_numpy().astype("<u8").tobytes()).hexdigest() == info["rk_sha256"]


def test_sample_moai_bit_pattern_strided_with_sentinels(moai):
    logn, n = 12, 1 << 12
    primes = O.coeff_modulus_create(n, [51, 46, 46, 58])
    ctx = moai.Context(logn, primes)
    pi, L, count = [3, 1, 0], 3, 5
    sel = [primes[i] for i in pi]
    seeds = [_seed(40 + i) for i in range(count)]
    stride = 2 * L * n
    sentinel = np.uint64(0xA5A5A5A5DEADBEEF)
    host = np.full((count, 2, L, n), sentinel, dtype=np.uint64)
    d = moai.DeviceBuffer.from_numpy(host)
    none, rejected, overflow = ctx.seal_sample_uniform(seeds, L, out=d.ptr + 8 * L * n, stride_words=stride, prime_index=pi)
    assert none is None and rejected == 0 and overflow is False
    got = d.to_numpy((count, 2, L, n))
    assert (got[:, 0] == sentinel).all()
    for b in range(count):
        want, rej = SF.sample_poly_uniform(seeds[b], sel, n)
        assert rej == [0, 0, 0] and (got[b, 1] == want).all(), b


def test_check_residues(moai):
    logn, n = 10, 1 << 10
    primes = O.coeff_modulus_create(n, [51, 46, 58])
    ctx = moai.Context(logn, primes)
    polys = O.uniform_rns(np.random.default_rng(3), primes, (2,), n)
    polys[1, :, n - 1] = [q - 1 for q in primes]
    assert ctx.check_residues(moai.DeviceBuffer.from_numpy(polys), 2, 3) is False
    for r in (0, 2):
        bad = polys.copy()
        bad[1, r, 5] = primes[r]
        assert ctx.check_residues(moai.DeviceBuffer.from_numpy(bad), 2, 3) is True
    assert ctx.check_residues(moai.DeviceBuffer.from_numpy(polys[:, ::-1].copy()), 2, 3, prime_index=[2, 1, 0]) is False


def test_argument_errors(moai):
    logn, n = 10, 1 << 10
    primes = O.coeff_modulus_create(n, [51, 46, 58])
    ctx = moai.Context(logn, primes)
    lib = moai.hip.lib()
    EINVAL = moai.hip.MOAI_EINVAL
    d = moai.DeviceBuffer.from_numpy(np.zeros((2, 2, 3, n), dtype=np.uint64))
    seeds = _seed(1) + _seed(2)

    def sample(*args):
        rc = lib.moai_seal_sample_uniform(*args)
        return rc, lib.moai_last_error()

    assert sample(ctx.h, None, d.ptr, 3 * n, 1, 3, None, None, None) == (EINVAL, b"null seed")
    assert sample(ctx.h, seeds, None, 3 * n, 1, 3, None, None, None) == (EINVAL, b"null argument")
    rc, msg = sample(ctx.h, seeds, d.ptr, 3 * n, 0, 3, None, None, None)
    assert rc == EINVAL and b"count" in msg
    assert sample(ctx.h, seeds, d.ptr, 4 * n, 1, 4, None, None, None) == (EINVAL, b"invalid level")
    assert sample(ctx.h, seeds, d.ptr, 3 * n, 1, 0, None, None, None) == (EINVAL, b"invalid level")
    rc, msg = sample(ctx.h, seeds, d.ptr, 3 * n - 2, 2, 3, None, None, None)
    assert rc == EINVAL and b"stride" in msg
    rc, msg = sample(ctx.h, seeds, d.ptr + 8, 3 * n, 1, 3, None, None, None)
    assert rc == EINVAL and b"aligned" in msg
    rc, msg = sample(ctx.h, seeds, d.ptr, 3 * n + 1, 2, 3, None, None, None)
    assert rc == EINVAL and b"aligned" in msg
    assert sample(None, seeds, d.ptr, 3 * n, 1, 3, None, None, None)[0] == EINVAL
    with pytest.raises(moai.MoaiError):
        ctx.seal_sample_uniform([_seed(1)], 2, prime_index=[0, 7])
    assert lib.moai_seal_prng_bytes(ctx.h, None, 0, 1, d.ptr, None) == EINVAL and lib.moai_last_error() == b"null seed"
    assert lib.moai_seal_prng_bytes(ctx.h, seeds, 0, 1, None, None) == EINVAL
    assert lib.moai_seal_prng_bytes(ctx.h, seeds, 0, 1, d.ptr + 8, None) == EINVAL and b"aligned" in lib.moai_last_error()
    assert lib.moai_seal_prng_bytes(ctx.h, seeds, 2**64 - 1, 2, d.ptr, None) == EINVAL and b"wraps" in lib.moai_last_error()
    assert lib.moai_seal_prng_bytes(ctx.h, seeds, 0, 0, None, None) == 0  # nothing to do is not an error
    with pytest.raises(moai.MoaiError, match="null argument"):
        ctx.check_residues(None, 1, 3)
    # nothing was enqueued: the buffer still holds zeros
    assert not d.to_numpy().any()


def test_argument_table(moai):
    """one fault per row: the return code and the text of moai_last_error().  Nothing is launched on a failing row."""
    logn, n = 10, 1 << 10
    primes = O.coeff_modulus_create(n, [51, 46, 58])
    ctx = moai.Context(logn, primes)
    lib = moai.hip.lib()
    EINVAL = moai.hip.MOAI_EINVAL
    d = moai.DeviceBuffer.from_numpy(np.zeros((2, 2, 3, n), dtype=np.uint64))
    flag = moai.DeviceBuffer.from_numpy(np.zeros(1, dtype=np.uint64))
    seeds = _seed(1) + _seed(2)
    h = ctx.h
    table = [
        (lib.moai_seal_prng_bytes, (h, None, 0, 1, d.ptr, None), EINVAL, b"null seed"),
        (lib.moai_seal_prng_bytes, (h, seeds, 0, 1, d.ptr + 8, None), EINVAL, b"out must be 16-byte aligned"),
        (lib.moai_seal_prng_bytes, (h, seeds, 2**64 - 1, 2, d.ptr, None), EINVAL, b"block range wraps around 2^64"),
        (lib.moai_seal_prng_bytes, (h, seeds, 0, 2**36 + 1, d.ptr, None), EINVAL, b"too many blocks"),
        (lib.moai_seal_prng_bytes, (h, seeds, 0, 0, None, None), 0, None),
        (lib.moai_seal_sample_uniform, (h, seeds, d.ptr, 4 * n, 1, 4, None, None, None), EINVAL, b"invalid level"),
        (lib.moai_seal_sample_uniform, (h, seeds, d.ptr, 3 * n, 1, 0, None, None, None), EINVAL, b"invalid level"),
        (lib.moai_seal_sample_uniform, (h, None, d.ptr, 3 * n, 1, 3, None, None, None), EINVAL, b"null seed"),
        (lib.moai_seal_sample_uniform, (h, seeds, d.ptr, 3 * n, 0, 3, None, None, None), EINVAL, b"count must be between 1 and 2^24"),
        (lib.moai_seal_sample_uniform, (h, seeds, d.ptr, 3 * n, 2**24 + 1, 3, None, None, None), EINVAL,
         b"count must be between 1 and 2^24"),
        (lib.moai_seal_sample_uniform, (h, seeds, d.ptr, 3 * n - 2, 2, 3, None, None, None), EINVAL,
         b"stride is smaller than a polynomial"),
        (lib.moai_seal_sample_uniform, (h, seeds, d.ptr, 3 * n + 1, 2, 3, None, None, None), EINVAL, b"out must be 16-byte aligned"),
        (lib.moai_check_residues, (h, d.ptr, 1, 4, None, flag.ptr, None), EINVAL, b"invalid level"),
        (lib.moai_check_residues, (h, d.ptr, 1, 0, None, flag.ptr, None), EINVAL, b"invalid level"),
        (lib.moai_check_residues, (h, d.ptr, 1, 3, None, None, None), EINVAL, b"null argument"),
        (lib.moai_check_residues, (h, None, 0, 3, None, None, None), 0, None),
        (lib.moai_total_coeff_modulus_bit_count, (h, 4, None), 0, b"invalid level"),
        (lib.moai_total_coeff_modulus_bit_count, (h, 0, None), 0, b"invalid level"),
    ]
    for fn, args, rc, text in table:
        assert fn(*args) == rc, (fn.__name__, args[1:])
        assert text is None or lib.moai_last_error() == text, (fn.__name__, args[1:], lib.moai_last_error())
    assert not d.to_numpy().any() and not flag.to_numpy().any()
