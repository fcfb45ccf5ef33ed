"""GPU parity of the wire form (include/moai_hip.h, "wire form: seeded objects and bit-packed rows"): moai_pack_rows /
moai_unpack_rows bit for bit against tests/wire_format.py (pinned by tests/test_wire_format.py), the validity flag, the
seeded encryption and key generation against a comparator assembled here from tests/client_sampling.py's primitives with two
different keys, their equality with the unseeded entry points when the keys are equal, moai_expand_seeded against
moai_sample_uniform, and the argument errors."""
import numpy as np
import pytest

import client_sampling as CS
import oracle as O
import wire_format as WF

pytestmark = pytest.mark.gpu

MOAI_BITS = [51] + [46] * 20 + [51] * 14 + [58]  # include/test/test_full_scheme.hpp:356-378
NOISE_KEY = bytes((7 * i + 3) & 0xFF for i in range(32))
SEED = bytes((11 * i + 5) & 0xFF for i in range(32))
SHAPES = [(4, [30, 31]), (10, [60, 60, 60]), (12, [51, 46, 46, 58]), (16, MOAI_BITS)]


def _setup(moai, logn, bits):
    primes = O.coeff_modulus_create(1 << logn, bits)
    return primes, O.Context(logn, primes), moai.Context(logn, primes)


def _secret(octx, rng, primes):
    s = rng.integers(-1, 2, size=octx.n)
    return s, octx.ntt(CS.to_rns(s, primes), len(primes))


def _words(buf, first_word, count, moai):
    out = np.empty(count, dtype=np.uint64)
    lib = moai.hip.lib()
    assert lib.moai_stream_sync(None) == 0
    assert lib.moai_memcpy_d2h(out.ctypes.data, buf.ptr + 8 * first_word, count * 8, None) == 0
    assert lib.moai_stream_sync(None) == 0
    return out


def _is_prime(q):
    if q < 2:
        return False
    for p in (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37):
        if q % p == 0:
            return q == p
    d, s = q - 1, 0
    while d % 2 == 0:
        d, s = d // 2, s + 1
    for a in (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37):  # deterministic below 3.3e24
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


def _ntt_prime(n, b):
    """the largest prime of exactly b bits that is 1 mod 2n, or None"""
    q = ((1 << b) - 1) // (2 * n) * (2 * n) + 1
    while q >= 1 << (b - 1):
        if _is_prime(q):
            return q
        q -= 2 * n
    return None


def _check_pack(moai, ctx, primes, n, n_poly, prime_index, rng):
    sel = [primes[i] for i in prime_index] if prime_index is not None else list(primes)
    L = len(sel)
    polys = O.uniform_rns(rng, sel, (n_poly,), n)
    polys[0, :, 0] = 0
    polys[-1, :, n - 1] = [q - 1 for q in sel]
    want = WF.pack_rows(polys, sel)
    pw = ctx.packed_words(L, prime_index)
    assert pw == WF.packed_words(n, sel) and want.size == n_poly * pw
    d = moai.DeviceBuffer.from_numpy(polys)
    packed = ctx.pack_rows(d, n_poly, L, prime_index)
    assert (packed.to_numpy() == want).all()
    back, invalid = ctx.unpack_rows(packed, n_poly, L, prime_index)
    assert invalid is False
    assert (back.to_numpy((n_poly, L, n)) == polys).all()
    # and from the comparator's words, without a flag
    back2, none = ctx.unpack_rows(moai.DeviceBuffer.from_numpy(want), n_poly, L, prime_index, check=False)
    assert none is None and (back2.to_numpy((n_poly, L, n)) == polys).all()


@pytest.mark.parametrize("logn,bits", SHAPES)
def test_pack_unpack_match_comparator(moai, logn, bits):
    primes, _, ctx = _setup(moai, logn, bits)
    n, k = 1 << logn, len(primes)
    rng = np.random.default_rng(logn)
    pi = list(range(k))[::-1][: max(1, k // 2)]
    for n_poly in (1, 3):
        _check_pack(moai, ctx, primes, n, n_poly, None, rng)
        _check_pack(moai, ctx, primes, n, n_poly, pi, rng)
    _check_pack(moai, ctx, primes[: k - 1], n, 2, list(range(k - 1)), rng)


@pytest.mark.parametrize("logn", [1, 6, 9])
def test_every_field_width(moai, logn):
    """every bit length a context can hold at this N (3 .. 61 at N = 2), one row each; N = 2 also has rows shorter than a word"""
    n = 1 << logn
    primes = [q for q in (_ntt_prime(n, b) for b in range(3, 62)) if q]
    assert len({int(q).bit_length() for q in primes}) == len(primes) >= 45
    ctx = moai.Context(logn, primes)
    _check_pack(moai, ctx, primes, n, 2, None, np.random.default_rng(logn))


@pytest.mark.parametrize("logn,bits", [(4, [30, 31]), (12, [51, 46, 46, 58])])
def test_validity_flag(moai, logn, bits):
    primes, _, ctx = _setup(moai, logn, bits)
    n, k = 1 << logn, len(primes)
    rng = np.random.default_rng(9)
    polys = O.uniform_rns(rng, primes, (2,), n)
    honest = WF.pack_rows(polys, primes)
    _, invalid = ctx.unpack_rows(moai.DeviceBuffer.from_numpy(honest), 2, k)
    assert invalid is False
    for r in (0, k - 1):
        b = int(primes[r]).bit_length()
        for value in (primes[r], (1 << b) - 1):  # q_r itself, and the largest value the field holds
            bad = polys.copy()
            bad[1, r, n - 3] = value
            words = WF.pack_rows(bad, primes)
            assert WF.unpack_rows(words, 2, n, primes)[1]
            out, invalid = ctx.unpack_rows(moai.DeviceBuffer.from_numpy(words), 2, k)
            assert invalid is True
            assert (out.to_numpy((2, k, n)) == bad).all()  # an error return: the data still comes out as it stands
            # without a flag the call has nothing to report
            out, none = ctx.unpack_rows(moai.DeviceBuffer.from_numpy(words), 2, k, check=False)
            assert none is None


def test_pack_unpack_past_one_launch(moai):
    """65535 + 2 polynomials: a launch holds 65535 (gridDim.z), so the second one starts from advanced pointers.  N = 16 with a
    30-bit and a 31-bit prime (rows of 8 words each, so the row offset matters): the round trip is bit-exact, the packed words
    on both sides of the boundary are the comparator's, and a residue equal to its prime past the boundary is reported"""
    logn, bits = 4, [30, 31]
    primes, _, ctx = _setup(moai, logn, bits)
    n, L, n_poly = 1 << logn, 2, 65535 + 2
    assert sorted(int(q).bit_length() for q in primes) == bits
    polys = O.uniform_rns(np.random.default_rng(65537), primes, (n_poly,), n)
    pw = WF.packed_words(n, primes)
    d = moai.DeviceBuffer.from_numpy(polys)
    packed = ctx.pack_rows(d, n_poly, L)
    words = packed.to_numpy().reshape(n_poly, pw)
    for p in (0, 65534, 65535, 65536):
        assert (words[p] == WF.pack_rows(polys[p:p + 1], primes)).all(), p
    back, invalid = ctx.unpack_rows(packed, n_poly, L)
    assert invalid is False and (back.to_numpy((n_poly, L, n)) == polys).all()
    assert ctx.check_residues(d, n_poly, L) is False
    bad = polys.copy()
    bad[65536, 1, 3] = primes[1]
    bad_words = words.copy()
    bad_words[65536] = WF.pack_rows(bad[65536:], primes)
    out, invalid = ctx.unpack_rows(moai.DeviceBuffer.from_numpy(bad_words), n_poly, L)
    assert invalid is True and (out.to_numpy((n_poly, L, n)) == bad).all()
    assert ctx.check_residues(moai.DeviceBuffer.from_numpy(bad), n_poly, L) is True


def _sym_c0(octx, noise_key, seed, seq, sk_ntt, L, rows=None):
    """(c0, a) of a symmetric encryption of zero: e from (noise_key, purpose 3), a from (seed, purpose 1)"""
    n, primes = octx.n, octx.primes[:L]
    e = octx.ntt(CS.to_rns(CS.cbd(noise_key, CS.nonce(CS.NOISE0, seq), n), primes), L)
    a = CS.uniform(seed, CS.nonce(CS.UNIFORM, seq), primes, n, rows)
    c0 = np.zeros((L, n), dtype=np.uint64)
    for r in range(L) if rows is None else rows:
        q = int(primes[r])
        c0[r] = ((e[r].astype(object) - a[r].astype(object) * sk_ntt[r].astype(object)) % q).astype(np.uint64)
    return c0, a


@pytest.mark.parametrize("logn,bits", [(10, [51, 46, 46, 58]), (12, [60, 40, 40, 50, 60])])
def test_encrypt_symmetric_seeded(moai, logn, bits):
    primes, octx, ctx = _setup(moai, logn, bits)
    n, k = octx.n, len(primes)
    rng = np.random.default_rng(logn)
    _, s_ntt = _secret(octx, rng, primes)
    d_sk = moai.DeviceBuffer.from_numpy(s_ntt)
    for L in (k, k - 1, 2):
        B, seq = 3, 100 + L
        plain = O.uniform_rns(rng, primes[:L], (B,), n)
        d_plain = moai.DeviceBuffer.from_numpy(plain)
        c0 = ctx.encrypt_symmetric_seeded(NOISE_KEY, SEED, seq, d_sk, L, B, plain=d_plain)
        got = c0.to_numpy((B, L, n))
        full = ctx.expand_seeded(SEED, seq, c0, B, L).to_numpy((B, 2, L, n))
        a_dev = ctx.sample_uniform(SEED, CS.nonce(CS.UNIFORM, seq), B, L).to_numpy((B, L, n))
        for b in range(B):
            want, a = _sym_c0(octx, NOISE_KEY, SEED, seq + b, s_ntt, L)
            for r in range(L):
                want[r] = (want[r].astype(object) + plain[b, r].astype(object)) % int(primes[r])
            assert (got[b] == want).all(), (L, b)
            assert (full[b, 0] == want).all() and (full[b, 1] == a).all() and (a_dev[b] == a).all(), (L, b)
        # encryptions of zero
        got0 = ctx.encrypt_symmetric_seeded(NOISE_KEY, SEED, seq, d_sk, L, 1).to_numpy((L, n))
        assert (got0 == _sym_c0(octx, NOISE_KEY, SEED, seq, s_ntt, L)[0]).all()
        # equal keys: the seeded call and its expansion are the unseeded entry point, bit for bit
        c0 = ctx.encrypt_symmetric_seeded(NOISE_KEY, NOISE_KEY, seq, d_sk, L, B, plain=d_plain)
        same = ctx.expand_seeded(NOISE_KEY, seq, c0, B, L).to_numpy((B, 2, L, n))
        assert (same == ctx.encrypt_symmetric(NOISE_KEY, seq, d_sk, L, B, plain=d_plain).to_numpy((B, 2, L, n))).all()
    # rows under a prime_index map
    pi = [k - 1, 0]
    sk_sel = moai.DeviceBuffer.from_numpy(s_ntt[pi])
    c0 = ctx.encrypt_symmetric_seeded(NOISE_KEY, SEED, 7, sk_sel, 2, 2, prime_index=pi)
    full = ctx.expand_seeded(SEED, 7, c0, 2, 2, prime_index=pi).to_numpy((2, 2, 2, n))
    a_dev = ctx.sample_uniform(SEED, CS.nonce(CS.UNIFORM, 7), 2, 2, prime_index=pi).to_numpy((2, 2, n))
    assert (full[:, 0] == c0.to_numpy((2, 2, n))).all() and (full[:, 1] == a_dev).all()
    assert (a_dev[1] == CS.uniform(SEED, CS.nonce(CS.UNIFORM, 8), [primes[i] for i in pi], n)).all()


def test_kswitch_keygen_seeded_small(moai):
    logn = 12
    for bits in ([51, 46, 46, 58], [60, 50, 40, 50, 46, 60]):
        primes, octx, ctx = _setup(moai, logn, bits)
        n, k = octx.n, len(primes)
        rng = np.random.default_rng(k)
        _, s_ntt = _secret(octx, rng, primes)
        _, s2_ntt = _secret(octx, rng, primes)
        d_s, d_s2 = moai.DeviceBuffer.from_numpy(s_ntt), moai.DeviceBuffer.from_numpy(s2_ntt)
        c0 = ctx.kswitch_keygen_seeded(NOISE_KEY, SEED, 500, d_s, d_s2)
        got = c0.to_numpy((k - 1, k, n))
        key = ctx.expand_seeded(SEED, 500, c0, k - 1, k).to_numpy((k - 1, 2, k, n))
        for J in range(k - 1):
            want, a = _sym_c0(octx, NOISE_KEY, SEED, 500 + J, s_ntt, k)
            qJ = int(primes[J])
            want[J] = (want[J].astype(object) + s2_ntt[J].astype(object) * (int(primes[k - 1]) % qJ)) % qJ
            assert (got[J] == want).all(), J
            assert (key[J, 0] == want).all() and (key[J, 1] == a).all(), J
        c0 = ctx.kswitch_keygen_seeded(NOISE_KEY, NOISE_KEY, 500, d_s, d_s2)
        same = ctx.expand_seeded(NOISE_KEY, 500, c0, k - 1, k).to_numpy((k - 1, 2, k, n))
        assert (same == ctx.kswitch_keygen(NOISE_KEY, 500, d_s, d_s2).to_numpy((k - 1, 2, k, n))).all()


def test_kswitch_keygen_seeded_moai_size(moai):
    """N = 2^16 on MOAI's 36 primes: digits 0, 17 and 34 bit-exact on rows {0, J, 35} (only their stream ranges computed), the
    expanded key against it, and the packed key's size and round trip"""
    logn = 16
    primes, octx, ctx = _setup(moai, logn, MOAI_BITS)
    n, k = octx.n, len(primes)
    rng = np.random.default_rng(36)
    _, s_ntt = _secret(octx, rng, primes)
    _, s2_ntt = _secret(octx, rng, primes)
    seq = 1 << 40
    c0 = ctx.kswitch_keygen_seeded(NOISE_KEY, SEED, seq, moai.DeviceBuffer.from_numpy(s_ntt), moai.DeviceBuffer.from_numpy(s2_ntt))
    key = ctx.expand_seeded(SEED, seq, c0, k - 1, k)
    for J in (0, 17, k - 2):
        rows = sorted({0, J, k - 1})
        want, a = _sym_c0(octx, NOISE_KEY, SEED, seq + J, s_ntt, k, rows)
        qJ = int(primes[J])
        want[J] = (want[J].astype(object) + s2_ntt[J].astype(object) * (int(primes[k - 1]) % qJ)) % qJ
        for r in rows:
            assert (_words(c0, (J * k + r) * n, n, moai) == want[r]).all(), (J, r)
            assert (_words(key, ((J * 2) * k + r) * n, n, moai) == want[r]).all(), (J, r)
            assert (_words(key, ((J * 2 + 1) * k + r) * n, n, moai) == a[r]).all(), (J, r)
    # the wire form of this key: 35 x 1743 bits x 65536 / 8 bytes, 37.8 % of the resident 1.32 GB
    pw = ctx.packed_words(k)
    assert pw * 64 == 1743 * n and (k - 1) * pw * 8 == 35 * 1743 * n // 8
    packed = ctx.pack_rows(c0, k - 1, k)
    for J, r in ((0, 0), (17, 17), (k - 2, k - 1)):
        off = J * pw + WF.packed_words(n, primes[:r])
        w = WF.row_words(n, int(primes[r]).bit_length())
        assert (_words(packed, off, w, moai) == WF.pack_row(_words(c0, (J * k + r) * n, n, moai), int(primes[r]).bit_length())).all()
    back, invalid = ctx.unpack_rows(packed, k - 1, k)
    assert invalid is False
    for J in (0, 17, k - 2):
        assert (_words(back, J * k * n, k * n, moai) == _words(c0, J * k * n, k * n, moai)).all()


def test_argument_errors(moai):
    logn = 10
    n = 1 << logn
    primes = O.coeff_modulus_create(n, [51, 46, 58])
    ctx = moai.Context(logn, primes)
    d = moai.DeviceBuffer.from_numpy(np.zeros((4, 2, 3, n), dtype=np.uint64))
    e = moai.DeviceBuffer.from_numpy(np.zeros((4, 2, 3, n), dtype=np.uint64))
    lib = moai.hip.lib()
    EINVAL = moai.hip.MOAI_EINVAL
    assert ctx.packed_words(3) == (51 + 46 + 58) * n // 64
    assert lib.moai_packed_words(ctx.h, 4, None) == 0 and lib.moai_packed_words(ctx.h, 0, None) == 0
    assert lib.moai_packed_words(None, 1, None) == 0
    with pytest.raises(moai.MoaiError, match="invalid level"):
        ctx.pack_rows(d, 1, 4)
    with pytest.raises(moai.MoaiError):
        ctx.pack_rows(d, 1, 2, prime_index=[0, 5])
    with pytest.raises(moai.MoaiError, match="null argument"):
        ctx.pack_rows(None, 1, 3)
    with pytest.raises(moai.MoaiError, match="null argument"):
        ctx.unpack_rows(None, 1, 3)
    assert lib.moai_pack_rows(ctx.h, d.ptr, d.ptr + 8 * n, 2, 3, None, None) == EINVAL
    assert b"overlap" in lib.moai_last_error()
    assert lib.moai_unpack_rows(ctx.h, d.ptr + 8 * n, d.ptr, 2, 3, None, None, None) == EINVAL
    assert b"overlap" in lib.moai_last_error()
    assert lib.moai_unpack_rows(ctx.h, d.ptr, e.ptr + 8, 1, 3, None, None, None) == EINVAL
    assert b"aligned" in lib.moai_last_error()
    assert lib.moai_pack_rows(None, d.ptr, e.ptr, 1, 3, None, None) == EINVAL
    # nothing to do is not an error
    assert lib.moai_pack_rows(ctx.h, None, None, 0, 3, None, None) == 0
    with pytest.raises(moai.MoaiError, match="null key"):
        ctx.encrypt_symmetric_seeded(None, SEED, 0, d, 2)
    with pytest.raises(moai.MoaiError, match="null seed"):
        ctx.encrypt_symmetric_seeded(NOISE_KEY, None, 0, d, 2)
    with pytest.raises(moai.MoaiError, match="2\\^56"):
        ctx.encrypt_symmetric_seeded(NOISE_KEY, SEED, 2**56 - 1, d, 2, n_batch=2)
    with pytest.raises(moai.MoaiError, match="invalid level"):
        ctx.encrypt_symmetric_seeded(NOISE_KEY, SEED, 0, d, 4)
    with pytest.raises(moai.MoaiError, match="null argument"):
        ctx.encrypt_symmetric_seeded(NOISE_KEY, SEED, 0, None, 2)
    with pytest.raises(moai.MoaiError, match="null key"):
        ctx.kswitch_keygen_seeded(None, SEED, 0, d, d)
    with pytest.raises(moai.MoaiError, match="null seed"):
        ctx.kswitch_keygen_seeded(NOISE_KEY, None, 0, d, d)
    with pytest.raises(moai.MoaiError, match="null argument"):
        ctx.kswitch_keygen_seeded(NOISE_KEY, SEED, 0, d, None)
    with pytest.raises(moai.MoaiError, match="2\\^56"):
        ctx.kswitch_keygen_seeded(NOISE_KEY, SEED, 2**56 - 1, d, d)
    one = moai.Context(logn, primes[:1])
    with pytest.raises(moai.MoaiError, match="keyswitching"):
        one.kswitch_keygen_seeded(NOISE_KEY, SEED, 0, d, d)
    with pytest.raises(moai.MoaiError, match="null key"):
        ctx.expand_seeded(None, 0, d, 1, 3)
    with pytest.raises(moai.MoaiError, match="invalid level"):
        ctx.expand_seeded(SEED, 0, d, 1, 0)
    with pytest.raises(moai.MoaiError, match="2\\^56"):
        ctx.expand_seeded(SEED, 2**56, d, 1, 3)
    with pytest.raises(moai.MoaiError, match="null argument"):
        ctx.expand_seeded(SEED, 0, None, 1, 3)
    assert lib.moai_expand_seeded(ctx.h, SEED, 0, d.ptr, d.ptr + 8 * 2 * n, 1, 3, None, None) == EINVAL
    assert b"overlap" in lib.moai_last_error()
    # nothing was enqueued: the buffers still hold zeros
    assert not d.to_numpy().any() and not e.to_numpy().any()


def test_argument_table(moai):
    """one fault per row: the return code and the text of moai_last_error().  Nothing is launched on a failing row."""
    logn = 10
    n = 1 << logn
    primes = O.coeff_modulus_create(n, [51, 46, 58])
    ctx = moai.Context(logn, primes)
    d = moai.DeviceBuffer.from_numpy(np.zeros((4, 2, 3, n), dtype=np.uint64))
    e = moai.DeviceBuffer.from_numpy(np.zeros((4, 2, 3, n), dtype=np.uint64))
    lib = moai.hip.lib()
    EINVAL = moai.hip.MOAI_EINVAL
    h = ctx.h
    pw8 = 8 * ctx.packed_words(3)
    table = [
        # in [2][3][N] before packed, and packed [2][pw] before in
        (lib.moai_pack_rows, (h, d.ptr, d.ptr + 8 * n, 2, 3, None, None), EINVAL, b"in and packed overlap"),
        (lib.moai_pack_rows, (h, d.ptr + pw8, d.ptr, 2, 3, None, None), EINVAL, b"in and packed overlap"),
        (lib.moai_unpack_rows, (h, d.ptr + 16 * n, d.ptr, 2, 3, None, None, None), EINVAL, b"packed and out overlap"),
        (lib.moai_unpack_rows, (h, d.ptr, d.ptr + pw8, 2, 3, None, None, None), EINVAL, b"packed and out overlap"),
        (lib.moai_unpack_rows, (h, d.ptr, e.ptr + 8, 1, 3, None, None, None), EINVAL, b"out must be 16-byte aligned"),
        (lib.moai_pack_rows, (h, d.ptr, e.ptr, 2**40 + 1, 3, None, None), EINVAL, b"too many polynomials"),
        (lib.moai_unpack_rows, (h, d.ptr, e.ptr, 2**40 + 1, 3, None, None, None), EINVAL, b"too many polynomials"),
        (lib.moai_expand_seeded, (h, SEED, 0, d.ptr, d.ptr + 8 * 2 * n, 1, 3, None, None), EINVAL, b"c0 and out overlap"),
        (lib.moai_expand_seeded, (h, SEED, 0, d.ptr + 8 * 3 * n, d.ptr, 1, 3, None, None), EINVAL, b"c0 and out overlap"),
    ]
    for fn, args, rc, text in table:
        assert fn(*args) == rc and text in lib.moai_last_error(), (fn.__name__, args[1:], lib.moai_last_error())
    assert not d.to_numpy().any() and not e.to_numpy().any()
