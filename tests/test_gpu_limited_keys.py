"""GPU parity of switching keys limited to a chain index (include/moai_hip.h, "keys limited to a chain index"):
moai_kswitch_keygen_limited against tests/client_sampling.py's key digits restricted to the rows {0 .. levels-1, k-1} (which
computes full-layout stream positions) and, word for word, against moai_key_trim of the full key; the seeded form and its
expansion; the packed round trip under the limited row map; a key switch with a limited key; moai_key_register /
moai_key_forget; and the argument errors, each of which must leave the output untouched."""
import numpy as np
import pytest

import client_sampling as CS
import oracle as O

pytestmark = pytest.mark.gpu

MOAI_BITS = [51] + [46] * 20 + [51] * 14 + [58]  # include/test/test_full_scheme.hpp:356-378
KEY = bytes((7 * i + 3) & 0xFF for i in range(32))
SEED = bytes((11 * i + 5) & 0xFF for i in range(32))
EINVAL, ELOGIC, ERANGE = -1, -2, -3


def _setup(moai, logn, bits):
    primes = O.coeff_modulus_create(1 << logn, bits)
    return primes, O.Context(logn, primes), moai.Context(logn, primes)


def _secret(octx, rng, primes):
    s = rng.integers(-1, 2, size=octx.n)
    return octx.ntt(CS.to_rns(s, primes), len(primes))


def _rows(k, levels):
    return list(range(levels)) + [k - 1]


def _comparator(octx, key, seq, s_ntt, s2_ntt, levels):
    """[levels][2][levels+1][N]: the rows {0 .. levels-1, k-1} of the digits J < levels of the full key"""
    rows = _rows(octx.k, levels)
    return np.stack([CS.kswitch_digit(octx, key, seq, s_ntt, s2_ntt, J, rows=rows)[:, rows] for J in range(levels)])


def _trim_host(full, levels):
    k = full.shape[2]
    return np.ascontiguousarray(full[:levels][:, :, _rows(k, levels)])


def _keys(moai, octx, primes, seed):
    rng = np.random.default_rng(seed)
    s_ntt, s2_ntt = _secret(octx, rng, primes), _secret(octx, rng, primes)
    return s_ntt, s2_ntt, moai.DeviceBuffer.from_numpy(s_ntt), moai.DeviceBuffer.from_numpy(s2_ntt)


@pytest.mark.parametrize("levels", [1, 2])
def test_limited_keygen_small_n(moai, levels):
    """N = 2^4, the small-N transform path: against the comparator and against the trim of the full key"""
    primes, octx, ctx = _setup(moai, 4, [30, 31, 32])
    n, k, seq = octx.n, len(primes), 40
    s_ntt, s2_ntt, d_s, d_s2 = _keys(moai, octx, primes, levels)
    got = ctx.kswitch_keygen_limited(KEY, seq, d_s, d_s2, levels)
    assert got.n_words == levels * 2 * (levels + 1) * n
    got = got.to_numpy((levels, 2, levels + 1, n))
    assert (got == _comparator(octx, KEY, seq, s_ntt, s2_ntt, levels)).all()
    full = ctx.kswitch_keygen(KEY, seq, d_s, d_s2).to_numpy((k - 1, 2, k, n))
    assert (got == _trim_host(full, levels)).all()


@pytest.fixture(scope="module")
def mid(moai):
    """N = 2^12, bits [51, 46, 46, 58]: exact-FP64 rows and a 58-bit integer special prime together; the full key once"""
    primes, octx, ctx = _setup(moai, 12, [51, 46, 46, 58])
    s_ntt, s2_ntt, d_s, d_s2 = _keys(moai, octx, primes, 12)
    seq = (1 << 33) + 5
    d_full = ctx.kswitch_keygen(KEY, seq, d_s, d_s2)
    full = d_full.to_numpy((len(primes) - 1, 2, len(primes), octx.n))
    full.setflags(write=False)
    return dict(primes=primes, octx=octx, ctx=ctx, s_ntt=s_ntt, s2_ntt=s2_ntt, d_s=d_s, d_s2=d_s2, seq=seq, d_full=d_full, full=full)


@pytest.mark.parametrize("levels", [1, 2, 3])
def test_limited_keygen_mid(moai, mid, levels):
    ctx, octx, primes, seq = mid["ctx"], mid["octx"], mid["primes"], mid["seq"]
    n, k = octx.n, len(primes)
    shape = (levels, 2, levels + 1, n)
    d_got = ctx.kswitch_keygen_limited(KEY, seq, mid["d_s"], mid["d_s2"], levels)
    got = d_got.to_numpy(shape)
    assert (got == _comparator(octx, KEY, seq, mid["s_ntt"], mid["s2_ntt"], levels)).all()
    # word for word the device's own trim of the full key
    d_trim = ctx.key_trim(mid["d_full"], levels)
    assert (got == d_trim.to_numpy(shape)).all()
    ctx.key_forget(d_trim)
    assert (got == _trim_host(mid["full"], levels)).all()
    if levels == k - 1:
        assert (got.reshape(-1) == mid["full"].reshape(-1)).all()  # the full key, word for word
    # seeded with noise_key == seed, then expanded: the same words
    c0 = ctx.kswitch_keygen_limited_seeded(KEY, KEY, seq, mid["d_s"], mid["d_s2"], levels)
    assert (c0.to_numpy((levels, levels + 1, n)) == got[:, 0]).all()
    assert (ctx.expand_seeded_limited(KEY, seq, c0, levels).to_numpy(shape) == got).all()
    # two different keys: c0 changes, the uniform half is the seed's full-layout draw
    c0 = ctx.kswitch_keygen_limited_seeded(KEY, SEED, seq, mid["d_s"], mid["d_s2"], levels)
    key2 = ctx.expand_seeded_limited(SEED, seq, c0, levels).to_numpy(shape)
    rows = _rows(k, levels)
    for J in range(levels):
        a = CS.uniform(SEED, CS.nonce(CS.UNIFORM, seq + J), primes, n, rows)[rows]
        assert (key2[J, 1] == a).all(), J
    full2 = ctx.expand_seeded(SEED, seq, ctx.kswitch_keygen_seeded(KEY, SEED, seq, mid["d_s"], mid["d_s2"]), k - 1, k)
    assert (key2 == _trim_host(full2.to_numpy((k - 1, 2, k, n)), levels)).all()
    # the wire form: pack_rows under the limited row map, unpack_rows, expand
    packed = ctx.pack_rows(c0, levels, levels + 1, prime_index=rows)
    assert packed.n_words * 64 == levels * sum(int(primes[r]).bit_length() for r in rows) * n
    back, invalid = ctx.unpack_rows(packed, levels, levels + 1, prime_index=rows)
    assert invalid is False and (back.to_numpy() == c0.to_numpy()).all()
    assert (ctx.expand_seeded_limited(SEED, seq, back, levels).to_numpy(shape) == key2).all()


def test_limited_keygen_moai_chain(moai):
    """N = 2^16 on MOAI's 36 primes, levels 3, device against device: special prime index 35, so the special row's stream
    positions (block (35 N + i) / 4) lie far from the compact ones ((3 N + i) / 4)"""
    primes, octx, ctx = _setup(moai, 16, MOAI_BITS)
    n, k, levels, seq = octx.n, len(primes), 3, 1 << 40
    rng = np.random.default_rng(36)
    d_s = moai.DeviceBuffer.from_numpy(O.uniform_rns(rng, primes, (1,), n))
    d_s2 = moai.DeviceBuffer.from_numpy(O.uniform_rns(rng, primes, (1,), n))
    got = ctx.kswitch_keygen_limited(KEY, seq, d_s, d_s2, levels).to_numpy()
    d_full = ctx.kswitch_keygen(KEY, seq, d_s, d_s2)
    d_trim = ctx.key_trim(d_full, levels)
    want = d_trim.to_numpy()
    ctx.key_forget(d_trim)
    assert got.size == levels * 2 * (levels + 1) * n and (got == want).all()
    assert got.reshape(levels, 2, levels + 1, n)[:, :, levels].any()


@pytest.mark.parametrize("levels", [1, 2])
def test_switch_key_with_a_limited_key(moai, mid, levels):
    """at l <= levels the limited key gives the full key's bits; l = levels + 1 is MOAI_ERANGE and the operand stays"""
    ctx, octx, primes, seq = mid["ctx"], mid["octx"], mid["primes"], mid["seq"]
    n = octx.n
    d_lim = ctx.kswitch_keygen_limited(KEY, seq, mid["d_s"], mid["d_s2"], levels)
    rng = np.random.default_rng(levels)
    for L in range(1, levels + 1):
        ct = O.uniform_rns(rng, primes[:L], (2, 2), n)
        target = O.uniform_rns(rng, primes[:L], (2,), n)
        d_t = moai.DeviceBuffer.from_numpy(target)
        outs = []
        for dk in (d_lim, mid["d_full"]):
            d = moai.DeviceBuffer.from_numpy(ct)
            ctx.switch_key(d, d_t, dk, L, 2)
            outs.append(d.to_numpy(ct.shape))
        assert (outs[0] == outs[1]).all() and (outs[0] != ct).any(), L
    # hoisted rotations work through the recorded layout
    elt = ctx.galois_elt_from_step(1)
    assert (ctx.hoist_correction(d_lim, elt, levels).to_numpy() == ctx.hoist_correction(mid["d_full"], elt, levels).to_numpy()).all()
    L = levels + 1
    ct = O.uniform_rns(rng, primes[:L], (1, 2), n)
    d, d_t = moai.DeviceBuffer.from_numpy(ct), moai.DeviceBuffer.from_numpy(ct[0, 1])
    with pytest.raises(moai.hip.MoaiError) as e:
        ctx.switch_key(d, d_t, d_lim, L, 1)
    assert e.value.code == ERANGE
    assert (d.to_numpy(ct.shape) == ct).all()


def test_key_register_and_forget(moai, mid):
    """a block that arrived unseeded from elsewhere: registered it serves as a limited key, forgotten it is a plain pointer"""
    ctx, octx, primes = mid["ctx"], mid["octx"], mid["primes"]
    n, k, levels = octx.n, len(primes), 2
    lib = moai.hip.lib()
    block = moai.DeviceBuffer.from_numpy(_trim_host(mid["full"], levels))
    ctx.key_register(block, levels)
    ctx.key_register(block, levels)  # the same layout again is not an error
    assert lib.moai_key_register(ctx.h, block.ptr, 1) == EINVAL and b"recorded" in lib.moai_last_error()
    assert lib.moai_key_register(ctx.h, None, levels) == EINVAL
    assert lib.moai_key_register(None, block.ptr, levels) == EINVAL
    for bad in (0, k):
        assert lib.moai_key_register(ctx.h, block.ptr + 8, bad) == EINVAL and b"levels must lie in 1 .. 3" in lib.moai_last_error()
    rng = np.random.default_rng(3)
    ct = O.uniform_rns(rng, primes[:levels], (1, 2), n)
    d_t = moai.DeviceBuffer.from_numpy(ct[0, 1])
    a, b = moai.DeviceBuffer.from_numpy(ct), moai.DeviceBuffer.from_numpy(ct)
    ctx.switch_key(a, d_t, block, levels, 1)
    ctx.switch_key(b, d_t, mid["d_full"], levels, 1)
    assert (a.to_numpy() == b.to_numpy()).all()
    big = O.uniform_rns(rng, primes[:3], (1, 2), n)
    d_big = moai.DeviceBuffer.from_numpy(big)
    with pytest.raises(moai.hip.MoaiError) as e:
        ctx.switch_key(d_big, moai.DeviceBuffer.from_numpy(big[0, 1]), block, 3, 1)
    assert e.value.code == ERANGE
    ctx.key_forget(block)
    ctx.key_register(block, 1)  # after forget another layout may be recorded
    ctx.key_forget(block)
    # the buffers the recording entry points return forget their record when they are freed
    d_lim = ctx.kswitch_keygen_limited(KEY, 0, mid["d_s"], mid["d_s2"], 1)
    ptr = d_lim.ptr
    assert lib.moai_key_register(ctx.h, ptr, 2) == EINVAL
    d_lim.free()
    assert lib.moai_key_register(ctx.h, ptr, 2) == 0  # only the record: nothing reads the freed block
    assert lib.moai_key_forget(ctx.h, ptr) == 0


def test_argument_errors_leave_the_output_untouched(moai):
    logn = 10
    n = 1 << logn
    primes = O.coeff_modulus_create(n, [51, 46, 58])
    ctx = moai.Context(logn, primes)
    lib = moai.hip.lib()
    h = ctx.h
    d = moai.DeviceBuffer.from_numpy(np.zeros((3, n), dtype=np.uint64))
    out = moai.DeviceBuffer.from_numpy(np.zeros((2, 2, 3, n), dtype=np.uint64))
    c0 = moai.DeviceBuffer.from_numpy(np.zeros((2, 3, n), dtype=np.uint64))
    one = moai.Context(logn, primes[:1])
    gen, gens, exp = lib.moai_kswitch_keygen_limited, lib.moai_kswitch_keygen_limited_seeded, lib.moai_expand_seeded_limited
    table = [
        (gen, (None, KEY, 0, d.ptr, d.ptr, 2, out.ptr, None), EINVAL, b"null context"),
        (gen, (h, None, 0, d.ptr, d.ptr, 2, out.ptr, None), EINVAL, b"null key"),
        (gen, (h, KEY, 0, None, d.ptr, 2, out.ptr, None), EINVAL, b"null argument"),
        (gen, (h, KEY, 0, d.ptr, None, 2, out.ptr, None), EINVAL, b"null argument"),
        (gen, (h, KEY, 0, d.ptr, d.ptr, 2, None, None), EINVAL, b"null argument"),
        (gen, (h, KEY, 0, d.ptr, d.ptr, 0, out.ptr, None), EINVAL, b"levels must lie in 1 .. 2"),
        (gen, (h, KEY, 0, d.ptr, d.ptr, 3, out.ptr, None), EINVAL, b"levels must lie in 1 .. 2"),
        (gen, (h, KEY, 2**56 - 1, d.ptr, d.ptr, 2, out.ptr, None), EINVAL, b"2^56"),
        (gen, (one.h, KEY, 0, d.ptr, d.ptr, 1, out.ptr, None), ELOGIC, b"keyswitching"),
        (gens, (None, KEY, SEED, 0, d.ptr, d.ptr, 2, out.ptr, None), EINVAL, b"null context"),
        (gens, (h, None, SEED, 0, d.ptr, d.ptr, 2, out.ptr, None), EINVAL, b"null key"),
        (gens, (h, KEY, None, 0, d.ptr, d.ptr, 2, out.ptr, None), EINVAL, b"null seed"),
        (gens, (h, KEY, SEED, 0, d.ptr, None, 2, out.ptr, None), EINVAL, b"null argument"),
        (gens, (h, KEY, SEED, 0, d.ptr, d.ptr, 3, out.ptr, None), EINVAL, b"levels must lie in 1 .. 2"),
        (gens, (h, KEY, SEED, 2**56 - 1, d.ptr, d.ptr, 2, out.ptr, None), EINVAL, b"2^56"),
        (gens, (one.h, KEY, SEED, 0, d.ptr, d.ptr, 1, out.ptr, None), ELOGIC, b"keyswitching"),
        (exp, (None, SEED, 0, c0.ptr, 2, out.ptr, None), EINVAL, b"null context"),
        (exp, (h, None, 0, c0.ptr, 2, out.ptr, None), EINVAL, b"null key"),
        (exp, (h, SEED, 0, None, 2, out.ptr, None), EINVAL, b"null argument"),
        (exp, (h, SEED, 0, c0.ptr, 2, None, None), EINVAL, b"null argument"),
        (exp, (h, SEED, 0, c0.ptr, 0, out.ptr, None), EINVAL, b"levels must lie in 1 .. 2"),
        (exp, (h, SEED, 0, c0.ptr, 3, out.ptr, None), EINVAL, b"levels must lie in 1 .. 2"),
        (exp, (h, SEED, 2**56 - 1, c0.ptr, 2, out.ptr, None), EINVAL, b"2^56"),
        (exp, (h, SEED, 0, out.ptr + 8 * n, 2, out.ptr, None), EINVAL, b"c0 and out overlap"),
        (exp, (one.h, SEED, 0, c0.ptr, 1, out.ptr, None), ELOGIC, b"keyswitching"),
    ]
    for fn, args, rc, text in table:
        assert fn(*args) == rc and text in lib.moai_last_error(), (fn.__name__, args[1:], lib.moai_last_error())
        assert not out.to_numpy().any(), (fn.__name__, args[1:])
    # and no failing call recorded a layout for `out`
    assert lib.moai_key_register(h, out.ptr, 1) == 0 and lib.moai_key_forget(h, out.ptr) == 0
    with pytest.raises(moai.hip.MoaiError, match="levels must lie"):
        ctx.kswitch_keygen_limited(KEY, 0, d, d, 7)
