"""csrc/wire.hip on its directed edges, bit for bit against tests/wire_format.py: what tests/test_gpu_wire.py leaves open.  Every
field width at the bit offsets of N = 2^12 and 2^16 (the reciprocal division, the three-field path and the field loop, the
clamped indices at the end of a row), input words with bits above the field, padding bits of a row's last word set, the
validity check in even and odd slots at both ends of a row, and a flag that a valid unpack leaves as it found it.  The inputs
come from tests/exchange_edge_cases.py and are pinned by tests/test_exchange_edges_cpu.py."""
import numpy as np
import pytest

import exchange_edge_cases as X
import oracle as O
import wire_format as WF

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("logn", [12, 16])
def test_every_field_width_at_large_offsets(moai, logn):
    n, primes = 1 << logn, X.width_primes(logn)
    L = len(primes)
    ctx = moai.Context(logn, primes)
    polys = X.canonical(primes, n, 1, np.random.default_rng(logn))
    want = WF.pack_rows(polys, primes)
    assert ctx.packed_words(L) == WF.packed_words(n, primes) == want.size
    packed = ctx.pack_rows(moai.DeviceBuffer.from_numpy(polys), 1, L)
    got = packed.to_numpy()
    assert np.array_equal(got, want), np.argwhere(got != want)[:4].tolist()
    for words in (packed, moai.DeviceBuffer.from_numpy(want)):
        back, invalid = ctx.unpack_rows(words, 1, L)
        assert invalid is False
        assert np.array_equal(back.to_numpy((1, L, n)), polys)


@pytest.mark.parametrize("logn", [6, 12])
def test_pack_ignores_bits_above_the_field(moai, logn):
    n, primes = 1 << logn, X.width_primes(logn)
    L = len(primes)
    ctx = moai.Context(logn, primes)
    rng = np.random.default_rng(60 + logn)
    polys = X.canonical(primes, n, 2, rng)
    want = WF.pack_rows(polys, primes)
    assert np.array_equal(ctx.pack_rows(moai.DeviceBuffer.from_numpy(polys), 2, L).to_numpy(), want)
    for garbage in (rng.integers(0, 1 << 63, size=polys.shape, dtype=np.uint64) * np.uint64(2) + np.uint64(1),
                    np.full(polys.shape, (1 << 64) - 1, dtype=np.uint64)):
        dirty = X.with_high_bits(polys, primes, garbage)
        assert not np.array_equal(dirty, polys)
        got = ctx.pack_rows(moai.DeviceBuffer.from_numpy(dirty), 2, L).to_numpy()
        assert np.array_equal(got, want), np.argwhere(got != want)[:4].tolist()


@pytest.mark.parametrize("logn", [1, 2, 3, 4, 5])
def test_unpack_ignores_padding_bits(moai, logn):
    n, primes = 1 << logn, X.width_primes(logn)
    L = len(primes)
    ctx = moai.Context(logn, primes)
    polys = X.canonical(primes, n, 2, np.random.default_rng(70 + logn))
    clean = WF.pack_rows(polys, primes)
    dirty = X.with_padding_ones(clean, n, primes, 2)
    assert X.padded_rows(n, primes) and not np.array_equal(dirty, clean)
    back, invalid = ctx.unpack_rows(moai.DeviceBuffer.from_numpy(dirty), 2, L)
    assert np.array_equal(back.to_numpy((2, L, n)), polys)
    assert invalid is False  # the padding does not reach the validity test either


@pytest.mark.parametrize("logn,bits", X.VALIDITY_SHAPES)
def test_validity_every_slot(moai, logn, bits):
    n, n_poly = 1 << logn, 3
    primes = O.coeff_modulus_create(n, bits)
    L = len(primes)
    ctx = moai.Context(logn, primes)
    polys = O.uniform_rns(np.random.default_rng(90 + logn), primes, (n_poly,), n)
    plants = X.validity_plants(logn, L, n_poly)
    # q_r - 1 at every one of the places at once: still valid
    edge = polys.copy()
    for p, r, i, _ in plants:
        edge[p, r, i] = primes[r] - 1
    out, invalid = ctx.unpack_rows(moai.DeviceBuffer.from_numpy(WF.pack_rows(edge, primes)), n_poly, L)
    assert invalid is False and np.array_equal(out.to_numpy((n_poly, L, n)), edge)
    for p, r, i, kind in plants:
        bad = polys.copy()
        bad[p, r, i] = X.bad_value(primes[r], kind)
        words = WF.pack_rows(bad, primes)
        assert WF.unpack_rows(words, n_poly, n, primes)[1]
        out, invalid = ctx.unpack_rows(moai.DeviceBuffer.from_numpy(words), n_poly, L)
        assert invalid is True, (p, r, i, kind)
        assert np.array_equal(out.to_numpy((n_poly, L, n)), bad), (p, r, i, kind)  # the data comes out as it stands


def test_flag_is_left_alone_when_valid(moai):
    """the flag is only ever set: the library neither clears it nor writes it on a valid unpack (Context.unpack_rows zeroes its
    own flag, so this goes through the C ABI)"""
    logn, n, n_poly = 12, 1 << 12, 2
    primes = O.coeff_modulus_create(n, [51, 46, 46, 58])
    L = len(primes)
    ctx = moai.Context(logn, primes)
    lib = moai.hip.lib()
    polys = O.uniform_rns(np.random.default_rng(12), primes, (n_poly,), n)
    out = moai.DeviceBuffer(n_poly * L * n)
    preset = 0xC0FFEE

    def unpack(data):
        flag = moai.DeviceBuffer.from_numpy(np.array([preset], dtype=np.uint64))  # the uint32 flag and an untouched word above it
        packed = moai.DeviceBuffer.from_numpy(WF.pack_rows(data, primes))
        assert lib.moai_unpack_rows(ctx.h, packed.ptr, out.ptr, n_poly, L, None, flag.ptr, None) == 0
        assert np.array_equal(out.to_numpy((n_poly, L, n)), data)
        return int(flag.to_numpy()[0])

    assert unpack(polys) == preset
    bad = polys.copy()
    bad[1, L - 1, 0] = primes[L - 1]
    word = unpack(bad)
    assert word & 0xFFFFFFFF != 0 and word >> 32 == 0
