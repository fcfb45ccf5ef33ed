"""CPU checks of switching keys limited to a chain index: the exports exist in the built library and are declared, cited, in
include/moai_hip.h and bound in hip.py; tests/wire_limited.py (record kind 10) gives the byte counts at MOAI's chain from the
prime bit lengths alone, round-trips its header and makes the loader's rejections."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import wire_format as WF
import wire_limited as WL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPORTS = ["moai_kswitch_keygen_limited", "moai_kswitch_keygen_limited_seeded", "moai_expand_seeded_limited", "moai_key_register"]
MOAI_BITS = [51] + [46] * 20 + [51] * 14 + [58]  # include/test/test_full_scheme.hpp:356-378
ID = (11, 22, 33, 44)


def test_exports_exist_and_are_cited(moai):
    hdr = open(os.path.join(ROOT, "include", "moai_hip.h")).read()
    L = C.CDLL(moai.lib_path())
    for name in EXPORTS:
        assert hasattr(L, name), name
        assert name in moai.hip.SYMBOLS, name
        m = re.search(r"\nint " + name + r"\(", hdr)
        assert m, name
        above = hdr[: m.start()].rstrip()
        assert above.endswith("*/"), name
        cited = above[above.rindex("/*"):]
        assert "SEAL/evaluator.cpp:2818,2831" in cited and re.search(r"SEAL/[a-z/_]+\.(cpp|h):\d+", cited), name
    for method in ("kswitch_keygen_limited", "kswitch_keygen_limited_seeded", "expand_seeded_limited", "key_register"):
        assert callable(getattr(moai.Context, method)), method


def test_null_context_is_refused_before_the_device(moai):
    lib = moai.hip.lib()
    key = bytes(32)
    assert lib.moai_kswitch_keygen_limited(None, key, 0, None, None, 1, None, None) == -1
    assert lib.moai_kswitch_keygen_limited_seeded(None, key, key, 0, None, None, 1, None, None) == -1
    assert lib.moai_expand_seeded_limited(None, key, 0, None, 1, None, None) == -1
    assert lib.moai_key_register(None, None, 1) == -1


def test_row_map():
    assert WL.limited_rows(36, 15) == list(range(15)) + [35]
    assert WL.limited_rows(4, 3) == [0, 1, 2, 3]  # levels == k-1: the full key's rows
    assert WL.limited_rows(2, 1) == [0, 1]
    for bad in (0, 36):
        with pytest.raises(AssertionError):
            WL.limited_rows(36, bad)


def test_byte_counts_at_moai_parameters():
    """15 and 22 levels (chain index 14 and 21) at N = 2^16 on MOAI's 36 primes, from the bit lengths alone"""
    n = 1 << 16
    primes = [(1 << b) - 1 for b in MOAI_BITS]  # only the bit lengths matter
    # chain index 14: rows 51 + 14 x 46 + 58 = 753 bits per coefficient, 15 stored polynomials when seeded
    assert WF.packed_words(n, WL.limited_primes(primes, 15)) * 64 == (51 + 14 * 46 + 58) * n == 753 * n
    k15 = WL.limited_record_bytes(n, primes, 15, True)
    assert k15 == WF.HEADER_BYTES + 15 * 753 * n // 8 == 120 + 92_528_640
    # chain index 21: 51 + 20 x 46 + 51 + 58 = 1080 bits, 22 stored polynomials
    assert WF.packed_words(n, WL.limited_primes(primes, 22)) * 64 == (51 + 20 * 46 + 51 + 58) * n == 1080 * n
    k22 = WL.limited_record_bytes(n, primes, 22, True)
    assert k22 == WF.HEADER_BYTES + 22 * 1080 * n // 8 == 120 + 194_641_920
    full = WF.record_bytes(n, primes, 2 * 35, True)
    assert full == WF.HEADER_BYTES + 35 * 1743 * n // 8 == 120 + 499_752_960
    assert round(1000 * k15 / full) == 185 and round(1000 * k22 / full) == 389
    # unseeded: twice the polynomials
    assert WL.limited_record_bytes(n, primes, 15, False) == WF.HEADER_BYTES + 2 * 15 * 753 * n // 8
    # levels == k-1 packs exactly the full key's rows
    assert WL.limited_record_bytes(n, primes, 35, True) == full
    # resident words of the trimmed layout, [levels][2][levels+1][N]: 19.0 % and 40.2 % of the full key
    assert round(1000 * 15 * 16 / (35 * 36)) == 190 and round(1000 * 22 * 23 / (35 * 36)) == 402
    # the generator's row encryptions: 15 x 16 against 35 x 36
    assert (15 * 16, 35 * 36) == (240, 1260)


def test_header_round_trip():
    n = 1 << 12
    primes = [(1 << b) - 1 for b in (60, 40, 40, 40, 60)]
    seed = bytes(range(32))
    for levels in (1, 2, 3, 4):
        for sd, seq in ((None, 0), (seed, (1 << 56) - 1)):
            buf = WL.write_limited_header(n, primes, levels, ID, sd, seq)
            assert len(buf) == WF.HEADER_BYTES
            h = WL.read_header(buf)
            assert h["kind"] == WL.KIND_NAME and h["count"] == 2 * levels and h["L"] == levels + 1 and h["n"] == n
            assert h["flags"] == WF.FLAG_NTT | (WF.FLAG_SEEDED if sd else 0) and h["seq"] == seq
            assert h["seed"] == (sd or bytes(32)) and h["parms_id"] == ID
            bits = sum(int(primes[r]).bit_length() for r in WL.limited_rows(5, levels))
            assert h["total_bytes"] == WF.HEADER_BYTES + (levels if sd else 2 * levels) * bits * n // 8
            assert WL.check_limited(h, n, primes, ID) == levels
    # the older kinds go through unchanged, and wire_format itself still does not know kind 10
    nine = WF.write_header("kswitch_key", WF.FLAG_NTT, 8, n, 5, WF.record_bytes(n, primes, 8, False), 1.0, ID)
    assert WL.read_header(nine) == WF.read_header(nine)
    with pytest.raises(ValueError, match="unknown kind"):
        WF.read_header(WL.write_limited_header(n, primes, 2, ID))
    # the header checks of every kind hold for kind 10 too
    buf = bytearray(WL.write_limited_header(n, primes, 2, ID))
    buf[16] |= 8
    with pytest.raises(ValueError, match="unknown flag"):
        WL.read_header(bytes(buf))


def _patched(buf, **fields):
    f = list(WF.HEADER.unpack(buf))
    names = ["magic", "version", "kind", "flags", "count", "n", "L", "total"]
    for name, value in fields.items():
        f[names.index(name)] = value
    return WF.HEADER.pack(*f)


def test_rejections():
    n = 1 << 12
    primes = [(1 << b) - 1 for b in (60, 40, 40, 40, 60)]
    k = len(primes)
    good = WL.write_limited_header(n, primes, 2, ID, bytes(range(32)), 7)
    assert WL.check_limited(WL.read_header(good), n, primes, ID) == 2
    bad = [
        _patched(good, L=1, count=0),            # levels = 0
        _patched(good, L=k + 1, count=2 * k),    # levels = k
        _patched(good, count=6),                 # count and L disagree
        _patched(good, L=4),                     # L and count disagree
        _patched(good, total=WF.HEADER.unpack(good)[7] + 8),  # a wrong total
        _patched(good, total=WL.limited_record_bytes(n, primes, 2, False)),  # the unseeded total in a seeded record
        _patched(good, n=n // 2),
    ]
    for buf in bad:
        with pytest.raises(ValueError, match="data is invalid"):
            WL.check_limited(WL.read_header(buf), n, primes, ID)
    with pytest.raises(ValueError, match="data is invalid"):
        WL.check_limited(WL.read_header(good), n, primes, (1, 2, 3, 4))
    # a residue >= its prime under the limited row map: the special prime's row is checked against the special prime
    sel = WL.limited_primes(primes, 2)
    polys = np.zeros((1, 3, n), dtype=np.uint64)
    polys[0, 2, 5] = sel[2] - 1
    assert not WF.unpack_rows(WF.pack_rows(polys, sel), 1, n, sel)[1]
    polys[0, 2, 5] = sel[2]
    assert WF.unpack_rows(WF.pack_rows(polys, sel), 1, n, sel)[1]
