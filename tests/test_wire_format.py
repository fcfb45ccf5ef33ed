"""CPU checks of the wire form: the new exports exist in the built library and are declared, cited, in include/moai_hip.h;
tests/wire_format.py (the comparator of tests/test_gpu_wire.py) round-trips every field width; the record header of
DESIGN.md section 5.0e written and parsed by a restatement that shares nothing with the C++ that implements it."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import wire_format as WF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPORTS = ["moai_packed_words", "moai_pack_rows", "moai_unpack_rows", "moai_encrypt_symmetric_seeded",
           "moai_kswitch_keygen_seeded", "moai_expand_seeded"]
MOAI_BITS = [51] + [46] * 20 + [51] * 14 + [58]  # include/test/test_full_scheme.hpp:356-378


def test_exports_exist_and_are_cited(moai):
    hdr = open(os.path.join(ROOT, "include", "moai_hip.h")).read()
    L = C.CDLL(moai.lib_path())
    for name in EXPORTS:
        assert hasattr(L, name), name
        assert name in moai.hip.SYMBOLS, name
        # the declaration, and directly above it a comment that names the reference lines it stands for
        m = re.search(r"\n(?:int|size_t) " + name + r"\(", hdr)
        assert m, name
        above = hdr[: m.start()].rstrip()
        assert above.endswith("*/"), name
        assert re.search(r"SEAL/[a-z/_]+\.(cpp|h):\d+", above[above.rindex("/*"):]), name
    assert "purpose 5" in hdr


def test_packed_words_arithmetic():
    assert WF.row_words(2, 3) == 1 and WF.row_words(64, 61) == 61 and WF.row_words(32, 61) == 31
    assert WF.row_words(1 << 16, 46) == 46 * 1024
    primes = [(1 << b) - 1 for b in MOAI_BITS]  # only the bit lengths matter
    n = 1 << 16
    # 1685 bits per coefficient over the 35 data primes, 1743 with the special prime (75.2 % / 75.7 % of 64 per row)
    assert WF.packed_words(n, primes[:35]) * 64 == 1685 * n
    assert WF.packed_words(n, primes) * 64 == 1743 * n
    # a seeded, packed fresh ciphertext: 13.8 MB, 37.6 % of the 36.7 MB resident; a seeded switching key: 500 MB, 37.8 %
    ct = WF.record_bytes(n, primes[:35], 2, True)
    assert ct == WF.HEADER_BYTES + 1685 * n // 8 and round(1000 * ct / (2 * 35 * n * 8)) == 376
    key = 35 * WF.record_bytes(n, primes, 2, True)
    assert round(1000 * key / (35 * 2 * 36 * n * 8)) == 378
    assert WF.record_bytes(n, primes[:35], 2, False) == WF.HEADER_BYTES + 2 * 1685 * n // 8


@pytest.mark.parametrize("b", range(2, 62))
def test_round_trip_every_width(b):
    rng = np.random.default_rng(b)
    q = (1 << b) - 1 if b > 2 else 3
    for logn in (1, 2, 5, 6, 7, 10):
        n = 1 << logn
        for row in (rng.integers(0, q, size=n, dtype=np.uint64), np.zeros(n, dtype=np.uint64), np.full(n, q - 1, dtype=np.uint64)):
            w = WF.pack_row(row, b)
            assert w.size == WF.row_words(n, b) == -(-n * b // 64)
            assert (WF.unpack_row(w, n, b) == row).all()
            # the definition, bit by bit: bit j of the stream is bit (j mod 64) of word j / 64
            big = sum(int(v) << (i * b) for i, v in enumerate(row))
            assert [int(x) for x in w] == [(big >> (64 * j)) & (2**64 - 1) for j in range(w.size)]


def test_round_trip_full_size():
    n = 1 << 16
    rng = np.random.default_rng(16)
    for b in (2, 46, 51, 58, 61):
        q = (1 << b) - 1 if b > 2 else 3
        row = rng.integers(0, q, size=n, dtype=np.uint64)
        row[:2] = (0, q - 1)
        w = WF.pack_row(row, b)
        assert w.size == n * b // 64
        assert (WF.unpack_row(w, n, b) == row).all()


def test_rows_start_on_word_boundaries_and_validity():
    primes = [1073741441, 2147483137, 13]  # 30, 31 and 4 bits
    n = 16
    rng = np.random.default_rng(3)
    polys = np.stack([[rng.integers(0, q, size=n, dtype=np.uint64) for q in primes] for _ in range(2)])
    w = WF.pack_rows(polys, primes)
    assert w.size == 2 * WF.packed_words(n, primes) == 2 * (8 + 8 + 1)
    assert (w[7] >> np.uint64(32)) == 0 and (w[15] >> np.uint64(48)) == 0  # the padding bits of a short row are zero
    back, invalid = WF.unpack_rows(w, 2, n, primes)
    assert (back == polys).all() and not invalid
    for bad in (13, 15):  # q itself, and 2^b - 1
        v = w.copy()
        v[16] = (v[16] & ~np.uint64(0xF0)) | np.uint64(bad << 4)  # field 1 of row 2
        got, invalid = WF.unpack_rows(v, 2, n, primes)
        assert invalid and got[0, 2, 1] == bad


def test_header_round_trip_and_rejections():
    parms_id = (0x0123456789ABCDEF, 2, 3, 2**64 - 1)
    seed = bytes(range(1, 33))
    total = WF.record_bytes(1 << 16, [(1 << b) - 1 for b in MOAI_BITS[:35]], 2, True)
    h = WF.write_header("ciphertext", WF.FLAG_SEEDED | WF.FLAG_NTT, 2, 1 << 16, 35, total, 2.0**40, parms_id, seed, seq=77)
    assert len(h) == WF.HEADER_BYTES == 120 and len(h) % 8 == 0
    # the layout DESIGN.md gives, byte by byte
    assert h[:8] == b"MOAIWIRE"
    assert [int.from_bytes(h[o:o + 4], "little") for o in (8, 12, 16, 20, 24, 28)] == [1, 1, 3, 2, 65536, 35]
    assert int.from_bytes(h[32:40], "little") == total
    assert np.frombuffer(h[40:48], dtype="<f8")[0] == 2.0**40
    assert tuple(int.from_bytes(h[48 + 8 * i:56 + 8 * i], "little") for i in range(4)) == parms_id
    assert int.from_bytes(h[80:88], "little") == 77 and h[88:120] == seed
    f = WF.read_header(h)
    assert f == {"kind": "ciphertext", "flags": 3, "count": 2, "n": 65536, "L": 35, "total_bytes": total, "scale": 2.0**40,
                 "parms_id": parms_id, "seq": 77, "seed": seed}
    with pytest.raises(ValueError, match="too small"):
        WF.read_header(h[:-1])
    with pytest.raises(ValueError, match="magic"):
        WF.read_header(b"X" + h[1:])
    with pytest.raises(ValueError, match="version"):
        WF.read_header(h[:8] + (2).to_bytes(4, "little") + h[12:])
    with pytest.raises(ValueError, match="kind"):
        WF.read_header(h[:12] + (10).to_bytes(4, "little") + h[16:])
    with pytest.raises(ValueError, match="flag"):
        WF.read_header(h[:16] + (4).to_bytes(4, "little") + h[20:])
    with pytest.raises(ValueError, match="seed"):
        WF.read_header(h[:16] + (2).to_bytes(4, "little") + h[20:])
    assert WF.read_header(WF.write_header("galois_keys", WF.FLAG_NTT, 70, 8, 36, 120, 1.0, (0, 0, 0, 0)))["seed"] == bytes(32)
    with pytest.raises(ValueError, match="2\\^56"):
        WF.read_header(h[:80] + (1 << 56).to_bytes(8, "little") + h[88:])


def test_public_seed_is_the_head_of_the_purpose_5_stream():
    import client_sampling as CS

    key = bytes((7 * i + 3) & 0xFF for i in range(32))
    s0, s1 = WF.public_seed(key, 0), WF.public_seed(key, 1)
    assert len(s0) == 32 and s0 != s1 and s0 != key
    blk = CS.chacha_blocks(key, (5 << 56) | 1, [0])[0]
    assert s1 == blk[:8].astype("<u4").tobytes()
