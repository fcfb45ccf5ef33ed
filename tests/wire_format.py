"""The wire form of include/moai_hip.h ("wire form: seeded objects and bit-packed rows") and DESIGN.md section 5.0e, restated
in numpy and struct: packed rows, the arithmetic of moai_packed_words, the record header and the purpose-5 public seed.
tests/test_wire_format.py pins this module; tests/test_gpu_wire.py compares the device with it.  CPU only: nothing here
calls the library."""
import struct

import numpy as np

import client_sampling as CS

PUBLIC_SEED = 5  # nonce purpose (client_sampling has 1 .. 4)

# ---- packed rows --------------------------------------------------------------------------------------------------------


def bit_length(q):
    return int(q).bit_length()


def row_words(n, b):
    """64-bit words of one packed row: ceil(n b / 64)"""
    return (n * b + 63) // 64


def packed_words(n, primes):
    """moai_packed_words: words of one packed polynomial with row r under primes[r]"""
    return sum(row_words(n, bit_length(q)) for q in primes)


def pack_row(row, b):
    """uint64 [ceil(n b / 64)]: coefficient i in bits [i b, (i + 1) b) of the little-endian bit stream"""
    row = np.asarray(row, dtype=np.uint64)
    n = row.size
    bits = ((row[:, None] >> np.arange(b, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(np.uint8).reshape(-1)
    stream = np.zeros(row_words(n, b) * 64, dtype=np.uint8)
    stream[: n * b] = bits
    return np.packbits(stream, bitorder="little").view("<u8").astype(np.uint64)


def unpack_row(words, n, b):
    """the inverse of pack_row: uint64 [n], every b-bit field as it stands (values >= q included)"""
    words = np.ascontiguousarray(words, dtype="<u8")
    assert words.size == row_words(n, b)
    bits = np.unpackbits(words.view(np.uint8), bitorder="little")[: n * b].reshape(n, b).astype(np.uint64)
    return (bits << np.arange(b, dtype=np.uint64)[None, :]).sum(axis=1, dtype=np.uint64)


def pack_rows(polys, primes):
    """polys [n_poly][L][n] -> uint64 [n_poly * packed_words]: rows in the order of the unpacked layout, each from a word boundary"""
    polys = np.asarray(polys, dtype=np.uint64)
    assert polys.ndim == 3 and polys.shape[1] == len(primes)
    out = [pack_row(polys[p, r], bit_length(q)) for p in range(polys.shape[0]) for r, q in enumerate(primes)]
    return np.concatenate(out) if out else np.zeros(0, dtype=np.uint64)


def unpack_rows(words, n_poly, n, primes):
    """(polys [n_poly][L][n], invalid): invalid is True when a field holds a value >= its row's prime"""
    words = np.asarray(words, dtype=np.uint64)
    out = np.empty((n_poly, len(primes), n), dtype=np.uint64)
    pos, invalid = 0, False
    for p in range(n_poly):
        for r, q in enumerate(primes):
            w = row_words(n, bit_length(q))
            out[p, r] = unpack_row(words[pos:pos + w], n, bit_length(q))
            invalid = invalid or bool((out[p, r] >= np.uint64(q)).any())
            pos += w
    assert pos == words.size
    return out, invalid


# ---- the public seed ----------------------------------------------------------------------------------------------------
def public_seed(noise_key, seq):
    """purpose 5: the first 32 bytes of the stream (noise key, 5 << 56 | seq)"""
    return CS.words(noise_key, CS.nonce(PUBLIC_SEED, seq), 0, 1)[:4].astype("<u8").tobytes()


# ---- the record header --------------------------------------------------------------------------------------------------
MAGIC = b"MOAIWIRE"
VERSION = 1
KINDS = {"ciphertext": 1, "plaintext": 2, "public_key": 3, "secret_key": 4, "kswitch_keys": 5, "relin_keys": 6,
         "galois_keys": 7, "encryption_parameters": 8, "kswitch_key": 9}
FLAG_SEEDED, FLAG_NTT = 1, 2
# magic, version, kind, flags, polynomial count, N, L, total bytes of the record, scale, parms_id[4], first sequence, seed[32]
HEADER = struct.Struct("<8sIIIIIIQd4QQ32s")
HEADER_BYTES = 120
assert HEADER.size == HEADER_BYTES


def write_header(kind, flags, count, n, L, total_bytes, scale, parms_id, seed=None, seq=0):
    seed = bytes(32) if seed is None else bytes(seed)
    assert len(seed) == 32 and (flags & FLAG_SEEDED or not (any(seed) or seq)) and 0 <= seq < 1 << 56
    return HEADER.pack(MAGIC, VERSION, KINDS[kind], flags, count, n, L, total_bytes, float(scale), *[int(x) for x in parms_id], seq, seed)


def read_header(buf):
    """dict of the fields; ValueError for a short buffer, an unknown magic, version, kind or flag"""
    if len(buf) < HEADER_BYTES:
        raise ValueError("buffer too small for a header")
    magic, version, kind, flags, count, n, L, total, scale, p0, p1, p2, p3, seq, seed = HEADER.unpack_from(buf)
    if magic != MAGIC:
        raise ValueError("unknown magic")
    if version != VERSION:
        raise ValueError("incompatible version")
    names = {v: k for k, v in KINDS.items()}
    if kind not in names:
        raise ValueError("unknown kind")
    if flags & ~(FLAG_SEEDED | FLAG_NTT):
        raise ValueError("unknown flag")
    if not flags & FLAG_SEEDED and (any(seed) or seq):
        raise ValueError("seed in an unseeded record")
    if seq >> 56:
        raise ValueError("sequence beyond 2^56")
    return {"kind": names[kind], "flags": flags, "count": count, "n": n, "L": L, "total_bytes": total, "scale": scale,
            "parms_id": (p0, p1, p2, p3), "seq": seq, "seed": seed}


def record_bytes(n, primes, count, seeded):
    """bytes of one record of `count` polynomials under `primes`: a seeded record carries every second polynomial as its seed"""
    stored = count // 2 if seeded else count
    return HEADER_BYTES + 8 * stored * packed_words(n, primes)
