"""Microsoft SEAL 4.1's serialized format and its Blake2xb sampler, restated in Python (pinned by tests/test_seal_format.py
against fixtures that SEAL itself wrote, tests/golden/seal_format/).  The device code (csrc/sealprng.hip) and the seal:: shim
(seal/moai_seal_format.h) are judged by this file.

  blake2b_compress        RFC 7693's F over a batch of states, in numpy uint64 (hashlib.blake2b refuses depth = 0, which
                          Blake2xb's output blocks use, so the compression is restated here)
  blake2b                 sequential BLAKE2b on top of it (tested against hashlib)
  prng_buffers            Blake2xbPRNG(seed): buffers c .. c + count - 1 of 4096 bytes (SEAL/randomgen.cpp:201-211,
                          SEAL/util/blake2xb.c:32-181)
  sample_poly_uniform     SEAL/util/rlwe.cpp:137-166 with a fresh generator, returning the residues and the rejections per row
  parms_id                SEAL/encryptionparams.cpp:124-158
  read_* / write_*        the byte format in compression mode none (SEAL/serialization.h:76-91 and the save_members of each type)
"""
import struct

import numpy as np

MAGIC = 0xA15E
HEADER_BYTES = 16
BUFFER_BYTES = 4096
PRNG_BLAKE2XB, PRNG_SHAKE256 = 1, 2
SCHEME_CKKS = 2

_IV = np.array([0x6A09E667F3BCC908, 0xBB67AE8584CAA73B, 0x3C6EF372FE94F82B, 0xA54FF53A5F1D36F1,
                0x510E527FADE682D1, 0x9B05688C2B3E6C1F, 0x1F83D9ABFB41BD6B, 0x5BE0CD19137E2179], dtype=np.uint64)
_SIGMA = [
    [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15],
    [14, 10, 4, 8, 9, 15, 13, 6, 1, 12, 0, 2, 11, 7, 5, 3],
    [11, 8, 12, 0, 5, 2, 15, 13, 10, 14, 3, 6, 7, 1, 9, 4],
    [7, 9, 3, 1, 13, 12, 11, 14, 2, 6, 5, 10, 4, 0, 15, 8],
    [9, 0, 5, 7, 2, 4, 10, 15, 14, 1, 11, 12, 6, 8, 3, 13],
    [2, 12, 6, 10, 0, 11, 8, 3, 4, 13, 7, 5, 15, 14, 1, 9],
    [12, 5, 1, 15, 14, 13, 4, 10, 0, 7, 6, 3, 9, 2, 8, 11],
    [13, 11, 7, 14, 12, 1, 3, 9, 5, 0, 15, 4, 8, 6, 2, 10],
    [6, 15, 14, 9, 11, 3, 0, 8, 12, 2, 13, 7, 1, 4, 10, 5],
    [10, 2, 8, 4, 7, 6, 1, 5, 15, 11, 9, 14, 3, 12, 13, 0],
]


def _rotr(x, r):
    return (x >> np.uint64(r)) | (x << np.uint64(64 - r))


def blake2b_compress(h, m, t, last):
    """h [8][B], m [16][B] uint64; t the byte counter (below 2^64) and `last` the finalisation flag, shared by the batch"""
    v = [h[i].copy() for i in range(8)] + [np.full_like(h[0], _IV[i]) for i in range(8)]
    v[12] = v[12] ^ np.uint64(t)
    if last:
        v[14] = ~v[14]

    def g(a, b, c, d, x, y):
        v[a] = v[a] + v[b] + x
        v[d] = _rotr(v[d] ^ v[a], 32)
        v[c] = v[c] + v[d]
        v[b] = _rotr(v[b] ^ v[c], 24)
        v[a] = v[a] + v[b] + y
        v[d] = _rotr(v[d] ^ v[a], 16)
        v[c] = v[c] + v[d]
        v[b] = _rotr(v[b] ^ v[c], 63)

    for r in range(12):
        s = _SIGMA[r % 10]
        g(0, 4, 8, 12, m[s[0]], m[s[1]])
        g(1, 5, 9, 13, m[s[2]], m[s[3]])
        g(2, 6, 10, 14, m[s[4]], m[s[5]])
        g(3, 7, 11, 15, m[s[6]], m[s[7]])
        g(0, 5, 10, 15, m[s[8]], m[s[9]])
        g(1, 6, 11, 12, m[s[10]], m[s[11]])
        g(2, 7, 8, 13, m[s[12]], m[s[13]])
        g(3, 4, 9, 14, m[s[14]], m[s[15]])
    return np.stack([h[i] ^ v[i] ^ v[i + 8] for i in range(8)])


def _param_words(digest_length, key_length=0, fanout=1, depth=1, leaf_length=0, node_offset=0, xof_length=0, node_depth=0,
                 inner_length=0):
    """the first 16 bytes of blake2b_param as two words (the reserved bytes, salt and personalisation are zero here)"""
    p = struct.pack("<BBBBIIIBB", digest_length, key_length, fanout, depth, leaf_length, node_offset, xof_length, node_depth,
                    inner_length) + bytes(46)
    return np.frombuffer(p, dtype="<u8").astype(np.uint64)


def _block(data):
    return np.frombuffer(data + bytes(128 - len(data)), dtype="<u8").astype(np.uint64).reshape(16, 1)


def blake2b(data, digest_size=64, key=b"", **param):
    """sequential BLAKE2b of one message"""
    h = (_IV ^ _param_words(digest_size, len(key), **param)).reshape(8, 1)
    if key:
        data = key + bytes(128 - len(key)) + data
    t = 0
    while len(data) - t > 128:
        h = blake2b_compress(h, _block(data[t:t + 128]), t + 128, False)
        t += 128
    h = blake2b_compress(h, _block(data[t:]), len(data), True)
    return h[:, 0].astype("<u8").tobytes()[:digest_size]


def prng_root(seed, counter):
    """the 64-byte root hash of buffer `counter`: two compressions (the padded key block, then the counter)"""
    assert len(seed) == 64
    return blake2b(struct.pack("<Q", counter), 64, seed, xof_length=BUFFER_BYTES)


def prng_buffers(seed, first, count):
    """buffers first .. first + count - 1 of Blake2xbPRNG(seed) as bytes"""
    if count == 0:
        return b""
    roots = np.stack([np.frombuffer(prng_root(seed, first + c), dtype="<u8").astype(np.uint64) for c in range(count)])  # [count][8]
    m = np.zeros((16, count, 64), dtype=np.uint64)
    m[:8] = roots.T[:, :, None]
    h = np.empty((8, count, 64), dtype=np.uint64)
    for i in range(64):
        h[:, :, i] = (_IV ^ _param_words(64, 0, 0, 0, 64, i, BUFFER_BYTES, 0, 64))[:, None]
    out = blake2b_compress(h.reshape(8, -1), m.reshape(16, -1), 64, True).reshape(8, count, 64)
    return np.ascontiguousarray(out.transpose(1, 2, 0)).astype("<u8").tobytes()


def max_multiple(q):
    """SEAL/util/rlwe.cpp:154: words at or above it are rejected"""
    top = (1 << 64) - 1
    return top - top % q - 1


class _Stream:
    def __init__(self, seed):
        self.seed, self.words, self.pos, self.next = seed, np.empty(0, dtype=np.uint64), 0, 0

    def take(self, count):
        while self.pos + count > self.words.size:
            more = max(1, -(-(self.pos + count - self.words.size) * 8 // BUFFER_BYTES))
            fresh = np.frombuffer(prng_buffers(self.seed, self.next, more), dtype="<u8").astype(np.uint64)
            self.words = np.concatenate([self.words[self.pos:], fresh])
            self.pos, self.next = 0, self.next + more
        out = self.words[self.pos:self.pos + count]
        self.pos += count
        return out


def sample_poly_uniform(seed, primes, n):
    """-> (residues [L][n] uint64, rejections per row, counting a replacement word that is itself rejected)"""
    s = _Stream(seed)
    L = len(primes)
    poly = s.take(L * n).reshape(L, n).copy()
    rejected = []
    for j, q in enumerate(primes):
        mm, count = max_multiple(int(q)), 0
        for i in np.nonzero(poly[j] >= np.uint64(mm))[0]:
            while int(poly[j, i]) >= mm:
                count += 1
                poly[j, i] = s.take(1)[0]
        poly[j] %= np.uint64(q)
        rejected.append(count)
    return poly, rejected


def parms_id(n, primes, scheme=SCHEME_CKKS, plain_modulus=0):
    data = struct.pack("<%dQ" % (3 + len(primes)), scheme, n, *[int(q) for q in primes], plain_modulus)
    return struct.unpack("<4Q", blake2b(data, 32))


# ---- the byte format, compression mode none ----------------------------------------------------------------------------------
def write_header(total, version=(4, 1), mode=0):
    return struct.pack("<HBBBBHQ", MAGIC, HEADER_BYTES, version[0], version[1], mode, 0, total)


def read_header(data, pos=0):
    magic, size, major, minor, mode, reserved, total = struct.unpack_from("<HBBBBHQ", data, pos)
    if magic != MAGIC or size != HEADER_BYTES:
        raise ValueError("loaded SEALHeader is invalid")
    if major != 4:
        raise ValueError("incompatible version")
    if mode != 0:
        raise ValueError("loaded SEALHeader is invalid")  # a build without zlib / zstd: SEAL/serialization.h:182-190
    return {"version": (major, minor), "total": total}


def _wrap(body):
    return write_header(HEADER_BYTES + len(body)) + body


def _open(data, pos):
    """-> (position of the members, position of the object's end)"""
    h = read_header(data, pos)
    if pos + h["total"] > len(data):
        raise ValueError("I/O error")
    return pos + HEADER_BYTES, pos + h["total"]


def write_dyn_array(words):
    words = np.ascontiguousarray(words, dtype="<u8").reshape(-1)
    return _wrap(struct.pack("<Q", words.size) + words.tobytes())


def read_dyn_array(data, pos):
    at, end = _open(data, pos)
    (size,) = struct.unpack_from("<Q", data, at)
    assert end == at + 8 + 8 * size
    return np.frombuffer(data, dtype="<u8", count=size, offset=at + 8).astype(np.uint64), end


def write_modulus(q):
    return _wrap(struct.pack("<Q", int(q)))


def write_parms(n, primes, scheme=SCHEME_CKKS, plain_modulus=0):
    body = struct.pack("<BQQ", scheme, n, len(primes)) + b"".join(write_modulus(q) for q in primes) + write_modulus(plain_modulus)
    return _wrap(body)


def read_parms(data, pos=0):
    at, end = _open(data, pos)
    scheme, n, L = struct.unpack_from("<BQQ", data, at)
    at += 17
    mods = []
    for _ in range(L + 1):
        a, e = _open(data, at)
        mods.append(struct.unpack_from("<Q", data, a)[0])
        at = e
    assert at == end
    return {"scheme": scheme, "n": n, "primes": mods[:-1], "plain_modulus": mods[-1], "end": end}


def write_prng_info(seed, kind=PRNG_BLAKE2XB):
    return _wrap(bytes([kind]) + seed)


def write_plaintext(pid, scale, words):
    """Plaintext and SecretKey (SEAL/plaintext.cpp:205-225, SEAL/secretkey.h)"""
    words = np.asarray(words).reshape(-1)
    return _wrap(struct.pack("<4QQd", *pid, words.size, scale) + write_dyn_array(words))


def read_plaintext(data, pos=0):
    at, end = _open(data, pos)
    f = struct.unpack_from("<4QQd", data, at)
    words, e = read_dyn_array(data, at + 48)
    assert e == end and words.size == f[4]
    return {"parms_id": f[:4], "scale": f[5], "data": words, "end": end}


def write_ciphertext(pid, ntt, size, n, L, scale, words, seed=None, correction_factor=1):
    """Ciphertext and PublicKey (SEAL/ciphertext.cpp:190-247); seeded: `words` is polynomial 0 alone"""
    body = struct.pack("<4QBQQQdQ", *pid, int(ntt), size, n, L, scale, correction_factor) + write_dyn_array(words)
    if seed is not None:
        body += write_prng_info(seed)
    return _wrap(body)


def read_ciphertext(data, pos=0):
    at, end = _open(data, pos)
    f = struct.unpack_from("<4QBQQQdQ", data, at)
    out = {"parms_id": f[:4], "ntt": bool(f[4]), "size": f[5], "n": f[6], "L": f[7], "scale": f[8], "correction_factor": f[9],
           "seed": None, "end": end}
    words, at = read_dyn_array(data, at + 73)
    if words.size == out["n"] * out["L"] and out["size"] == 2:
        a, e = _open(data, at)
        assert e == end == a + 65
        out["prng_type"], out["seed"] = data[a], bytes(data[a + 1:a + 65])
        out["data"] = words.reshape(1, out["L"], out["n"])
    else:
        assert at == end
        out["data"] = words.reshape(out["size"], out["L"], out["n"])
    return out


def expand_ciphertext(c, primes):
    """a seeded ciphertext as SEAL's load leaves it -> (data [2][L][n], rejections per row)"""
    a, rejected = sample_poly_uniform(c["seed"], primes[:c["L"]], c["n"])
    return np.stack([c["data"][0], a]), rejected


def write_kswitch_keys(pid, keys):
    """keys: per slot a list of digits (possibly empty), each the bytes of a PublicKey (SEAL/kswitchkeys.cpp:45-84)"""
    body = struct.pack("<4QQ", *pid, len(keys))
    for digits in keys:
        body += struct.pack("<Q", len(digits)) + b"".join(digits)
    return _wrap(body)


def read_kswitch_keys(data, pos=0):
    at, end = _open(data, pos)
    f = struct.unpack_from("<4QQ", data, at)
    at += 40
    keys = []
    for _ in range(f[4]):
        (dim2,) = struct.unpack_from("<Q", data, at)
        at += 8
        digits = []
        for _ in range(dim2):
            digits.append(read_ciphertext(data, at))
            at = digits[-1]["end"]
        keys.append(digits)
    assert at == end
    return {"parms_id": f[:4], "keys": keys, "end": end}
