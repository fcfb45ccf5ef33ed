"""Record kind 10 of the wire form, "limited switching key" (include/moai_hip.h, "keys limited to a
chain index"), restated in numpy and struct on top of tests/wire_format.py: the row map {0 .. levels-1, k-1}, the byte count
from the prime bit lengths, the header, and the checks a loader makes.  tests/test_wire_limited.py pins this module;
tests/test_gpu_limited_keys_shim.py reads the library's files with it.  CPU only: nothing here calls the library."""
import wire_format as WF

KIND_LIMITED = 10
KIND_NAME = "kswitch_key_limited"


def limited_rows(k, levels):
    """prime indices of the rows of a key limited to `levels` data primes: the special prime's row last"""
    assert 1 <= levels <= k - 1
    return list(range(levels)) + [k - 1]


def limited_primes(primes, levels):
    return [primes[i] for i in limited_rows(len(primes), levels)]


def limited_record_bytes(n, primes, levels, seeded):
    """bytes of one record of kind 10: 2 levels polynomials (levels stored when seeded) of levels + 1 packed rows"""
    return WF.record_bytes(n, limited_primes(primes, levels), 2 * levels, seeded)


def write_limited_header(n, primes, levels, parms_id, seed=None, seq=0):
    """the header of a record of kind 10 (NTT form; seeded when a seed is given); wire_format.write_header knows kinds 1 .. 9"""
    flags = WF.FLAG_NTT | (WF.FLAG_SEEDED if seed is not None else 0)
    total = limited_record_bytes(n, primes, levels, seed is not None)
    seed = bytes(32) if seed is None else bytes(seed)
    assert len(seed) == 32 and 0 <= seq < 1 << 56
    return WF.HEADER.pack(WF.MAGIC, WF.VERSION, KIND_LIMITED, flags, 2 * levels, n, levels + 1, total, 1.0,
                          *[int(x) for x in parms_id], seq, seed)


def read_header(buf):
    """wire_format.read_header, with kind 10 known"""
    if len(buf) >= WF.HEADER_BYTES and WF.HEADER.unpack_from(buf)[2] == KIND_LIMITED:
        nine = bytearray(buf[:WF.HEADER_BYTES])
        nine[12:16] = WF.KINDS["kswitch_key"].to_bytes(4, "little")
        h = WF.read_header(bytes(nine))
        h["kind"] = KIND_NAME
        return h
    return WF.read_header(buf)


def check_limited(h, n, primes, key_parms_id):
    """what load checks of a kind-10 header inside a key set over `primes` (k of them); returns levels.  ValueError("data is
    invalid") when levels lies outside 1 .. k-1 or count / L / total disagree"""
    k = len(primes)
    levels = h["L"] - 1
    ok = h["kind"] == KIND_NAME and h["n"] == n and tuple(h["parms_id"]) == tuple(key_parms_id) and 1 <= levels <= k - 1
    ok = ok and h["count"] == 2 * levels
    ok = ok and h["total_bytes"] == limited_record_bytes(n, primes, levels, bool(h["flags"] & WF.FLAG_SEEDED))
    if not ok:
        raise ValueError("data is invalid")
    return levels
