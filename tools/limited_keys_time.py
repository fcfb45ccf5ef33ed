#!/usr/bin/env python3
"""Switching keys limited to a chain index (include/moai_hip.h, "keys limited to a chain index") at MOAI's parameters
(N = 2^16, the 36-prime chain): a full key beside a key limited to chain index 14 (15 data primes, MOAI's 31 default rotation
keys) and to chain index 21 (22 data primes), every comparison inside this one run, for

1. generate (seeded): moai_kswitch_keygen_seeded against moai_kswitch_keygen_limited_seeded, device events on one stream;
2. pack and save: moai_pack_rows (the limited row map for a limited key) + ONE device-to-host copy into page-locked memory;
3. load and expand: host-to-device copy of the packed bytes + moai_unpack_rows + moai_expand_seeded / _limited.
2 and 3 synchronise inside and are timed by the host clock.  The byte counts are not measurements: they follow from the prime
bit lengths and are printed beside the times, with the resident bytes of MOAI's 31 default keys both ways.
The loaded limited key is compared, word for word, with the trim of the loaded full key.  Prints one JSON line."""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import __graft_entry__ as g  # noqa: E402
import oracle as O  # noqa: E402

m = g.load_package()
lib = m.hip.lib()
chk = m.hip._check
N, LOGN = 1 << 16, 16
BITS = [51] + [46] * 20 + [51] * 14 + [58]
primes = O.coeff_modulus_create(N, BITS)
k = len(primes)
ctx = m.Context(LOGN, primes)
NOISE_KEY = bytes(range(32))
SEED = bytes(range(32, 64))
st = None  # the default stream


def timed(run, reps, warm=1):
    """milliseconds per run: device events around `reps` runs after `warm` untimed ones"""
    for _ in range(warm):
        run()
    ctx.sync()
    e0, e1 = m.hip.Event(), m.hip.Event()
    e0.record(st)
    for _ in range(reps):
        run()
    e1.record(st)
    ctx.sync()
    return e1.elapsed_ms_since(e0) / reps


def wall(run, reps, warm=1):
    """milliseconds per run by the host clock, for paths that synchronise inside"""
    for _ in range(warm):
        run()
    ctx.sync()
    t0 = time.perf_counter()
    for _ in range(reps):
        run()
    ctx.sync()
    return (time.perf_counter() - t0) * 1e3 / reps


def pinned(nbytes):
    p = C.c_void_p()
    chk(lib.moai_host_malloc(C.byref(p), nbytes))
    return p


def rows_of(levels):
    return list(range(levels)) + [k - 1]


def wire_bytes(levels):
    """stored polynomials x bits per coefficient x N / 8, from the bit lengths alone"""
    return levels * sum(BITS[r] for r in rows_of(levels)) * N // 8


sk = ctx.sample_ternary(NOISE_KEY, 7, 1, k)
ctx.ntt_forward(sk, 1, k)
s2 = ctx.sample_ternary(NOISE_KEY, 8, 1, k)
ctx.ntt_forward(s2, 1, k)
flag = m.DeviceBuffer(1)
chk(lib.moai_memset_zero(flag.ptr, 8, st))
out = {"N": N, "k": k, "keys": {}}
loaded = {}

for name, levels in (("full", k - 1), ("chain_index_21", 22), ("chain_index_14", 15)):
    full = levels == k - 1
    L = levels + 1
    pidx = None if full else (C.c_uint32 * L)(*rows_of(levels))
    pw = ctx.packed_words(L, None if full else rows_of(levels))
    assert levels * pw * 8 == wire_bytes(levels)
    c0 = m.DeviceBuffer(levels * L * N)
    packed = m.DeviceBuffer(levels * pw)
    key = m.hip.KeyBuffer(ctx, levels * 2 * L * N)
    host = pinned(levels * pw * 8)

    def generate():
        if full:
            chk(lib.moai_kswitch_keygen_seeded(ctx.h, NOISE_KEY, SEED, 0, sk.ptr, s2.ptr, c0.ptr, st))
        else:
            chk(lib.moai_kswitch_keygen_limited_seeded(ctx.h, NOISE_KEY, SEED, 0, sk.ptr, s2.ptr, levels, c0.ptr, st))

    def save():
        chk(lib.moai_pack_rows(ctx.h, c0.ptr, packed.ptr, levels, L, pidx, st))
        chk(lib.moai_memcpy_d2h(host, packed.ptr, levels * pw * 8, st))
        ctx.sync()

    def load():
        chk(lib.moai_memcpy_h2d(packed.ptr, host, levels * pw * 8, st))
        chk(lib.moai_unpack_rows(ctx.h, packed.ptr, c0.ptr, levels, L, pidx, flag.ptr, st))
        if full:
            chk(lib.moai_expand_seeded(ctx.h, SEED, 0, c0.ptr, key.ptr, levels, L, None, st))
        else:
            chk(lib.moai_expand_seeded_limited(ctx.h, SEED, 0, c0.ptr, levels, key.ptr, st))
        ctx.sync()

    t_gen = timed(generate, 3)
    t_save = wall(save, 3)
    t_load = wall(load, 3)
    assert flag.to_numpy()[0] == 0
    out["keys"][name] = {
        "levels": levels, "row_encryptions": levels * L, "wire_bytes": levels * pw * 8, "resident_bytes": levels * 2 * L * N * 8,
        "generate_seeded_ms": round(t_gen, 2), "pack_save_ms": round(t_save, 2), "load_expand_ms": round(t_load, 2),
    }
    print(name, out["keys"][name], file=sys.stderr, flush=True)
    if full:
        loaded["full"] = key
    else:
        # the contract, at full size: the loaded limited key is the trim of the loaded full key
        trim = ctx.key_trim(loaded["full"], levels)
        same = bool((trim.to_numpy() == key.to_numpy()).all())
        ctx.key_forget(trim)
        assert same, "the limited key differs from the trim of the full key"
        del trim
    del c0, packed
    if not full:
        del key

f = out["keys"]["full"]
for name in ("chain_index_21", "chain_index_14"):
    r = out["keys"][name]
    r["wire_fraction"] = round(r["wire_bytes"] / f["wire_bytes"], 4)
    r["resident_fraction"] = round(r["resident_bytes"] / f["resident_bytes"], 4)
    for t in ("generate_seeded_ms", "pack_save_ms", "load_expand_ms"):
        r[t.replace("_ms", "_speedup")] = round(f[t] / r[t], 2)
# MOAI's 31 default rotation keys, all used at chain index <= 14 (Ct_ct_matrix_mul.hpp:29,95,112,147)
out["moai_31_default_keys"] = {
    "resident_bytes_full": 31 * f["resident_bytes"], "resident_bytes_limited": 31 * out["keys"]["chain_index_14"]["resident_bytes"],
    "wire_bytes_full": 31 * f["wire_bytes"], "wire_bytes_limited": 31 * out["keys"]["chain_index_14"]["wire_bytes"],
}
print(json.dumps(out))
