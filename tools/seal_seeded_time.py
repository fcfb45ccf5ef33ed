#!/usr/bin/env python3
"""Three routes from fresh randomness to bytes a peer can load, at MOAI's parameters (N = 2^16, the 36-prime chain), for 32
ciphertexts at the top data level and for one switching key, every comparison inside this one run:

(a) the parent commit's route to SEAL's format: moai_*_seeded (ChaCha20 seed), moai_expand_seeded, then what save_seal does
    with the full object, one device-to-host copy of [2][L][N] per ciphertext or key digit into ordinary memory, each followed
    by a synchronise;
(b) the SEAL-seeded route: moai_*_seal_seeded (a from Blake2xb seeds, expanded on the device), then one copy of [L][N] per
    ciphertext or digit; the 64-byte seeds are host data;
(c) this library's own seeded format, for scale: moai_*_seeded, moai_pack_rows, ONE copy of the packed bytes.

The bytes are those the formats write (headers included).  Times are host-clock milliseconds around work that ends in a
synchronise, the median of REPS rounds after one warm-up round, the routes taking turns inside a round.  The share of (b)
spent in the Blake2xb expansion is moai_seal_sample_uniform over the same polynomials, timed with device events, over (b).
Nothing here passes or fails on a time.  Prints one table per object on stderr and one JSON line on stdout."""
import json
import os
import statistics
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
primes = O.coeff_modulus_create(N, [51] + [46] * 20 + [51] * 14 + [58])
k = len(primes)
ctx = m.Context(LOGN, primes)
NOISE_KEY = bytes(range(32))
SEED = bytes(range(32, 64))
REPS = 5
st = None  # the default stream
# SEAL's format (seal_shim/seal/moai_seal_format.h): SEALHeader 16, Ciphertext members 73, DynArray header 16 + size 8,
# UniformRandomGeneratorInfo 16 + 1 + 64; this library's own record header is 120 bytes
SEAL_FULL = lambda L: 16 + 73 + 24 + 2 * L * N * 8  # noqa: E731
SEAL_SEEDED = lambda L: 16 + 73 + 24 + L * N * 8 + 81  # noqa: E731


def seal_seeds(count, first):
    return b"".join(bytes((first + t + i) % 256 for i in range(64)) for t in range(count))


def rounds(routes):
    """{name: median ms} of REPS rounds in which the routes take turns, after one untimed round"""
    times = {name: [] for name in routes}
    for r in range(REPS + 1):
        for name, run in routes.items():
            ctx.sync()
            t0 = time.perf_counter()
            run()
            ctx.sync()
            if r:
                times[name].append((time.perf_counter() - t0) * 1e3)
    return {name: statistics.median(v) for name, v in times.items()}, {name: [round(x, 2) for x in v] for name, v in times.items()}


def events(run, reps=REPS, warm=1):
    """milliseconds per run by device events"""
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


def download_each(dev, host, count, words):
    for b in range(count):
        chk(lib.moai_memcpy_d2h(host[b].ctypes.data, dev.ptr + b * words * 8, words * 8, st))
        ctx.sync()


def table(title, med, nbytes, share):
    print(title, file=sys.stderr)
    print("  %-44s %12s %16s" % ("route", "median ms", "bytes"), file=sys.stderr)
    for name in med:
        print("  %-44s %12.2f %16d" % (name, med[name], nbytes[name]), file=sys.stderr)
    print("  Blake2xb expansion: %.2f ms, %.1f %% of (b)" % share, file=sys.stderr, flush=True)


out = {"N": N, "primes": k, "reps": REPS}
sk = ctx.sample_ternary(NOISE_KEY, 7, 1, k)
ctx.ntt_forward(sk, 1, k)
flags = m.DeviceBuffer(1)
chk(lib.moai_memset_zero(flags.ptr, 8, st))

# ---- 32 ciphertexts at the top data level ------------------------------------------------------------------------------------
B, L = 32, k - 1
LN = L * N
pw = ctx.packed_words(L)
plain = ctx.sample_uniform(SEED, 100, B, L)
seeds = seal_seeds(B, 0)
c0 = m.DeviceBuffer(B * LN)
full = m.DeviceBuffer(B * 2 * LN)
packed = m.DeviceBuffer(B * pw)
host_full = np.empty((B, 2 * LN), dtype=np.uint64)  # ordinary memory, as the caller's buffer is
host_c0 = np.empty((B, LN), dtype=np.uint64)
host_packed = np.empty(B * pw, dtype=np.uint64)


def ct_parent():
    chk(lib.moai_encrypt_symmetric_seeded(ctx.h, NOISE_KEY, SEED, 0, sk.ptr, plain.ptr, c0.ptr, B, L, None, st))
    chk(lib.moai_expand_seeded(ctx.h, SEED, 0, c0.ptr, full.ptr, B, L, None, st))
    download_each(full, host_full, B, 2 * LN)


def ct_seal_seeded():
    chk(lib.moai_encrypt_symmetric_seal_seeded(ctx.h, NOISE_KEY, seeds, 0, sk.ptr, plain.ptr, c0.ptr, B, L, None, flags.ptr, st))
    download_each(c0, host_c0, B, LN)


def ct_own():
    chk(lib.moai_encrypt_symmetric_seeded(ctx.h, NOISE_KEY, SEED, 0, sk.ptr, plain.ptr, c0.ptr, B, L, None, st))
    chk(lib.moai_pack_rows(ctx.h, c0.ptr, packed.ptr, B, L, None, st))
    chk(lib.moai_memcpy_d2h(host_packed.ctypes.data, packed.ptr, B * pw * 8, st))
    ctx.sync()


names = ("(a) ChaCha20 seed, expand, full SEAL format", "(b) SEAL seed, seeded SEAL format", "(c) own format, seeded and packed")
med, raw = rounds(dict(zip(names, (ct_parent, ct_seal_seeded, ct_own))))
t_exp = events(lambda: chk(lib.moai_seal_sample_uniform(ctx.h, seeds, full.ptr, LN, B, L, None, flags.ptr, st)))
nbytes = dict(zip(names, (B * SEAL_FULL(L), B * SEAL_SEEDED(L), B * (120 + pw * 8))))
table("32 fresh ciphertexts, L = %d" % L, med, nbytes, (t_exp, 100 * t_exp / med[names[1]]))
out["ciphertexts"] = {"count": B, "L": L, "median_ms": {n[:3]: round(v, 2) for n, v in med.items()},
                      "all_ms": {n[:3]: v for n, v in raw.items()}, "bytes": {n[:3]: v for n, v in nbytes.items()},
                      "blake2xb_expansion_ms": round(t_exp, 2), "blake2xb_share_of_b": round(t_exp / med[names[1]], 3)}
del plain, c0, full, packed, host_full, host_c0, host_packed

# ---- one switching key ---------------------------------------------------------------------------------------------------------
D = k - 1
kN = k * N
pwk = ctx.packed_words(k)
s2 = ctx.sample_ternary(NOISE_KEY, 8, 1, k)
ctx.ntt_forward(s2, 1, k)
seeds = seal_seeds(D, 64)
kc0 = m.DeviceBuffer(D * kN)
kfull = m.DeviceBuffer(D * 2 * kN)
kpacked = m.DeviceBuffer(D * pwk)
host_full = np.empty((D, 2 * kN), dtype=np.uint64)
host_c0 = np.empty((D, kN), dtype=np.uint64)
host_packed = np.empty(D * pwk, dtype=np.uint64)


def key_parent():
    chk(lib.moai_kswitch_keygen_seeded(ctx.h, NOISE_KEY, SEED, 0, sk.ptr, s2.ptr, kc0.ptr, st))
    chk(lib.moai_expand_seeded(ctx.h, SEED, 0, kc0.ptr, kfull.ptr, D, k, None, st))
    download_each(kfull, host_full, D, 2 * kN)


def key_seal_seeded():
    chk(lib.moai_kswitch_keygen_seal_seeded(ctx.h, NOISE_KEY, seeds, 0, sk.ptr, s2.ptr, kc0.ptr, flags.ptr, st))
    download_each(kc0, host_c0, D, kN)


def key_own():
    chk(lib.moai_kswitch_keygen_seeded(ctx.h, NOISE_KEY, SEED, 0, sk.ptr, s2.ptr, kc0.ptr, st))
    chk(lib.moai_pack_rows(ctx.h, kc0.ptr, kpacked.ptr, D, k, None, st))
    chk(lib.moai_memcpy_d2h(host_packed.ctypes.data, kpacked.ptr, D * pwk * 8, st))
    ctx.sync()


med, raw = rounds(dict(zip(names, (key_parent, key_seal_seeded, key_own))))
t_exp = events(lambda: chk(lib.moai_seal_sample_uniform(ctx.h, seeds, kfull.ptr, kN, D, k, None, flags.ptr, st)))
# a key set of one key: SEALHeader 16, parms_id 32, slot count 8, one digit count 8; own: set header 120, index 8, record
set_head = 16 + 32 + 8 + 8
nbytes = dict(zip(names, (set_head + D * SEAL_FULL(k), set_head + D * SEAL_SEEDED(k), 120 + 8 + 120 + D * pwk * 8)))
table("one switching key, %d digits of %d rows" % (D, k), med, nbytes, (t_exp, 100 * t_exp / med[names[1]]))
out["switching_key"] = {"digits": D, "rows": k, "median_ms": {n[:3]: round(v, 2) for n, v in med.items()},
                        "all_ms": {n[:3]: v for n, v in raw.items()}, "bytes": {n[:3]: v for n, v in nbytes.items()},
                        "blake2xb_expansion_ms": round(t_exp, 2), "blake2xb_share_of_b": round(t_exp / med[names[1]], 3)}
word = int(flags.to_numpy()[0])
assert word >> 32 == 0, "an expansion ran over its bound"
out["rejected_words"] = word & 0xFFFFFFFF
print(json.dumps(out))
