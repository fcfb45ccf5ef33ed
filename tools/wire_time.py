#!/usr/bin/env python3
"""The wire form (include/moai_hip.h, "wire form: seeded objects and bit-packed rows") at MOAI's parameters (N = 2^16, the
36-prime chain), timed with the library's events on one stream, every comparison inside this one run:

1. moai_pack_rows and moai_unpack_rows over 64 polynomials of the 35 data rows (1.17 GB unpacked, past the 256 MiB cache)
   beside moai_memcpy_d2d of the same unpacked bytes.  With X unpacked bytes the copy moves 2 X and each kernel 1.75 X, so the
   copy's time is the yardstick: GB/s of unpacked bytes and the ratio to the copy.
2. Saving a batch of 32 fresh ciphertexts: moai_encrypt_symmetric_seeded + moai_pack_rows + ONE device-to-host copy of the
   packed bytes into page-locked memory, against what the entry points of the parent commit offer for the same ciphertexts:
   moai_encrypt_symmetric of the batch, then one device-to-host copy of [2][L][N] per ciphertext into ordinary memory, each
   followed by a synchronise (Ciphertext::download).  Both sides encrypt symmetrically, so the difference is the wire form.
3. Loading one switching key: host-to-device copy of the seeded, packed key (500 MB, page-locked) + moai_unpack_rows +
   moai_expand_seeded, against the host-to-device copy of the raw 1.32 GB key from ordinary memory (Ciphertext::upload) and
   against generating it on the device (moai_kswitch_keygen).
Prints one JSON line."""
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
primes = O.coeff_modulus_create(N, [51] + [46] * 20 + [51] * 14 + [58])
k = len(primes)
ctx = m.Context(LOGN, primes)
NOISE_KEY = bytes(range(32))
SEED = bytes(range(32, 64))
st = None  # the default stream


def timed(run, reps, warm=2):
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


out = {"N": N}

# ---- 1. the two kernels beside a copy ------------------------------------------------------------------------------------
L, P = k - 1, 64
pw = ctx.packed_words(L)
src = ctx.sample_uniform(SEED, 1, P, L)  # canonical residues
dst = m.DeviceBuffer(P * L * N)
packed = m.DeviceBuffer(P * pw)
flag = m.DeviceBuffer(1)
chk(lib.moai_memset_zero(flag.ptr, 8, st))
X = P * L * N * 8
t_copy = timed(lambda: chk(lib.moai_memcpy_d2d(dst.ptr, src.ptr, X, st)), 10)
t_pack = timed(lambda: chk(lib.moai_pack_rows(ctx.h, src.ptr, packed.ptr, P, L, None, st)), 10)
t_unpack = timed(lambda: chk(lib.moai_unpack_rows(ctx.h, packed.ptr, dst.ptr, P, L, None, flag.ptr, st)), 10)
t_unpack_nf = timed(lambda: chk(lib.moai_unpack_rows(ctx.h, packed.ptr, dst.ptr, P, L, None, None, st)), 10)
t_copy2 = timed(lambda: chk(lib.moai_memcpy_d2d(dst.ptr, src.ptr, X, st)), 10)  # again, behind the kernels: the spread
assert flag.to_numpy()[0] == 0
out["kernels"] = {
    "unpacked_GB": round(X / 1e9, 3), "packed_fraction": round(pw * 8 / (L * N * 8), 4),
    "copy_d2d_ms": [round(t_copy, 3), round(t_copy2, 3)], "pack_ms": round(t_pack, 3), "unpack_ms": round(t_unpack, 3),
    "unpack_noflag_ms": round(t_unpack_nf, 3),
    "copy_GBps_unpacked": round(X / t_copy / 1e6, 1), "pack_GBps_unpacked": round(X / t_pack / 1e6, 1),
    "unpack_GBps_unpacked": round(X / t_unpack / 1e6, 1),
    "pack_over_copy": round(t_pack / min(t_copy, t_copy2), 3), "unpack_over_copy": round(t_unpack / min(t_copy, t_copy2), 3),
}
print("kernels", out["kernels"], file=sys.stderr, flush=True)
del src, dst, packed

# ---- 2. saving a batch of fresh ciphertexts --------------------------------------------------------------------------------
B = 32
sk = ctx.sample_ternary(NOISE_KEY, 7, 1, k)
ctx.ntt_forward(sk, 1, k)
plain = ctx.sample_uniform(SEED, 100, B, L)
c0 = m.DeviceBuffer(B * L * N)
pk = m.DeviceBuffer(B * pw)
full = m.DeviceBuffer(B * 2 * L * N)
host_packed = pinned(B * pw * 8)
host_raw = np.empty((B, 2 * L * N), dtype=np.uint64)  # ordinary memory, as std::vector is


def save_new():
    chk(lib.moai_encrypt_symmetric_seeded(ctx.h, NOISE_KEY, SEED, 0, sk.ptr, plain.ptr, c0.ptr, B, L, None, st))
    chk(lib.moai_pack_rows(ctx.h, c0.ptr, pk.ptr, B, L, None, st))
    chk(lib.moai_memcpy_d2h(host_packed, pk.ptr, B * pw * 8, st))
    ctx.sync()


def save_parent():
    chk(lib.moai_encrypt_symmetric(ctx.h, NOISE_KEY, 0, sk.ptr, plain.ptr, full.ptr, B, L, None, st))
    for b in range(B):
        chk(lib.moai_memcpy_d2h(host_raw[b].ctypes.data, full.ptr + b * 2 * L * N * 8, 2 * L * N * 8, st))
        ctx.sync()


t_new, t_old = wall(save_new, 3), wall(save_parent, 3)
out["save_batch"] = {"ciphertexts": B, "bytes_new": B * pw * 8, "bytes_parent": B * 2 * L * N * 8,
                     "seeded_packed_pinned_ms": round(t_new, 2), "parent_download_each_ms": round(t_old, 2),
                     "speedup": round(t_old / t_new, 2)}
print("save_batch", out["save_batch"], file=sys.stderr, flush=True)
del plain, c0, pk, full, host_raw

# ---- 3. loading one switching key ------------------------------------------------------------------------------------------
D = k - 1
pwk = ctx.packed_words(k)
s2 = ctx.sample_ternary(NOISE_KEY, 8, 1, k)
ctx.ntt_forward(s2, 1, k)
kc0 = ctx.kswitch_keygen_seeded(NOISE_KEY, SEED, 0, sk, s2)
kpacked = ctx.pack_rows(kc0, D, k)
host_key = pinned(D * pwk * 8)
chk(lib.moai_memcpy_d2h(host_key, kpacked.ptr, D * pwk * 8, st))
ctx.sync()
key = m.DeviceBuffer(D * 2 * k * N)
host_full = np.empty(D * 2 * k * N, dtype=np.uint64)
expanded = ctx.expand_seeded(SEED, 0, kc0, D, k)
chk(lib.moai_memcpy_d2h(host_full.ctypes.data, expanded.ptr, host_full.nbytes, st))
ctx.sync()
del expanded


def load_new():
    chk(lib.moai_memcpy_h2d(kpacked.ptr, host_key, D * pwk * 8, st))
    chk(lib.moai_unpack_rows(ctx.h, kpacked.ptr, kc0.ptr, D, k, None, flag.ptr, st))
    chk(lib.moai_expand_seeded(ctx.h, SEED, 0, kc0.ptr, key.ptr, D, k, None, st))
    ctx.sync()


def load_raw():
    chk(lib.moai_memcpy_h2d(key.ptr, host_full.ctypes.data, host_full.nbytes, st))
    ctx.sync()


def generate():
    chk(lib.moai_kswitch_keygen(ctx.h, NOISE_KEY, 0, sk.ptr, s2.ptr, key.ptr, st))
    ctx.sync()


t_load, t_raw, t_gen = wall(load_new, 3), wall(load_raw, 3), wall(generate, 3)
got = np.empty(host_full.size, dtype=np.uint64)
load_new()
chk(lib.moai_memcpy_d2h(got.ctypes.data, key.ptr, got.nbytes, st))
ctx.sync()
assert (got == host_full).all() and flag.to_numpy()[0] == 0, "the loaded key differs from the expanded one"
out["load_key"] = {"bytes_wire": D * pwk * 8, "bytes_raw": host_full.nbytes, "copy_unpack_expand_ms": round(t_load, 2),
                   "upload_raw_ms": round(t_raw, 2), "generate_on_device_ms": round(t_gen, 2)}
print("load_key", out["load_key"], file=sys.stderr, flush=True)
print(json.dumps(out))
