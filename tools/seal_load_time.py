#!/usr/bin/env python3
"""SEAL's seed expansion on the device (include/moai_hip.h, "SEAL's own format: the generator of seeded objects") at MOAI's
parameters (N = 2^16, the 36-prime chain), timed with the library's events on one stream, every comparison inside this one run:

1. moai_seal_sample_uniform for the seeded half of one fresh ciphertext (count 1, L = 35: 18 MB of output) and of one
   switching key (count 35, L = 36: 660 MB, past the 256 MiB cache), writing polynomial 1 of each [2][L][N] in place;
2. beside it moai_expand_seeded (this library's own seeded form, ChaCha20) on the same shapes, which also copies c0, and
3. moai_memcpy_d2d of the bytes moai_seal_sample_uniform writes.
Rates are achieved bytes per second of OUTPUT (the sampled polynomials).  Each figure is the median of 7 timed groups after 3
untimed runs; a group is as many back-to-back runs as take about 100 ms, and the kernels take turns group by group.
moai_seal_prng_bytes (the generator without the accept test and the reduction) runs on the same byte count too: what the
sampler adds to the hash is the difference.
Prints one JSON line; there is no pass / fail threshold."""
import hashlib
import json
import os
import sys

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
CHACHA_SEED = bytes(range(32, 64))
st = None  # the default stream


def group_ms(run, reps):
    e0, e1 = m.hip.Event(), m.hip.Event()
    e0.record(st)
    for _ in range(reps):
        run()
    e1.record(st)
    ctx.sync()
    return e1.elapsed_ms_since(e0) / reps


def timed(runs):
    """{name: (median, min, max milliseconds per run, runs per group)}: 7 rounds, each timing one group of every kernel in turn"""
    reps = {}
    for name, run in runs.items():
        for _ in range(3):
            run()
        ctx.sync()
        reps[name] = max(1, min(2000, int(100.0 / max(group_ms(run, 1), 1e-3))))
    groups = {name: [] for name in runs}
    for _ in range(7):
        for name, run in runs.items():
            groups[name].append(group_ms(run, reps[name]))
    return {name: (sorted(v)[3], min(v), max(v), reps[name]) for name, v in groups.items()}


def shape(name, count, L):
    LN = L * N
    out_bytes = count * LN * 8
    seeds = b"".join(hashlib.sha512(b"%d" % i).digest() for i in range(count))
    obj = m.DeviceBuffer(count * 2 * LN)
    c0 = m.DeviceBuffer(count * LN)
    flat = m.DeviceBuffer(count * LN)
    flag = m.DeviceBuffer(1)
    chk(lib.moai_memset_zero(obj.ptr, count * 2 * LN * 8, st))
    chk(lib.moai_memset_zero(c0.ptr, count * LN * 8, st))
    chk(lib.moai_memset_zero(flag.ptr, 8, st))
    runs = {
        "seal_sample_uniform": lambda: chk(lib.moai_seal_sample_uniform(ctx.h, seeds, obj.ptr + LN * 8, 2 * LN, count, L, None, flag.ptr, st)),
        "expand_seeded_chacha20": lambda: chk(lib.moai_expand_seeded(ctx.h, CHACHA_SEED, 0, c0.ptr, obj.ptr, count, L, None, st)),
        "copy_d2d": lambda: chk(lib.moai_memcpy_d2d(flat.ptr, c0.ptr, out_bytes, st)),
        "seal_prng_bytes": lambda: chk(lib.moai_seal_prng_bytes(ctx.h, seeds[:64], 0, out_bytes // 4096, flat.ptr, st)),
    }
    res = {"count": count, "L": L, "output_MB": round(out_bytes / 1e6, 1)}
    for key, (med, lo, hi, reps) in timed(runs).items():
        res[key] = {"ms": round(med, 4), "min_ms": round(lo, 4), "max_ms": round(hi, 4), "runs_per_group": reps,
                    "GBps_output": round(out_bytes / med / 1e6, 1)}
    word = int(flag.to_numpy()[0])
    res["rejected_words"] = word & 0xFFFFFFFF
    res["blake2xb_over_chacha20"] = round(res["seal_sample_uniform"]["ms"] / res["expand_seeded_chacha20"]["ms"], 2)
    res["blake2xb_over_copy"] = round(res["seal_sample_uniform"]["ms"] / res["copy_d2d"]["ms"], 2)
    res["sampler_over_generator"] = round(res["seal_sample_uniform"]["ms"] / res["seal_prng_bytes"]["ms"], 3)
    print(name, res, file=sys.stderr, flush=True)
    return res


out = {"N": N, "device": m.hip.device_info()[0]}
out["ciphertext"] = shape("ciphertext", 1, k - 1)
out["switching_key"] = shape("switching_key", k - 1, k)
out["galois_keys_31_s"] = round(31 * out["switching_key"]["seal_sample_uniform"]["ms"] / 1e3, 3)
print(json.dumps(out))
