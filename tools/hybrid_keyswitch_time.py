#!/usr/bin/env python3
"""The hybrid key switch (include/moai_hip.h, "hybrid key switching") against the SEAL-style one at N = 2^16, inside one process
per cell with the legs taken in turns (A B C D A B C D ...), so that clock and thermal drift fall on all of them alike; per leg the
median of the rounds on device events and their spread, in ms per ciphertext:
  seal     moai_switch_key on MOAI's own 36-prime chain (35 data primes, one 58-bit special prime)
  hybrid_a moai_switch_key_hybrid on MOAI's 35 data primes plus alpha 60-bit special primes, alpha in {4, 6, 12}
for l in {35, 15} data primes x batch in {16, 64}, with the key bytes a switch at that level reads and the scratch bytes per leg.
Keys and operands are zero-filled or random blocks: their words do not change the time.

Without arguments this process starts one child per cell (`--cell L BATCH`), each under its own time limit, and stops at the first
that fails.  Prints a table, then one JSON line."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

ap = argparse.ArgumentParser()
ap.add_argument("--cell", nargs=2, type=int, metavar=("L", "BATCH"))
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--timeout", type=int, default=240, help="seconds per cell")
args = ap.parse_args()

N, LOGN = 1 << 16, 16
DATA_BITS = [51] + [46] * 20 + [51] * 14  # include/test/test_full_scheme.hpp:356-378
ALPHAS = (4, 6, 12)
CELLS = [(35, 16), (35, 64), (15, 16), (15, 64)]


def spread(v, per):
    return {"median_ms": round(statistics.median(v) / per, 4), "min_ms": round(min(v) / per, 4), "max_ms": round(max(v) / per, 4)}


def cell(L, B):
    import numpy as np

    import __graft_entry__ as g
    import oracle as O

    m = g.load_package()
    lib, chk = m.hip.lib(), m.hip._check
    st = None
    rng = np.random.default_rng(1)

    def zeros(words):
        b = m.DeviceBuffer(words)
        chk(lib.moai_memset_zero(b.ptr, words * 8, st))
        return b

    legs, info = {}, {}
    keep = []

    def leg(name, primes, alpha):
        ctx = m.Context(LOGN, primes)
        k = len(primes)
        one = m.DeviceBuffer.from_numpy(O.uniform_rns(rng, primes[:L], (3,), N))
        ct, target = m.DeviceBuffer(B * 2 * L * N), m.DeviceBuffer(B * L * N)
        for b in range(B):
            chk(lib.moai_memcpy_d2d(ct.ptr + b * 2 * L * N * 8, one.ptr, 2 * L * N * 8, st))
            chk(lib.moai_memcpy_d2d(target.ptr + b * L * N * 8, one.ptr + 2 * L * N * 8, L * N * 8, st))
        if alpha:
            digits = ctx.hybrid_digits(alpha, k - alpha)
            key = zeros(digits * 2 * k * N)
            beta = ctx.hybrid_digits(alpha, L)
            info[name] = {"key_bytes_read": beta * 2 * (L + alpha) * N * 8,
                          "scratch_bytes_per_ct": (beta * (L + alpha) + 4 * L + 4 * alpha) * N * 8}
            legs[name] = lambda: ctx.switch_key_hybrid(ct, target, key, L, alpha, B)
        else:
            key = zeros((k - 1) * 2 * k * N)
            info[name] = {"key_bytes_read": L * 2 * (L + 1) * N * 8}
            legs[name] = lambda: ctx.switch_key(ct, target, key, L, B)
        keep.append((ctx, one, ct, target, key))
        return ctx

    sync_ctx = leg("seal", O.coeff_modulus_create(N, DATA_BITS + [58]), 0)
    for alpha in ALPHAS:
        leg("hybrid_%d" % alpha, O.coeff_modulus_create(N, DATA_BITS + [60] * alpha), alpha)

    def timed(run, reps):
        e0, e1 = m.hip.Event(), m.hip.Event()
        e0.record(st)
        for _ in range(reps):
            run()
        e1.record(st)
        sync_ctx.sync()
        return e1.elapsed_ms_since(e0) / reps

    for run in legs.values():  # warm: arena growth, constant tables
        run()
    sync_ctx.sync()
    t = {name: [] for name in legs}
    for _ in range(args.rounds):
        for name, run in legs.items():
            t[name].append(timed(run, 2))
    out = {"l": L, "batch": B, "device": m.hip.device_info()[0]}
    for name in legs:
        out[name] = dict(spread(t[name], B), **info[name])
    print(json.dumps(out))


def main():
    results = []
    for L, B in CELLS:
        cmd = [sys.executable, os.path.abspath(__file__), "--cell", str(L), str(B), "--rounds", str(args.rounds)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout)
        if r.returncode != 0:
            raise SystemExit("cell l = %d, batch %d failed (%d): %s" % (L, B, r.returncode, (r.stdout + r.stderr)[-2000:]))
        row = json.loads(r.stdout.strip().splitlines()[-1])
        results.append(row)
        print("l = %2d  batch %2d  ms per ciphertext, median (min-max)" % (L, B))
        for name in ["seal"] + ["hybrid_%d" % a for a in ALPHAS]:
            v = row[name]
            print("  %-10s %8.4f (%.4f-%.4f)  x%.2f of seal   key read %7.1f MB%s" % (
                name, v["median_ms"], v["min_ms"], v["max_ms"], v["median_ms"] / row["seal"]["median_ms"], v["key_bytes_read"] / 1e6,
                "   scratch %6.1f MB per ciphertext" % (v["scratch_bytes_per_ct"] / 1e6) if "scratch_bytes_per_ct" in v else ""), flush=True)
    print(json.dumps(results))


if args.cell:
    cell(*args.cell)
else:
    main()
