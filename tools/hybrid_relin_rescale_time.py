#!/usr/bin/env python3
"""relinearize + rescale over hybrid keys at N = 2^16: the merged call (include/moai_hip.h, "hybrid relinearize + rescale") against
the composition it replaces, inside one process per cell with the legs taken in turns (A B C A B C ...), so that clock and thermal
drift fall on all of them alike; per leg the median of the rounds on device events and their spread, in ms per ciphertext:
  a  moai_relinearize_hybrid + moai_rescale          MOAI's 35 data primes plus alpha 60-bit special primes
  b  moai_relinearize_rescale_hybrid                 the same chain and key
  c  moai_relinearize + moai_rescale                 MOAI's own 36-prime chain (35 data primes, one 58-bit special prime)
for l in {35, 15} data primes x alpha in {12, 6} x batch in {1, 16}.  Expected from the transform counts per ciphertext,
l + (beta (l + alpha) - l) + 2 (alpha + l) + 2 l for the composition and 2 l fewer merged: 305 -> 235 at l = 35, alpha = 12 and
138 -> 108 at l = 15, alpha = 12.  Keys are zero-filled and the operands random blocks: their words do not change the time.

Without arguments this process starts one child per cell (`--cell L ALPHA BATCH`), each under its own time limit, and stops at the
first that fails.  Prints a table, then one JSON line."""
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
ap.add_argument("--cell", nargs=3, type=int, metavar=("L", "ALPHA", "BATCH"))
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--timeout", type=int, default=180, help="seconds per cell")
args = ap.parse_args()

N, LOGN = 1 << 16, 16
DATA_BITS = [51] + [46] * 20 + [51] * 14  # include/test/test_full_scheme.hpp:356-378
CELLS = [(L, alpha, B) for L in (35, 15) for alpha in (12, 6) for B in (1, 16)]
LEGS = ("a", "b", "c")


def transforms(L, alpha, merged):
    beta = -(-L // alpha)
    return L + (beta * (L + alpha) - L) + 2 * (alpha + L) + 2 * L - (2 * L if merged else 0)


def spread(v, per):
    return {"median_ms": round(statistics.median(v) / per, 4), "min_ms": round(min(v) / per, 4), "max_ms": round(max(v) / per, 4)}


def cell(L, alpha, B):
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

    def operands(ctx, primes):
        one = m.DeviceBuffer.from_numpy(O.uniform_rns(rng, primes[:L], (3,), N))
        ct3 = m.DeviceBuffer(B * 3 * L * N)
        for b in range(B):
            chk(lib.moai_memcpy_d2d(ct3.ptr + b * 3 * L * N * 8, one.ptr, 3 * L * N * 8, st))
        return ct3, m.DeviceBuffer(B * 2 * L * N), m.DeviceBuffer(B * 2 * (L - 1) * N)

    hy_primes = O.coeff_modulus_create(N, DATA_BITS + [60] * alpha)
    hy = m.Context(LOGN, hy_primes)
    hkey = zeros(hy.hybrid_digits(alpha, len(hy_primes) - alpha) * 2 * len(hy_primes) * N)
    h3, hmid, hout = operands(hy, hy_primes)
    seal_primes = O.coeff_modulus_create(N, DATA_BITS + [58])
    seal = m.Context(LOGN, seal_primes)
    skey = zeros((len(seal_primes) - 1) * 2 * len(seal_primes) * N)
    s3, smid, sout = operands(seal, seal_primes)

    def leg_a():
        hy.relinearize_hybrid(h3, hkey, hmid, L, alpha, B)
        hy.rescale(hmid, hout, 2, L, B)

    def leg_b():
        hy.relinearize_rescale_hybrid(h3, hkey, hout, L, alpha, B)

    def leg_c():
        seal.relinearize(s3, skey, smid, L, B)
        seal.rescale(smid, sout, 2, L, B)

    legs = {"a": leg_a, "b": leg_b, "c": leg_c}

    def timed(run, reps):
        e0, e1 = m.hip.Event(), m.hip.Event()
        e0.record(st)
        for _ in range(reps):
            run()
        e1.record(st)
        hy.sync()
        return e1.elapsed_ms_since(e0) / reps

    for run in legs.values():  # warm: arena growth, constant tables
        run()
    hy.sync()
    t = {name: [] for name in legs}
    for _ in range(args.rounds):
        for name, run in legs.items():
            t[name].append(timed(run, 2))
    out = {"l": L, "alpha": alpha, "batch": B, "device": m.hip.device_info()[0],
           "transforms_a": transforms(L, alpha, False), "transforms_b": transforms(L, alpha, True)}
    for name in legs:
        out[name] = spread(t[name], B)
    print(json.dumps(out))


def main():
    results = []
    print("ms per ciphertext, median of %d rounds (min-max); transforms per ciphertext a -> b" % args.rounds)
    for L, alpha, B in CELLS:
        cmd = [sys.executable, os.path.abspath(__file__), "--cell", str(L), str(alpha), str(B), "--rounds", str(args.rounds)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout)
        if r.returncode != 0:
            raise SystemExit("cell l = %d, alpha = %d, batch %d failed (%d): %s" % (L, alpha, B, r.returncode, (r.stdout + r.stderr)[-2000:]))
        row = json.loads(r.stdout.strip().splitlines()[-1])
        results.append(row)
        print("l = %2d  alpha = %2d  batch %2d  transforms %d -> %d (x%.2f)" % (L, alpha, B, row["transforms_a"], row["transforms_b"],
                                                                              row["transforms_b"] / row["transforms_a"]))
        for name in LEGS:
            v = row[name]
            print("  %s %9.4f (%.4f-%.4f)" % (name, v["median_ms"], v["min_ms"], v["max_ms"]))
        print("  b/a %.3f   b/c %.3f" % (row["b"]["median_ms"] / row["a"]["median_ms"], row["b"]["median_ms"] / row["c"]["median_ms"]), flush=True)
    print(json.dumps(results))


if args.cell:
    cell(*args.cell)
else:
    main()
