#!/usr/bin/env python3
"""R rotations of ONE ciphertext over the hybrid key switch (include/moai_hip.h, "hoisted rotations over the hybrid key switch") at
N = 2^16, inside one process per cell with the legs taken in turns (a b4 b2 b1 c a b4 ...), so that clock and thermal drift fall on
all of them alike; per leg the median of the rounds on device events and their spread, in ms per rotation and ciphertext:
  a     R separate moai_apply_galois_hybrid calls, each on a device copy of the input (the copy is timed)
  b4/b2/b1  one moai_apply_galois_hybrid_hoisted call with MOAI_HYBRID_HOIST_NR = 4, 2, 1
  c     one moai_apply_galois_hoisted call with SEAL-style keys on MOAI's own 36-prime chain (35 data primes, one 58-bit special prime)
a and b run on MOAI's 35 data primes plus alpha 60-bit special primes.  Cells: l in {35, 15} x alpha in {12, 6} x R in {4, 8, 16} x
batch in {1, 16}.  Keys and corrections are zero-filled blocks, the inputs random: the words do not change the time, but a zero
coefficient in INTT(c1) would take the fallback, which every leg reports.

Without arguments this process starts one child per cell (`--cell L ALPHA R BATCH`), each under its own time limit, and stops at
the first that fails.  Prints a table, then one JSON line."""
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
ap.add_argument("--cell", nargs=4, type=int, metavar=("L", "ALPHA", "R", "BATCH"))
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--timeout", type=int, default=240, help="seconds per cell")
args = ap.parse_args()

N, LOGN = 1 << 16, 16
DATA_BITS = [51] + [46] * 20 + [51] * 14  # include/test/test_full_scheme.hpp:356-378
LEVELS = (35, 15)
ALPHAS = (12, 6)
ROTATIONS = (4, 8, 16)
BATCHES = (1, 16)
LEGS = ("a", "b4", "b2", "b1", "c")


def spread(v, per):
    return {"median_ms": round(statistics.median(v) / per, 4), "min_ms": round(min(v) / per, 4), "max_ms": round(max(v) / per, 4)}


def cell(L, alpha, R, B):
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
        """(input [B][2][L][N]: one random ciphertext B times, outputs [R][B][2][L][N], Galois elements)"""
        one = m.DeviceBuffer.from_numpy(O.uniform_rns(rng, primes[:L], (2,), N))
        ct = m.DeviceBuffer(B * 2 * L * N)
        for b in range(B):
            chk(lib.moai_memcpy_d2d(ct.ptr + b * 2 * L * N * 8, one.ptr, 2 * L * N * 8, st))
        return ct, m.DeviceBuffer(R * B * 2 * L * N), [ctx.galois_elt_from_step(s + 1) for s in range(R)]

    words = B * 2 * L * N
    fell_back = {}

    # a, b: the hybrid chain
    hp = O.coeff_modulus_create(N, DATA_BITS + [60] * alpha)
    hctx = m.Context(LOGN, hp)
    hk = len(hp)
    hct, hout, helts = operands(hctx, hp)
    hkeys = [zeros(hctx.hybrid_digits(alpha, hk - alpha) * 2 * hk * N) for _ in range(R)]
    hcorrs = [zeros(2 * (L + alpha) * N) for _ in range(R)]

    def separate():
        for r in range(R):
            chk(lib.moai_memcpy_d2d(hout.ptr + r * words * 8, hct.ptr, words * 8, st))
            hctx.apply_galois_hybrid(hout.ptr + r * words * 8, L, alpha, helts[r], hkeys[r], B)

    def hoisted(per_pass):
        def run():
            m.hip.set_tuning("MOAI_HYBRID_HOIST_NR", per_pass)
            fell_back["b%d" % per_pass] = hctx.apply_galois_hybrid_hoisted(hct, hout, L, alpha, helts, hkeys, hcorrs, B)
        return run

    # c: the SEAL-style chain
    sp = O.coeff_modulus_create(N, DATA_BITS + [58])
    sctx = m.Context(LOGN, sp)
    sk = len(sp)
    sct, sout, selts = operands(sctx, sp)
    skeys = [zeros((sk - 1) * 2 * sk * N) for _ in range(R)]
    scorrs = [zeros(2 * (L + 1) * N) for _ in range(R)]

    def seal_hoisted():
        fell_back["c"] = sctx.apply_galois_hoisted(sct, sout, L, selts, skeys, scorrs, B)

    legs = {"a": separate, "b4": hoisted(4), "b2": hoisted(2), "b1": hoisted(1), "c": seal_hoisted}

    def timed(run, reps):
        e0, e1 = m.hip.Event(), m.hip.Event()
        e0.record(st)
        for _ in range(reps):
            run()
        e1.record(st)
        hctx.sync()
        return e1.elapsed_ms_since(e0) / reps

    for run in legs.values():  # warm: arena growth, constant tables, Galois tables
        run()
    hctx.sync()
    t = {name: [] for name in legs}
    for _ in range(args.rounds):
        for name, run in legs.items():
            t[name].append(timed(run, 2))
    out = {"l": L, "alpha": alpha, "R": R, "batch": B, "device": m.hip.device_info()[0],
           "fell_back": sorted(name for name, fb in fell_back.items() if fb)}
    for name in legs:
        out[name] = spread(t[name], R * B)
    print(json.dumps(out))


def main():
    results = []
    for L in LEVELS:
        for alpha in ALPHAS:
            for B in BATCHES:
                for R in ROTATIONS:
                    cmd = [sys.executable, os.path.abspath(__file__), "--cell", str(L), str(alpha), str(R), str(B), "--rounds", str(args.rounds)]
                    r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout)
                    if r.returncode != 0:
                        raise SystemExit("cell l = %d, alpha = %d, R = %d, batch %d failed (%d): %s" % (
                            L, alpha, R, B, r.returncode, (r.stdout + r.stderr)[-2000:]))
                    row = json.loads(r.stdout.strip().splitlines()[-1])
                    results.append(row)
                    print("l = %2d  alpha = %2d  batch %2d  R = %2d   ms per rotation and ciphertext, median (min-max)%s" % (
                        L, alpha, B, R, "   FELL BACK: " + " ".join(row["fell_back"]) if row["fell_back"] else ""))
                    for name in LEGS:
                        v = row[name]
                        print("  %-3s %8.4f (%.4f-%.4f)  x%.2f of a" % (
                            name, v["median_ms"], v["min_ms"], v["max_ms"], v["median_ms"] / row["a"]["median_ms"]), flush=True)
    print(json.dumps(results))


if args.cell:
    cell(*args.cell)
else:
    main()
