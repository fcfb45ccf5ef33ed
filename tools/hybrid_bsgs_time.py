#!/usr/bin/env python3
"""One whole baby-step / giant-step linear transform of ONE ciphertext -- n_giant giant steps over the same R baby steps -- at
N = 2^16 (include/moai_hip.h, "giant steps summed in the extended basis"), inside one process per cell with the legs taken in turns
(a b c a b ...), so that clock and thermal drift fall on all of them alike; per leg the median of the rounds on device events and
their spread, in ms per ciphertext (the whole transform of it):
  a     one moai_hybrid_rotate_pt_dot call with n_giant outputs, one moai_apply_galois_hybrid call per giant step, n_giant - 1
        additions: the composition the library offered before moai_hybrid_bsgs_dot
  b     one moai_hybrid_bsgs_dot call
  c     the SEAL-style hoisted composition on MOAI's own 36-prime chain (35 data primes, one 58-bit special prime): one
        moai_apply_galois_hoisted call, n_giant moai_ct_pt_dot calls over the R rotated ciphertexts, one moai_apply_galois call per
        giant step, n_giant - 1 additions
a and b run on MOAI's 35 data primes plus alpha 60-bit special primes.  Cells: l in {35, 15} x alpha in {12, 6} x batch in {1, 16} x
(R, n_giant) in {(16, 4), (8, 8)}; every term is present and no element is 1 on either side.  Keys, corrections and plaintexts are
zero-filled blocks, the inputs random: the words do not change the time, but a zero coefficient in INTT(c1) would take the
fallback, which every leg reports.

Without arguments this process starts one child per cell (`--cell L ALPHA R NGIANT BATCH`), each under its own time limit, and stops
at the first that fails.  Prints a table, then one JSON line."""
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
ap.add_argument("--cell", nargs=5, type=int, metavar=("L", "ALPHA", "R", "NGIANT", "BATCH"))
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--timeout", type=int, default=240, help="seconds per cell")
args = ap.parse_args()

N, LOGN = 1 << 16, 16
DATA_BITS = [51] + [46] * 20 + [51] * 14  # include/test/test_full_scheme.hpp:356-378
LEVELS = (35, 15)
ALPHAS = (12, 6)
BATCHES = (1, 16)
SHAPES = ((16, 4), (8, 8))  # (R, n_giant)
LEGS = ("a", "b", "c")


def spread(v, per):
    return {"median_ms": round(statistics.median(v) / per, 4), "min_ms": round(min(v) / per, 4), "max_ms": round(max(v) / per, 4)}


def cell(L, alpha, R, G, B):
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

    words = B * 2 * L * N

    def operands(ctx, primes):
        """(input [B][2][L][N]: one random ciphertext B times, inner sums [G][B][2][L][N], baby elements, giant elements)"""
        one = m.DeviceBuffer.from_numpy(O.uniform_rns(rng, primes[:L], (2,), N))
        ct = m.DeviceBuffer(words)
        for b in range(B):
            chk(lib.moai_memcpy_d2d(ct.ptr + b * 2 * L * N * 8, one.ptr, 2 * L * N * 8, st))
        baby = [ctx.galois_elt_from_step(s + 1) for s in range(R)]
        giant = [ctx.galois_elt_from_step((s + 1) * (R + 1)) for s in range(G)]
        return ct, m.DeviceBuffer(G * words), baby, giant

    fell_back = {}

    def giant_steps_and_sum(ctx, rotate, sums, giant, keys):
        """every inner sum rotated in place by its giant step, then added up into the first"""
        for o in range(G):
            rotate(sums.ptr + o * words * 8, giant[o], keys[o])
        for o in range(1, G):
            ctx.add(sums.ptr, sums.ptr + o * words * 8, sums.ptr, B * 2, L)

    # a, b: the hybrid chain
    hp = O.coeff_modulus_create(N, DATA_BITS + [60] * alpha)
    hctx = m.Context(LOGN, hp)
    hk = len(hp)
    hct, hsums, hbaby, hgiant = operands(hctx, hp)
    hout = m.DeviceBuffer(words)
    key_words = hctx.hybrid_digits(alpha, hk - alpha) * 2 * hk * N
    hkeys = [zeros(key_words) for _ in range(R)]
    hgkeys = [zeros(key_words) for _ in range(G)]
    hcorrs = [zeros(2 * (L + alpha) * N) for _ in range(R)]
    eplain = zeros(G * R * (L + alpha) * N)                                         # [G * R][L + alpha][N]
    eplains = [[eplain.ptr + (o * R + r) * (L + alpha) * N * 8 for r in range(R)] for o in range(G)]

    def composed():
        fell_back["a"] = hctx.hybrid_rotate_pt_dot(hct, hsums, L, alpha, hbaby, hkeys, hcorrs, eplains, B)
        giant_steps_and_sum(hctx, lambda ct, elt, key: hctx.apply_galois_hybrid(ct, L, alpha, elt, key, B), hsums, hgiant, hgkeys)

    def fused():
        fell_back["b"] = hctx.hybrid_bsgs_dot(hct, hout, L, alpha, hbaby, hkeys, hcorrs, hgiant, hgkeys, eplains, B)

    # c: the SEAL-style chain
    sp = O.coeff_modulus_create(N, DATA_BITS + [58])
    sctx = m.Context(LOGN, sp)
    sk = len(sp)
    sct, ssums, sbaby, sgiant = operands(sctx, sp)
    srot = m.DeviceBuffer(R * words)
    skeys = [zeros((sk - 1) * 2 * sk * N) for _ in range(R)]
    sgkeys = [zeros((sk - 1) * 2 * sk * N) for _ in range(G)]
    scorrs = [zeros(2 * (L + 1) * N) for _ in range(R)]
    splains = zeros(G * R * L * N)
    x_index = list(range(R))

    def seal_composed():
        fell_back["c"] = sctx.apply_galois_hoisted(sct, srot, L, sbaby, skeys, scorrs, B)
        for o in range(G):
            sctx.ct_pt_dot(srot, splains, ssums.ptr + o * words * 8, x_index, [o * R + r for r in range(R)], B * 2, L)
        giant_steps_and_sum(sctx, lambda ct, elt, key: sctx.apply_galois(ct, L, elt, key, B), ssums, sgiant, sgkeys)

    legs = {"a": composed, "b": fused, "c": seal_composed}

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
    out = {"l": L, "alpha": alpha, "R": R, "n_giant": G, "batch": B, "device": m.hip.device_info()[0],
           "fell_back": sorted(name for name, fb in fell_back.items() if fb)}
    for name in legs:
        out[name] = spread(t[name], B)
    print(json.dumps(out))


def main():
    results = []
    for L in LEVELS:
        for alpha in ALPHAS:
            for B in BATCHES:
                for R, G in SHAPES:
                    cmd = [sys.executable, os.path.abspath(__file__), "--cell", str(L), str(alpha), str(R), str(G), str(B), "--rounds",
                           str(args.rounds)]
                    r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout)
                    if r.returncode != 0:
                        raise SystemExit("cell l = %d, alpha = %d, R = %d, n_giant = %d, batch %d failed (%d): %s" % (
                            L, alpha, R, G, B, r.returncode, (r.stdout + r.stderr)[-2000:]))
                    row = json.loads(r.stdout.strip().splitlines()[-1])
                    results.append(row)
                    print("l = %2d  alpha = %2d  batch %2d  R = %2d  n_giant = %d   ms per ciphertext, median (min-max)%s" % (
                        L, alpha, B, R, G, "   FELL BACK: " + " ".join(row["fell_back"]) if row["fell_back"] else ""))
                    for name in LEGS:
                        v = row[name]
                        print("  %-3s %8.4f (%.4f-%.4f)  x%.2f of a  x%.2f of c" % (
                            name, v["median_ms"], v["min_ms"], v["max_ms"], v["median_ms"] / row["a"]["median_ms"],
                            v["median_ms"] / row["c"]["median_ms"]), flush=True)
    print(json.dumps(results))


if args.cell:
    cell(*args.cell)
else:
    main()
