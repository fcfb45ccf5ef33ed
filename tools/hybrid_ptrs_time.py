#!/usr/bin/env python3
"""Hybrid key switches on a list of ciphertexts (include/moai_hip.h, "hybrid key switches on a list of ciphertexts") at N = 2^16,
alpha = 12: n single ciphertexts, each in its own block, inside one process per cell with the legs taken in turns (A B C D A B C D
...), so that clock and thermal drift fall on all of them alike; per leg the median of the rounds on device events and their spread,
in ms per ciphertext.  Rotation:
  a  n moai_apply_galois_hybrid calls of one ciphertext           MOAI's 35 data primes plus 12 60-bit special primes
  b  one moai_apply_galois_hybrid_ptrs                            the same chain and keys
  c  one moai_apply_galois_ptrs, keys trimmed to l levels         MOAI's own 36-prime chain (35 data primes, one 58-bit special prime)
  d  one moai_apply_galois_hybrid at batch n with one key         a lower bound for b: no gather, one key in cache
for l in {35, 15} data primes x n in {16, 64} x keys in {one: every member the same key and element, own: every member its own key,
four elements in turn}.  a, b and c use the cell's keys; d always has one.  At l = 35 leg c has at most 16 keys (1.3 GB each), used
in turn.  Relinearize + rescale, in the cells with one key (the call takes one):
  a  n moai_relinearize_rescale_hybrid calls of one ciphertext
  b  one moai_relinearize_rescale_hybrid_ptrs
  c  one moai_relinearize_ptrs into the blocks of one buffer + one moai_rescale at batch n     the 36-prime chain
  d  one moai_relinearize_rescale_hybrid at batch n
Keys are zero-filled and the operands random blocks: their words do not change the time, their addresses do.

Without arguments this process starts one child per cell (`--cell L N KEYS`), each under its own time limit, and stops at the first
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
ap.add_argument("--cell", nargs=3, metavar=("L", "N", "KEYS"))
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--timeout", type=int, default=240, help="seconds per cell")
args = ap.parse_args()

N, LOGN, ALPHA = 1 << 16, 16, 12
DATA_BITS = [51] + [46] * 20 + [51] * 14  # include/test/test_full_scheme.hpp:356-378
CELLS = [(L, n, keys) for L in (35, 15) for n in (16, 64) for keys in ("one", "own")]
LEGS = ("a", "b", "c", "d")


def spread(v, per):
    return {"median_ms": round(statistics.median(v) / per, 4), "min_ms": round(min(v) / per, 4), "max_ms": round(max(v) / per, 4)}


def cell(L, n, own):
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

    def copies(one, words, count):
        """`count` blocks of their own and one contiguous buffer, every ciphertext a copy of `one`"""
        blocks, packed = [m.DeviceBuffer(words) for _ in range(count)], m.DeviceBuffer(count * words)
        for i, d in enumerate(blocks):
            chk(lib.moai_memcpy_d2d(d.ptr, one.ptr, words * 8, st))
            chk(lib.moai_memcpy_d2d(packed.ptr + i * words * 8, one.ptr, words * 8, st))
        return blocks, packed

    hy_primes = O.coeff_modulus_create(N, DATA_BITS + [60] * ALPHA)
    hy = m.Context(LOGN, hy_primes)
    k = len(hy_primes)
    key_words = hy.hybrid_digits(ALPHA, k - ALPHA) * 2 * k * N
    hkeys = [zeros(key_words) for _ in range(n if own else 1)]
    seal_primes = O.coeff_modulus_create(N, DATA_BITS + [58])
    seal = m.Context(LOGN, seal_primes)
    skeys = []
    for _ in range(min(n, 16 if L == 35 else 64) if own else 1):
        b = zeros(lib.moai_key_words(seal.h, L))
        seal.key_register(b, L)
        skeys.append(b)
    helts = [hy.galois_elt_from_step(s) for s in (1, 2, 4, 8)]
    selts = [seal.galois_elt_from_step(s) for s in (1, 2, 4, 8)]
    pick = (lambda xs, i: xs[i % len(xs)]) if own else (lambda xs, i: xs[0])

    def timed(run, reps):
        e0, e1 = m.hip.Event(), m.hip.Event()
        e0.record(st)
        for _ in range(reps):
            run()
        e1.record(st)
        hy.sync()
        seal.sync()
        return e1.elapsed_ms_since(e0) / reps

    def turns(legs):
        for run in legs.values():  # warm: arena growth, constant tables, Galois tables
            run()
        hy.sync()
        seal.sync()
        t = {name: [] for name in legs}
        for _ in range(args.rounds):
            for name, run in legs.items():
                t[name].append(timed(run, 2))
        return {name: spread(v, n) for name, v in t.items()}

    out = {"l": L, "n": n, "keys": "own" if own else "one", "alpha": ALPHA, "device": m.hip.device_info()[0]}
    # ---- the rotation
    words = 2 * L * N
    h_in, h_packed = copies(m.DeviceBuffer.from_numpy(O.uniform_rns(rng, hy_primes[:L], (2,), N)), words, n)
    s_in, _ = copies(m.DeviceBuffer.from_numpy(O.uniform_rns(rng, seal_primes[:L], (2,), N)), words, n)
    del _
    h_out, s_out = [m.DeviceBuffer(words) for _ in range(n)], [m.DeviceBuffer(words) for _ in range(n)]
    hk, he = [pick(hkeys, i) for i in range(n)], [pick(helts, i) for i in range(n)]
    sk, se = [pick(skeys, i) for i in range(n)], [pick(selts, i) for i in range(n)]

    def rot_a():
        for i in range(n):
            hy.apply_galois_hybrid(h_in[i], L, ALPHA, he[i], hk[i], 1)

    out["rotation"] = turns({
        "a": rot_a,
        "b": lambda: hy.apply_galois_hybrid_ptrs(h_in, h_out, L, ALPHA, he, hk),
        "c": lambda: seal.apply_galois_ptrs(s_in, s_out, L, se, sk),
        "d": lambda: hy.apply_galois_hybrid(h_packed, L, ALPHA, helts[0], hkeys[0], n),
    })
    del h_in, h_packed, s_in, h_out, s_out
    # ---- relinearize + rescale: one key by construction
    if not own:
        words3, words_out = 3 * L * N, 2 * (L - 1) * N
        h3, h3_packed = copies(m.DeviceBuffer.from_numpy(O.uniform_rns(rng, hy_primes[:L], (3,), N)), words3, n)
        s3, _ = copies(m.DeviceBuffer.from_numpy(O.uniform_rns(rng, seal_primes[:L], (3,), N)), words3, n)
        del _
        h_out, h_out_packed = [m.DeviceBuffer(words_out) for _ in range(n)], m.DeviceBuffer(n * words_out)
        s_mid, s_out_packed = m.DeviceBuffer(n * words), m.DeviceBuffer(n * words_out)
        s_mid_blocks = [s_mid.ptr + i * words * 8 for i in range(n)]

        def rr_a():
            for i in range(n):
                hy.relinearize_rescale_hybrid(h3[i], hkeys[0], h_out[i], L, ALPHA, 1)

        def rr_c():
            seal.relinearize_ptrs(s3, s_mid_blocks, skeys[0], L)
            seal.rescale(s_mid, s_out_packed, 2, L, n)

        out["relin_rescale"] = turns({
            "a": rr_a,
            "b": lambda: hy.relinearize_rescale_hybrid_ptrs(h3, h_out, hkeys[0], L, ALPHA),
            "c": rr_c,
            "d": lambda: hy.relinearize_rescale_hybrid(h3_packed, hkeys[0], h_out_packed, L, ALPHA, n),
        })
    for b in skeys:
        seal.key_forget(b)
    print(json.dumps(out))


def main():
    results = []
    print("alpha = %d, ms per ciphertext, median of %d rounds of two calls (min-max)" % (ALPHA, args.rounds))
    for L, n, keys in CELLS:
        cmd = [sys.executable, os.path.abspath(__file__), "--cell", str(L), str(n), keys, "--rounds", str(args.rounds)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout)
        if r.returncode != 0:
            raise SystemExit("cell l = %d, n = %d, keys %s failed (%d): %s" % (L, n, keys, r.returncode, (r.stdout + r.stderr)[-2000:]))
        row = json.loads(r.stdout.strip().splitlines()[-1])
        results.append(row)
        for what in ("rotation", "relin_rescale"):
            if what not in row:
                continue
            v = row[what]
            print("l = %2d  n = %2d  keys %s  %s" % (L, n, keys, what))
            for name in LEGS:
                print("  %s %9.4f (%.4f-%.4f)" % (name, v[name]["median_ms"], v[name]["min_ms"], v[name]["max_ms"]))
            print("  b/a %.3f   b/c %.3f   b/d %.3f" % tuple(v["b"]["median_ms"] / v[x]["median_ms"] for x in ("a", "c", "d")), flush=True)
    print(json.dumps(results))


if args.cell:
    cell(int(args.cell[0]), int(args.cell[1]), args.cell[2] == "own")
else:
    main()
