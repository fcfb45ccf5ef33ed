#!/usr/bin/env python3
"""The fused hybrid mod-down (MOAI_HYBRID_FUSED_DOWN = 1; include/moai_hip.h, "hybrid key switching") against the unfused stages, beside
the fused steps 2-4 (MOAI_HYBRID_FUSED), at N = 2^16: the four combinations of the two knobs on the same library and the same call,
inside one process per cell with the legs taken in turns (A B C ... A B C ...), so that clock and thermal drift fall on all of them
alike; per leg the median of the rounds on device events and their spread, in ms per ciphertext.  A round of a leg is one window of as
many calls as make it at least WINDOW_MS long (sized from a first pass).  Both knobs at 0 is the launch sequence of the library
without either.
  galois_FD    moai_apply_galois_hybrid with MOAI_HYBRID_FUSED = F and MOAI_HYBRID_FUSED_DOWN = D, on MOAI's 35 data primes plus
               alpha 60-bit special primes
  rescale_FD   moai_relinearize_rescale_hybrid, same knobs, same chain
  seal_galois  moai_apply_galois on MOAI's own 36-prime chain (35 data primes, one 58-bit special prime)
  seal_rescale moai_relinearize + moai_rescale on that chain
for alpha in {12, 4} x l in {35, 15} data primes x batch in {1, 16, 64}.  Keys are zero-filled and operands random blocks: their
words do not change the time.

Without arguments this process starts one child per cell (`--cell ALPHA L BATCH`), each under its own time limit, and stops at
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
ap.add_argument("--cell", nargs=3, type=int, metavar=("ALPHA", "L", "BATCH"))
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--timeout", type=int, default=240, help="seconds per cell")
ap.add_argument("--alphas", type=int, nargs="+", default=[12, 4])
ap.add_argument("--levels", type=int, nargs="+", default=[35, 15])
ap.add_argument("--batches", type=int, nargs="+", default=[1, 16, 64])
args = ap.parse_args()

N, LOGN = 1 << 16, 16
WINDOW_MS = 30.0
DATA_BITS = [51] + [46] * 20 + [51] * 14  # include/test/test_full_scheme.hpp:356-378
KNOBS = ["00", "01", "10", "11"]  # MOAI_HYBRID_FUSED, MOAI_HYBRID_FUSED_DOWN
LEGS = ["galois_" + k for k in KNOBS] + ["rescale_" + k for k in KNOBS] + ["seal_galois", "seal_rescale"]


def spread(v, per):
    return {"median_ms": round(statistics.median(v) / per, 4), "min_ms": round(min(v) / per, 4), "max_ms": round(max(v) / per, 4)}


def cell(alpha, L, B):
    import numpy as np

    import __graft_entry__ as g
    import oracle as O

    m = g.load_package()
    lib, chk = m.hip.lib(), m.hip._check
    rng = np.random.default_rng(1)

    def zeros(words):
        b = m.DeviceBuffer(words)
        chk(lib.moai_memset_zero(b.ptr, words * 8, None))
        return b

    def operands(ctx, primes):
        one = m.DeviceBuffer.from_numpy(O.uniform_rns(rng, primes[:L], (3,), N))
        ct3, rot = m.DeviceBuffer(B * 3 * L * N), m.DeviceBuffer(B * 2 * L * N)
        for b in range(B):
            chk(lib.moai_memcpy_d2d(ct3.ptr + b * 3 * L * N * 8, one.ptr, 3 * L * N * 8, None))
            chk(lib.moai_memcpy_d2d(rot.ptr + b * 2 * L * N * 8, one.ptr, 2 * L * N * 8, None))
        return ct3, rot, m.DeviceBuffer(B * 2 * (L - 1) * N)

    hp = O.coeff_modulus_create(N, DATA_BITS + [60] * alpha)
    hctx = m.Context(LOGN, hp)
    hkey = zeros(hctx.hybrid_digits(alpha, len(hp) - alpha) * 2 * len(hp) * N)
    hct3, hrot, hout = operands(hctx, hp)
    sp = O.coeff_modulus_create(N, DATA_BITS + [58])
    sctx = m.Context(LOGN, sp)
    skey = zeros((len(sp) - 1) * 2 * len(sp) * N)
    sct3, srot, sout = operands(sctx, sp)
    srel = m.DeviceBuffer(B * 2 * L * N)
    elt = hctx.galois_elt_from_step(1)

    def knobs(fd, run):
        def leg():
            m.hip.set_tuning("MOAI_HYBRID_FUSED", int(fd[0]))
            m.hip.set_tuning("MOAI_HYBRID_FUSED_DOWN", int(fd[1]))
            run()
        return leg

    def seal_rescale():
        sctx.relinearize(sct3, skey, srel, L, B)
        sctx.rescale(srel, sout, 2, L, B)

    galois = lambda: hctx.apply_galois_hybrid(hrot, L, alpha, elt, hkey, B)  # noqa: E731 (in place: residues stay residues)
    rescale = lambda: hctx.relinearize_rescale_hybrid(hct3, hkey, hout, L, alpha, B)  # noqa: E731
    legs = {"galois_" + k: knobs(k, galois) for k in KNOBS}
    legs.update({"rescale_" + k: knobs(k, rescale) for k in KNOBS})
    legs.update({"seal_galois": lambda: sctx.apply_galois(srot, L, elt, skey, B), "seal_rescale": seal_rescale})

    def timed(run, reps):
        e0, e1 = m.hip.Event(), m.hip.Event()
        e0.record(None)
        for _ in range(reps):
            run()
        e1.record(None)
        hctx.sync()
        return e1.elapsed_ms_since(e0) / reps

    for run in legs.values():  # warm: arena growth, constant tables
        run()
    hctx.sync()
    reps = {name: max(2, int(WINDOW_MS / timed(run, 2)) + 1) for name, run in legs.items()}
    t = {name: [] for name in legs}
    for _ in range(args.rounds):
        for name, run in legs.items():
            t[name].append(timed(run, reps[name]))
    m.hip.set_tuning("MOAI_HYBRID_FUSED_DOWN", 1)
    out = {"alpha": alpha, "l": L, "batch": B, "device": m.hip.device_info()[0],
           "down_launches": [hctx.hybrid_fused_down_launches(L, alpha, 2 * B), hctx.hybrid_fused_down_launches(L - 1, alpha, 2 * B)],
           "calls_per_window": reps}
    for name in legs:
        out[name] = spread(t[name], B)
    print(json.dumps(out))


def main():
    results = []
    for alpha in args.alphas:
        for L in args.levels:
            for B in args.batches:
                cmd = [sys.executable, os.path.abspath(__file__), "--cell", str(alpha), str(L), str(B), "--rounds", str(args.rounds)]
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout)
                if r.returncode != 0:
                    raise SystemExit("cell alpha = %d, l = %d, batch %d failed (%d): %s" % (alpha, L, B, r.returncode,
                                                                                           (r.stdout + r.stderr)[-2000:]))
                row = json.loads(r.stdout.strip().splitlines()[-1])
                results.append(row)
                print("alpha = %2d  l = %2d  batch %2d  (%d launch pairs per mod-down)  ms per ciphertext, median (min-max)"
                      % (alpha, L, B, row["down_launches"][0]))
                for name in LEGS:
                    v = row[name]
                    base = row[name[:-2] + "00"]["median_ms"] if name[-2:] in KNOBS else None
                    print("  %-13s %8.4f (%.4f-%.4f)%s" % (name, v["median_ms"], v["min_ms"], v["max_ms"],
                                                          "  x%.3f of knobs 00" % (v["median_ms"] / base) if base else ""), flush=True)
    print(json.dumps(results))


if args.cell:
    cell(*args.cell)
else:
    main()
