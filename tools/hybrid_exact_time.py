#!/usr/bin/env python3
"""The exact rounding mode of the hybrid mod-downs (include/moai_hip.h, "hybrid rounding mode") against the default at N = 2^16 on
MOAI's 35 data primes plus twelve 60-bit special primes: moai_switch_key_hybrid and moai_relinearize_rescale_hybrid at l in {35, 15},
batch 16.  One process per cell; inside it the legs are taken in turns (fast exact fast exact ...), so that clock and thermal drift
fall on both alike; per leg the median of the rounds on device events and their spread, in ms per ciphertext.  Keys and operands
are zero-filled or random blocks: their words do not change the time.

`--root DIR` loads the package of another checkout (one that has been built), e.g. the parent commit: where that package has no
rounding mode only the fast leg runs, which shows whether the default path moved.

Without `--cell` this process starts one child per cell (`--cell CALL L BATCH`), each under its own time limit, and stops at the
first that fails.  Prints a table, then one JSON line."""
import argparse
import importlib.util
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

ap = argparse.ArgumentParser()
ap.add_argument("--cell", nargs=3, metavar=("CALL", "L", "BATCH"))
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--timeout", type=int, default=240, help="seconds per cell")
ap.add_argument("--root", default=ROOT, help="the checkout whose package is timed")
args = ap.parse_args()

N, LOGN, ALPHA = 1 << 16, 16, 12
DATA_BITS = [51] + [46] * 20 + [51] * 14  # include/test/test_full_scheme.hpp:356-378
CALLS = ("switch_key_hybrid", "relinearize_rescale_hybrid")
CELLS = [(call, L, 16) for L in (35, 15) for call in CALLS]
FAST, EXACT = 0, 1


def spread(v, per):
    return {"median_ms": round(statistics.median(v) / per, 4), "min_ms": round(min(v) / per, 4), "max_ms": round(max(v) / per, 4)}


def cell(call, L, B):
    import numpy as np

    import oracle as O

    spec = importlib.util.spec_from_file_location("graft_entry_timed", os.path.join(args.root, "__graft_entry__.py"))
    g = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(g)
    m = g.load_package()
    lib, chk = m.hip.lib(), m.hip._check
    st = None
    rng = np.random.default_rng(1)
    primes = O.coeff_modulus_create(N, DATA_BITS + [60] * ALPHA)
    ctx = m.Context(LOGN, primes)
    k = len(primes)
    key = m.DeviceBuffer(ctx.hybrid_digits(ALPHA, k - ALPHA) * 2 * k * N)
    chk(lib.moai_memset_zero(key.ptr, key.n_words * 8, st))
    one = m.DeviceBuffer.from_numpy(O.uniform_rns(rng, primes[:L], (3,), N))
    ct3 = m.DeviceBuffer(B * 3 * L * N)
    for b in range(B):
        chk(lib.moai_memcpy_d2d(ct3.ptr + b * 3 * L * N * 8, one.ptr, 3 * L * N * 8, st))
    if call == "switch_key_hybrid":
        ct = m.DeviceBuffer(B * 2 * L * N)
        chk(lib.moai_memset_zero(ct.ptr, ct.n_words * 8, st))
        run = lambda: ctx.switch_key_hybrid(ct, ct3, key, L, ALPHA, B)  # noqa: E731 (the target: the first B L rows of ct3)
    else:
        out = m.DeviceBuffer(B * 2 * (L - 1) * N)
        run = lambda: ctx.relinearize_rescale_hybrid(ct3, key, out, L, ALPHA, B)  # noqa: E731
    modes = {"fast": FAST, "exact": EXACT} if hasattr(ctx, "hybrid_set_rounding") else {"fast": None}

    def leg(mode):
        if mode is not None:
            ctx.hybrid_set_rounding(mode)
        e0, e1 = m.hip.Event(), m.hip.Event()
        e0.record(st)
        for _ in range(2):
            run()
        e1.record(st)
        ctx.sync()
        return e1.elapsed_ms_since(e0) / 2

    for mode in modes.values():  # warm: arena growth, constant tables
        leg(mode)
    t = {name: [] for name in modes}
    for _ in range(args.rounds):
        for name, mode in modes.items():
            t[name].append(leg(mode))
    if "exact" in modes:
        ctx.hybrid_set_rounding(FAST)
    out = {"call": call, "l": L, "batch": B, "alpha": ALPHA, "device": m.hip.device_info()[0]}
    for name in modes:
        out[name] = spread(t[name], B)
    print(json.dumps(out))


def main():
    results = []
    for call, L, B in CELLS:
        cmd = [sys.executable, os.path.abspath(__file__), "--cell", call, str(L), str(B), "--rounds", str(args.rounds), "--root", args.root]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout)
        if r.returncode != 0:
            raise SystemExit("cell %s l = %d, batch %d failed (%d): %s" % (call, L, B, r.returncode, (r.stdout + r.stderr)[-2000:]))
        row = json.loads(r.stdout.strip().splitlines()[-1])
        results.append(row)
        print("%-28s l = %2d  batch %2d  ms per ciphertext, median (min-max)" % (call, L, B))
        for name in ("fast", "exact"):
            if name in row:
                v = row[name]
                print("  %-6s %8.4f (%.4f-%.4f)  x%.4f of fast" % (name, v["median_ms"], v["min_ms"], v["max_ms"],
                                                                 v["median_ms"] / row["fast"]["median_ms"]), flush=True)
    print(json.dumps(results))


if args.cell:
    cell(args.cell[0], int(args.cell[1]), int(args.cell[2]))
else:
    main()
