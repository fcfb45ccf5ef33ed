#!/usr/bin/env python3
"""Key switches on a list of ciphertexts (include/moai_hip.h, moai_apply_galois_ptrs) at MOAI's parameters (N = 2^16, the
36-prime chain), every comparison inside one run on one box, the legs taken in turns (A B C D A B C D ...) so that clock and
thermal drift fall on all of them alike; per leg the median of the rounds and their spread.

(a) n = 16 and 64 single ciphertexts at l = 3, 15 and 35 data primes, four ways:
      singles   n moai_apply_galois_to calls of one ciphertext
      gather    moai_gather_blocks + one moai_apply_galois of batch n with one key + moai_scatter_blocks (the call combiner until now)
      ptrs      one moai_apply_galois_ptrs with one key and one element
      ptrs_mix  one moai_apply_galois_ptrs with different keys and four different elements
    Keys are blocks in the trimmed layout of l levels (moai_key_register), zero-filled: their words do not change the time, their
    addresses do.  ptrs_mix has n keys, at l = 35 at most 16 (1.3 GB each), used in turn.
(b) moai_apply_galois at batch 64, l = 35 and 15: `--batch-only` times just that and prints one JSON line; with `--parent-lib
    PATH` (a libmoai_hip.so built from the parent commit) this process starts children in turns, one library each, and reports both
    with the parent's own run-to-run spread, which is the tolerance for "the batch form did not move".
(c) `--attention BINARY`: tools/cpp/bench_attention (MOAI's unchanged loops) with MOAI_SHIM_COMBINE_ANY_KEY unset and =1 in turns,
    `--attention-runs` processes each after one that is not counted;
    the Q K^T and the diagonal-packed .V lines of its report.
Prints a table, then one JSON line."""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

ap = argparse.ArgumentParser()
ap.add_argument("--lib", help="libmoai_hip.so to load instead of the tree's")
ap.add_argument("--batch-only", action="store_true")
ap.add_argument("--parent-lib")
ap.add_argument("--attention")
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--attention-runs", type=int, default=5, help="processes per knob setting in (c), after one untimed process")
ap.add_argument("--skip-list", action="store_true", help="leave (a) out")
args = ap.parse_args()

N, LOGN = 1 << 16, 16
BITS = [51] + [46] * 20 + [51] * 14 + [58]  # include/test/test_full_scheme.hpp:356-378
NEW = ("moai_apply_galois_ptrs", "moai_relinearize_ptrs")


def spread(v):
    return {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}


def device_part():
    import __graft_entry__ as g  # noqa: E402
    import oracle as O  # noqa: E402

    m = g.load_package()
    if args.lib:
        m.hip._SO = args.lib
        for name in NEW:  # a parent library does not export them
            if not hasattr(__import__("ctypes").CDLL(args.lib), name):
                m.hip.SYMBOLS.pop(name, None)
    lib = m.hip.lib()
    chk = m.hip._check
    primes = O.coeff_modulus_create(N, BITS)
    ctx = m.Context(LOGN, primes)
    st = None
    import numpy as np

    rng = np.random.default_rng(1)

    def timed(run, reps):
        e0, e1 = m.hip.Event(), m.hip.Event()
        e0.record(st)
        for _ in range(reps):
            run()
        e1.record(st)
        ctx.sync()
        return e1.elapsed_ms_since(e0) / reps

    def zero_key(levels):
        b = m.DeviceBuffer(lib.moai_key_words(ctx.h, levels))
        chk(lib.moai_memset_zero(b.ptr, b.n_words * 8, st))
        ctx.key_register(b, levels)
        return b

    def turns(legs, rounds, reps):
        t = {name: [] for name in legs}
        for name, run in legs.items():  # warm: arena growth, Galois tables
            run()
        ctx.sync()
        for _ in range(rounds):
            for name, run in legs.items():
                t[name].append(timed(run, reps))
        return {name: spread(v) for name, v in t.items()}

    out = {}
    elts = [ctx.galois_elt_from_step(s) for s in (1, 2, 4, 8)]
    if args.batch_only:
        for L in (35, 15):
            B = 64
            key = zero_key(L)
            one = m.DeviceBuffer.from_numpy(O.uniform_rns(rng, primes[:L], (2,), N))
            ct = m.DeviceBuffer(B * 2 * L * N)
            for b in range(B):
                chk(lib.moai_memcpy_d2d(ct.ptr + b * 2 * L * N * 8, one.ptr, 2 * L * N * 8, st))
            out["batch64_l%d" % L] = turns({"batch": lambda: ctx.apply_galois(ct, L, elts[0], key, B)}, args.rounds, 3)["batch"]
            ctx.key_forget(key)
            del ct, key
        print(json.dumps(out))
        return
    for L in (3, 15, 35):
        words = 2 * L * N
        one = m.DeviceBuffer.from_numpy(O.uniform_rns(rng, primes[:L], (2,), N))
        n_keys = 16 if L == 35 else 64
        keys = [zero_key(L) for _ in range(n_keys)]
        for n in (16, 64):
            ins = [m.DeviceBuffer(words) for _ in range(n)]
            outs = [m.DeviceBuffer(words) for _ in range(n)]
            packed = m.DeviceBuffer(n * words)
            for d in ins:
                chk(lib.moai_memcpy_d2d(d.ptr, one.ptr, words * 8, st))

            def singles():
                for i in range(n):
                    ctx.apply_galois_to(ins[i], outs[i], L, elts[0], keys[0], 1)

            def gather():
                ctx.gather_blocks(ins, packed, words)
                ctx.apply_galois(packed, L, elts[0], keys[0], n)
                ctx.scatter_blocks(packed, outs, words)

            def ptrs():
                ctx.apply_galois_ptrs(ins, outs, L, [elts[0]] * n, [keys[0]] * n)

            def ptrs_mix():
                ctx.apply_galois_ptrs(ins, outs, L, [elts[i % 4] for i in range(n)], [keys[i % n_keys] for i in range(n)])

            r = turns({"singles": singles, "gather": gather, "ptrs": ptrs, "ptrs_mix": ptrs_mix}, args.rounds, 2)
            out["l%d_n%d" % (L, n)] = r
            print("l = %2d  n = %2d  ms per ciphertext: " % (L, n) +
                  "  ".join("%s %.4f (%.4f-%.4f)" % (k, v["median_ms"] / n, v["min_ms"] / n, v["max_ms"] / n) for k, v in r.items()), flush=True)
            del ins, outs, packed
        for key in keys:
            ctx.key_forget(key)
        del keys
    return out


def child(lib_path):
    cmd = [sys.executable, os.path.abspath(__file__), "--batch-only", "--rounds", str(args.rounds)] + (["--lib", lib_path] if lib_path else [])
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        raise SystemExit("child failed: " + r.stderr[-2000:])
    return json.loads(r.stdout.strip().splitlines()[-1])


def batch_part():
    """(b): branch and parent in turns, a fresh process each"""
    runs = {"parent": [], "branch": []}
    for _ in range(3):
        runs["parent"].append(child(args.parent_lib))
        runs["branch"].append(child(None))
    out = {}
    for case in runs["parent"][0]:
        row = {}
        for who in runs:
            med = [r[case]["median_ms"] for r in runs[who]]
            row[who] = {"median_ms": round(statistics.median(med), 4), "runs_ms": med}
        p = row["parent"]["runs_ms"]
        row["parent_spread_percent"] = round(100 * (max(p) - min(p)) / statistics.median(p), 2)
        row["branch_over_parent"] = round(row["branch"]["median_ms"] / row["parent"]["median_ms"], 4)
        out[case] = row
        print("%s  parent %.3f ms %s  branch %.3f ms %s  ratio %.4f (parent's own spread %.2f %%)" % (
            case, row["parent"]["median_ms"], p, row["branch"]["median_ms"], row["branch"]["runs_ms"], row["branch_over_parent"],
            row["parent_spread_percent"]), flush=True)
    return out


def attention_part():
    """(c): MOAI's unchanged products with the knob off and on, in turns"""
    pick = {"qkt": r"Q K\^T \(colpacking.*?:\s+([0-9.]+) s", "dot_v": r"softmax\(QK\^T\) V \(diagpacking.*?:\s+([0-9.]+) s"}
    t = {"off": {k: [] for k in pick}, "on": {k: [] for k in pick}}
    for i in range(args.attention_runs + 1):
        for knob in ("off", "on") if i else ("warm",):  # the first process of a session pays for the box's cold caches: not counted
            env = {k: v for k, v in os.environ.items() if k != "MOAI_SHIM_COMBINE_ANY_KEY"}
            if knob == "on":
                env["MOAI_SHIM_COMBINE_ANY_KEY"] = "1"
            r = subprocess.run([args.attention, "16", "768"], capture_output=True, text=True, timeout=170, env=env)
            if r.returncode != 0:
                raise SystemExit("bench_attention failed: " + r.stdout[-1000:] + r.stderr[-1000:])
            for k, pat in pick.items():
                if knob != "warm":
                    t[knob][k].append(float(re.search(pat, r.stdout).group(1)))
    for k in pick:
        print("%s  knob off %s s (median %.3f)  knob on %s s (median %.3f)" % (k, t["off"][k], statistics.median(t["off"][k]), t["on"][k],
                                                                                 statistics.median(t["on"][k])), flush=True)
    return t


if args.batch_only:
    device_part()
else:
    result = {}
    if not args.skip_list:
        result["list"] = device_part()
    if args.parent_lib:
        result["batch"] = batch_part()
    if args.attention:
        result["attention"] = attention_part()
    print(json.dumps(result))
