#!/usr/bin/env python3
"""Full-slot against sparse-slot bootstrapping at N = 2^16 on MOAI's chain: ms per ciphertext for logn = 15 (full) and the
sparse logn 12, 13, 14, at packs of 1 and 16 (tools/cpp/bench_bootstrap_sparse, built by build()).  Prints the driver's lines,
then a table with each sparse row's time as a fraction of the full-slot time at the same pack.

    python3 tools/boot_sparse_time.py [--reps 3] [--packs 1,16] [--logn 12,13,14] [--json OUT]"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tools", "cpp", "bench_bootstrap_sparse")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--packs", default="1,16")
    ap.add_argument("--logn", default="12,13,14")
    ap.add_argument("--json", default=None, help="write the rows here")
    a = ap.parse_args()
    if not os.path.exists(EXE):
        sys.exit("%s is missing: run build() first" % EXE)
    r = subprocess.run([EXE, str(a.reps), a.packs, a.logn], capture_output=True, text=True)
    rows = []
    for line in r.stdout.splitlines():
        if line.startswith("{"):
            rows.append(json.loads(line))
        else:
            print(line)
    if r.returncode != 0:
        sys.stderr.write(r.stderr[-4000:])
        sys.exit(r.returncode)
    full = {row["pack"]: row["ms_per_ct"] for row in rows if row["kind"] == "full"}
    print("%-6s %-6s %5s %12s %10s" % ("logn", "kind", "pack", "ms per ct", "vs full"))
    for row in rows:
        ratio = row["ms_per_ct"] / full[row["pack"]] if row["pack"] in full else float("nan")
        print("%-6d %-6s %5d %12.2f %10.3f" % (row["logn"], row["kind"], row["pack"], row["ms_per_ct"], ratio))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
