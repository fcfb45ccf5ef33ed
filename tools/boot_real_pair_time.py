#!/usr/bin/env python3
"""Two real ciphertexts per bootstrap against one, at N = 2^16 on MOAI's chain, full slots: ms per ciphertext for 96 real
ciphertexts through bootstrap_3 and bootstrap_real_3 in packs of 48 and through bootstrap_real_many_3 (48 pairs in one pack),
and the two element-wise kernels behind the pairing next to moai_add (tools/cpp/bench_bootstrap_real_pair, built by
build()).  Prints the driver's lines, then each leg's time as a fraction of the bootstrap_3 leg of the same run.

    python3 tools/boot_real_pair_time.py [--reps 3] [--total 96] [--pack 48] [--json OUT]"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tools", "cpp", "bench_bootstrap_real_pair")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--total", type=int, default=96)
    ap.add_argument("--pack", type=int, default=48)
    ap.add_argument("--json", default=None, help="write the rows here")
    a = ap.parse_args()
    if not os.path.exists(EXE):
        sys.exit("%s is missing: run build() first" % EXE)
    env = dict(os.environ)
    env.pop("MOAI_BOOT_PAIR_REAL", None)  # the legs choose their path themselves
    r = subprocess.run([EXE, str(a.reps), str(a.total), str(a.pack)], capture_output=True, text=True, env=env)
    rows = []
    for line in r.stdout.splitlines():
        if line.startswith("{"):
            rows.append(json.loads(line))
        else:
            print(line)
    if r.returncode != 0:
        sys.stderr.write(r.stderr[-4000:])
        sys.exit(r.returncode)
    legs = [row for row in rows if "leg" in row]
    base = next(row["ms_per_ct"] for row in legs if row["leg"] == "bootstrap_3")
    print("%-22s %12s %16s %12s" % ("leg", "ms per ct", "vs bootstrap_3", "max |error|"))
    for row in legs:
        print("%-22s %12.2f %16.3f %12.2e" % (row["leg"], row["ms_per_ct"], row["ms_per_ct"] / base, row["max_error"]))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
