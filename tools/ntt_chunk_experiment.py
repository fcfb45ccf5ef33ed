#!/usr/bin/env python3
"""Does the intermediate of the two-pass NTT stay in the Infinity Cache when a launch pair is kept small?
Times the forward and inverse transform of bench.py's workload (N = 2^16, 44 x 60-bit primes, 512 polynomials) as ONE call per
direction, under the library's own chunk schedule: chunks of c polynomials (c * 44 * 512 KiB between the strided and the
contiguous pass, MOAI_NTT_CHUNK_MB) dealt to K side streams (MOAI_NTT_PIPE; K = 0 is the chunk loop on the caller's stream, the
round-2 experiment of profiles/r02_g_ntt_subbatch_experiment.txt).  The unchunked call is timed first, last and between the
values of K, so that a drift of the box shows.

    python tools/ntt_chunk_experiment.py [--k 0,1,2,3] [--chunks 22,44,88,176] [--polys 512] [--reps 5]"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import __graft_entry__ as g
import bench

ap = argparse.ArgumentParser()
ap.add_argument("--k", default="0,1,2,3", help="side streams to try (0: the caller's stream)")
ap.add_argument("--chunks", default="22,44,88,176", help="chunk sizes in MiB")
ap.add_argument("--polys", type=int, default=512)
ap.add_argument("--reps", type=int, default=5)
args = ap.parse_args()

m = g.load_package()
N, L, TOTAL = 65536, 44, args.polys
primes = bench.primes_44x60()
ctx = m.Context(16, primes)
dev = torch.device("cuda")
st = torch.cuda.current_stream().cuda_stream
x = torch.empty((TOTAL, L, N), dtype=torch.int64, device=dev)
for i, q in enumerate(primes):
    x[:, i, :] = torch.randint(0, q, (TOTAL, N), dtype=torch.int64, device=dev)
torch.cuda.synchronize()
psz = L * N * 8


def timed(k, mb):
    """median and spread (max - min) in ms over --reps of one forward and one inverse call"""
    m.hip.set_tuning("MOAI_NTT_CHUNK_MB", mb)
    m.hip.set_tuning("MOAI_NTT_PIPE", k)
    m.hip.set_tuning("MOAI_NTT_PIPE_MIN", 1)  # the sweep is what the default minimum comes from
    out = []
    for fn in (ctx.ntt_forward, ctx.ntt_inverse):
        fn(x.data_ptr(), TOTAL, L, stream=st)
        fn(x.data_ptr(), TOTAL, L, stream=st)
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.reps):
            e0, e1 = m.hip.Event(), m.hip.Event()
            e0.record(st)
            fn(x.data_ptr(), TOTAL, L, stream=st)
            e1.record(st)
            torch.cuda.synchronize()
            ms.append(e1.elapsed_ms_since(e0))
        out.append((statistics.median(ms), max(ms) - min(ms)))
    m.hip.reset_tuning()
    return out


def line(k, mb):
    (f, fs), (i, is_) = timed(k, mb)
    what = "whole batch, one stream" if mb == 0 else "K = %d, chunk %3d MiB (%2d polys, plan %3d)" % (
        k, mb, max(1, (mb << 20) // psz), m.hip.ntt_pipe_plan(TOTAL, L, N, mb << 20, k))
    print("%-44s forward %7.3f ms (+-%5.3f)  inverse %7.3f ms (+-%5.3f)  sum %7.3f ms  %7.1f GB/s algorithmic" % (
        what, f, fs, i, is_, f + i, 2 * TOTAL * psz * 2 / (f + i) / 1e6), flush=True)


print("# %d polynomials x %d rows x 2^16 = %.1f GiB; median (max - min) of %d calls per direction" % (TOTAL, L, TOTAL * psz / 2**30, args.reps))
line(0, 0)
for k in [int(v) for v in args.k.split(",")]:
    for mb in [int(v) for v in args.chunks.split(",")]:
        line(k, mb)
    line(0, 0)
