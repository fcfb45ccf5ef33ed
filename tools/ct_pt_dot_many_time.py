#!/usr/bin/env python3
"""The giant-step sums of a baby-step / giant-step transform two ways in one process, alternating: one moai_ct_pt_dot_many against
the composition of moai_bootstrap_lt.h (one moai_ct_pt_dot2 per pair of giant steps whose baby lists nest, one moai_ct_pt_dot for
an odd last one), at pack 48 (n_poly = 96) and N = 2^16.  The outputs are compared before anything is timed.
Shapes (R baby steps, n_g giant steps, L primes).  At logn = 15 the level-three split (moai_level_three.h) gives every group
totlen = 31: a plain transform has 63 diagonals, giantstep(63) = 7 baby steps and 9 giant steps of 7 terms; a rotated one has 32,
giantstep(32) = 4 baby steps and 8 giant steps of 4 terms (BsgsLinearTransform's constructor).  Coefficient-to-slot runs at 17, 16
and 15 primes, slot-to-coefficient at 6, 5 and 4 (profiles/boot_one_engine_parent_vs_branch.txt).  Beside them one small-R and one
large-R shape that no transform of the bootstrap has.
Floors of the new call, computed from the shapes alone --
  memory   every operand, plaintext and output word once at the 5.3 TB/s a copy reaches on this part
  integer  per product the least a 64 x 64 -> 128-bit product and its 128-bit addition take: 4 v_mad_u64_u32 at a quarter of the
           VALU rate (16 lane-cycles) and 6 full-rate instructions of carries, on CUs * 4 SIMDs * 16 lanes at the part's 2.4 GHz
           peak clock (the compiled kernel spends more per product, profiles/ctpt_many_isa.txt)."""
import os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import __graft_entry__ as g
import bench

m = g.load_package()
N, NPOLY, REPS, CALLS = 65536, 96, 5, 3
SHAPES = (("coefficient-to-slot, rotated", 4, 8, 17), ("coefficient-to-slot, plain", 7, 9, 16), ("slot-to-coefficient, plain", 7, 9, 5),
          ("slot-to-coefficient, rotated", 4, 8, 4), ("small R", 2, 3, 6), ("large R", 32, 12, 4))


def primes_of(bits):
    out, seen = [], set()
    for b in bits:
        v = ((1 << b) - 1) // (2 * N) * (2 * N) + 1
        while v in seen or not bench.is_prime(v):
            v -= 2 * N
        seen.add(v)
        out.append(v)
    return out


dev = torch.device("cuda")
st = torch.cuda.current_stream().cuda_stream
dev_name, cus, _ = m.hip.device_info()
lane_hz = cus * 4 * 16 * 2.4e9
print("device: %s, %d CUs" % (dev_name, cus))
for name, R, NG, L in SHAPES:
    primes = primes_of([51] + [46] * (L - 1))
    ctx = m.Context(16, primes)
    gen = torch.Generator(device=dev).manual_seed(7)
    draw = lambda *shape: torch.stack([torch.randint(0, q, shape + (N,), dtype=torch.int64, device=dev, generator=gen) for q in primes],
                                      dim=-2).contiguous()
    x, p = draw(R, NPOLY), draw(NG * R)
    outs = {k: torch.empty((NG, NPOLY, L, N), dtype=torch.int64, device=dev) for k in ("parent", "many")}
    xi = [list(range(R))] * NG                                     # every giant step uses every baby step, in order
    pi = [list(range(j * R, (j + 1) * R)) for j in range(NG)]      # and has its own diagonals
    block = NPOLY * L * N

    def parent():
        o = outs["parent"]
        for j in range(0, NG - 1, 2):
            ctx.ct_pt_dot2(x.data_ptr(), p.data_ptr(), o[j].data_ptr(), o[j + 1].data_ptr(), xi[j], pi[j], pi[j + 1], NPOLY, L, stream=st)
        if NG % 2:
            ctx.ct_pt_dot(x.data_ptr(), p.data_ptr(), o[NG - 1].data_ptr(), xi[NG - 1], pi[NG - 1], NPOLY, L, stream=st)

    def many():
        ctx.ct_pt_dot_many(x.data_ptr(), p.data_ptr(), outs["many"].data_ptr(), block, xi, pi, NPOLY, L, stream=st)

    modes = (("parent", parent), ("many", many))
    for _, call in modes:  # warm-up and the outputs that are compared
        call()
    torch.cuda.synchronize()
    same = torch.equal(outs["parent"], outs["many"])
    print("\n%s: R = %d, n_g = %d, %d primes: outputs equal: %s" % (name, R, NG, L, same))
    assert same
    times = {k: [] for k, _ in modes}
    e0, e1 = m.hip.Event(), m.hip.Event()
    for rep in range(REPS):
        for mode, call in modes:
            call()
            e0.record(st)
            for _ in range(CALLS):
                call()
            e1.record(st)
            torch.cuda.synchronize()
            times[mode].append(e1.elapsed_ms_since(e0) / CALLS)
    for mode, what in (("parent", "%d dot2 + %d dot" % (NG // 2, NG % 2)), ("many", "one moai_ct_pt_dot_many")):
        t = times[mode]
        med = statistics.median(t)
        print("  %-24s ms: %s  median %.2f, spread %.1f %%" % (what, " ".join("%.2f" % v for v in t), med, 100 * (max(t) - min(t)) / med))
    passes = (NG + 11) // 12
    t_mem = (passes * R * NPOLY + NG * R + NG * NPOLY) * L * N * 8 / 5.3e12 * 1e3
    t_int = NG * R * NPOLY * L * N * (4 * 4 + 6) / lane_hz * 1e3
    print("  one call against the composition: %.2fx; floors of the one call (computed): %.2f ms of operand, plaintext and output traffic, "
          "%.2f ms of integer issue" % (statistics.median(times["parent"]) / statistics.median(times["many"]), t_mem, t_int))
    ctx.close()
    del x, p, outs
