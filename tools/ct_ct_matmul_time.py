#!/usr/bin/env python3
"""The giant-step products of softmax(QK^T) V two ways in one process, alternating, at MOAI's shape (N = 2^16, col_W = 64 columns,
col_X = 128 diagonals: g = 12 baby steps, b = 11 giant steps, the last one 8 ciphertexts and 4 zero ones): one moai_ct_ct_matmul
against the 64 * 11 moai_ct_dot calls of the parent's shim, at a low level of MOAI's chain (4 primes, where the product runs) and a
middle one (15 primes, the highest its rotation keys serve).  The outputs are compared before anything is timed.  Beside the times,
the floors of the new call from the shapes alone --
  memory  every distinct operand ciphertext read once and the output written once at the 5.3 TB/s a copy reaches on this part
  MFMA    N * M tiles * N tiles * K-steps * (13 or 15 per prime) instructions at 16 clocks each on CUs * 4 SIMDs at the part's
          2.4 GHz peak clock."""
import os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import __graft_entry__ as g
import bench

m = g.load_package()
N, M, G, NB, NX, REPS, CALLS = 65536, 64, 12, 11, 128, 5, 2


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
simd_hz = cus * 4 * 2.4e9
print("device: %s, %d CUs" % (dev_name, cus))
for name, L in (("chain index 3", 4), ("chain index 14", 15)):
    primes = primes_of([51] + [46] * (L - 1))
    ctx = m.Context(16, primes)
    gen = torch.Generator(device=dev).manual_seed(7)
    a, b = (torch.stack([torch.randint(0, q, (cts, G, 2, N), dtype=torch.int64, device=dev, generator=gen) for q in primes], dim=3).contiguous()
            for cts in (M, NB))
    b.view(NB * G, 2, L, N)[NX:] = 0  # the zero ciphertexts behind the short last giant step
    outs = {k: torch.empty((NB, M, 3, L, N), dtype=torch.int64, device=dev) for k in ("dots", "matmul")}
    ctw = 2 * L * N * 8  # bytes per ciphertext

    def dots():
        for i in range(M):
            for j in range(NB):
                ctx.ct_dot(a.data_ptr() + i * G * ctw, b.data_ptr() + j * G * ctw, outs["dots"][j, i].data_ptr(), min(G, NX - j * G), L, stream=st)

    def matmul():
        ctx.ct_ct_matmul(a.data_ptr(), b.data_ptr(), outs["matmul"].data_ptr(), M, NB, G, L, stream=st)

    modes = (("dots", dots), ("matmul", matmul))
    for _, call in modes:  # warm-up and the outputs that are compared
        call()
    torch.cuda.synchronize()
    same = torch.equal(outs["dots"], outs["matmul"])
    print("\n%s, %d primes: outputs equal: %s" % (name, L, same))
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
    for mode, what in (("dots", "%d moai_ct_dot calls" % (M * NB)), ("matmul", "one moai_ct_ct_matmul")):
        t = times[mode]
        med = statistics.median(t)
        print("  %-22s ms: %s  median %.2f, spread %.1f %%" % (what, " ".join("%.2f" % v for v in t), med, 100 * (max(t) - min(t)) / med))
    t_mem = ((M + NB) * G * 2 + NB * M * 3) * L * N * 8 / 5.3e12 * 1e3
    mfmas = N * ((M + 7) // 8) * ((NB + 7) // 8) * ((G + 7) // 8) * sum(13 if q <= 1 << 54 else 15 for q in primes)
    print("  one call against the %d: %.2fx; floors of the one call: %.2f ms of operand and output traffic, %.2f ms of MFMA issue" % (
        M * NB, statistics.median(times["dots"]) / statistics.median(times["matmul"]), t_mem, mfmas * 16 / simd_hz * 1e3))
    ctx.close()
    del a, b, outs
