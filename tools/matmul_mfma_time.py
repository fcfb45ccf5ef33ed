#!/usr/bin/env python3
"""moai_ct_pt_matmul three ways -- the FP64 kernel, the integer kernel, the int8 matrix cores (MOAI_MATMUL_MFMA=1) -- in one
process, alternating, at N = 2^16 and 16 primes: MOAI's attention shape 768 x 64, a 768 x 256 slice of the intermediate product,
and 768 x 64 on a level with a 58-bit prime (where the default is the integer kernel).  The outputs of the three are compared
before anything is timed.  Beside the times: the floors of the matrix-core path, from the shapes alone --
  MFMA   rows/8 * cols/16 * N/16 * size * (13 or 15 per prime) instructions at 16 clocks each on CUs * 4 SIMDs at the part's
         2.4 GHz peak clock
  X      one read of X and one write of the output at the 5.3 TB/s a copy reaches on this part."""
import os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import __graft_entry__ as g
import bench

m = g.load_package()
N, L, ROWS, REPS = 65536, 16, 768, 5
MODES = [("fp64", dict(MOAI_MATMUL_MFMA=0, MOAI_MATMUL_FP=1)), ("int", dict(MOAI_MATMUL_MFMA=0, MOAI_MATMUL_FP=0)),
         ("mfma", dict(MOAI_MATMUL_MFMA=1))]


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
for name, bits, cols, calls in (("768x64 attention", [51] + [46] * 15, 64, 6), ("768x256 intermediate slice", [51] + [46] * 15, 256, 2),
                                ("768x64, level with a 58-bit prime", [58, 51] + [46] * 14, 64, 6)):
    primes = primes_of(bits)
    ctx = m.Context(16, primes)
    gen = torch.Generator(device=dev).manual_seed(7)
    x = torch.stack([torch.randint(0, q, (ROWS, 2, N), dtype=torch.int64, device=dev, generator=gen) for q in primes], dim=2).contiguous()
    w = torch.stack([torch.randint(0, q, (ROWS, cols), dtype=torch.int64, device=dev, generator=gen) for q in primes]).contiguous()
    outs = {k: torch.empty((cols, 2, L, N), dtype=torch.int64, device=dev) for k, _ in MODES}

    def call(mode, knobs):
        for k, v in knobs.items():
            m.hip.set_tuning(k, v)
        ctx.ct_pt_matmul(x.data_ptr(), w.data_ptr(), outs[mode].data_ptr(), ROWS, cols, 2, L, stream=st)

    paths = {}
    for mode, knobs in MODES:  # warm-up and the outputs that are compared
        call(mode, knobs)
        paths[mode] = ctx.ct_pt_matmul_path(ROWS, cols, 2, L)
    torch.cuda.synchronize()
    same = all(torch.equal(outs["mfma"], outs[k]) for k in ("fp64", "int"))
    print("\n%s: paths %s, outputs equal: %s" % (name, paths, same))
    assert same
    times = {k: [] for k, _ in MODES}
    e0, e1 = m.hip.Event(), m.hip.Event()
    for rep in range(REPS):
        for mode, knobs in MODES:
            call(mode, knobs)
            e0.record(st)
            for _ in range(calls):
                call(mode, knobs)
            e1.record(st)
            torch.cuda.synchronize()
            times[mode].append(e1.elapsed_ms_since(e0) / calls)
    m.hip.reset_tuning()
    default = "int" if max(primes) >= 1 << 51 else "fp64"
    macs = ROWS * cols * 2 * L * N
    for mode, _ in MODES:
        t = times[mode]
        med = statistics.median(t)
        print("  %-5s ms per call: %s  median %.2f, spread %.1f %%, %.2f T modular MAC/s%s" % (
            mode, " ".join("%.2f" % v for v in t), med, 100 * (max(t) - min(t)) / med, macs / med / 1e9,
            "  <- the default path of this level" if mode == default else ""))
    mfmas = (ROWS // 8) * ((cols + 15) // 16) * (N // 16) * 2 * sum(13 if q <= 1 << 54 else 15 for q in primes)
    t_mfma = mfmas * 16 / simd_hz * 1e3
    t_mem = (x.numel() + outs["mfma"].numel()) * 8 / 5.3e12 * 1e3
    print("  mfma against the default path: %.2fx; floors of the mfma path: %.2f ms of MFMA issue, %.2f ms of X and output traffic" % (
        statistics.median(times[default]) / statistics.median(times["mfma"]), t_mfma, t_mem))
    ctx.close()
    del x, w, outs
