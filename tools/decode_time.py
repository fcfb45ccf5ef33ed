#!/usr/bin/env python3
"""Decryptor::decrypt and CKKSEncoder::decode on the device at MOAI's parameters (N = 2^16, the 36-prime chain): moai_decrypt
and moai_ckks_decode timed separately with the library's events on one stream, for L in {3, 8, 21, 36} x n_batch in
{1, 64, 768}.  Inputs are uniformly random residues (size-2 ciphertexts; plaintexts for the decode).  Prints one JSON line:
microseconds per ciphertext for each (L, n_batch)."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import torch  # noqa: E402  (before the library: one HIP runtime per process, tests/conftest.py)

import __graft_entry__ as g  # noqa: E402
import oracle as O  # noqa: E402

m = g.load_package()
N = 1 << 16
primes = O.coeff_modulus_create(N, [51] + [46] * 20 + [51] * 14 + [58])
ctx = m.Context(16, primes)
dev = torch.device("cuda")
st = torch.cuda.current_stream().cuda_stream
lib = m.hip.lib()
gen = torch.Generator(device=dev)
gen.manual_seed(0)


def residues(shape_prefix, L):
    """int64 [*shape_prefix][L][N], row r uniform in [0, q_r)"""
    t = torch.empty(tuple(shape_prefix) + (L, N), dtype=torch.int64, device=dev)
    for r in range(L):
        t[..., r, :] = torch.randint(0, primes[r], tuple(shape_prefix) + (N,), generator=gen, device=dev, dtype=torch.int64)
    return t


def timed(run, reps):
    run()
    torch.cuda.synchronize()
    e0, e1 = m.hip.Event(), m.hip.Event()
    e0.record(st)
    for _ in range(reps):
        run()
    e1.record(st)
    return e1.elapsed_ms_since(e0) / reps


out = {"N": N, "unit": "us per ciphertext", "decrypt": {}, "decode": {}}
sk = residues((), len(primes))
for L in (3, 8, 21, 36):
    for B in (1, 64, 768):
        reps = 20 if B * L <= 64 * 8 else 3
        ct = residues((B, 2), L)
        pt = torch.empty((B, L, N), dtype=torch.int64, device=dev)
        vals = torch.empty((B, N // 2), dtype=torch.float64, device=dev)
        scales = (m.hip.C.c_double * B)(*([2.0**46] * B))

        def dec():
            m.hip._check(lib.moai_decrypt(ctx.h, ct.data_ptr(), 2, sk.data_ptr(), pt.data_ptr(), B, L, None, st))

        def decode():
            m.hip._check(lib.moai_ckks_decode(ctx.h, pt.data_ptr(), B, L, None, scales, 0, vals.data_ptr(), st))

        key = "%d,%d" % (L, B)
        out["decrypt"][key] = round(timed(dec, reps) * 1e3 / B, 2)
        out["decode"][key] = round(timed(decode, reps) * 1e3 / B, 2)
        print("L %2d batch %4d: decrypt %9.2f us/ct, decode %9.2f us/ct" % (L, B, out["decrypt"][key], out["decode"][key]),
              file=sys.stderr, flush=True)
        del ct, pt, vals
        torch.cuda.empty_cache()
print(json.dumps(out))
