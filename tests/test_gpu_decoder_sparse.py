"""GPU parity of moai_ckks_decode_sparse (CKKSEncoder::decode with sparse_slots set, SEAL/ckks.h:703-713, :757-760)
against the comparator tests/seal_decode_sparse.py, bit for bit; at sparse_slots = N/2 against moai_ckks_decode; invalid
sparse_slots refused before anything is enqueued; and the seal:: shim's CKKSEncoder / moai_fused::decrypt_decode with
EncryptionParameters::set_sparse_slots (tests/cpp_sparse/test_bootstrap_sparse.cpp, mode decode)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import oracle as O
import seal_decode_sparse as SDS

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MOAI_BITS = [51] + [46] * 20 + [51] * 14 + [58]  # include/test/test_full_scheme.hpp:356-378


def assert_same(got, want):
    """bit-identical where the comparator is finite; non-finite exactly where it is non-finite"""
    got = np.ascontiguousarray(got).view(np.float64).ravel()
    want = np.ascontiguousarray(want).view(np.float64).ravel()
    fin = np.isfinite(want)
    assert (np.isfinite(got) == fin).all(), "non-finite positions differ"
    mism = np.nonzero(got[fin].view(np.uint64) != want[fin].view(np.uint64))[0]
    assert mism.size == 0, "%d of %d values differ, first at %d: %r vs %r" % (
        mism.size, fin.sum(), mism[0], got[fin][mism[0]], want[fin][mism[0]])


def _setup(logn, bits):
    primes = O.coeff_modulus_create(1 << logn, bits)
    return primes, O.Context(logn, primes), O.CkksEncoder(O.Context(logn, primes))


@pytest.mark.parametrize("logn,bits", [(10, [51, 46, 46, 58]), (16, MOAI_BITS[:3] + [58])])
@pytest.mark.parametrize("L", [1, 3])
def test_decode_sparse_matches_comparator(moai, logn, bits, L):
    n = 1 << logn
    primes, octx, enc = _setup(logn, bits)
    ctx = moai.Context(logn, primes)
    rng = np.random.default_rng(7 * logn + L)
    slots = n // 2
    scales = [2.0**40, 2.0**30 * 1.5, 2.0**46]
    plain = np.stack([enc.encode(np.tile(rng.normal(size=8) + 1j * rng.normal(size=8), slots // 8), L, scales[0]),
                      enc.encode(rng.uniform(-4, 4, size=slots) + 0j, L, scales[1]),
                      O.uniform_rns(rng, primes[:L], (), n)])  # every conversion branch
    d = moai.DeviceBuffer.from_numpy(plain)
    for sparse in (slots, slots // 4, slots // 16, 8):
        for is_complex in (False, True):
            got = ctx.ckks_decode_sparse(d, L, scales, sparse, n_batch=3, is_complex=is_complex)
            assert got.shape == (3, sparse)
            for b in range(3):
                assert_same(got[b], SDS.decode(octx, enc, plain[b], L, scales[b], sparse, is_complex=is_complex))
            if sparse == slots:
                full = ctx.ckks_decode(d, L, scales, n_batch=3, is_complex=is_complex)
                assert (np.ascontiguousarray(got).view(np.uint64) == np.ascontiguousarray(full).view(np.uint64)).all()
    assert (d.to_numpy(plain.shape) == plain).all()  # the input is not modified


def test_decode_sparse_rejects_bad_slot_counts(moai):
    logn = 10
    n = 1 << logn
    primes, octx, enc = _setup(logn, [51, 46, 58])
    ctx = moai.Context(logn, primes)
    plain = enc.encode(np.ones(n // 2), 2, 2.0**40)
    d = moai.DeviceBuffer.from_numpy(plain)
    for bad in (3, 12, n, n // 2 + 1):
        with pytest.raises(moai.hip.MoaiError) as e:
            ctx.ckks_decode_sparse(d, 2, 2.0**40, bad)
        assert e.value.code == -1 and "sparse_slots" in str(e.value)  # MOAI_EINVAL
    with pytest.raises(ValueError):
        ctx.ckks_decode_sparse(d, 2, 2.0**40, 0)
    # 0 at the C entry point itself: refused before the (null) output is touched
    scale = (ctypes.c_double * 1)(2.0**40)
    lib = moai.hip.lib()
    assert lib.moai_ckks_decode_sparse(ctx.h, d.ptr, 1, 2, None, scale, 0, 0, None, None) == -1
    assert "sparse_slots" in lib.moai_last_error().decode()
    # the context is still usable: nothing was enqueued
    assert_same(ctx.ckks_decode_sparse(d, 2, 2.0**40, 4)[0], SDS.decode(octx, enc, plain, 2, 2.0**40, 4))


def test_shim_sparse_decode():
    exe = os.path.join(ROOT, "tests", "cpp_sparse", "test_bootstrap_sparse")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", os.path.dirname(exe), "-s", "test_bootstrap_sparse"])
    r = subprocess.run([exe, "decode"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "ALL OK" in r.stdout
