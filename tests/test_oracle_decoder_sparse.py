"""Pins the sparse-decode comparator (tests/seal_decode_sparse.py) that moai_ckks_decode_sparse is held to bit for bit:
against a direct evaluation of the projected plaintext polynomial at the sparse roots, and at sparse_slots = N/2 against
the full-slot comparator.  CPU only."""
import numpy as np
import pytest

import oracle as O
import seal_decode as SD
import seal_decode_sparse as SDS


def _centred(x, Q):
    return [int(v) - Q if int(v) >= (Q + 1) // 2 else int(v) for v in x]


@pytest.mark.parametrize("logn", [3, 5, 7])
def test_matches_evaluation_at_sparse_roots(logn):
    n = 1 << logn
    primes = O.coeff_modulus_create(n, [51, 46, 58])
    ctx = O.Context(logn, primes)
    enc = O.CkksEncoder(ctx)
    rng = np.random.default_rng(40 + logn)
    plain = O.uniform_rns(rng, primes, (), n)
    coeff = ctx.ntt(plain[None], 3, inverse=True)[0]
    c = _centred(SD.compose(coeff, primes), SD.product(primes))
    scale = 2.0**60
    for sparse in [n // 2, n // 4, 2, 1]:
        sparsity = (n // 2) // sparse
        got = SDS.decode(ctx, enc, plain, 3, scale, sparse, is_complex=True)
        assert got.shape == (sparse,)
        # the projected polynomial sum_j c_{j s} Y^j, Y = X^s, at X = zeta^(5^i): Y = exp(2 pi i 5^i / (4 sparse))
        j = np.arange(2 * sparse)
        cj = np.array([float(c[k * sparsity]) for k in range(2 * sparse)])
        want = np.array([np.sum(cj * np.exp(2j * np.pi * ((pow(5, i, 4 * sparse) * j) % (4 * sparse)) / (4 * sparse)))
                         for i in range(sparse)]) / scale
        assert np.allclose(got, want, rtol=1e-9, atol=1e-9 * np.max(np.abs(want)))


@pytest.mark.parametrize("logn", [4, 6])
def test_full_slot_count_is_the_full_decode(logn):
    n = 1 << logn
    primes = O.coeff_modulus_create(n, [40, 50, 60])
    ctx = O.Context(logn, primes)
    enc = O.CkksEncoder(ctx)
    rng = np.random.default_rng(logn)
    plain = O.uniform_rns(rng, primes, (), n)
    for is_complex in (False, True):
        a = SDS.decode(ctx, enc, plain, 3, 2.0**50, n // 2, is_complex=is_complex)
        b = SD.decode(ctx, enc, plain, 3, 2.0**50, is_complex=is_complex)
        assert (np.ascontiguousarray(a).view(np.uint64) == np.ascontiguousarray(b).view(np.uint64)).all()


def test_sparse_encoding_round_trip():
    # a message of n values replicated N/(2n) times (what a sparse-slot caller encodes) decodes to itself
    logn, sparse = 7, 8
    n = 1 << logn
    primes = O.coeff_modulus_create(n, [60, 60, 60])
    ctx = O.Context(logn, primes)
    enc = O.CkksEncoder(ctx)
    rng = np.random.default_rng(3)
    z = rng.normal(size=sparse) + 1j * rng.normal(size=sparse)
    plain = enc.encode(np.tile(z, (n // 2) // sparse), 3, 2.0**40)
    got = SDS.decode(ctx, enc, plain, 3, 2.0**40, sparse, is_complex=True)
    assert np.max(np.abs(got - z)) < 1e-8
    # and the projection zeroes exactly the coefficients off the subring
    coeff = ctx.ntt(plain[None], 3, inverse=True)[0]
    x = SD.compose(coeff, primes)
    px = SDS.project(x, sparse)
    s = (n // 2) // sparse
    assert all(int(px[i]) == (int(x[i]) if i % s == 0 else 0) for i in range(n))
