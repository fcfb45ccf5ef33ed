"""Pins the decode comparator (tests/seal_decode.py) that the device decoder is held to bit for bit: round trips with the
oracle encoder, agreement with the independent Vandermonde decoder, the sign threshold, and that the conversion follows
the reference's word-by-word arithmetic (ckks.h:713-753) rather than exact arithmetic.  CPU only."""
import numpy as np
import pytest

import oracle as O
import seal_decode as SD
from ckks_toy import decode_slots


@pytest.mark.parametrize("logn", range(3, 14))
def test_round_trip_with_oracle_encoder(logn):
    n = 1 << logn
    ctx = O.Context(logn, O.coeff_modulus_create(n, [60, 60, 60, 60]))
    enc = O.CkksEncoder(ctx)
    rng = np.random.default_rng(logn)
    # integer data below 2^30 at delta 2^40: |error| < 0.5 (native/tests/seal/ckks.cpp:20-137, test_oracle_encoder.py)
    vals = rng.integers(0, 1 << 30, size=n // 2).astype(np.float64)
    back = SD.decode(ctx, enc, enc.encode(vals, 4, 2.0**40), 4, 2.0**40)
    assert np.max(np.abs(back - vals)) < 0.5
    # complex values at delta 2^40 (test_complex_values_and_levels: 1e-8 at n = 128; the error grows like n)
    z = rng.normal(size=n // 2) + 1j * rng.normal(size=n // 2)
    back = SD.decode(ctx, enc, enc.encode(z, 3, 2.0**40), 3, 2.0**40, is_complex=True)
    assert np.max(np.abs(back - z)) < 1e-8 * max(1, n // 128)


@pytest.mark.parametrize("logn", [3, 5, 7])
def test_agrees_with_vandermonde_decoder(logn):
    n = 1 << logn
    primes = O.coeff_modulus_create(n, [51, 46, 58])
    ctx = O.Context(logn, primes)
    enc = O.CkksEncoder(ctx)
    rng = np.random.default_rng(7 + logn)
    plain = O.uniform_rns(rng, primes, (), n)
    got = SD.decode(ctx, enc, plain, 3, 2.0**60, is_complex=True)
    coeff = ctx.ntt(plain[None], 3, inverse=True)[0]
    x = SD.compose(coeff, primes)
    Q = SD.product(primes)
    centred = [int(v) - Q if int(v) > Q // 2 else int(v) for v in x]
    want = decode_slots(centred, n, 2.0**60)
    assert np.allclose(got, want, rtol=1e-9, atol=1e-9 * np.max(np.abs(want)))


def test_sign_threshold_edges():
    logn = 4
    n = 1 << logn
    primes = O.coeff_modulus_create(n, [40, 50, 60])
    Q = SD.product(primes)
    xs = np.array([0, (Q - 1) // 2, (Q + 1) // 2, Q - 1], dtype=object)
    res = SD.convert(xs, primes, 1.0)
    assert res[0] == 0.0
    assert res[1] > 0 and res[2] < 0  # the branch flips exactly between (Q-1)/2 and (Q+1)/2
    assert res[1] == pytest.approx(Q / 2, rel=1e-15) and res[2] == pytest.approx(-Q / 2, rel=1e-15)
    assert res[3] == -1.0
    # through the whole decode: a constant polynomial c decodes to c / scale in every slot, exactly
    ctx = O.Context(logn, primes)
    enc = O.CkksEncoder(ctx)
    for x, want in zip(xs, res):
        coeff = np.zeros((3, n), dtype=np.uint64)
        coeff[:, 0] = [int(x) % q for q in primes]
        plain = ctx.ntt(coeff[None], 3)[0]
        out = SD.decode(ctx, enc, plain, 3, 1.0)
        assert (out.view(np.uint64) == np.float64(want).view(np.uint64)).all()


def test_negative_branch_is_not_exact_arithmetic():
    # The reference converts a negative coefficient word by word, x_j > Q_j ? +(x_j - Q_j) : -(Q_j - x_j), each term rounded
    # on its own: not float(x - Q).  Find an x where the two differ in the last bit and check the comparator gives the
    # reference's value.
    primes = O.coeff_modulus_create(16, [60, 60, 60])
    Q = SD.product(primes)
    qw = [(Q >> (64 * j)) & ((1 << 64) - 1) for j in range(3)]
    rng = np.random.default_rng(11)
    found = None
    for _ in range(2000):
        # close to Q: the top word difference is small, the lower words' differences are rounded on their own
        x = Q - 1 - int.from_bytes(rng.bytes(16), "little")
        xw = [(x >> (64 * j)) & ((1 << 64) - 1) for j in range(3)]
        seal = 0.0
        f = 1.0
        for j in range(3):
            d = xw[j] - qw[j]
            if d > 0:
                seal += float(d) * f
            else:
                seal -= float(-d) * f if d else 0.0
            f *= 2.0**64
        if seal != float(x - Q):
            found = (x, seal)
            break
    assert found is not None, "no x within the search where word-by-word and exact conversion differ"
    x, seal = found
    got = SD.convert(np.array([x], dtype=object), primes, 1.0)[0]
    assert got == seal and got != float(x - Q)
