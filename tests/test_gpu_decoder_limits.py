"""csrc/decoder.hip at the limit primes of tests/mode_limits.py and on the directed edges of its composition and conversion, bit
for bit against the comparator tests/seal_decode.py and Python integers; the inputs come from tests/client_limit_cases.py, pinned by
tests/test_client_limits_cpu.py.

1. decode on both orders of the nine limit primes (the inverse transform before dec_compose in every arithmetic class at its limit),
   all nine rows and five permuted ones, at N = 8, 2^12, 2^13 and 2^16: encodings, uniform residues and the five residue patterns of
   ML.pattern_rows taken as NTT-form input;
2. every instantiation of dec_compose, NW = 1 .. 64, at both ends of its range of words, on 64 primes of 61 bits at N = 8, with the
   directed x of CL.composed_values: each alone in coefficient 0 (every slot then holds the conversion of x itself, so one wrong word
   shows on its own) and eight at a time in the coefficients of one plaintext;
3. dec_decrypt at sizes 2 .. 5 (the recurrence of the powers of s from size 4 on) with operands q - 1 against q - 1, 0, q/2 against
   q/2 + 1 under every limit prime."""
import numpy as np
import pytest

import client_limit_cases as CL
import mode_limits as ML
import oracle as O
import seal_decode as SD
from test_gpu_decoder import _decrypt_ints, assert_same

pytestmark = pytest.mark.gpu

K = 9
ROWS5 = [7, 2, 8, 0, 4]
_ctxs = {}


@pytest.fixture(scope="module", autouse=True)
def release_device_contexts():
    yield
    for entry in _ctxs.values():
        entry[-1].close()
    _ctxs.clear()


def contexts(moai, logn, primes):
    """(oracle context, oracle encoder, device context), one chain at a time"""
    key = (logn, tuple(primes))
    if key not in _ctxs:
        for k in list(_ctxs):
            _ctxs.pop(k)[-1].close()
        octx = O.Context(logn, primes)
        _ctxs[key] = (octx, O.CkksEncoder(octx), moai.Context(logn, primes))
    return _ctxs[key]


def up(moai, a):
    return moai.DeviceBuffer.from_numpy(a)


# ---- 1. the limit chains ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", CL.ORDER_NAMES)
@pytest.mark.parametrize("logn", [3, 12, 13, 16])
def test_decode_limit_chains(moai, logn, order):
    n = 1 << logn
    slots = n // 2
    primes = ML.ordered(logn, order)
    octx, enc, ctx = contexts(moai, logn, primes)
    rng = np.random.default_rng(6400 + logn)
    scale = 2.0**40
    vals = [rng.normal(size=slots) + 1j * rng.normal(size=slots), rng.uniform(-100, 100, size=slots)]
    # two encodings, uniform residues, the five patterns; under all nine rows and under the permuted five
    for L, pidx in ((K, None), (len(ROWS5), ROWS5)):
        sub = primes if pidx is None else [primes[i] for i in pidx]
        plain = np.concatenate([np.stack([enc.encode(v, L, scale, prime_index=pidx) for v in vals]),
                                O.uniform_rns(rng, sub, (1,), n), ML.pattern_rows(sub, n, rng)])
        B = plain.shape[0]
        d = up(moai, plain)
        got_c = ctx.ckks_decode(d, L, scale, n_batch=B, prime_index=pidx, is_complex=True)
        got_r = ctx.ckks_decode(d, L, scale, n_batch=B, prime_index=pidx)
        for b in range(B):
            want = SD.decode(octx, enc, plain[b], L, scale, prime_index=pidx, is_complex=True)
            assert np.isfinite(want).all()
            assert_same(got_c[b], want)
            assert_same(got_r[b], np.ascontiguousarray(want.real))  # from_complex<double>: the real part of the same value
        assert (d.to_numpy(plain.shape) == plain).all()


# ---- 2. the directed values on every instantiation of dec_compose -----------------------------------------------------------
@pytest.mark.parametrize("L", CL.DEC_LEVELS)
def test_decode_directed_values(moai, L):
    logn, n = CL.DEC_LOGN, 1 << CL.DEC_LOGN
    chain = CL.decoder_chain()
    octx, enc, ctx = contexts(moai, logn, chain)
    primes = chain[:L]
    names, xs, res = CL.composed_values(primes)
    scale = CL.decoder_scale(L)
    conv = SD.convert(np.array(xs, dtype=object), primes, scale)
    overflow = CL.overflow_names(L)
    assert {nm for nm, v in zip(names, conv) if not np.isfinite(v)} == overflow
    # layout one: x alone in coefficient 0
    plain = octx.ntt(CL.coefficient_rows(res, n), L).reshape(len(xs), L, n)
    got_c = ctx.ckks_decode(up(moai, plain), L, scale, n_batch=len(xs), is_complex=True)
    got_r = ctx.ckks_decode(up(moai, plain), L, scale, n_batch=len(xs))
    for i, nm in enumerate(names):
        want = SD.decode(octx, enc, plain[i], L, scale, is_complex=True)
        try:
            assert_same(got_c[i], want)
            assert_same(got_r[i], np.ascontiguousarray(want.real))
            if nm not in overflow:
                # every slot is the conversion of x itself
                assert (got_c[i].real.view(np.uint64) == conv[i:i + 1].view(np.uint64)).all()
                assert (np.ascontiguousarray(got_c[i].imag).view(np.uint64) == 0).all()
        except AssertionError as e:
            raise AssertionError("x = %s (L = %d): %s" % (nm, L, e)) from None
    # layout two: eight values at a time in the coefficients of one plaintext
    plain = octx.ntt(CL.coefficient_rows(res, n, fill=True), L).reshape(-1, L, n)
    B = plain.shape[0]
    got_c = ctx.ckks_decode(up(moai, plain), L, scale, n_batch=B, is_complex=True)
    got_r = ctx.ckks_decode(up(moai, plain), L, scale, n_batch=B)
    for b in range(B):
        want = SD.decode(octx, enc, plain[b], L, scale, is_complex=True)
        try:
            assert_same(got_c[b], want)
            assert_same(got_r[b], np.ascontiguousarray(want.real))
        except AssertionError as e:
            raise AssertionError("x = %s (L = %d): %s" % (names[n * b:n * b + n], L, e)) from None


# ---- 3. decrypt -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", CL.ORDER_NAMES)
@pytest.mark.parametrize("logn", [3, 8, 12])
def test_decrypt_limit_operands(moai, logn, order):
    """ciphertext 0: c_1 against the key on the operand pairs of ML.pair_rows, the other polynomials from the patterns (all q - 1 first);
    ciphertext 1: uniform.  Two keys: the pair operand, and all q - 1 (then q - 1 meets q - 1 in every product and power)."""
    n = 1 << logn
    primes = ML.ordered(logn, order)
    octx, enc, ctx = contexts(moai, logn, primes)
    rng = np.random.default_rng(6500 + logn)
    for L, pidx in ((K, list(range(K))), (len(ROWS5), ROWS5)):
        sub = [primes[i] for i in pidx]
        a, b = ML.pair_rows(sub, 1, n, rng)
        pat = ML.pattern_rows(sub, n, rng)
        keys = {"pairs": b[0], "all q-1": pat[0]}
        for size in (2, 3, 4, 5):
            ct = O.uniform_rns(rng, sub, (2, size), n)
            ct[0, 0] = pat[0]
            ct[0, 1] = a[0]
            for p in range(2, size):
                ct[0, p] = pat[(0, 3, 2)[p - 2]]
            for name, sk in keys.items():
                s_full = np.zeros((K, n), dtype=np.uint64)
                s_full[pidx] = sk
                got = ctx.decrypt(up(moai, ct), size, up(moai, np.ascontiguousarray(sk)), L, n_batch=2,
                                  prime_index=None if L == K else pidx).to_numpy((2, L, n))
                for i in range(2):
                    assert (got[i] == _decrypt_ints(ct[i], s_full, primes, pidx)).all(), (L, size, name, i)
