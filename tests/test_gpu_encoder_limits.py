"""csrc/encoder.hip at the limit primes of tests/mode_limits.py and on its directed edges, bit for bit against the oracle's
CKKSEncoder (tests/oracle.py); the inputs come from tests/client_limit_cases.py, pinned by tests/test_client_limits_cpu.py.

1. every degree class of the two kernels (logn 3 .. 5: fewer coefficients than a workgroup has lanes; 8, 9, 11: one LDS tile, 11 the
   largest; 12: the sixteen-per-thread tile; 13 and 16: one and four strided stages in ckks_fft_finish) on both orders of the nine
   limit primes, so that the forward transform after ckks_fft_finish runs in every arithmetic class at its limit, with all nine rows
   and with five permuted ones; complex, real and short complex input; max_coeff bit for bit against the restated coefficients,
   three different maxima per call (the atomic maximum across workgroups, the idle lanes below N = 256);
2. coefficients mantissa * 2^sh on the arms of split_rounded (sh = 0, 1 .. 11, 12 and up), on the 63-bit steps of residue_shifted
   and on the reference's 64- and 128-bit branch boundaries, both signs, among them negative multiples of a chain prime (the sign
   fix's r == 0);
3. constants on the boundaries of std::round;
4. slot vectors whose coefficients straddle 2^53 and 2^64 inside one thread of ckks_fft_finish (any_shift sends coefficients without
   a shift through residue_shifted)."""
import numpy as np
import pytest

import client_limit_cases as CL
import mode_limits as ML
import oracle as O

pytestmark = pytest.mark.gpu

K = 9
ROWS5 = [7, 2, 8, 0, 4]  # a permuted subset: row r is not prime r, classes interleave in both orders
_ctxs = {}


@pytest.fixture(scope="module", autouse=True)
def release_device_contexts():
    yield
    for entry in _ctxs.values():
        entry[3].close()
    _ctxs.clear()


def contexts(moai, logn, order):
    """(primes, oracle context, oracle encoder, device context), one degree at a time"""
    if (logn, order) not in _ctxs:
        for key in [k for k in _ctxs if k[0] != logn]:
            _ctxs.pop(key)[3].close()
        primes = ML.ordered(logn, order)
        octx = O.Context(logn, primes)
        _ctxs[(logn, order)] = (primes, octx, O.CkksEncoder(octx), moai.Context(logn, primes))
    return _ctxs[(logn, order)]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.mark.parametrize("order", CL.ORDER_NAMES)
@pytest.mark.parametrize("logn", [3, 4, 5, 8, 9, 11, 12, 13, 16])
def test_encode_limit_chains(moai, logn, order):
    n = 1 << logn
    slots = n // 2
    primes, octx, enc, ctx = contexts(moai, logn, order)
    idx, roots = ctx.ckks_tables()
    assert (idx == enc.index_map).all() and (roots.view(np.uint64) == enc.inv_root_powers.view(np.uint64)).all()
    rng = np.random.default_rng(6100 + logn)
    scale = 2.0**40
    factors = np.array([1.0, 1000.0, 1e-3])[:, None]  # three maxima per call
    short = max(slots // 3, 1)
    batches = [(rng.normal(size=(3, slots)) + 1j * rng.normal(size=(3, slots))) * factors,
               rng.normal(size=(3, slots)) * factors,
               (rng.normal(size=(3, short)) + 1j * rng.normal(size=(3, short))) * factors]
    for vals in batches:
        want_mx = [np.abs(CL.restated_coefficients(enc, v, scale)).max() for v in vals]
        assert len(set(want_mx)) == 3
        for L, pidx in ((K, None), (len(ROWS5), ROWS5)):
            out, mx = ctx.ckks_encode(vals, L, scale, prime_index=pidx)
            got = out.to_numpy((3, L, n))
            for b in range(3):
                assert (got[b] == enc.encode(vals[b], L, scale, prime_index=pidx)).all(), (L, b)
            assert (_bits(mx) == _bits(want_mx)).all(), (L, mx, want_mx)
    # values_size 0 and 1
    for vals in (np.zeros((2, 0)), np.array([[1.25], [-3e3]]), np.array([[0.5 - 2j], [1e3 + 1j]])):
        out, mx = ctx.ckks_encode(vals, K, scale)
        got = out.to_numpy((2, K, n))
        for b in range(2):
            assert (got[b] == enc.encode(vals[b], K, scale)).all(), vals[b]
            assert _bits(mx[b]) == _bits(np.abs(CL.restated_coefficients(enc, vals[b], scale)).max())
    assert not ctx.ckks_encode(np.zeros((2, 0)), K, scale)[0].to_numpy().any()


@pytest.mark.parametrize("logn", [3, 12, 13, 16])
def test_encode_directed_magnitudes(moai, logn):
    """one call per sh, the four mantissas and two signs as its batch of eight constant vectors"""
    n = 1 << logn
    primes, octx, enc, ctx = contexts(moai, logn, "g61_last")
    cases = CL.encoder_magnitudes(primes)
    for sh in CL.ENC_SHIFTS:
        batch = [(m, s) for m, sh_, s in cases if sh_ == sh]
        assert len(batch) == 8
        vals = np.stack([CL.constant_slots(s * m, logn) for m, s in batch])
        out, mx = ctx.ckks_encode(vals, K, 2.0**sh)
        got = out.to_numpy((8, K, n))
        for b, (m, s) in enumerate(batch):
            assert (got[b] == enc.encode(vals[b], K, 2.0**sh)).all(), (sh, m, s)
            assert _bits(mx[b]) == _bits(float(m) * 2.0**sh), (sh, m, s)


@pytest.mark.parametrize("logn", [3, 13])
def test_encode_rounding_constants(moai, logn):
    n = 1 << logn
    primes, octx, enc, ctx = contexts(moai, logn, "g61_last")
    consts = CL.rounding_constants()
    vals = np.stack([CL.constant_slots(c, logn) for c, _ in consts])
    out, mx = ctx.ckks_encode(vals, K, 1.0)
    got = out.to_numpy((len(consts), K, n))
    coeff = octx.ntt(got, K, inverse=True).reshape(got.shape)
    for b, (c, v) in enumerate(consts):
        assert (got[b] == enc.encode(vals[b], K, 1.0)).all(), c
        # and the integer itself: coefficient 0 is v, the rest 0
        assert coeff[b, :, 0].tolist() == [v % q for q in primes] and not coeff[b, :, 1:].any(), c
        assert _bits(mx[b]) == _bits(abs(c))


@pytest.mark.parametrize("logn", [13, 16])
def test_encode_straddling_coefficients(moai, logn):
    n = 1 << logn
    primes, octx, enc, ctx = contexts(moai, logn, "g61_last")
    for v, scale in CL.straddling_vectors(enc, logn, np.random.default_rng(6300 + logn)):
        out, mx = ctx.ckks_encode(v, K, scale)
        assert (out.to_numpy((K, n)) == enc.encode(v, K, scale)).all(), scale
        assert _bits(mx[0]) == _bits(np.abs(CL.restated_coefficients(enc, v, scale)).max())
