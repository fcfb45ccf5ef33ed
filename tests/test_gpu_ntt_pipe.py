"""The pipelined chunk schedule of the two-pass transform (MOAI_NTT_PIPE side streams over MOAI_NTT_CHUNK_MB / _KB chunks,
csrc/ntt.hip ntt_launch) against the CPU oracle, bit for bit, and against the same call with MOAI_NTT_PIPE=0: ragged schedules
at the smallest two-pass size (a stream with a single chunk, a short last chunk), N = 2^16, the inverse transform that reads a
slice of another buffer (inside a key switch), the order of the work on the caller's stream with one and with two caller
streams in flight, and a batch below the schedule's threshold."""
import numpy as np
import pytest

import mode_limits as ML
import oracle as O

pytestmark = pytest.mark.gpu

_cases = {}


def case(logn, primes, n_poly, seed):
    """random canonical input [n_poly][L][N] with the oracle's forward and inverse transforms of it, computed once and never
    written to"""
    key = (logn, tuple(primes), n_poly)
    if key not in _cases:
        n, L = 1 << logn, len(primes)
        x = O.uniform_rns(np.random.default_rng(seed), primes, (n_poly,), n)
        octx = O.Context(logn, primes)
        c = dict(x=x, fwd=octx.ntt(x, L), inv=octx.ntt(x, L, inverse=True))
        for v in c.values():
            v.setflags(write=False)
        _cases[key] = c
    return _cases[key]


def set_schedule(moai, poly_bytes, chunk_polys, k, inner=0):
    """chunks of chunk_polys whole polynomials on k side streams (k = 0: one stream, the chunk loop alone)"""
    b = poly_bytes * chunk_polys
    assert b % 1024 == 0
    moai.hip.set_tuning("MOAI_NTT_CHUNK_MB", b >> 20)
    moai.hip.set_tuning("MOAI_NTT_CHUNK_KB", (b >> 10) & 1023)
    moai.hip.set_tuning("MOAI_NTT_PIPE", k)
    moai.hip.set_tuning("MOAI_NTT_PIPE_MIN", 1)  # the default keeps batches this small on the caller's stream
    moai.hip.set_tuning("MOAI_NTT_PIPE_INNER", inner)


def three_class_primes(moai, logn):
    """one prime just below 2^60, one of 61 bits, one of 46 bits: three arithmetic classes, so three pairs of launches per chunk"""
    primes = [ML.prime_at_most(logn, (1 << 60) - 1), ML.prime_at_most(logn, (1 << 61) - 1), ML.prime_at_most(logn, (1 << 46) - 1)]
    ctx = moai.Context(logn, primes)
    H = moai.hip
    for op in (H.MODE_OF_NTT_FORWARD, H.MODE_OF_NTT_INVERSE):
        assert len({ctx.arith_mode(i, op) for i in range(3)}) == 3
    return primes, ctx


def check_transforms(moai, ctx, c, n_poly, L, poly_bytes, chunk_polys, k, plan):
    """forward, inverse of the forward's output (the round trip) and inverse of the input under the schedule, each against the
    oracle and against MOAI_NTT_PIPE=0"""
    x = c["x"]
    assert moai.hip.ntt_pipe_plan(n_poly, L, ctx.n, poly_bytes * chunk_polys, k) == plan
    got = {}
    for pipe in (k, 0):
        set_schedule(moai, poly_bytes, chunk_polys, pipe)
        d = moai.DeviceBuffer.from_numpy(x)
        ctx.ntt_forward(d, n_poly, L)
        f = d.to_numpy(x.shape)
        ctx.ntt_inverse(d, n_poly, L)
        r = d.to_numpy(x.shape)
        d.upload(x)
        ctx.ntt_inverse(d, n_poly, L)
        got[pipe] = (f, r, d.to_numpy(x.shape))
    for name, i, exp in (("forward", 0, c["fwd"]), ("round trip", 1, x), ("inverse", 2, c["inv"])):
        assert (got[k][i] == exp).all(), name + " differs from the oracle"
        assert (got[k][i] == got[0][i]).all(), name + " differs from MOAI_NTT_PIPE=0"


@pytest.mark.parametrize("k", [2, 3])
@pytest.mark.parametrize("chunk_polys", [1, 2])
def test_ragged_schedule_at_the_smallest_two_pass_size(moai, chunk_polys, k):
    """N = 2^12, five polynomials of three rows in three arithmetic classes.  Chunks of one polynomial: 5 chunks, which K = 2
    deals 3 + 2 and K = 3 deals 2 + 2 + 1 (a stream with a single chunk).  Chunks of two: 2 + 2 + 1 polynomials (a short last
    chunk), which K = 2 deals 2 + 1 and K = 3 one to each stream."""
    logn, n_poly = 12, 5
    primes, ctx = three_class_primes(moai, logn)
    L, poly_bytes = 3, 3 * 8 << logn
    plan = {(1, 2): 3, (1, 3): 2, (2, 2): 2, (2, 3): 1}[(chunk_polys, k)]
    try:
        check_transforms(moai, ctx, case(logn, primes, n_poly, 1201), n_poly, L, poly_bytes, chunk_polys, k, plan)
    finally:
        moai.hip.reset_tuning()


def test_n16_chunks_of_one_polynomial(moai):
    """N = 2^16, a 60-bit and a 51-bit prime, six polynomials as six chunks of 1 MiB on two side streams"""
    logn, n_poly, L = 16, 6, 2
    primes = [ML.prime_at_most(logn, (1 << 60) - 1), ML.prime_at_most(logn, (1 << 51) - 1)]
    ctx = moai.Context(logn, primes)
    try:
        check_transforms(moai, ctx, case(logn, primes, n_poly, 1601), n_poly, L, L * 8 << logn, 1, 2, 3)
    finally:
        moai.hip.reset_tuning()


def test_inverse_from_a_source_slice_inside_a_key_switch(moai):
    """No entry point hands the tests the inverse transform that reads a slice of another buffer; the key switch starts with
    one (c1 of every ciphertext, csrc/keyswitch.hip switch_key_impl).  N = 2^12, l = 3, four ciphertexts = four polynomials
    for that transform, chunks of one polynomial on two side streams, the schedule switched on for the library's own transforms
    (MOAI_NTT_PIPE_INNER)."""
    logn, L, B = 12, 3, 4
    n = 1 << logn
    primes = O.coeff_modulus_create(n, [51, 46, 46, 58])
    octx = O.Context(logn, primes)
    ctx = moai.Context(logn, primes)
    rng = np.random.default_rng(1203)
    key = O.uniform_rns(rng, primes, (len(primes) - 1, 2), n)
    ct = O.uniform_rns(rng, primes[:L], (B, 2), n)
    elt = ctx.galois_elt_from_step(1)
    exp = np.stack([octx.apply_galois(ct[b], L, elt, key).reshape(2, L, n) for b in range(B)])
    dkey = moai.DeviceBuffer.from_numpy(key)
    assert moai.hip.ntt_pipe_plan(B, L, n, L * n * 8, 2) == 2
    got = {}
    try:
        for pipe in (2, 0):
            set_schedule(moai, L * n * 8, 1, pipe, inner=1)
            d = moai.DeviceBuffer.from_numpy(ct)
            ctx.apply_galois(d, L, elt, dkey, B)
            got[pipe] = d.to_numpy(ct.shape)
    finally:
        moai.hip.reset_tuning()
    assert (got[2] == exp).all(), "key switch under the schedule differs from the oracle"
    assert (got[2] == got[0]).all(), "key switch under the schedule differs from MOAI_NTT_PIPE=0"


@pytest.mark.parametrize("callers", [1, 2])
def test_order_on_the_callers_stream(moai, callers):
    """On a torch stream that is not the default one: a torch kernel fills the input, ntt_forward follows with no
    synchronisation, a torch copy of the result follows on the same stream; one synchronisation at the end.  The fork has to
    hold the side streams behind the fill and the join the copy behind the side streams.  With two caller streams in flight on
    disjoint buffers, each has side streams of its own."""
    import torch

    logn, n_poly = 12, 5
    primes, ctx = three_class_primes(moai, logn)
    L, n = 3, 1 << logn
    c = case(logn, primes, n_poly, 1201)
    dev = torch.device("cuda", 0)
    host = torch.from_numpy(np.array(c["x"]).view(np.int64)).pin_memory()
    streams = [torch.cuda.Stream(device=dev) for _ in range(callers)]
    staged = [torch.empty(host.shape, dtype=torch.int64, device=dev) for _ in streams]
    work = [torch.zeros(host.shape, dtype=torch.int64, device=dev) for _ in streams]
    out = [torch.zeros(host.shape, dtype=torch.int64, device=dev) for _ in streams]
    for t in staged:
        t.copy_(host)
    torch.cuda.synchronize()
    try:
        set_schedule(moai, L * n * 8, 1, 3)
        for _ in range(2):  # the second round reuses the side streams and events of the first
            for w, o in zip(work, out):
                w.zero_()
                o.zero_()
            torch.cuda.synchronize()
            for s, st, w, o in zip(streams, staged, work, out):
                with torch.cuda.stream(s):
                    w.add_(st)  # a torch kernel on s writes the input
                    ctx.ntt_forward(w.data_ptr(), n_poly, L, stream=s.cuda_stream)
                    o.copy_(w)
            torch.cuda.synchronize()
            for o in out:
                assert (o.cpu().numpy().view(np.uint64) == c["fwd"]).all()
    finally:
        moai.hip.reset_tuning()


def test_single_polynomial_stays_on_the_callers_stream(moai):
    """n_poly = 1 with the schedule on: one chunk, nothing to run beside, the plan is 0 and the result is right"""
    logn, n_poly = 12, 1
    primes, ctx = three_class_primes(moai, logn)
    try:
        check_transforms(moai, ctx, case(logn, primes, n_poly, 1202), n_poly, 3, 3 * 8 << logn, 1, 3, 0)
    finally:
        moai.hip.reset_tuning()
